// evh_image.hip -- K0: area-average downscale, the MI355X counterpart of imutils.resize(frame, width=) ->
// cv2.resize(INTER_AREA) at evenvizion/processing/video_processing.py:62,73.  Shrinking (the reference's
// "resize_width to speed up" use) = area sums; enlarging = the operator's bilinear emulation (k_resize_linear_area);
// equal sizes are a plain copy.  Weights are float32 tables built on the host
// exactly as the operator builds them; each output value is accumulated in float32 in table order
// (inner sum over source columns, outer sum over source rows), then rounded half-to-even and saturated.
#include "evh_devmath.h"
#include "evh_internal.h"
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

namespace {

struct AreaTabDev {
  const int* xs; const int* xcnt; const int* xsi; const float* xal;   // per dst column: first entry, count; entries
  const int* ys; const int* ycnt; const int* ysi; const float* yal;
};

// One thread per output pixel computes the rounded uint8 of each of its channels; the INGEST flag of a kernel says where
// they go.  !INGEST: the cn bytes into the caller's packed rows (the stand-alone resize).  INGEST, N2, the
// fused ingest: the full-size frame is read ONCE, cvtColor's gray weights are applied to the rounded bytes -- exactly what
// the resized image would hold -- and the gray goes straight into pyramid level 0; the resized BGR image of
// video_processing.py:62,73 never exists in memory.  The store keeps its row offset inside the subscript: formed ahead of
// the gray weights (a named offset, a helper) it reorders the INGEST kernels (profiles/match_image_fold_isa.txt).
__device__ __forceinline__ uint8_t gray_of(int b, int g, int r) { return (uint8_t)((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14); }
__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }
// level 0's row stride is an int; the caller's of the stand-alone resize is whatever the ABI hands in
template <bool INGEST> using area_stride_t = std::conditional_t<INGEST, int, int64_t>;

// The kernels are templated on where a source pixel's channel bytes come from: SRC::row(img, y) hands out a row,
// Row::px(x, v) the pixel's bytes v[0 .. channels).
struct PackedSrc {       // rows of cn bytes per pixel (BGR or gray)
  const uint8_t* p; int cn; int64_t stride, img_stride;
  struct Row {
    const uint8_t* r; int cn;
    __device__ __forceinline__ void px(int x, int (&v)[3]) const {
      const uint8_t* q = r + (int64_t)x * cn;
#pragma unroll
      for (int c = 0; c < 3; c++) if (c < cn) v[c] = q[c];
    }
  };
  __device__ __forceinline__ int channels() const { return cn; }
  __device__ __forceinline__ Row row(int img, int y) const { return {p + (int64_t)img * img_stride + (int64_t)y * stride, cn}; }
};

// yuv420p -> bgr24 as capture.read() delivers it (video_processing.py:58,70; EVCAP_BGR_SWSCALE_X86 of include/evcap.h,
// SwsX86::px in capture/evcap_api.cpp): 13-bit BT.601 limited-range coefficients, arithmetic shifts, one saturation per
// channel (the 16-bit saturations of the original never act).  The chroma terms are shared by the luma pixels of a sample.
struct ChromaTerms { int b, g, r; };
__device__ __forceinline__ ChromaTerms chroma_terms(int u, int v) {
  const int cu = (u << 3) - 1024, cv = (v << 3) - 1024;
  return {(cu * 16525) >> 16, ((cu * -3209) >> 16) + ((cv * -6660) >> 16), (cv * 13075) >> 16};
}
__device__ __forceinline__ void yuv_px(int y, const ChromaTerms& t, int (&v)[3]) {
  const int Y = (((y << 3) - 128) * 9539) >> 16;
  v[0] = sat8(Y + t.b); v[1] = sat8(Y + t.g); v[2] = sat8(Y + t.r);
}
struct Yuv420Src {       // 4:2:0 planes, chroma pixel stride cps = 1 (I420 / YV12) or 2 (NV12 / NV21)
  const uint8_t* y; const uint8_t* cb; const uint8_t* cr;
  int64_t ys, cs, yfs, cfs; int cps;
  struct Row {
    const uint8_t* y; const uint8_t* cb; const uint8_t* cr; int cps;
    __device__ __forceinline__ void px(int x, int (&v)[3]) const {
      const int cx = (x >> 1) * cps;
      yuv_px(y[x], chroma_terms(cb[cx], cr[cx]), v);
    }
  };
  __device__ __forceinline__ int channels() const { return 3; }
  __device__ __forceinline__ Row row(int img, int yy) const {
    const int64_t co = (int64_t)img * cfs + (int64_t)(yy >> 1) * cs;
    return {y + (int64_t)img * yfs + (int64_t)yy * ys, cb + co, cr + co, cps};
  }
};

// INTER_AREA when shrinking by a non-integer ratio: float32 tables, accumulated in table order (see the head of the file)
template <bool INGEST, class SRC>
__global__ __launch_bounds__(256) void k_area(SRC src, uint8_t* __restrict__ dst, int64_t dst_img_stride, int dw, int dh,
                                              area_stride_t<INGEST> dst_stride, AreaTabDev T) {
  const int img = blockIdx.z, dy = blockIdx.y;
  const int dx = blockIdx.x * blockDim.x + threadIdx.x;
  if (dx >= dw) return;
  const int cn = src.channels();
  const int x0 = T.xs[dx], xn = T.xcnt[dx], y0 = T.ys[dy], yn = T.ycnt[dy];
  float sum[3] = {0.f, 0.f, 0.f};
  for (int j = 0; j < yn; j++) {
    const typename SRC::Row row = src.row(img, T.ysi[y0 + j]);
    float buf[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < xn; k++) {
      int px[3] = {0, 0, 0};
      row.px(T.xsi[x0 + k], px);
      const float a = T.xal[x0 + k];
#pragma unroll
      for (int c = 0; c < 3; c++) if (c < cn) buf[c] = buf[c] + (float)px[c] * a;
    }
    const float beta = T.yal[y0 + j];
#pragma unroll
    for (int c = 0; c < 3; c++) { const float term = beta * buf[c]; sum[c] = j == 0 ? term : sum[c] + term; }
  }
  int v[3];
#pragma unroll
  for (int c = 0; c < 3; c++) v[c] = sat8((int)rintf(sum[c]));
  if constexpr (INGEST) {
    dst[(int64_t)img * dst_img_stride + (int64_t)dy * dst_stride + dx] = cn == 3 ? gray_of(v[0], v[1], v[2]) : (uint8_t)v[0];
  } else {
#pragma unroll
    for (int c = 0; c < 3; c++) if (c < cn) dst[(int64_t)img * dst_img_stride + (int64_t)dy * dst_stride + dx * cn + c] = (uint8_t)v[c];
  }
}

// ... by integer ratios: integer block sums; 2 x 2 rounds as (sum + 2) >> 2, every other block through float32.  The two
// forms keep kernels of their own: the stand-alone one with a thread per output pixel measured 0.6 % slower than this
// thread per channel element (profiles/match_image_fold_stats.txt), so only the dispatch is shared.
__global__ void k_resize_area_int(const uint8_t* __restrict__ src, int cn, int64_t src_stride, int64_t src_img_stride,
                                  uint8_t* __restrict__ dst, int dw, int dh, int64_t dst_stride, int64_t dst_img_stride,
                                  int isx, int isy) {
  const int img = blockIdx.z, dy = blockIdx.y;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= dw * cn) return;
  const int dx = e / cn, c = e - dx * cn;
  const uint8_t* S = src + (int64_t)img * src_img_stride;
  int sum = 0;
  for (int j = 0; j < isy; j++)
    for (int i = 0; i < isx; i++) sum += S[(int64_t)(dy * isy + j) * src_stride + (int64_t)(dx * isx + i) * cn + c];
  int v;
  if (isx == 2 && isy == 2) v = (sum + 2) >> 2;
  else {
    const float scale = 1.f / (float)(isx * isy);
    v = (int)rintf((float)sum * scale);
  }
  dst[(int64_t)img * dst_img_stride + (int64_t)dy * dst_stride + e] = (uint8_t)min(max(v, 0), 255);
}

template <class SRC>
__global__ __launch_bounds__(256) void k_ingest_area_int(SRC src, uint8_t* __restrict__ pyr, int64_t pyr_frame_bytes, int dw,
                                                         int dh, int dst_stride, int isx, int isy) {
  const int img = blockIdx.z, dy = blockIdx.y;
  const int dx = blockIdx.x * blockDim.x + threadIdx.x;
  if (dx >= dw) return;
  const int cn = src.channels();
  int sum[3] = {0, 0, 0};
  for (int j = 0; j < isy; j++) {
    const typename SRC::Row row = src.row(img, dy * isy + j);
    for (int i = 0; i < isx; i++) {
      int px[3] = {0, 0, 0};
      row.px(dx * isx + i, px);
#pragma unroll
      for (int c = 0; c < 3; c++) if (c < cn) sum[c] += px[c];
    }
  }
  int v[3];
  const float scale = 1.f / (float)(isx * isy);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int r = (isx == 2 && isy == 2) ? (sum[c] + 2) >> 2 : (int)rintf((float)sum[c] * scale);
    v[c] = min(max(r, 0), 255);
  }
  pyr[(int64_t)img * pyr_frame_bytes + (int64_t)dy * dst_stride + dx] = cn == 3 ? gray_of(v[0], v[1], v[2]) : (uint8_t)v[0];
}

// INTER_AREA when ENLARGING (imutils.resize(frame, width=) with width > frame width, video_processing.py:62,73): the
// operator emulates it with its 8-bit bilinear machinery -- 11-bit coefficients from area-mode tables
//   s = floor(d*scale), f = (float)((d+1) - (s+1)*inv_scale), f = f <= 0 ? 0 : f - floor(f),
// horizontal pass in int (x2048), vertical pass ((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2 >> 2.  One thread per
// output pixel; the coefficients are recomputed per thread in the operator's own f64/f32 arithmetic.
struct LinAreaCoef { int s; int a0, a1; };
__device__ __forceinline__ LinAreaCoef lin_area_coef(int d, int ssize, double scale, double inv) {
  int s = (int)floor((double)d * scale);
  float f = (float)((double)(d + 1) - (double)(s + 1) * inv);
  f = f <= 0.f ? 0.f : f - floorf(f);
  if (s < 0) { f = 0.f; s = 0; }
  bool edge = false;
  if (s + 1 >= ssize) { edge = true; if (s >= ssize - 1) { f = 0.f; s = ssize - 1; } }
  LinAreaCoef c;
  c.s = s;
  c.a0 = min(max((int)rintf((1.f - f) * 2048.f), -32768), 32767);
  c.a1 = min(max((int)rintf(f * 2048.f), -32768), 32767);
  if (edge) { c.a0 = 2048; c.a1 = 0; }           // D[dx] = S[sx] * ONE beyond xmax
  return c;
}
// vertical coefficients: no edge substitution (the operator clips the ROWS instead)
__device__ __forceinline__ void lin_area_beta(int dy, double scale, double inv, int& sy, int& b0, int& b1) {
  sy = (int)floor((double)dy * scale);
  float f = (float)((double)(dy + 1) - (double)(sy + 1) * inv);
  f = f <= 0.f ? 0.f : f - floorf(f);
  b0 = min(max((int)rintf((1.f - f) * 2048.f), -32768), 32767);
  b1 = min(max((int)rintf(f * 2048.f), -32768), 32767);
}
template <bool INGEST, class SRC>
__global__ __launch_bounds__(256) void k_resize_linear_area(SRC src, int sw, int sh, uint8_t* __restrict__ dst, int dw, int dh,
                                                            int64_t dst_stride, int64_t dst_img_stride, double scale_x,
                                                            double inv_x, double scale_y, double inv_y) {
  const int img = blockIdx.z, dy = blockIdx.y;
  const int dx = blockIdx.x * blockDim.x + threadIdx.x;
  if (dx >= dw) return;
  const int cn = src.channels();
  const LinAreaCoef X = lin_area_coef(dx, sw, scale_x, inv_x);
  int sy, b0, b1;
  lin_area_beta(dy, scale_y, inv_y, sy, b0, b1);
  sy = min(max(sy, 0), sh - 1);
  const typename SRC::Row r0 = src.row(img, min(sy, sh - 1)), r1 = src.row(img, min(sy + 1, sh - 1));
  const int x1 = min(X.s + 1, sw - 1);
  int p00[3] = {0, 0, 0}, p01[3] = {0, 0, 0}, p10[3] = {0, 0, 0}, p11[3] = {0, 0, 0};
  r0.px(X.s, p00); r0.px(x1, p01); r1.px(X.s, p10); r1.px(x1, p11);
  int v[3] = {0, 0, 0};
#pragma unroll
  for (int c = 0; c < 3; c++) if (c < cn) {
    const int h0 = p00[c] * X.a0 + p01[c] * X.a1;
    const int h1 = p10[c] * X.a0 + p11[c] * X.a1;
    v[c] = ((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2) & 0xFF;
  }
  uint8_t* D = dst + (int64_t)img * dst_img_stride + (int64_t)dy * dst_stride;
  if (INGEST) D[dx] = cn == 3 ? gray_of(v[0], v[1], v[2]) : (uint8_t)v[0];
  else
#pragma unroll
    for (int c = 0; c < 3; c++) if (c < cn) D[dx * cn + c] = (uint8_t)v[c];
}

// The stand-alone converter (evh_yuv420_to_bgr) and, with GRAY, level 0 of frames that are not resized.  A streaming
// kernel: one thread owns 16 luma pixels of the TWO rows that share a chroma row, so chroma is fetched once -- per row one
// 16-byte luma load, 8 + 8 chroma bytes (16 + 16 interleaved), three 16-byte BGR stores (one 16-byte gray store).  `vec`:
// 0 = bytewise everywhere (some pointer or stride is not aligned for the wide form), 1 = planar chroma, 2 = interleaved
// chroma with Cb first, 3 = with Cr first; runs cut by the right edge are always bytewise.  Bytes past a row's w pixels
// are neither read nor written.
#define YUV_RUN 16
template <bool GRAY>
__global__ __launch_bounds__(256) void k_yuv420_rows(Yuv420Src src, int w, int h, uint8_t* __restrict__ dst, int64_t dst_stride,
                                                     int64_t dst_img_stride, int runs_per_row, int nruns, int vec) {
  const int img = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nruns) return;
  const int ry = t / runs_per_row, x = (t - ry * runs_per_row) * YUV_RUN;
  const int n = min(YUV_RUN, w - x), nrows = min(2, h - 2 * ry);
  const bool wide = vec != 0 && n == YUV_RUN;
  const Yuv420Src::Row R0 = src.row(img, 2 * ry);
  uint8_t u8[YUV_RUN / 2], v8[YUV_RUN / 2];
  if (wide && vec == 1) {
    const uint2 a = *reinterpret_cast<const uint2*>(R0.cb + (x >> 1)), b = *reinterpret_cast<const uint2*>(R0.cr + (x >> 1));
#pragma unroll
    for (int k = 0; k < 4; k++) {
      u8[k] = (uint8_t)(a.x >> (8 * k)); u8[4 + k] = (uint8_t)(a.y >> (8 * k));
      v8[k] = (uint8_t)(b.x >> (8 * k)); v8[4 + k] = (uint8_t)(b.y >> (8 * k));
    }
  } else if (wide) {
    const uint4 a = *reinterpret_cast<const uint4*>((vec == 2 ? R0.cb : R0.cr) + x);
    const uint32_t q[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint8_t lo = (uint8_t)(q[k >> 1] >> (16 * (k & 1))), hi = (uint8_t)(q[k >> 1] >> (16 * (k & 1) + 8));
      u8[k] = vec == 2 ? lo : hi; v8[k] = vec == 2 ? hi : lo;
    }
  } else {
#pragma unroll
    for (int k = 0; k < YUV_RUN / 2; k++) {
      const bool in = 2 * k < n;
      u8[k] = in ? R0.cb[((x >> 1) + k) * R0.cps] : 0; v8[k] = in ? R0.cr[((x >> 1) + k) * R0.cps] : 0;
    }
  }
  ChromaTerms T[YUV_RUN / 2];
#pragma unroll
  for (int k = 0; k < YUV_RUN / 2; k++) T[k] = chroma_terms(u8[k], v8[k]);
  for (int r = 0; r < nrows; r++) {
    const uint8_t* yrow = R0.y + (int64_t)r * src.ys + x;
    uint8_t* D = dst + (int64_t)img * dst_img_stride + (int64_t)(2 * ry + r) * dst_stride + (int64_t)x * (GRAY ? 1 : 3);
    uint8_t y8[YUV_RUN];
    if (wide) {
      const uint4 a = *reinterpret_cast<const uint4*>(yrow);
      const uint32_t q[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int k = 0; k < YUV_RUN; k++) y8[k] = (uint8_t)(q[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
      for (int k = 0; k < YUV_RUN; k++) y8[k] = k < n ? yrow[k] : 0;
    }
    uint32_t out[GRAY ? YUV_RUN / 4 : 3 * YUV_RUN / 4];
#pragma unroll
    for (int k = 0; k < (GRAY ? YUV_RUN / 4 : 3 * YUV_RUN / 4); k++) out[k] = 0;
#pragma unroll
    for (int k = 0; k < YUV_RUN; k++) {
      int p[3];
      yuv_px(y8[k], T[k >> 1], p);
      if (GRAY) out[k >> 2] |= (uint32_t)gray_of(p[0], p[1], p[2]) << (8 * (k & 3));
      else
#pragma unroll
        for (int c = 0; c < 3; c++) out[(3 * k + c) >> 2] |= (uint32_t)p[c] << (8 * ((3 * k + c) & 3));
    }
    if (wide) {
#pragma unroll
      for (int k = 0; k < (GRAY ? 1 : 3); k++)
        reinterpret_cast<uint4*>(D)[k] = make_uint4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
    } else {
      const int nb = n * (GRAY ? 1 : 3);
#pragma unroll
      for (int k = 0; k < YUV_RUN * (GRAY ? 1 : 3); k++) if (k < nb) D[k] = (uint8_t)(out[k >> 2] >> (8 * (k & 3)));
    }
  }
}

// N3: fixed-plane coordinate field of processing_visualization.py:407-408 -- every pixel (x, y) of
// the resized frame mapped through the frame's superposed H (np.apply_along_axis(homography_transformation): hdot,
// then one division per coordinate) -- and np.max of it (the value heatmap_video_processing returns and
// evenvizion_component.py writes to metrics_file.txt).  np.max semantics: a NaN anywhere gives NaN, an all -inf
// field gives -inf (out_max is seeded with the key of -inf by k_seed_fixed_plane_max).  w * h <= INT_MAX (the entry
// checks), so the unsigned index plus one grid stride cannot wrap.

// order-preserving key of a double, so that an integer atomicMax gives the floating-point maximum; every NaN is
// keyed as the positive quiet NaN, above +inf
__device__ __forceinline__ unsigned long long max_key(double m) {
  if (m != m) return 0xFFF8000000000000ull;
  const unsigned long long b = (unsigned long long)__double_as_longlong(m);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// np.max's pairwise rule: a NaN wins and stays (fmax would drop it); +0 outranks -0, as in the key order
__device__ __forceinline__ double nan_max(double m, double v) {
  if (m != m) return m;
  return (v != v || v > m || (v == m && signbit(m))) ? v : m;
}

__global__ __launch_bounds__(256) void k_seed_fixed_plane_max(unsigned long long* __restrict__ out_max, int n) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < n) out_max[f] = max_key(-INFINITY);
}

__global__ __launch_bounds__(256) void k_fixed_plane(const double* __restrict__ Hs, int w, int h,
                                                     double* __restrict__ field, unsigned long long* __restrict__ out_max) {
  const int f = blockIdx.y;
  const double* H = Hs + 9 * f;
  const unsigned wh = (unsigned)w * (unsigned)h;
  double m = -INFINITY;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < wh; i += gridDim.x * blockDim.x) {
    const unsigned y = i / (unsigned)w, x = i - y * (unsigned)w;
    double tx, ty, tw;
    hdot(H, (double)x, (double)y, &tx, &ty, &tw);
    const double u = tx / tw, v = ty / tw;
    if (field) { field[((int64_t)f * wh + i) * 2] = u; field[((int64_t)f * wh + i) * 2 + 1] = v; }
    m = nan_max(m, nan_max(u, v));
  }
  for (int s = 32; s > 0; s >>= 1) m = nan_max(m, __shfl_xor(m, s));
  if ((threadIdx.x & 63) == 0 && m != -INFINITY) atomicMax(&out_max[f], max_key(m));
}

// N1: utils.superposition_dict (utils.py:184-211) as one sequential scan: out[0] = H[0] (matrix_H_first),
// out[i] = np.dot(H[i], out[i-1]) / [2][2].  np.dot(3x3, 3x3) = the forward FMA chain pinned by the reference-captured
// fixtures (tests/golden/glue_goldens.json "sup_false"), the same order k_ransac_final_stream uses.
__global__ __launch_bounds__(64) void k_superposition_scan(const double* __restrict__ H, int n, double* __restrict__ out) {
  __shared__ double S[9];
  const int lane = threadIdx.x;
  if (lane < 9) { S[lane] = H[lane]; out[lane] = H[lane]; }
  __syncthreads();
  for (int i = 1; i < n; i++) {
    double P = 0;
    if (lane < 9) {
      const double* Hi = H + 9 * (int64_t)i;
      const int r = lane / 3, c = lane - 3 * r;
      P = fma(Hi[3 * r + 2], S[6 + c], fma(Hi[3 * r + 1], S[3 + c], Hi[3 * r] * S[c]));
    }
    const double P8 = __shfl(P, 8);
    __syncthreads();
    if (lane < 9) { const double v = P / P8; S[lane] = v; out[9 * (int64_t)i + lane] = v; }
    __syncthreads();
  }
}

// N1: fixed_coordinate_system.from_original_to_fix / from_fix_to_original (fixed_coordinate_system.py:19-69, 72-122)
// batched: point i -> np.around(np.dot(M[idx[i]], (kx*x, ky*y, 1))[:2] / [2], decimals).  M is H itself or (for the
// inverse direction) the caller's inverted matrix.  np.dot(3x3, vec) = fma(h0, x, h1*y) + h2 (fixture "hv"); np.around
// = rint(v * 10^d) / 10^d (half to even); decimals < 0: no rounding.
__global__ __launch_bounds__(256) void k_transform_points(const double* __restrict__ M, const int* __restrict__ idx,
                                                          const double* __restrict__ pts, int n, double kx, double ky,
                                                          int decimals, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* H = M + 9 * (int64_t)idx[i];
  const double x = kx * pts[2 * i], y = ky * pts[2 * i + 1];
  double tx, ty, tw;
  hdot(H, x, y, &tx, &ty, &tw);
  double u = tx / tw, v = ty / tw;
  if (decimals >= 0) {
    double sc = 1.0;
    for (int d = 0; d < decimals; d++) sc *= 10.0;
    u = __builtin_rint(u * sc) / sc;
    v = __builtin_rint(v * sc) / sc;
  }
  out[2 * i] = u; out[2 * i + 1] = v;
}

// Stabilised output (stabilization.py:129-172, 220-249): frames resampled through their superposed H onto a canvas of the
// fixed plane; canvas pixel (x, y) is the plane point (x + ox, y + oy).  The arithmetic is the one include/evhip.h states
// for evh_warp_fixed_plane, one IEEE float64 operation at a time (no fma: the tests restate it in numpy byte for byte).
// A thread owns WARP_RUN adjacent canvas pixels of a row: the frame's matrix is formed once for them, and their bytes
// leave as 32-bit words (`wide`: every pointer and stride involved is a multiple of 4; runs cut by the right edge go
// bytewise).  Bytes past a row's dw pixels are neither read nor written.
#define WARP_RUN 4
struct WarpMap { double a[9]; };
// canvas -> frame: M itself (inverse_map) or its adjugate -- not divided by the determinant, a projective map does not care
__device__ __forceinline__ WarpMap warp_map(const double* __restrict__ M, int inverse_map) {
  const double m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3], m4 = M[4], m5 = M[5], m6 = M[6], m7 = M[7], m8 = M[8];
  if (inverse_map) return {{m0, m1, m2, m3, m4, m5, m6, m7, m8}};
  return {{m4 * m8 - m5 * m7, m2 * m7 - m1 * m8, m1 * m5 - m2 * m4,
           m5 * m6 - m3 * m8, m0 * m8 - m2 * m6, m2 * m3 - m0 * m5,
           m3 * m7 - m4 * m6, m1 * m6 - m0 * m7, m0 * m4 - m1 * m3}};
}
// Frame `img` at plane point (X, Y): false = the frame does not cover it (v is left alone).  The source position comes in
// 1/32 pixels (INTER_BITS = 5), rounded half to even; the comparisons are made in double, so NaN and +-inf (a zero, singular
// or NaN matrix, the horizon) cover nothing.  A covered position has 0 <= sx <= sw - 1, and sx + 1 is read only with fx != 0,
// i.e. sx <= sw - 2 (rows alike): no tap leaves the frame.
template <class SRC>
__device__ __forceinline__ bool warp_sample(const SRC& src, int img, const WarpMap& A, double X, double Y, int sw, int sh,
                                            int (&v)[3]) {
  const double tx = (A.a[0] * X + A.a[1] * Y) + A.a[2];
  const double ty = (A.a[3] * X + A.a[4] * Y) + A.a[5];
  const double tw = (A.a[6] * X + A.a[7] * Y) + A.a[8];
  const double U = __builtin_rint(tx / tw * 32.0), V = __builtin_rint(ty / tw * 32.0);
  if (!(U >= 0.0 && U <= (double)(32 * (sw - 1)) && V >= 0.0 && V <= (double)(32 * (sh - 1)))) return false;
  const int u = (int)U, w = (int)V;
  const int sx = u >> 5, fx = u & 31, sy = w >> 5, fy = w & 31;
  const int cn = src.channels();
  int p00[3] = {0, 0, 0}, p01[3] = {0, 0, 0}, p10[3] = {0, 0, 0}, p11[3] = {0, 0, 0};
  const typename SRC::Row r0 = src.row(img, sy);
  r0.px(sx, p00);
  if (fx) r0.px(sx + 1, p01);
  if (fy) {
    const typename SRC::Row r1 = src.row(img, sy + 1);
    r1.px(sx, p10);
    if (fx) r1.px(sx + 1, p11);
  }
  const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
#pragma unroll
  for (int c = 0; c < 3; c++) if (c < cn) v[c] = (p00[c] * w00 + p01[c] * w01 + p10[c] * w10 + p11[c] * w11 + 512) >> 10;
  return true;
}
// the n <= WARP_RUN pixels of a run, CN bytes each, from / to canvas rows
template <int CN>
__device__ __forceinline__ void warp_run_load(const uint8_t* S, int n, bool wide, int (&v)[WARP_RUN][3]) {
  if (wide) {
    uint32_t q[CN];
#pragma unroll
    for (int k = 0; k < CN; k++) q[k] = reinterpret_cast<const uint32_t*>(S)[k];
#pragma unroll
    for (int k = 0; k < WARP_RUN * CN; k++) v[k / CN][k % CN] = (q[k >> 2] >> (8 * (k & 3))) & 255;
  } else {
#pragma unroll
    for (int k = 0; k < WARP_RUN * CN; k++) if (k < n * CN) v[k / CN][k % CN] = S[k];
  }
}
template <int CN>
__device__ __forceinline__ void warp_run_store(uint8_t* D, int n, bool wide, const int (&v)[WARP_RUN][3]) {
  if (wide) {
    uint32_t q[CN];
#pragma unroll
    for (int k = 0; k < CN; k++) q[k] = 0;
#pragma unroll
    for (int k = 0; k < WARP_RUN * CN; k++) q[k >> 2] |= (uint32_t)v[k / CN][k % CN] << (8 * (k & 3));
#pragma unroll
    for (int k = 0; k < CN; k++) reinterpret_cast<uint32_t*>(D)[k] = q[k];
  } else {
#pragma unroll
    for (int k = 0; k < WARP_RUN * CN; k++) if (k < n * CN) D[k] = (uint8_t)v[k / CN][k % CN];
  }
}
// MODE EVH_WARP_EACH: grid.y = frame, out[k] = frame k over the background.  EVH_WARP_HISTORY: the frames upward with the
// run in registers, out[k] stored at every step (the last covering frame wins).  EVH_WARP_MOSAIC: the frames downward, a
// pixel is settled by the first frame that covers it; bg may BE out (a thread reads only the bytes it writes, before it
// writes them), hence no __restrict__ on either.
template <int MODE, int CN, class SRC>
__global__ __launch_bounds__(256) void k_warp_fixed_plane(SRC src, int nframes, int sw, int sh, const double* __restrict__ M,
                                                          int inverse_map, const uint8_t* bg, uint8_t* out, int dw,
                                                          int64_t out_stride, int64_t out_img_stride, int ox, int oy,
                                                          int runs_per_row, unsigned nruns, int vec) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nruns) return;
  const int y = (int)(t / (unsigned)runs_per_row), x0 = ((int)t - y * runs_per_row) * WARP_RUN;
  const int n = min(WARP_RUN, dw - x0);
  const bool wide = vec != 0 && n == WARP_RUN;
  const int64_t at = (int64_t)y * out_stride + (int64_t)x0 * CN;
  const double Y = (double)((int64_t)y + oy);
  double X[WARP_RUN];
#pragma unroll
  for (int p = 0; p < WARP_RUN; p++) X[p] = (double)((int64_t)x0 + p + ox);
  int v[WARP_RUN][3];
#pragma unroll
  for (int p = 0; p < WARP_RUN; p++) v[p][0] = v[p][1] = v[p][2] = 0;
  if constexpr (MODE == EVH_WARP_HISTORY) {
    if (bg) warp_run_load<CN>(bg + at, n, wide, v);
    for (int k = 0; k < nframes; k++) {
      const WarpMap A = warp_map(M + 9 * (int64_t)k, inverse_map);
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++) if (p < n) warp_sample(src, k, A, X[p], Y, sw, sh, v[p]);
      warp_run_store<CN>(out + (int64_t)k * out_img_stride + at, n, wide, v);
    }
  } else {
    unsigned open = (1u << n) - 1;                      // pixels of the run no frame has covered yet
    const int first = MODE == EVH_WARP_EACH ? (int)blockIdx.y : nframes - 1, last = MODE == EVH_WARP_EACH ? first : 0;
    for (int k = first; k >= last && open; k--) {
      const WarpMap A = warp_map(M + 9 * (int64_t)k, inverse_map);
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++)
        if (((open >> p) & 1) && warp_sample(src, k, A, X[p], Y, sw, sh, v[p])) open &= ~(1u << p);
    }
    if (open && bg) {
      int b[WARP_RUN][3];
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++) b[p][0] = b[p][1] = b[p][2] = 0;
      warp_run_load<CN>(bg + at, n, wide, b);
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++) if ((open >> p) & 1) { v[p][0] = b[p][0]; v[p][1] = b[p][1]; v[p][2] = b[p][2]; }
    }
    warp_run_store<CN>(out + (MODE == EVH_WARP_EACH ? (int64_t)blockIdx.y * out_img_stride : 0) + at, n, wide, v);
  }
}

// The motion-compensated residual of a pair (include/evhip.h states the contract for evh_pair_residual): grid.y = pair, previous
// frame p * frame_step, current frame p * frame_step + 1.  A thread owns WARP_RUN adjacent pixels of a row of the current frame:
// it loads them and the previous frame's pixels at the same place (as words where vec bit 1 allows; planes are converted pixel by
// pixel), forms the pair's matrix once, samples the previous frame through warp_sample and keeps six partial sums.  No warped
// frame is ever written.  Bounds of the sums, all unsigned: a thread holds at most WARP_RUN * 255^2 = 260 100 per statistic, a
// workgroup 256 * 4 * 65025 = 66 585 600 < 2^32, so the registers, the __shfl_xor steps across the wave and the LDS sums across
// the four waves are 32-bit; a pair holds at most INT_MAX * 65025 < 2^47 (w * h <= INT_MAX), so d_stats is 64-bit and takes one
// integer atomicAdd per statistic per workgroup.  Integer sums do not depend on the order of the atomics; there is no
// floating-point accumulation.  The 256 threads of a block all reach the barrier; those past the last run add zeros.
template <int CN, class SRC>
__global__ __launch_bounds__(256) void k_pair_residual(SRC src, int frame_step, int w, int h, const double* __restrict__ M,
                                                       int threshold, unsigned long long* __restrict__ stats,
                                                       uint8_t* __restrict__ out, int kind, int64_t out_stride,
                                                       int64_t out_img_stride, int runs_per_row, unsigned nruns, int vec) {
  __shared__ uint32_t part[4][EVH_RES_NSTATS];
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const int pair = blockIdx.y;
  uint32_t s[EVH_RES_NSTATS];
#pragma unroll
  for (int k = 0; k < EVH_RES_NSTATS; k++) s[k] = 0;
  if (t < nruns) {
    const int prev = pair * frame_step, cur = prev + 1;
    const int y = (int)(t / (unsigned)runs_per_row), x0 = ((int)t - y * runs_per_row) * WARP_RUN;
    const int n = min(WARP_RUN, w - x0);
    const bool full = n == WARP_RUN;
    int a[WARP_RUN][3], b[WARP_RUN][3];                   // the current and the previous frame's pixels of the run
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) a[p][0] = a[p][1] = a[p][2] = b[p][0] = b[p][1] = b[p][2] = 0;
    if constexpr (std::is_same_v<SRC, PackedSrc>) {
      const int64_t at = (int64_t)y * src.stride + (int64_t)x0 * CN;
      warp_run_load<CN>(src.p + (int64_t)cur * src.img_stride + at, n, full && (vec & 2), a);
      warp_run_load<CN>(src.p + (int64_t)prev * src.img_stride + at, n, full && (vec & 2), b);
    } else {
      const typename SRC::Row ra = src.row(cur, y), rb = src.row(prev, y);
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++) if (p < n) { ra.px(x0 + p, a[p]); rb.px(x0 + p, b[p]); }
    }
    const WarpMap A = warp_map(M + 9 * (int64_t)pair, 1);
    const double Y = (double)y;
    int q[WARP_RUN][3];
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) {
      q[p][0] = q[p][1] = q[p][2] = 0;
      int r[3] = {0, 0, 0};
      if (p < n && warp_sample(src, prev, A, (double)(x0 + p), Y, w, h, r)) {
        const int g_cur = CN == 3 ? gray_of(a[p][0], a[p][1], a[p][2]) : a[p][0];
        const int g_prev = CN == 3 ? gray_of(b[p][0], b[p][1], b[p][2]) : b[p][0];
        const int g_reg = CN == 3 ? gray_of(r[0], r[1], r[2]) : r[0];
        const uint32_t d = (uint32_t)abs(g_cur - g_reg), d0 = (uint32_t)abs(g_cur - g_prev);
        s[EVH_RES_COVERED] += 1;
        s[EVH_RES_SAD] += d; s[EVH_RES_SSD] += d * d;
        s[EVH_RES_SAD0] += d0; s[EVH_RES_SSD0] += d0 * d0;
        s[EVH_RES_MOVING] += d > (uint32_t)threshold ? 1 : 0;
        q[p][0] = kind == EVH_RESIDUAL_MASK ? (d > (uint32_t)threshold ? 255 : 0) : (int)d;
      }
    }
    if (out) warp_run_store<1>(out + (int64_t)pair * out_img_stride + (int64_t)y * out_stride + x0, n, full && (vec & 1), q);
  }
#pragma unroll
  for (int k = 0; k < EVH_RES_NSTATS; k++)
    for (int m = 32; m > 0; m >>= 1) s[k] += __shfl_xor(s[k], m);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < EVH_RES_NSTATS; k++) part[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < EVH_RES_NSTATS) {
    const uint32_t sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (sum) atomicAdd(&stats[(int64_t)pair * EVH_RES_NSTATS + threadIdx.x], (unsigned long long)sum);
  }
}

// The trail (stabilization.py:21-44, 129-172, 252-290): EVH_WARP_HISTORY with the colour step include/evhip.h states for
// evh_trail_fixed_plane between the frames.  g_trail_tab holds S[256] | H[256], built by the launcher on the host in double
// and uploaded once per context; a workgroup stages it in LDS, two entries per thread (the look-ups are per lane).
__device__ int32_t g_trail_tab[512];
// BGR -> (h, s, v), int32: h in [0, 179], s and v in [0, 255]
__device__ __forceinline__ void trail_to_hsv(const int32_t* tab, const int (&p)[3], int& h, int& s, int& v) {
  const int b = p[0], g = p[1], r = p[2];
  v = max(b, max(g, r));
  const int d = v - min(b, min(g, r));
  s = (d * tab[v] + 2048) >> 12;
  const int t = v == r ? g - b : v == g ? b - r + 2 * d : r - g + 4 * d;
  h = (t * tab[256 + d] + 2048) >> 12;
  if (h < 0) h += 180;
}
// (h, s, v) -> BGR, IEEE float32 with one rounding per operation (the unit is built with -ffp-contract=off; the intrinsics say
// so where a product feeds a sum).  s == 0 needs no case of its own: sf = 0 makes every entry of tab vf * 1.
__device__ __forceinline__ void trail_from_hsv(int h, int s, int v, int (&o)[3]) {
  float hf = __fmul_rn((float)h, __uint_as_float(0x3D088889u));   // 6.f / 180.f
  while (hf >= 6.f) hf = __fsub_rn(hf, 6.f);
  const int k = (int)hf;                                         // floor: hf >= 0
  const float f = __fsub_rn(hf, (float)k);
  const float K = __uint_as_float(0x3B808081u);                  // 1.f / 255.f
  const float sf = __fmul_rn((float)s, K), vf = __fmul_rn((float)v, K);
  const float t0 = vf, t1 = __fmul_rn(vf, __fsub_rn(1.f, sf)), t2 = __fmul_rn(vf, __fsub_rn(1.f, __fmul_rn(sf, f))),
              t3 = __fmul_rn(vf, __fsub_rn(1.f, __fmul_rn(sf, __fsub_rn(1.f, f))));
  // sector k -> which of t0..t3 is b, g, r: {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}, two bits per sector
  const unsigned sel[3] = {0x835u, 0x583u, 0x358u};
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const unsigned i = (sel[ch] >> (2 * k)) & 3u;
    const float x = i == 0 ? t0 : i == 1 ? t1 : i == 2 ? t2 : t3;
    o[ch] = (int)fminf(fmaxf(__builtin_rintf(__fmul_rn(x, 255.f)), 0.f), 255.f);
  }
}
// canvas and out are distinct buffers (the entry refuses an overlap); a thread reads only the canvas bytes it later writes.
// vec bit 0: out moves as words, bit 1: canvas does.  The 256 threads of a block all reach the barrier; those past the last
// run then leave.
template <class SRC>
__global__ __launch_bounds__(256) void k_trail_fixed_plane(SRC src, int nframes, int sw, int sh, const double* __restrict__ M,
                                                           int inverse_map, const int32_t* __restrict__ rect, uint8_t* canvas,
                                                           int64_t canvas_stride, uint8_t* out, int64_t out_stride,
                                                           int64_t out_img_stride, int dw, int ox, int oy, int runs_per_row,
                                                           unsigned nruns, int vec) {
  __shared__ int32_t tab[512];
  tab[threadIdx.x] = g_trail_tab[threadIdx.x];
  tab[256 + threadIdx.x] = g_trail_tab[256 + threadIdx.x];
  __syncthreads();
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nruns) return;
  const int y = (int)(t / (unsigned)runs_per_row), x0 = ((int)t - y * runs_per_row) * WARP_RUN;
  const int n = min(WARP_RUN, dw - x0);
  const bool full = n == WARP_RUN;
  const double Y = (double)((int64_t)y + oy);
  double X[WARP_RUN];
#pragma unroll
  for (int p = 0; p < WARP_RUN; p++) X[p] = (double)((int64_t)x0 + p + ox);
  // the two pictures that need no pixel: show of a colour with V < 2, and show of the white outline
  int dark[3] = {0, 0, 0}, white[3] = {0, 0, 0};
  if (out) {
    const int w255[3] = {255, 255, 255};
    int h, s, v;
    trail_to_hsv(tab, w255, h, s, v);
    trail_from_hsv(h, s, v - 2, white);
    trail_from_hsv(222, 12, 31, dark);
  }
  uint8_t* const crow = canvas + (int64_t)y * canvas_stride + (int64_t)x0 * 3;
  int c[WARP_RUN][3];
#pragma unroll
  for (int p = 0; p < WARP_RUN; p++) c[p][0] = c[p][1] = c[p][2] = 0;
  warp_run_load<3>(crow, n, full && (vec & 2), c);
  for (int k = 0; k < nframes; k++) {
    const WarpMap A = warp_map(M + 9 * (int64_t)k, inverse_map);
    int rx0 = 0, ry0 = 0, rx1 = -1, ry1 = -1;
    if (rect) { rx0 = rect[4 * k]; ry0 = rect[4 * k + 1]; rx1 = rect[4 * k + 2]; ry1 = rect[4 * k + 3]; }
    const bool yin = y >= ry0 && y <= ry1, yedge = y == ry0 || y == ry1;
    int q[WARP_RUN][3];
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) {
      q[p][0] = q[p][1] = q[p][2] = 0;
      if (p >= n) continue;
      warp_sample(src, k, A, X[p], Y, sw, sh, c[p]);
      const int x = x0 + p;
      const bool outline = yin && x >= rx0 && x <= rx1 && (yedge || x == rx0 || x == rx1);
      // keep(c); where V >= 2 it is show(c) too, where V < 2 it is black and the picture is the constant
      const bool lit = max(c[p][0], max(c[p][1], c[p][2])) >= 2;
      q[p][0] = dark[0]; q[p][1] = dark[1]; q[p][2] = dark[2];
      if (lit) {
        int h, s, v;
        trail_to_hsv(tab, c[p], h, s, v);
        trail_from_hsv(h, s, v - 2, c[p]);
        q[p][0] = c[p][0]; q[p][1] = c[p][1]; q[p][2] = c[p][2];
      } else {
        c[p][0] = c[p][1] = c[p][2] = 0;
      }
      if (outline) { q[p][0] = white[0]; q[p][1] = white[1]; q[p][2] = white[2]; }
    }
    if (out) warp_run_store<3>(out + (int64_t)k * out_img_stride + (int64_t)y * out_stride + (int64_t)x0 * 3, n, full && (vec & 1), q);
  }
  warp_run_store<3>(crow, n, full && (vec & 2), c);
}

// The background plate (include/evhip.h states the contract for evh_plate_fixed_plane): the per-pixel, per-channel lower
// median of the frames that cover a canvas pixel, the number of those frames, and per frame the mask of the pixels that
// differ from the plate.  One canvas pixel per thread, one wave per workgroup; dynamic LDS u32[nframes][64], the column
// lds[.][lane] is this thread's alone (bank = lane: every access is conflict-free, and no barrier is needed, so threads past
// the last pixel leave at once).
//   pass 1  every frame sampled once through warp_sample; the samples of the n covering frames are kept, in frame order, at
//           the head of the column as b | g << 8 | r << 16 | k << 24 (gray: the byte | k << 24; k <= 254);
//   pass 2  the element of rank (n - 1) >> 1 by an MSB-first radix select, 8 rounds over the n kept words, the three channels
//           side by side in the word: with P the packed prefixes found so far, a sample's byte of (word ^ P) & HI (HI = the
//           bits from `bit` upward in each of the three bytes) is zero iff it agrees with the prefix above `bit` and has a 0
//           there; ((t & 0x7f7f7f) + 0x7f7f7f | t) >> 7 & 0x010101 is 1 in each byte that is NOT zero, and the three counts
//           (<= 255 each, no carry) add up in one register;
//   pass 3  only with masks: frame by frame along the kept words, one byte per frame (64 adjacent pixels of a row: one
//           64-byte store a wave).
// The samples never sit in a private array: indexed at run time it would go to scratch.
template <int CN, class SRC>
__global__ __launch_bounds__(64) void k_plate_fixed_plane(SRC src, int nframes, int sw, int sh, const double* __restrict__ M,
                                                          int inverse_map, int min_cover, const uint8_t* __restrict__ bg,
                                                          uint8_t* __restrict__ plate, int64_t plate_stride,
                                                          uint8_t* __restrict__ count, int64_t count_stride,
                                                          uint8_t* __restrict__ mask, int threshold, int64_t mask_stride,
                                                          int64_t mask_img_stride, int dw, int ox, int oy, unsigned npix) {
  extern __shared__ uint32_t plate_col[];
  const unsigned t = blockIdx.x * 64u + threadIdx.x;
  if (t >= npix) return;
  const int y = (int)(t / (unsigned)dw), x = (int)t - y * dw;
  const double X = (double)((int64_t)x + ox), Y = (double)((int64_t)y + oy);
  uint32_t* const col = plate_col + threadIdx.x;
  int n = 0;
  for (int k = 0; k < nframes; k++) {
    const WarpMap A = warp_map(M + 9 * (int64_t)k, inverse_map);
    int v[3] = {0, 0, 0};
    if (warp_sample(src, k, A, X, Y, sw, sh, v)) {
      col[64 * n] = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)k << 24;
      n++;
    }
  }
  const bool settled = n >= min_cover;                  // min_cover >= 1: a settled pixel has a sample
  int p[3] = {0, 0, 0};
  if (settled) {
    uint32_t P = 0;
    int rank[3];
    rank[0] = rank[1] = rank[2] = (n - 1) >> 1;
    for (int bit = 7; bit >= 0; bit--) {
      const uint32_t HI = ((0xffu << bit) & 0xffu) * 0x010101u;
      uint32_t differ = 0;
      for (int j = 0; j < n; j++) {
        const uint32_t d = (col[64 * j] ^ P) & HI;
        differ += ((((d & 0x7f7f7fu) + 0x7f7f7fu) | d) >> 7) & 0x010101u;
      }
#pragma unroll
      for (int c = 0; c < CN; c++) {
        const int zeros = n - (int)((differ >> (8 * c)) & 255u);
        if (rank[c] >= zeros) { rank[c] -= zeros; P |= 1u << (bit + 8 * c); }
      }
    }
#pragma unroll
    for (int c = 0; c < CN; c++) p[c] = (int)((P >> (8 * c)) & 255u);
  } else if (bg) {
#pragma unroll
    for (int c = 0; c < CN; c++) p[c] = bg[(int64_t)y * plate_stride + (int64_t)x * CN + c];
  }
#pragma unroll
  for (int c = 0; c < CN; c++) plate[(int64_t)y * plate_stride + (int64_t)x * CN + c] = (uint8_t)p[c];
  if (count) count[(int64_t)y * count_stride + x] = (uint8_t)n;
  if (mask) {
    const int gp = CN == 3 ? gray_of(p[0], p[1], p[2]) : p[0];
    const uint32_t none = 0xffffffffu;                  // frame 255: no frame has that number
    uint8_t* m = mask + (int64_t)y * mask_stride + x;
    int j = 0;
    uint32_t word = settled ? col[0] : none;
    for (int k = 0; k < nframes; k++, m += mask_img_stride) {
      int moving = 0;
      if ((int)(word >> 24) == k) {
        const int g = CN == 3 ? gray_of(word & 255u, (word >> 8) & 255u, (word >> 16) & 255u) : (int)(word & 255u);
        moving = abs(g - gp) > threshold ? 255 : 0;
        j++;
        word = j < n ? col[64 * j] : none;
      }
      *m = (uint8_t)moving;
    }
  }
}

// Match rows whose points sit on something that differs from the plate are dropped (include/evhip.h states the contract for
// evh_rows_moving_filter).  One workgroup of four waves per pair, walking the pair's rows in tiles of MOVING_TILE:
//   phase A  one (row, end point) per thread: the end point through its frame's matrix to the canvas pixel (cx, cy), kept in LDS
//            (cx == INT_MIN: the end point cannot be moving);
//   phase B  the lanes spread over (end point, window pixel), window pixels of an end point on adjacent lanes: the count byte
//            first (a pixel below min_cover costs no division), then warp_sample and the gray difference from the plate.  The
//            hits of a wave are one ballot; the first lane of every end point's run inside the wave adds the popcount of the
//            run to the end point's LDS counter (runs of one end point meet only across waves and tiles of 256 items);
//   phase C  one row per thread: its flags, and the survivors compacted in order -- ballot and popcount inside the wave, the
//            four wave totals through LDS, a running offset across the tiles.
// A pair left with fewer than min_keep rows is then copied whole by the same workgroup (the barrier that ends every tile
// orders the two writes of a slot).  The two frames' matrices and adjugates sit in LDS, formed once by warp_map.
#define MOVING_TILE 256
template <int CN, class SRC>
__global__ __launch_bounds__(MOVING_TILE) void k_rows_moving_filter(
    SRC src, int sw, int sh, const double* __restrict__ M, const uint8_t* __restrict__ plate, int64_t plate_stride,
    const uint8_t* __restrict__ count, int64_t count_stride, int dw, int dh, int ox, int oy, int min_cover, int threshold,
    int radius, int min_hits, double row_sx, double row_sy, const float* __restrict__ rows, int row_cap,
    const int32_t* __restrict__ counts, const int32_t* __restrict__ status1, int frame_step, int min_keep,
    float* __restrict__ out_rows, int32_t* __restrict__ out_counts, int32_t* __restrict__ moving_out, uint8_t* __restrict__ flags) {
  __shared__ double s_fwd[2][9], s_adj[2][9];          // [0]: the current frame (point a), [1]: the previous frame (point b)
  __shared__ int s_cx[2 * MOVING_TILE], s_cy[2 * MOVING_TILE], s_hits[2 * MOVING_TILE];
  __shared__ int s_wtot[MOVING_TILE / 64];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int given = counts[p];
  const int n = min(max(given, 0), row_cap);
  if (status1[p] != EVH_PAIR_OK || n == 0) {
    if (tid == 0) {
      out_counts[p] = given;
      if (moving_out) moving_out[p] = 0;
    }
    return;
  }
  const int fprev = p * frame_step;
  if (tid < 2) {
    const double* m = M + 9 * (int64_t)(fprev + 1 - tid);
    const WarpMap A = warp_map(m, 0);
#pragma unroll
    for (int k = 0; k < 9; k++) { s_fwd[tid][k] = m[k]; s_adj[tid][k] = A.a[k]; }
  }
  const uint4* const in4 = reinterpret_cast<const uint4*>(rows) + (int64_t)p * row_cap;
  uint4* const out4 = reinterpret_cast<uint4*>(out_rows) + (int64_t)p * row_cap;
  const unsigned W = 2u * (unsigned)radius + 1u, W2 = W * W;
  int kept = 0;                                        // the running offset: rows kept in the tiles before this one
  for (int base = 0; base < n; base += MOVING_TILE) {
    const int tn = min(n - base, MOVING_TILE);
    __syncthreads();                                   // the matrices are there; the tile before is done with LDS
    for (int e = tid; e < 2 * tn; e += MOVING_TILE) {
      const int s = e & 1;
      const float* q = rows + ((int64_t)p * row_cap + base + (e >> 1)) * 4 + 2 * s;
      const double px = (double)q[0] * row_sx, py = (double)q[1] * row_sy;
      const double tx = (s_fwd[s][0] * px + s_fwd[s][1] * py) + s_fwd[s][2];
      const double ty = (s_fwd[s][3] * px + s_fwd[s][4] * py) + s_fwd[s][5];
      const double tw = (s_fwd[s][6] * px + s_fwd[s][7] * py) + s_fwd[s][8];
      const double cx = __builtin_rint(tx / tw), cy = __builtin_rint(ty / tw);
      const bool on = __builtin_fabs(cx) <= 1073741824.0 && __builtin_fabs(cy) <= 1073741824.0;      // NaN fails
      s_cx[e] = on ? (int)cx : INT_MIN;
      s_cy[e] = on ? (int)cy : 0;
      s_hits[e] = 0;
    }
    __syncthreads();
    const unsigned items = 2u * (unsigned)tn * W2;      // <= 512 * 225
    for (unsigned first = 0; first < items; first += MOVING_TILE) {
      const unsigned idx = first + (unsigned)tid;
      const bool active = idx < items;
      const unsigned e = active ? idx / W2 : 0u, wp = active ? idx - e * W2 : 0u;
      bool hit = false;
      const int cx = s_cx[e];
      if (active && cx != INT_MIN) {
        const int s = (int)(e & 1u);
        const int wj = (int)(wp / W), wi = (int)wp - wj * (int)W;
        const int64_t PX = (int64_t)cx + (wi - radius), PY = (int64_t)s_cy[e] + (wj - radius);      // the plane point
        const int64_t X = PX - ox, Y = PY - oy;                                                    // the canvas pixel
        if (X >= 0 && X < dw && Y >= 0 && Y < dh && (int)count[Y * count_stride + X] >= min_cover) {
          WarpMap A;
#pragma unroll
          for (int k = 0; k < 9; k++) A.a[k] = s_adj[s][k];
          int v[3] = {0, 0, 0};
          if (warp_sample(src, fprev + 1 - s, A, (double)PX, (double)PY, sw, sh, v)) {
            const uint8_t* pl = plate + Y * plate_stride + X * CN;
            const int g = CN == 3 ? gray_of(v[0], v[1], v[2]) : v[0];
            const int gp = CN == 3 ? gray_of(pl[0], pl[1], pl[2]) : pl[0];
            hit = abs(g - gp) > threshold;
          }
        }
      }
      const unsigned long long m = __ballot(hit);
      if (active && (lane == 0 || wp == 0)) {           // the first lane of this end point's run inside the wave
        const unsigned run = min(64u - (unsigned)lane, W2 - wp);
        const unsigned long long span = (run >= 64u ? ~0ull : ((1ull << run) - 1ull)) << lane;
        const int c = __popcll(m & span);
        if (c) atomicAdd(&s_hits[e], c);
      }
    }
    __syncthreads();
    const bool mine = tid < tn;
    const int fa = mine && s_hits[2 * tid] >= min_hits, fb = mine && s_hits[2 * tid + 1] >= min_hits;
    const bool keep = mine && !(fa | fb);
    const unsigned long long km = __ballot(keep);
    if (lane == 0) s_wtot[wv] = __popcll(km);
    if (mine && flags) flags[(int64_t)p * row_cap + base + tid] = (uint8_t)(fa | fb << 1);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < MOVING_TILE / 64; k++) { const int t = s_wtot[k]; before += k < wv ? t : 0; total += t; }
    if (keep) out4[kept + before + __popcll(km & ((1ull << lane) - 1ull))] = in4[base + tid];
    kept += total;
  }
  __syncthreads();                                     // every slot written above is visible to whoever writes it again
  const bool starved = kept < min_keep;
  if (starved)
    for (int i = tid; i < n; i += MOVING_TILE) out4[i] = in4[i];
  if (tid == 0) {
    out_counts[p] = starved ? n : kept;
    if (moving_out) moving_out[p] = n - kept;
  }
}

// Heat-map pictures (processing_visualization.py:336-344 without part_line): k_fixed_plane's field taken to a colour index,
// looked up in a 256-entry BGR table and laid over the frame, in the arithmetic include/evhip.h states for evh_heatmap_render.
// grid.y = frame; a thread owns WARP_RUN adjacent pixels of a row and moves their 12 bytes as three words where the pointers and
// strides allow (vec bit 0: output, bit 1: frames), bytewise otherwise and in runs cut by the right edge.  The table is staged
// in LDS once per workgroup, one packed entry per thread.  GENERAL = false: the entry is staged already multiplied,
// a = min(255, rint(c * alpha)), and a pixel is min(255, p + a) -- what rint(c * alpha + p) gives when p = 0 (no frames) or
// alpha is exactly 0.8 (c * 0.8 is never within 0.1 of a half; the launcher tests for the constant).  GENERAL = true: the
// float64 blend per byte.  The 256 threads of a block all reach the barrier; those past the last run then leave.
__device__ __forceinline__ int heat_index(const double* __restrict__ H, double x, double y, double heatmap_constant, int saturate) {
  double tx, ty, tw;
  hdot(H, x, y, &tx, &ty, &tw);
  const double u = tx / tw, v = ty / tw;
  const double s = u * u + v * v;
  const double t = 255.0 * (__builtin_sqrt(s) / heatmap_constant);
  if (saturate && t >= 255.0) return 255;                  // +inf included; NaN fails every comparison and ends as 0
  return (t >= 0.0 && t < 2147483648.0) ? ((int)t & 255) : 0;
}
template <bool GENERAL>
__global__ __launch_bounds__(256) void k_heatmap_render(const double* __restrict__ Hs, int w, const uint8_t* __restrict__ frames,
                                                        int64_t row_stride, int64_t frame_stride,
                                                        const uint8_t* __restrict__ lut, double heatmap_constant, double alpha,
                                                        int saturate, uint8_t* __restrict__ out, int64_t out_stride,
                                                        int64_t out_img_stride, int runs_per_row, unsigned nruns, int vec) {
  __shared__ uint32_t table[256];
  {
    uint32_t e = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      uint32_t c = lut[3 * threadIdx.x + ch];
      if (!GENERAL) c = (uint32_t)fmin(255.0, __builtin_rint((double)c * alpha));
      e |= c << (8 * ch);
    }
    table[threadIdx.x] = e;
  }
  __syncthreads();
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nruns) return;
  const int f = blockIdx.y;
  const double* H = Hs + 9 * (int64_t)f;
  const int y = (int)(t / (unsigned)runs_per_row), x0 = ((int)t - y * runs_per_row) * WARP_RUN;
  const int n = min(WARP_RUN, w - x0);
  const bool full = n == WARP_RUN;
  int v[WARP_RUN][3];
#pragma unroll
  for (int p = 0; p < WARP_RUN; p++) v[p][0] = v[p][1] = v[p][2] = 0;
  if (frames) warp_run_load<3>(frames + (int64_t)f * frame_stride + (int64_t)y * row_stride + (int64_t)x0 * 3, n, full && (vec & 2), v);
#pragma unroll
  for (int p = 0; p < WARP_RUN; p++) {
    if (p >= n) break;
    const uint32_t e = table[heat_index(H, (double)(x0 + p), (double)y, heatmap_constant, saturate)];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const int c = (e >> (8 * ch)) & 255;
      if (GENERAL) v[p][ch] = (int)fmin(255.0, __builtin_rint((double)c * alpha + (double)v[p][ch]));
      else v[p][ch] = min(255, v[p][ch] + c);
    }
  }
  warp_run_store<3>(out + (int64_t)f * out_img_stride + (int64_t)y * out_stride + (int64_t)x0 * 3, n, full && (vec & 1), v);
}

// Matching pictures (processing_visualization.py:22-57 as video_processing.py:78-81 calls it), in the rule include/evhip.h states
// for evh_draw_matches: two launches, the frames first and the lines on top.
// k_draw_paste: picture p = frame p * frame_step | frame p * frame_step + 1.  grid.x covers the runs of a picture row, both
// halves; rows and pictures are walked by grid.y / grid.z.  A thread owns WARP_RUN adjacent pixels of one half and moves their 12
// bytes as three words where the pointers and strides allow (vec bit 1: frames, bit 0: the left half of the pictures, bit 2: the
// right half, which begins 3*w bytes into a row), bytewise otherwise and in runs cut by a half's right edge.
__global__ __launch_bounds__(256) void k_draw_paste(const uint8_t* __restrict__ frames, int npairs, int frame_step, int w, int h,
                                                    int64_t row_stride, int64_t frame_stride, uint8_t* __restrict__ out,
                                                    int64_t out_stride, int64_t out_img_stride, int runs_per_half, int vec) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= 2 * runs_per_half) return;
  const int half = u >= runs_per_half ? 1 : 0, x0 = (u - half * runs_per_half) * WARP_RUN;
  const int n = min(WARP_RUN, w - x0);
  const bool full = n == WARP_RUN, wide_in = full && (vec & 2), wide_out = full && (vec & (half ? 4 : 1));
  for (int p = blockIdx.z; p < npairs; p += gridDim.z) {
    const uint8_t* S = frames + ((int64_t)p * frame_step + half) * frame_stride + (int64_t)x0 * 3;
    uint8_t* D = out + (int64_t)p * out_img_stride + ((int64_t)half * w + x0) * 3;
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
      int v[WARP_RUN][3];
#pragma unroll
      for (int q = 0; q < WARP_RUN; q++) v[q][0] = v[q][1] = v[q][2] = 0;
      warp_run_load<3>(S + (int64_t)y * row_stride, n, wide_in, v);
      warp_run_store<3>(D + (int64_t)y * out_stride, n, wide_out, v);
    }
  }
}
// k_draw_lines: one wave per line, the waves of grid.x stride over the rows of a pair, grid.y over the pairs.  The lanes take
// the pixels k = lane, lane + 64, ... <= D of the walk through the closed form of the minor offset, (2*d*k + D - 1) div (2*D): in
// 32 bits while D < 2^15 (2*d*k + D - 1 < 2^31 then, as d <= D and k <= D), in 64 bits for the long lines that leave the picture
// (D <= 81 918).  Every line of a call stores the same three bytes, so lines that share pixels need no order.
__global__ __launch_bounds__(256) void k_draw_lines(const float* __restrict__ rows, int row_cap, const int32_t* __restrict__ counts,
                                                    const int32_t* __restrict__ status, int npairs, int points, int w, int h,
                                                    uint32_t color, uint8_t* __restrict__ out, int64_t out_stride,
                                                    int64_t out_img_stride) {
  const int lane = threadIdx.x & 63, wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = gridDim.x * (blockDim.x >> 6);
  const uint8_t c0 = (uint8_t)color, c1 = (uint8_t)(color >> 8), c2 = (uint8_t)(color >> 16);
  for (int p = blockIdx.y; p < npairs; p += gridDim.y) {
    if (status && status[p] != EVH_PAIR_OK) continue;
    const int n = min(max(counts[p], 0), row_cap);
    uint8_t* pic = out + (int64_t)p * out_img_stride;
    for (int r = wave; r < n; r += nwaves) {
      const float* q = rows + ((int64_t)p * row_cap + r) * 4;
      const float t0 = truncf(q[0]), t1 = truncf(q[1]), t2 = truncf(q[2]), t3 = truncf(q[3]);
      // NaN and +-inf fail a comparison too; inside the range the conversions are exact
      if (!(t0 >= -32768.f && t0 <= 32767.f && t1 >= -32768.f && t1 <= 32767.f && t2 >= -32768.f && t2 <= 32767.f &&
            t3 >= -32768.f && t3 <= 32767.f))
        continue;
      int x1, y1, x2, y2;
      if (points == EVH_DRAW_REFERENCE) { x1 = (int)t0; y1 = (int)t1; x2 = (int)t2 + w; y2 = (int)t3; }
      else { x1 = (int)t2; y1 = (int)t3; x2 = (int)t0 + w; y2 = (int)t1; }
      int dx = x2 - x1, dy = y2 - y1;
      if (dx < 0) { x1 = x2; y1 = y2; dx = -dx; dy = -dy; }       // leftToRight: the walk starts at the left end
      const int sy = dy < 0 ? -1 : 1, ady = dy < 0 ? -dy : dy;
      const bool steep = ady > dx;                                // the major axis is y
      const int D = steep ? ady : dx, d = steep ? dx : ady;
      for (int k = lane; k <= D; k += 64) {
        int m = 0;
        if (D > 0)
          m = D < 32768 ? (int)((2u * (unsigned)d * (unsigned)k + (unsigned)D - 1u) / (2u * (unsigned)D))
                        : (int)((2ull * (unsigned)d * (unsigned)k + (unsigned)D - 1ull) / (2ull * (unsigned)D));
        const int x = steep ? x1 + m : x1 + k, y = steep ? y1 + sy * k : y1 + sy * m;
        if ((unsigned)x < 2u * (unsigned)w && (unsigned)y < (unsigned)h) {
          uint8_t* o = pic + (int64_t)y * out_stride + 3 * (int64_t)x;
          o[0] = c0; o[1] = c1; o[2] = c2;
        }
      }
    }
  }
}

struct HostTab { std::vector<int> start, cnt, si; std::vector<float> al; };

void build_area_tab(int ssize, int dsize, double scale, HostTab& t) {
  for (int dx = 0; dx < dsize; dx++) {
    double fsx1 = dx * scale, fsx2 = fsx1 + scale;
    double cell = std::min(scale, ssize - fsx1);
    int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
    sx2 = std::min(sx2, ssize - 1);
    sx1 = std::min(sx1, sx2);
    t.start.push_back((int)t.si.size());
    if (sx1 - fsx1 > 1e-3) { t.si.push_back(sx1 - 1); t.al.push_back((float)((sx1 - fsx1) / cell)); }
    for (int sx = sx1; sx < sx2; sx++) { t.si.push_back(sx); t.al.push_back((float)(1.0 / cell)); }
    if (fsx2 - sx2 > 1e-3) { t.si.push_back(sx2); t.al.push_back((float)(std::min(std::min(fsx2 - sx2, 1.), cell) / cell)); }
    t.cnt.push_back((int)t.si.size() - t.start.back());
  }
}

// INTER_AREA tables of one (source, destination) geometry, kept on the device by the context: a stream resizes every
// chunk with the same geometry.  A change of geometry drains the stream once (the previous tables may still be in use)
// and uploads; calls at the cached geometry enqueue nothing and never synchronise.
int area_tables(evh_ctx* c, int sw, int sh, int dw, int dh, double scale_x, double scale_y, AreaTabDev& T) {
  const int geom[4] = {sw, sh, dw, dh};
  if (std::memcmp(c->area_geom, geom, sizeof geom) != 0 || !c->d_area_tab) {
    HostTab xt, yt;
    build_area_tab(sw, dw, scale_x, xt);
    build_area_tab(sh, dh, scale_y, yt);
    std::vector<int> blob;
    for (const HostTab* t : {&xt, &yt}) {
      blob.insert(blob.end(), t->start.begin(), t->start.end());
      blob.insert(blob.end(), t->cnt.begin(), t->cnt.end());
      blob.insert(blob.end(), t->si.begin(), t->si.end());
      for (float f : t->al) { int v; std::memcpy(&v, &f, 4); blob.push_back(v); }
    }
    EVH_HIP(c, hipStreamSynchronize(c->stream));
    std::memset(c->area_geom, 0, sizeof geom);              // no geometry until the upload below has succeeded
    if (int rc = grow(c, &c->d_area_tab, &c->area_tab_bytes, blob.size() * sizeof(int))) return rc;
    EVH_HIP(c, hipMemcpy(c->d_area_tab, blob.data(), blob.size() * sizeof(int), hipMemcpyHostToDevice));
    std::memcpy(c->area_geom, geom, sizeof geom); c->area_nx = (int)xt.si.size(); c->area_ny = (int)yt.si.size();
  }
  int* p = c->d_area_tab;
  const size_t nx = (size_t)c->area_nx, ny = (size_t)c->area_ny;
  T.xs = p; p += dw; T.xcnt = p; p += dw; T.xsi = p; p += nx; T.xal = reinterpret_cast<float*>(p); p += nx;
  T.ys = p; p += dh; T.ycnt = p; p += dh; T.ysi = p; p += ny; T.yal = reinterpret_cast<float*>(p);
  return EVH_SUCCESS;
}

// nimg frames of sw x sh resized to dw x dh rows at dst (the sizes differ): gray rows of level 0 (INGEST) or the source's
// channels packed.  Enlarging in either direction = k_resize_linear_area, integer ratios = k_ingest_area_int /
// k_resize_area_int, else k_area.
template <bool INGEST, class SRC>
int launch_area(evh_ctx* c, const SRC& src, int nimg, int sw, int sh, uint8_t* dst, int dw, int dh, int64_t dst_stride,
                int64_t dst_img_stride) {
  const double inv_x = (double)dw / sw, inv_y = (double)dh / sh;      // the operator's own arithmetic
  const double sx = 1. / inv_x, sy = 1. / inv_y;
  const dim3 grid((dw + 255) / 256, dh, nimg);
  const int isx = (int)std::lrint(sx), isy = (int)std::lrint(sy);
  const area_stride_t<INGEST> stride = (area_stride_t<INGEST>)dst_stride;
  if (sx < 1 || sy < 1) {                    // the operator's bilinear emulation of INTER_AREA
    hipLaunchKernelGGL((k_resize_linear_area<INGEST, SRC>), grid, dim3(256), 0, c->stream, src, sw, sh, dst, dw, dh, dst_stride,
                       dst_img_stride, sx, inv_x, sy, inv_y);
  } else if (std::fabs(sx - isx) < 2.220446049250313e-16 && std::fabs(sy - isy) < 2.220446049250313e-16) {
    if constexpr (INGEST) {
      hipLaunchKernelGGL(k_ingest_area_int<SRC>, grid, dim3(256), 0, c->stream, src, dst, dst_img_stride, dw, dh, stride, isx, isy);
    } else {                                 // PackedSrc: one thread per channel element
      hipLaunchKernelGGL(k_resize_area_int, dim3((dw * src.cn + 255) / 256, dh, nimg), dim3(256), 0, c->stream, src.p, src.cn,
                         src.stride, src.img_stride, dst, dw, dh, dst_stride, dst_img_stride, isx, isy);
    }
  } else {
    AreaTabDev T;
    if (int rc = area_tables(c, sw, sh, dw, dh, sx, sy, T)) return rc;
    hipLaunchKernelGGL((k_area<INGEST, SRC>), grid, dim3(256), 0, c->stream, src, dst, dst_img_stride, dw, dh, stride, T);
  }
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

// level 0 of every frame straight from the source frames
template <class SRC>
int launch_ingest(evh_ctx* c, const SRC& src, int nimg, int sw, int sh, int dw, int dh) {
  const EvhLevel& L = c->g.lv[0];
  return launch_area<true>(c, src, nimg, sw, sh, c->d_pyr + L.off, dw, dh, L.stride, c->g.pyr_frame_bytes);
}

}  // namespace

int evh_launch_resize_area(evh_ctx* c, const uint8_t* d_src, int nimg, int sw, int sh, int cn, int64_t src_stride,
                           int64_t src_img_stride, uint8_t* d_dst, int dw, int dh, int64_t dst_stride,
                           int64_t dst_img_stride) {
  if (dw == sw && dh == sh) {
    for (int i = 0; i < nimg; i++)
      EVH_HIP(c, hipMemcpy2DAsync(d_dst + i * dst_img_stride, dst_stride, d_src + i * src_img_stride, src_stride,
                                  (size_t)sw * cn, sh, hipMemcpyDeviceToDevice, c->stream));
    return EVH_SUCCESS;
  }
  return launch_area<false>(c, PackedSrc{d_src, cn, src_stride, src_img_stride}, nimg, sw, sh, d_dst, dw, dh, dst_stride,
                            dst_img_stride);
}

static Yuv420Src yuv420_src(const evh_yuv420& s) {
  return {s.d_y, s.d_cb, s.d_cr, s.y_stride, s.c_stride, s.y_frame_stride, s.c_frame_stride, s.c_pixel_stride};
}

// k_yuv420_rows over nimg frames: BGR rows (GRAY = false) or gray rows at dst
template <bool GRAY>
static int launch_yuv420_rows(evh_ctx* c, const evh_yuv420& s, int nimg, int w, int h, uint8_t* dst, int64_t dst_stride,
                              int64_t dst_img_stride) {
  // the wide form needs 16-byte luma loads and stores, 8-byte (planar) or 16-byte (interleaved pair) chroma loads; the
  // frame strides of a single frame are never used
  const uintptr_t yfs = nimg > 1 ? (uintptr_t)s.y_frame_stride : 0, cfs = nimg > 1 ? (uintptr_t)s.c_frame_stride : 0;
  const uintptr_t dfs = nimg > 1 ? (uintptr_t)dst_img_stride : 0;
  const uintptr_t a16 = (uintptr_t)s.d_y | (uintptr_t)s.y_stride | yfs | (uintptr_t)dst | (uintptr_t)dst_stride | dfs;
  const uintptr_t ac = (uintptr_t)s.c_stride | cfs;
  int vec = 0;
  if (!(a16 & 15)) {
    if (s.c_pixel_stride == 1 && !(((uintptr_t)s.d_cb | (uintptr_t)s.d_cr | ac) & 7)) vec = 1;
    else if (s.c_pixel_stride == 2 && s.d_cr == s.d_cb + 1 && !(((uintptr_t)s.d_cb | ac) & 15)) vec = 2;
    else if (s.c_pixel_stride == 2 && s.d_cb == s.d_cr + 1 && !(((uintptr_t)s.d_cr | ac) & 15)) vec = 3;
  }
  const int runs_per_row = (w + YUV_RUN - 1) / YUV_RUN, nruns = runs_per_row * ((h + 1) / 2);
  hipLaunchKernelGGL(k_yuv420_rows<GRAY>, dim3((nruns + 255) / 256, nimg), dim3(256), 0, c->stream, yuv420_src(s), w, h, dst,
                     dst_stride, dst_img_stride, runs_per_row, nruns, vec);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

int evh_launch_yuv420_to_bgr(evh_ctx* c, const evh_yuv420& src, int nimg, int w, int h, uint8_t* d_dst, int64_t dst_stride,
                             int64_t dst_img_stride) {
  return launch_yuv420_rows<false>(c, src, nimg, w, h, d_dst, dst_stride, dst_img_stride);
}

int evh_launch_ingest_level0(evh_ctx* c, const EvhFrames& src, int nimg, int sw, int sh, int dw, int dh) {
  c->level1_fused = false;
  if (!src.yuv) return launch_ingest(c, PackedSrc{src.packed, src.channels, src.row_stride, src.frame_stride}, nimg, sw, sh, dw, dh);
  if (sw == dw && sh == dh) {          // no resize: converted and weighted in one pass, level 1 by the ordinary pyramid kernel
    const EvhLevel& L = c->g.lv[0];
    return launch_yuv420_rows<true>(c, *src.yuv, nimg, dw, dh, c->d_pyr + L.off, L.stride, c->g.pyr_frame_bytes);
  }
  return launch_ingest(c, yuv420_src(*src.yuv), nimg, sw, sh, dw, dh);
}

// k_warp_fixed_plane over the canvas (the entry has checked dw * dh <= INT_MAX, so the runs fit an unsigned)
template <int CN, class SRC>
static int launch_warp(evh_ctx* c, const SRC& src, int nframes, int sw, int sh, const double* d_M, int inverse_map, int mode,
                       const uint8_t* bg, uint8_t* out, int dw, int dh, int64_t out_stride, int64_t out_img_stride, int ox,
                       int oy) {
  const int runs_per_row = (dw + WARP_RUN - 1) / WARP_RUN;
  const unsigned nruns = (unsigned)runs_per_row * (unsigned)dh;
  // the image stride is only used between the canvases of EACH / HISTORY
  const uintptr_t ois = (mode != EVH_WARP_MOSAIC && nframes > 1) ? (uintptr_t)out_img_stride : 0;
  const int vec = (((uintptr_t)out | (uintptr_t)bg | (uintptr_t)out_stride | ois) & 3) == 0;
  const dim3 grid((nruns + 255) / 256, mode == EVH_WARP_EACH ? nframes : 1);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->stream, src, nframes, sw, sh, d_M, inverse_map, bg, out, dw, out_stride,
                       out_img_stride, ox, oy, runs_per_row, nruns, vec);
  };
  if (mode == EVH_WARP_EACH) go(k_warp_fixed_plane<EVH_WARP_EACH, CN, SRC>);
  else if (mode == EVH_WARP_HISTORY) go(k_warp_fixed_plane<EVH_WARP_HISTORY, CN, SRC>);
  else go(k_warp_fixed_plane<EVH_WARP_MOSAIC, CN, SRC>);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

int evh_launch_warp_fixed_plane(evh_ctx* c, const EvhFrames& src, int nframes, int sw, int sh, const double* d_M,
                                int inverse_map, int mode, const uint8_t* d_bg, uint8_t* d_out, int dw, int dh,
                                int64_t out_stride, int64_t out_img_stride, int ox, int oy) {
  if (src.yuv)
    return launch_warp<3>(c, yuv420_src(*src.yuv), nframes, sw, sh, d_M, inverse_map, mode, d_bg, d_out, dw, dh, out_stride,
                          out_img_stride, ox, oy);
  const PackedSrc P{src.packed, src.channels, src.row_stride, src.frame_stride};
  if (src.channels == 3)
    return launch_warp<3>(c, P, nframes, sw, sh, d_M, inverse_map, mode, d_bg, d_out, dw, dh, out_stride, out_img_stride, ox, oy);
  return launch_warp<1>(c, P, nframes, sw, sh, d_M, inverse_map, mode, d_bg, d_out, dw, dh, out_stride, out_img_stride, ox, oy);
}

// d_stats zeroed, then k_pair_residual over npairs >= 1 pairs of w x h (the entry has checked w * h <= INT_MAX and
// npairs <= 65535); d_out may be NULL
int evh_launch_pair_residual(evh_ctx* c, const EvhFrames& src, int npairs, int frame_step, int w, int h, const double* d_M,
                             int threshold, uint64_t* d_stats, uint8_t* d_out, int kind, int64_t out_stride,
                             int64_t out_img_stride) {
  EVH_HIP(c, hipMemsetAsync(d_stats, 0, (size_t)npairs * EVH_RES_NSTATS * sizeof(uint64_t), c->stream));
  const int runs_per_row = (w + WARP_RUN - 1) / WARP_RUN;
  const unsigned nruns = (unsigned)runs_per_row * (unsigned)h;
  // the pictures' stride is only used between the pictures of a call; the frames' always (a pair takes two frames)
  const uintptr_t ois = npairs > 1 ? (uintptr_t)out_img_stride : 0;
  const int vec = (d_out && (((uintptr_t)d_out | (uintptr_t)out_stride | ois) & 3) == 0 ? 1 : 0) |
                  (!src.yuv && (((uintptr_t)src.packed | (uintptr_t)src.row_stride | (uintptr_t)src.frame_stride) & 3) == 0 ? 2 : 0);
  const dim3 grid((nruns + 255) / 256, npairs);
  auto go = [&](auto kernel, const auto& S) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->stream, S, frame_step, w, h, d_M, threshold,
                       reinterpret_cast<unsigned long long*>(d_stats), d_out, kind, out_stride, out_img_stride, runs_per_row, nruns, vec);
  };
  const PackedSrc P{src.packed, src.channels, src.row_stride, src.frame_stride};
  if (src.yuv) go(k_pair_residual<3, Yuv420Src>, yuv420_src(*src.yuv));
  else if (src.channels == 3) go(k_pair_residual<3, PackedSrc>, P);
  else go(k_pair_residual<1, PackedSrc>, P);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

// the tables of evh_trail_fixed_plane's colour step, in double on the host: S[i] = rint((255 << 12) / i),
// H[i] = rint((180 << 12) / (6 i)), halves to even; entry 0 of both is 0
static const int32_t* trail_tables() {
  static int32_t T[512];
  static const bool built = [] {
    T[0] = T[256] = 0;
    for (int i = 1; i < 256; i++) {
      T[i] = (int32_t)std::rint(1044480.0 / i);
      T[256 + i] = (int32_t)std::rint(737280.0 / (6.0 * i));
    }
    return true;
  }();
  (void)built;
  return T;
}

// k_trail_fixed_plane over the canvas (the entry has checked dw * dh <= INT_MAX); d_out may be NULL
int evh_launch_trail_fixed_plane(evh_ctx* c, const EvhFrames& src, int nframes, int sw, int sh, const double* d_M,
                                 int inverse_map, const int32_t* d_rect, uint8_t* d_canvas, int64_t canvas_stride,
                                 uint8_t* d_out, int64_t out_stride, int64_t out_img_stride, int dw, int dh, int ox, int oy) {
  if (!c->trail_tab_ready) {          // once per context, stream-ordered in front of the first launch that reads it
    EVH_HIP(c, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_trail_tab), trail_tables(), 512 * sizeof(int32_t), 0, hipMemcpyHostToDevice,
                                      c->stream));
    c->trail_tab_ready = true;
  }
  const int runs_per_row = (dw + WARP_RUN - 1) / WARP_RUN;
  const unsigned nruns = (unsigned)runs_per_row * (unsigned)dh;
  // the picture stride is only used between the pictures of a call
  const uintptr_t ois = nframes > 1 ? (uintptr_t)out_img_stride : 0;
  const int vec = (d_out && (((uintptr_t)d_out | (uintptr_t)out_stride | ois) & 3) == 0 ? 1 : 0) |
                  ((((uintptr_t)d_canvas | (uintptr_t)canvas_stride) & 3) == 0 ? 2 : 0);
  auto go = [&](auto kernel, const auto& S) {
    hipLaunchKernelGGL(kernel, dim3((nruns + 255) / 256), dim3(256), 0, c->stream, S, nframes, sw, sh, d_M, inverse_map, d_rect,
                       d_canvas, canvas_stride, d_out, out_stride, out_img_stride, dw, ox, oy, runs_per_row, nruns, vec);
  };
  if (src.yuv) go(k_trail_fixed_plane<Yuv420Src>, yuv420_src(*src.yuv));
  else go(k_trail_fixed_plane<PackedSrc>, PackedSrc{src.packed, 3, src.row_stride, src.frame_stride});
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

// k_plate_fixed_plane over the canvas (the entry has checked dw * dh <= INT_MAX and nframes <= EVH_PLATE_MAX_FRAMES, so the
// column of samples, 256 bytes per frame, stays below the 64 KiB a workgroup gets without asking); nframes may be 0, d_bg,
// d_count and d_mask may be NULL
int evh_launch_plate_fixed_plane(evh_ctx* c, const EvhFrames& src, int nframes, int sw, int sh, const double* d_M,
                                 int inverse_map, int min_cover, const uint8_t* d_bg, uint8_t* d_plate, int64_t plate_stride,
                                 uint8_t* d_count, int64_t count_stride, uint8_t* d_mask, int threshold, int64_t mask_stride,
                                 int64_t mask_img_stride, int dw, int dh, int ox, int oy) {
  const unsigned npix = (unsigned)dw * (unsigned)dh;
  const size_t lds = (size_t)nframes * 64 * sizeof(uint32_t);
  auto go = [&](auto kernel, const auto& S) {
    hipLaunchKernelGGL(kernel, dim3((npix + 63) / 64), dim3(64), lds, c->stream, S, nframes, sw, sh, d_M, inverse_map, min_cover,
                       d_bg, d_plate, plate_stride, d_count, count_stride, d_mask, threshold, mask_stride, mask_img_stride, dw,
                       ox, oy, npix);
  };
  const PackedSrc P{src.packed, src.channels, src.row_stride, src.frame_stride};
  if (src.yuv) go(k_plate_fixed_plane<3, Yuv420Src>, yuv420_src(*src.yuv));
  else if (src.channels == 3) go(k_plate_fixed_plane<3, PackedSrc>, P);
  else go(k_plate_fixed_plane<1, PackedSrc>, P);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

// k_rows_moving_filter, one workgroup per pair (the entry has checked 1 <= npairs <= 65535, that the frames reach the last pair and
// that every output lies apart from every input); d_moving and d_flags may be NULL
int evh_launch_rows_moving_filter(evh_ctx* c, const EvhFrames& src, int sw, int sh, const double* d_M, const uint8_t* d_plate,
                                  int64_t plate_stride, const uint8_t* d_count, int64_t count_stride, int dw, int dh, int ox, int oy,
                                  int min_cover, int threshold, int radius, int min_hits, double row_sx, double row_sy,
                                  const float* d_rows, int row_cap, const int32_t* d_counts, const int32_t* d_status1, int npairs,
                                  int frame_step, int min_keep, float* d_out_rows, int32_t* d_out_counts, int32_t* d_moving,
                                  uint8_t* d_flags) {
  auto go = [&](auto kernel, const auto& S) {
    hipLaunchKernelGGL(kernel, dim3(npairs), dim3(MOVING_TILE), 0, c->stream, S, sw, sh, d_M, d_plate, plate_stride, d_count,
                       count_stride, dw, dh, ox, oy, min_cover, threshold, radius, min_hits, row_sx, row_sy, d_rows, row_cap,
                       d_counts, d_status1, frame_step, min_keep, d_out_rows, d_out_counts, d_moving, d_flags);
  };
  const PackedSrc P{src.packed, src.channels, src.row_stride, src.frame_stride};
  if (src.yuv) go(k_rows_moving_filter<3, Yuv420Src>, yuv420_src(*src.yuv));
  else if (src.channels == 3) go(k_rows_moving_filter<3, PackedSrc>, P);
  else go(k_rows_moving_filter<1, PackedSrc>, P);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

// k_heatmap_render over n frames of w x h (the entry has checked w * h <= INT_MAX and n <= 65535)
int evh_launch_heatmap_render(evh_ctx* c, const double* d_H, int n, int w, int h, const uint8_t* d_frames, int64_t row_stride,
                              int64_t frame_stride, const uint8_t* d_lut, double heatmap_constant, double alpha, int saturate,
                              uint8_t* d_out, int64_t out_stride, int64_t out_img_stride) {
  const int runs_per_row = (w + WARP_RUN - 1) / WARP_RUN;
  const unsigned nruns = (unsigned)runs_per_row * (unsigned)h;
  // the frame strides are only used between the pictures of a call
  const uintptr_t ois = n > 1 ? (uintptr_t)out_img_stride : 0, fs = n > 1 ? (uintptr_t)frame_stride : 0;
  const int vec = ((((uintptr_t)d_out | (uintptr_t)out_stride | ois) & 3) == 0 ? 1 : 0) |
                  (d_frames && (((uintptr_t)d_frames | (uintptr_t)row_stride | fs) & 3) == 0 ? 2 : 0);
  const dim3 grid((nruns + 255) / 256, n);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->stream, d_H, w, d_frames, row_stride, frame_stride, d_lut, heatmap_constant,
                       alpha, saturate, d_out, out_stride, out_img_stride, runs_per_row, nruns, vec);
  };
  if (!d_frames || alpha == 0.8) go(k_heatmap_render<false>);      // the integer blend, behind the exact test for its constant
  else go(k_heatmap_render<true>);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

// k_draw_paste, then k_draw_lines on top, over npairs >= 1 pictures (the entry has checked the arguments: w <= 16383)
int evh_launch_draw_matches(evh_ctx* c, const uint8_t* d_frames, int npairs, int frame_step, int w, int h, int64_t row_stride,
                            int64_t frame_stride, const float* d_rows, int row_cap, const int32_t* d_counts,
                            const int32_t* d_status, int points, uint32_t color_bgr, uint8_t* d_out, int64_t out_stride,
                            int64_t out_img_stride) {
  const int runs_per_half = (w + WARP_RUN - 1) / WARP_RUN;
  // the pictures' stride is only used between the pictures of a call; the frames' always (a picture takes two frames)
  const uintptr_t ois = npairs > 1 ? (uintptr_t)out_img_stride : 0;
  const bool out_words = (((uintptr_t)d_out | (uintptr_t)out_stride | ois) & 3) == 0;
  const int vec = (out_words ? 1 : 0) | ((((uintptr_t)d_frames | (uintptr_t)row_stride | (uintptr_t)frame_stride) & 3) == 0 ? 2 : 0) |
                  (out_words && (w & 3) == 0 ? 4 : 0);
  const dim3 pgrid((2 * runs_per_half + 255) / 256, std::min(h, 65535), std::min(npairs, 65535));
  hipLaunchKernelGGL(k_draw_paste, pgrid, dim3(256), 0, c->stream, d_frames, npairs, frame_step, w, h, row_stride, frame_stride,
                     d_out, out_stride, out_img_stride, runs_per_half, vec);
  EVH_HIP(c, hipGetLastError());
  const dim3 lgrid(std::min(64, (row_cap + 3) / 4), std::min(npairs, 65535));
  hipLaunchKernelGGL(k_draw_lines, lgrid, dim3(256), 0, c->stream, d_rows, row_cap, d_counts, d_status, npairs, points, w, h,
                     color_bgr, d_out, out_stride, out_img_stride);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

int evh_launch_superposition_scan(evh_ctx* c, const double* d_H, int n, double* d_out) {
  hipLaunchKernelGGL(k_superposition_scan, dim3(1), dim3(64), 0, c->stream, d_H, n, d_out);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}
int evh_launch_transform_points(evh_ctx* c, const double* d_M, const int* d_idx, const double* d_pts, int n, double kx,
                                double ky, int decimals, double* d_out) {
  hipLaunchKernelGGL(k_transform_points, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_M, d_idx, d_pts, n, kx, ky,
                     decimals, d_out);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

int evh_launch_fixed_plane(evh_ctx* c, const double* d_H, int n, int w, int h, double* d_field, unsigned long long* d_max) {
  hipLaunchKernelGGL(k_seed_fixed_plane_max, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_max, n);
  EVH_HIP(c, hipGetLastError());
  const int blocks = (int)std::min(((int64_t)w * h + 255) / 256, (int64_t)1024);
  hipLaunchKernelGGL(k_fixed_plane, dim3(blocks, n), dim3(256), 0, c->stream, d_H, w, h, d_field, d_max);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}
