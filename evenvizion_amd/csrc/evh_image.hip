// evh_image.hip -- K0: area-average downscale, the MI355X counterpart of imutils.resize(frame, width=) ->
// cv2.resize(INTER_AREA) at evenvizion/processing/video_processing.py:62,73.  Shrinking (the reference's
// "resize_width to speed up" use) = area sums; enlarging = the operator's bilinear emulation (k_resize_linear_area);
// equal sizes are a plain copy.  Weights are float32 tables built on the host
// exactly as the operator builds them; each output value is accumulated in float32 in table order
// (inner sum over source columns, outer sum over source rows), then rounded half-to-even and saturated.
#include "evh_devmath.h"
#include "evh_internal.h"
#include "evh_pixels.h"
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
// level 0's row stride is an int; the caller's of the stand-alone resize is whatever the ABI hands in
template <bool INGEST> using area_stride_t = std::conditional_t<INGEST, int, int64_t>;

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
  if (!src.yuv) return launch_ingest(c, packed_src(src), nimg, sw, sh, dw, dh);
  if (sw == dw && sh == dh) {          // no resize: converted and weighted in one pass, level 1 by the ordinary pyramid kernel
    const EvhLevel& L = c->g.lv[0];
    return launch_yuv420_rows<true>(c, *src.yuv, nimg, dw, dh, c->d_pyr + L.off, L.stride, c->g.pyr_frame_bytes);
  }
  return launch_ingest(c, yuv420_src(*src.yuv), nimg, sw, sh, dw, dh);
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
