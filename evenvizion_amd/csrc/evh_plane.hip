// evh_plane.hip -- the products on the fixed plane and the pictures drawn from a batch's results: evh_warp_fixed_plane,
// evh_warp_ray_surface, evh_blend_fixed_plane, evh_blend_ray_surface, evh_pair_residual, evh_pair_exposure, evh_pair_refine,
// evh_canvas_refine, evh_trail_fixed_plane, evh_plate_fixed_plane, evh_rows_moving_filter (each also on decoded 4:2:0 planes), evh_heatmap_render and
// evh_draw_matches.  Kernels first, then the host side: what the entries share (the checks of evh_frame_checks.h, launch
// plumbing), then per product its arguments, check() -- every refusal comes before anything is enqueued -- and launch().
#include "evh_devmath.h"
#include "evh_frame_checks.h"
#include "evh_internal.h"
#include "evh_pixels.h"
#include <climits>
#include <cmath>
#include <type_traits>

namespace {

// Stabilised output (stabilization.py:129-172, 220-249): frames resampled through their superposed H onto a canvas of the
// fixed plane; canvas pixel (x, y) is the plane point (x + ox, y + oy).  The arithmetic is the one include/evhip.h states
// for evh_warp_fixed_plane, one IEEE float64 operation at a time (no fma: the tests restate it in numpy byte for byte).
// A thread owns WARP_RUN adjacent canvas pixels of a row: the frame's matrix is formed once for them, and their bytes
// leave as 32-bit words (`wide`: every pointer and stride involved is a multiple of 4; runs cut by the right edge go
// bytewise).  Bytes past a row's dw pixels are neither read nor written.
#define WARP_RUN 4
// a pixel's gray: cvtColor's weights on BGR, the byte itself on gray frames
template <int CN> __device__ __forceinline__ int gray_px(const int (&v)[3]) { return CN == 3 ? gray_of(v[0], v[1], v[2]) : v[0]; }
struct WarpMap { double a[9]; };
// run t of a picture `width` pixels wide: its row, its first pixel and how many of its WARP_RUN pixels lie inside the row
struct RunPos { int y, x0, n; };
__device__ __forceinline__ RunPos run_pos(unsigned t, int runs_per_row, int width) {
  const int y = (int)(t / (unsigned)runs_per_row), x0 = ((int)t - y * runs_per_row) * WARP_RUN;
  return {y, x0, min(WARP_RUN, width - x0)};
}
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
// or NaN matrix, the horizon) cover nothing.  The three rows stay written out here and in phase A of k_rows_moving_filter: a
// helper shared by the two reorders that kernel (profiles/plane_unit_fold.txt).  A covered position has 0 <= sx <= sw - 1,
// and sx + 1 is read only with fx != 0, i.e. sx <= sw - 2 (rows alike): no tap leaves the frame.
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
  const RunPos rp = run_pos(t, runs_per_row, dw);
  const int y = rp.y, x0 = rp.x0, n = rp.n;
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

// Fixed surfaces that do not end at a horizon (include/evhip.h states the contract for evh_warp_ray_surface): canvas pixel (x, y)
// is the viewing ray (a[x], b[y], c[x]) of two caller tables -- cylinder, sphere or plane is the caller's choice of tables, no
// trigonometry runs here -- and frame k's matrix takes the ray to homogeneous frame pixels as it is.  A ray and its antipode meet
// the same frame pixel: only tw > 0, the ray in front of the camera, is covered (NaN fails the comparison).
// The sampling is warp_sample itself, whole: a split of it into position and taps moved instructions in the existing kernels
// (profiles/surface_warp.txt).  It is handed the point (a, 1) and the map {A0, A1*b, A2*c; ...}: its (a0*X + a1*Y) + a2 is then
// (A0*a + (A1*b)*1) + A2*c, and a product with 1 is exact, so tx, ty, tw come out as the header states them, with A1*b formed
// once per frame for the run (RayMap) and A2*c once per pixel.
struct RayMap { double a[9], b[3]; };
__device__ __forceinline__ RayMap ray_map(const double* __restrict__ A, double b) {
  RayMap R = {{A[0], A[1], A[2], A[3], A[4], A[5], A[6], A[7], A[8]}, {0.0, 0.0, 0.0}};
  R.b[0] = R.a[1] * b; R.b[1] = R.a[4] * b; R.b[2] = R.a[7] * b;
  return R;
}
template <class SRC>
__device__ __forceinline__ bool ray_sample(const SRC& src, int img, const RayMap& R, double a, double c, int sw, int sh,
                                           int (&v)[3]) {
  const WarpMap M = {{R.a[0], R.b[0], R.a[2] * c, R.a[3], R.b[1], R.a[5] * c, R.a[6], R.b[2], R.a[8] * c}};
  const double tw = (M.a[6] * a + M.a[7]) + M.a[8];
  if (!(tw > 0.0)) return false;
  return warp_sample(src, img, M, a, 1.0, sw, sh, v);
}
// The modes, the run of WARP_RUN pixels per thread and the stores are k_warp_fixed_plane's.  col: f64[dw,2] = (a, c) per column,
// the run's four pairs are 64 contiguous bytes (a run cut by the right edge loads only its own columns); row: f64[dh].
// HISTORY and MOSAIC load them once for all frames, each thread its own; EACH, see below.
template <int MODE, int CN, class SRC>
__global__ __launch_bounds__(256) void k_warp_ray_surface(SRC src, int nframes, int sw, int sh, const double* __restrict__ A,
                                                          const double* __restrict__ col, const double* __restrict__ row,
                                                          const uint8_t* bg, uint8_t* out, int dw, int64_t out_stride,
                                                          int64_t out_img_stride, int runs_per_row, unsigned nruns, int vec) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = t < nruns;
  if (MODE != EVH_WARP_EACH && !live) return;
  const RunPos rp = MODE == EVH_WARP_EACH && !live ? RunPos{0, 0, 0} : run_pos(t, runs_per_row, dw);
  const int y = rp.y, x0 = rp.x0, n = rp.n;
  double ra[WARP_RUN], rc[WARP_RUN];
  if constexpr (MODE == EVH_WARP_EACH) {
    // One frame per thread: the table loads are not shared among frames, and 64 lanes that each read their own 64 bytes open
    // 64 pieces of memory per load instruction (profiles/surface_warp.txt).  So a wave loads its 256 pixels lane by lane --
    // lane i takes pixel p = i & 3 of the run of lane 16 j + i / 4, j = 0 .. 3: neighbouring lanes, neighbouring columns --
    // and hands them over through LDS.  Every thread of the workgroup comes here, the ones past the last run with n = 0.
    __shared__ double2 stage[256 * WARP_RUN];
    const int lane = threadIdx.x & 63, first = (threadIdx.x - lane) * WARP_RUN;
#pragma unroll
    for (int j = 0; j < WARP_RUN; j++) {
      const int s = 64 * j + lane, owner = s >> 2, p = s & 3;
      const int ox0 = __shfl(x0, owner, 64), on = __shfl(n, owner, 64);
      double2 ac = {0.0, 0.0};
      if (p < on) { ac.x = col[2 * ((int64_t)ox0 + p)]; ac.y = col[2 * ((int64_t)ox0 + p) + 1]; }
      stage[first + s] = ac;
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) { ra[p] = stage[threadIdx.x * WARP_RUN + p].x; rc[p] = stage[threadIdx.x * WARP_RUN + p].y; }
  } else {
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) {
      ra[p] = p < n ? col[2 * ((int64_t)x0 + p)] : 0.0;
      rc[p] = p < n ? col[2 * ((int64_t)x0 + p) + 1] : 0.0;
    }
  }
  const bool wide = vec != 0 && n == WARP_RUN;
  const int64_t at = (int64_t)y * out_stride + (int64_t)x0 * CN;
  const double b = row[y];
  int v[WARP_RUN][3];
#pragma unroll
  for (int p = 0; p < WARP_RUN; p++) v[p][0] = v[p][1] = v[p][2] = 0;
  if constexpr (MODE == EVH_WARP_HISTORY) {
    if (bg) warp_run_load<CN>(bg + at, n, wide, v);
    for (int k = 0; k < nframes; k++) {
      const RayMap R = ray_map(A + 9 * (int64_t)k, b);
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++) if (p < n) ray_sample(src, k, R, ra[p], rc[p], sw, sh, v[p]);
      warp_run_store<CN>(out + (int64_t)k * out_img_stride + at, n, wide, v);
    }
  } else {
    unsigned open = (1u << n) - 1;                      // pixels of the run no frame has covered yet
    const int first = MODE == EVH_WARP_EACH ? (int)blockIdx.y : nframes - 1, last = MODE == EVH_WARP_EACH ? first : 0;
    for (int k = first; k >= last && open; k--) {
      const RayMap R = ray_map(A + 9 * (int64_t)k, b);
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++)
        if (((open >> p) & 1) && ray_sample(src, k, R, ra[p], rc[p], sw, sh, v[p])) open &= ~(1u << p);
    }
    if (open && bg) {
      int q[WARP_RUN][3];
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++) q[p][0] = q[p][1] = q[p][2] = 0;
      warp_run_load<CN>(bg + at, n, wide, q);
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++) if ((open >> p) & 1) { v[p][0] = q[p][0]; v[p][1] = q[p][1]; v[p][2] = q[p][2]; }
    }
    warp_run_store<CN>(out + (MODE == EVH_WARP_EACH ? (int64_t)blockIdx.y * out_img_stride : 0) + at, n, wide, v);
  }
}

// The blended mosaic (include/evhip.h states the contract for evh_blend_fixed_plane and evh_blend_ray_surface): every covering
// frame enters a canvas pixel's state u64[CN + 1] -- FEATHER: the sums of w * s * g and of w; SEAM: s * g of the frame with the
// largest w, and that w -- where w = min(d, F) + 1 and d is the sample's distance to the nearest frame edge in 1/32 pixels.
// warp_sample does not hand out its position, and taking it apart moves instructions in the existing kernels
// (profiles/surface_warp.txt), so edge_distance forms the position once more from the same operands in the same order: the two
// are one computation to the compiler (profiles/blend.txt counts the divisions), and the integers are warp_sample's by
// construction.  Only called for a covered position: U and V lie inside the frame, every difference is >= 0.
__device__ __forceinline__ int edge_distance(const WarpMap& A, double X, double Y, int sw, int sh) {
  const double tx = (A.a[0] * X + A.a[1] * Y) + A.a[2];
  const double ty = (A.a[3] * X + A.a[4] * Y) + A.a[5];
  const double tw = (A.a[6] * X + A.a[7] * Y) + A.a[8];
  const int u = (int)__builtin_rint(tx / tw * 32.0), v = (int)__builtin_rint(ty / tw * 32.0);
  return min(min(u, 32 * (sw - 1) - u), min(v, 32 * (sh - 1) - v));
}
// min(255, num / den) for den > 0, num < 2^63, den < 2^56 (the header's bounds leave room): is the quotient above 255, else its
// eight bits from the top, a compare and a subtraction each.  The general 64-bit division, which also works out 56 bits nobody
// needs, is 67 instructions longer per channel (profiles/blend.txt); the result is the same.
__device__ __forceinline__ int quotient_u8(unsigned long long num, unsigned long long den) {
  if ((num >> 8) >= den) return 255;                    // num >= den << 8, without the shift that could leave 64 bits
  int q = 0;
#pragma unroll
  for (int b = 7; b >= 0; b--)
    if (num >= den << b) { num -= den << b; q |= 1 << b; }
  return q;
}
// where the canvas pixels of a blend are: the plane entry's matrices and origin, or the ray entry's tables (col != NULL)
struct BlendGeo { const double* M; int inverse_map, ox, oy; const double* col; const double* row; };
// One canvas pixel per thread, its state in registers over all frames, as in k_plate_fixed_plane and unlike the warp kernels: those
// stop at the first covering frame, this one samples every frame, and a thread that owns a run of WARP_RUN pixels goes through
// 4 x nframes dependent position-and-tap chains at twice the registers -- 204 us against 124 us for 16 frames of 1280x720
// (profiles/blend.txt).  vec bit 1: the state moves as 128-bit words (d_acc 16-byte aligned: a pixel's state starts at a multiple
// of 16 bytes from it, CN + 1 being even).  The picture's bytes go one by one, adjacent lanes to adjacent pixels.  bg may BE out: a
// pixel no frame has entered (den == 0) reads its bytes before the store; acc is apart from everything.
template <int MODE, int CN, class SRC, bool RAY>
__global__ __launch_bounds__(256) void k_blend(SRC src, int nframes, int sw, int sh, BlendGeo G, int feather,
                                               const uint16_t* __restrict__ gain, unsigned long long* __restrict__ acc,
                                               int acc_in, const uint8_t* bg, uint8_t* out, int dw, int64_t out_stride,
                                               unsigned npix, int vec) {
  constexpr int NS = CN + 1;
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npix) return;
  const int y = (int)(t / (unsigned)dw), x = (int)t - y * dw;
  // the plane: (X, Y); the rays: (a, 1) with c beside them
  double X, Y = 1.0, rc = 0.0, b = 0.0;
  if constexpr (RAY) {
    X = G.col[2 * (int64_t)x]; rc = G.col[2 * (int64_t)x + 1]; b = G.row[y];
  } else {
    X = (double)((int64_t)x + G.ox); Y = (double)((int64_t)y + G.oy);
  }
  unsigned long long st[NS];
  unsigned long long* const sp = acc ? acc + (int64_t)t * NS : nullptr;
#pragma unroll
  for (int c = 0; c < NS; c++) st[c] = 0;
  if (sp && acc_in) {
    if (vec & 2) {
#pragma unroll
      for (int k = 0; k < NS / 2; k++) {
        const ulonglong2 q = reinterpret_cast<const ulonglong2*>(sp)[k];
        st[2 * k] = q.x; st[2 * k + 1] = q.y;
      }
    } else {
#pragma unroll
      for (int c = 0; c < NS; c++) st[c] = sp[c];
    }
  }
  for (int k = 0; k < nframes; k++) {
    uint32_t g[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) g[c] = gain ? gain[3 * (int64_t)k + c] : 4096u;
    int s[3] = {0, 0, 0};
    WarpMap A;
    if constexpr (RAY) {
      const RayMap R = ray_map(G.M + 9 * (int64_t)k, b);
      if (!ray_sample(src, k, R, X, rc, sw, sh, s)) continue;
      A = {{R.a[0], R.b[0], R.a[2] * rc, R.a[3], R.b[1], R.a[5] * rc, R.a[6], R.b[2], R.a[8] * rc}};         // ray_sample's
    } else {
      A = warp_map(G.M + 9 * (int64_t)k, G.inverse_map);
      if (!warp_sample(src, k, A, X, Y, sw, sh, s)) continue;
    }
    const uint32_t w = (uint32_t)min(edge_distance(A, X, Y, sw, sh), feather) + 1u;
    if constexpr (MODE == EVH_BLEND_FEATHER) {
#pragma unroll
      for (int c = 0; c < CN; c++) st[c] += (unsigned long long)w * ((uint32_t)s[c] * g[c]);
      st[CN] += w;
    } else if (w > st[CN]) {
#pragma unroll
      for (int c = 0; c < CN; c++) st[c] = (uint32_t)s[c] * g[c];
      st[CN] = w;
    }
  }
  if (sp) {
    if (vec & 2) {
#pragma unroll
      for (int k = 0; k < NS / 2; k++) {
        ulonglong2 q;
        q.x = st[2 * k]; q.y = st[2 * k + 1];
        reinterpret_cast<ulonglong2*>(sp)[k] = q;
      }
    } else {
#pragma unroll
      for (int c = 0; c < NS; c++) sp[c] = st[c];
    }
  }
  if (!out) return;
  const int64_t at = (int64_t)y * out_stride + (int64_t)x * CN;
  const unsigned long long den = st[CN];
#pragma unroll
  for (int c = 0; c < CN; c++) {
    int v;
    if (den == 0) v = bg ? bg[at + c] : 0;
    else if constexpr (MODE == EVH_BLEND_FEATHER) v = quotient_u8(st[c] + (den << 11), den << 12);
    else v = (int)min((st[c] + 2048) >> 12, 255ull);
    out[at + c] = (uint8_t)v;
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
    const RunPos rp = run_pos(t, runs_per_row, w);
    const int y = rp.y, x0 = rp.x0, n = rp.n;
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
        const int g_cur = gray_px<CN>(a[p]);
        const int g_prev = gray_px<CN>(b[p]);
        const int g_reg = gray_px<CN>(r);
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

// The sums behind exposure gains (include/evhip.h states the contract for evh_pair_exposure): grid.y = pair, the pair's two frame
// numbers come from device memory and are checked here -- a pair that names a frame outside 0 .. nframes-1 leaves as a whole
// workgroup, before the barrier, and keeps the zeros of the memset.  The pixels considered are those of the grid x % step == 0,
// y % step == 0 of frame i, `gw` per row; a thread owns WARP_RUN adjacent ones.  Bounds as in k_pair_residual: a workgroup holds at
// most 256 * 4 * 255 < 2^32 per sum, a pair at most INT_MAX * 255 < 2^39.
template <int CN, class SRC>
__global__ __launch_bounds__(256) void k_pair_exposure(SRC src, int nframes, int w, int h, const int32_t* __restrict__ pairs,
                                                       const double* __restrict__ M, int step, int lo, int hi,
                                                       unsigned long long* __restrict__ stats, int gw, int runs_per_row,
                                                       unsigned nruns) {
  __shared__ uint32_t part[4][EVH_EXPO_NSTATS];
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const int pair = blockIdx.y;
  const int fi = pairs[2 * (int64_t)pair], fj = pairs[2 * (int64_t)pair + 1];
  if ((unsigned)fi >= (unsigned)nframes || (unsigned)fj >= (unsigned)nframes) return;
  uint32_t s[EVH_EXPO_NSTATS];
#pragma unroll
  for (int k = 0; k < EVH_EXPO_NSTATS; k++) s[k] = 0;
  if (t < nruns) {
    const RunPos rp = run_pos(t, runs_per_row, gw);
    const int y = rp.y * step;
    const typename SRC::Row ra = src.row(fi, y);
    const WarpMap A = warp_map(M + 9 * (int64_t)pair, 1);
    const double Y = (double)y;
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) {
      const int x = (rp.x0 + p) * step;
      int a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
      if (p >= rp.n || !warp_sample(src, fj, A, (double)x, Y, w, h, b)) continue;
      ra.px(x, a);
      bool in = true;
#pragma unroll
      for (int c = 0; c < CN; c++) in = in && a[c] >= lo && a[c] <= hi && b[c] >= lo && b[c] <= hi;
      if (!in) continue;
      s[0] += 1;
#pragma unroll
      for (int c = 0; c < CN; c++) { s[1 + c] += (uint32_t)a[c]; s[4 + c] += (uint32_t)b[c]; }
    }
  }
#pragma unroll
  for (int k = 0; k < EVH_EXPO_NSTATS; k++)
    for (int m = 32; m > 0; m >>= 1) s[k] += __shfl_xor(s[k], m);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < EVH_EXPO_NSTATS; k++) part[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < EVH_EXPO_NSTATS) {
    const uint32_t sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (sum) atomicAdd(&stats[(int64_t)pair * EVH_EXPO_NSTATS + threadIdx.x], (unsigned long long)sum);
  }
}

// Direct alignment of a pair (include/evhip.h states the contract for evh_pair_refine): k_pair_refine_eval evaluates one matrix
// per pair -- the cost and the 45 normal sums -- and k_pair_refine_step, launched behind it, adds the workgroups' partial sums,
// judges the trial and forms the next one.  Per pair the state below lives in the context's workspace, followed by the partial
// sums: REFINE_SLOTS doubles per workgroup, [0..44] the normal sums, [45] and [46] covered and ssd as 64-bit integers.
// The evaluation: grid.y = pair, grid.x = REFINE_GROUPS(w, h) workgroups whose threads stride over the runs of WARP_RUN pixels,
// run t of thread (g, i) being i + 256 * g, then + 256 * groups: the assignment depends on w and h only.  A thread keeps the 45
// sums in registers over all of its runs (pixels in ascending order), the wave adds them by __shfl_xor (every lane forms the same
// commutative tree), the four waves go through LDS and are added in wave order.  Nothing is accumulated by atomics.
#define REFINE_SLOTS 48
struct RefineState {
  double M[9], Mtry[9], N[EVH_REFINE_NSUMS], lambda;
  unsigned long long cov, ssd, cov_in, ssd_in, n_in;
  int done, stop, evals, accepted;
};
// (the row by value: taken by reference, the packed instances of every other kernel of the unit compile differently)
template <int CN, class ROW> __device__ __forceinline__ int gray_at(const ROW r, int x) {
  int v[3] = {0, 0, 0};
  r.px(x, v);
  return gray_px<CN>(v);
}
template <int CN, class SRC>
__global__ __launch_bounds__(256) void k_pair_refine_eval(SRC src, int frame_step, int w, int h, const double* __restrict__ M_in,
                                                          const RefineState* __restrict__ state, double* __restrict__ part,
                                                          int clip, int runs_per_row, unsigned nruns) {
  __shared__ double wsum[4][REFINE_SLOTS];
  const int pair = blockIdx.y;
  if (!M_in && state[pair].done) return;                  // the whole workgroup: nobody waits at the barrier below
  const double* M = M_in ? M_in + 9 * (int64_t)pair : state[pair].Mtry;
  const WarpMap A = warp_map(M, 1);
  const int prev = pair * frame_step, cur = prev + 1;
  double acc[EVH_REFINE_NSUMS];
#pragma unroll
  for (int k = 0; k < EVH_REFINE_NSUMS; k++) acc[k] = 0.0;
  unsigned long long cov = 0, ssd = 0;
  for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < nruns; t += gridDim.x * 256u) {
    const RunPos rp = run_pos(t, runs_per_row, w);
    const int y = rp.y, x0 = rp.x0, n = rp.n;
    const typename SRC::Row rc = src.row(cur, y);
    const bool yin = y >= 1 && y <= h - 2;
    const double Y = (double)y, Yc = (double)(2 * y - (h - 1));
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) {
      int s[3] = {0, 0, 0};
      const int x = x0 + p;
      if (p >= n || !warp_sample(src, prev, A, (double)x, Y, w, h, s)) continue;
      const int r = gray_at<CN>(rc, x) - gray_px<CN>(s);
      cov += 1; ssd += (unsigned)(r * r);
      if (!yin || x < 1 || x > w - 2 || abs(r) > clip) continue;
      const int gxi = gray_at<CN>(rc, x + 1) - gray_at<CN>(rc, x - 1);
      const int gyi = gray_at<CN>(src.row(cur, y + 1), x) - gray_at<CN>(src.row(cur, y - 1), x);
      const double gx = (double)gxi, gy = (double)gyi, Xc = (double)(2 * x - (w - 1)), rd = (double)r;
      const double sxy = gx * Xc + gy * Yc;                 // integers below 2^53: every operation here is exact
      const double J[8] = {gx * Xc, gx * Yc, gx, gy * Xc, gy * Yc, gy, -Xc * sxy, -Yc * sxy};
      int k = 0;
#pragma unroll
      for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = i; j < 8; j++) acc[k++] += J[i] * J[j];
#pragma unroll
      for (int i = 0; i < 8; i++) acc[36 + i] += J[i] * rd;
      acc[44] += 1.0;
    }
  }
#pragma unroll
  for (int k = 0; k < EVH_REFINE_NSUMS; k++)
    for (int m = 32; m > 0; m >>= 1) acc[k] += __shfl_xor(acc[k], m);
  for (int m = 32; m > 0; m >>= 1) { cov += __shfl_xor(cov, m); ssd += __shfl_xor(ssd, m); }
  if ((threadIdx.x & 63) == 0) {
    double* o = wsum[threadIdx.x >> 6];
#pragma unroll
    for (int k = 0; k < EVH_REFINE_NSUMS; k++) o[k] = acc[k];
    o[45] = __longlong_as_double((long long)cov); o[46] = __longlong_as_double((long long)ssd);
  }
  __syncthreads();
  if (threadIdx.x < REFINE_SLOTS - 1) {
    const int k = threadIdx.x;
    double* o = part + ((int64_t)pair * gridDim.x + blockIdx.x) * REFINE_SLOTS + k;
    if (k < EVH_REFINE_NSUMS) {
      *o = ((wsum[0][k] + wsum[1][k]) + wsum[2][k]) + wsum[3][k];
    } else {
      unsigned long long u = 0;
      for (int v = 0; v < 4; v++) u += (unsigned long long)__double_as_longlong(wsum[v][k]);
      *o = __longlong_as_double((long long)u);
    }
  }
}
// Frame against canvas (include/evhip.h states the contract for evh_canvas_refine): k_pair_refine_eval with the previous frame
// replaced by a canvas of dw x dh that has holes.  canvas_sample is warp_sample on the canvas -- the same position, coverage test,
// taps and rounding, written out again because taking warp_sample apart moves instructions in the existing kernels
// (profiles/surface_warp.txt) -- with the count read beside each tap: a tap of non-zero weight whose count lies below min_cover makes
// the sample invalid, a tap of weight 0 is neither read nor asked.  count == NULL: every pixel is valid.  No tap leaves the canvas
// (see warp_sample), so no count read does.
__device__ __forceinline__ bool canvas_sample(const PackedSrc& canvas, const uint8_t* __restrict__ count, int64_t count_stride,
                                              int min_cover, const WarpMap& A, double X, double Y, int dw, int dh, int (&v)[3]) {
  const double tx = (A.a[0] * X + A.a[1] * Y) + A.a[2];
  const double ty = (A.a[3] * X + A.a[4] * Y) + A.a[5];
  const double tw = (A.a[6] * X + A.a[7] * Y) + A.a[8];
  const double U = __builtin_rint(tx / tw * 32.0), V = __builtin_rint(ty / tw * 32.0);
  if (!(U >= 0.0 && U <= (double)(32 * (dw - 1)) && V >= 0.0 && V <= (double)(32 * (dh - 1)))) return false;
  const int u = (int)U, w = (int)V;
  const int sx = u >> 5, fx = u & 31, sy = w >> 5, fy = w & 31;
  const int cn = canvas.channels();
  int p00[3] = {0, 0, 0}, p01[3] = {0, 0, 0}, p10[3] = {0, 0, 0}, p11[3] = {0, 0, 0};
  int lowest = 255;                                       // the smallest count under a tap of non-zero weight
  const uint8_t* c0 = count ? count + (int64_t)sy * count_stride + sx : nullptr;
  const PackedSrc::Row r0 = canvas.row(0, sy);
  r0.px(sx, p00);
  if (count) lowest = c0[0];
  if (fx) {
    r0.px(sx + 1, p01);
    if (count) lowest = min(lowest, (int)c0[1]);
  }
  if (fy) {
    const PackedSrc::Row r1 = canvas.row(0, sy + 1);
    r1.px(sx, p10);
    if (count) lowest = min(lowest, (int)c0[count_stride]);
    if (fx) {
      r1.px(sx + 1, p11);
      if (count) lowest = min(lowest, (int)c0[count_stride + 1]);
    }
  }
  if (count && lowest < min_cover) return false;
  const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
#pragma unroll
  for (int c = 0; c < 3; c++) if (c < cn) v[c] = (p00[c] * w00 + p01[c] * w01 + p10[c] * w10 + p11[c] * w11 + 512) >> 10;
  return true;
}
// grid.y = frame; the runs, the accumulation, the tree and the partial sums are k_pair_refine_eval's for the same w, h (the frame is
// the current frame there, the canvas the previous one), so k_pair_refine_step adds and judges them as they are.  The body is written
// out a second time: folded onto one body templated on the sampler, k_pair_refine_eval's instances compile differently
// (profiles/canvas_refine.txt).
template <int CN, class SRC>
__global__ __launch_bounds__(256) void k_canvas_refine_eval(SRC src, PackedSrc canvas, const uint8_t* __restrict__ count,
                                                            int64_t count_stride, int min_cover, int w, int h, int dw, int dh,
                                                            const double* __restrict__ M_in, const RefineState* __restrict__ state,
                                                            double* __restrict__ part, int clip, int runs_per_row, unsigned nruns) {
  __shared__ double wsum[4][REFINE_SLOTS];
  const int cur = blockIdx.y;
  if (!M_in && state[cur].done) return;                   // the whole workgroup: nobody waits at the barrier below
  const double* M = M_in ? M_in + 9 * (int64_t)cur : state[cur].Mtry;
  const WarpMap A = warp_map(M, 1);
  double acc[EVH_REFINE_NSUMS];
#pragma unroll
  for (int k = 0; k < EVH_REFINE_NSUMS; k++) acc[k] = 0.0;
  unsigned long long cov = 0, ssd = 0;
  for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < nruns; t += gridDim.x * 256u) {
    const RunPos rp = run_pos(t, runs_per_row, w);
    const int y = rp.y, x0 = rp.x0, n = rp.n;
    const typename SRC::Row rc = src.row(cur, y);
    const bool yin = y >= 1 && y <= h - 2;
    const double Y = (double)y, Yc = (double)(2 * y - (h - 1));
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) {
      int s[3] = {0, 0, 0};
      const int x = x0 + p;
      if (p >= n || !canvas_sample(canvas, count, count_stride, min_cover, A, (double)x, Y, dw, dh, s)) continue;
      const int r = gray_at<CN>(rc, x) - gray_px<CN>(s);
      cov += 1; ssd += (unsigned)(r * r);
      if (!yin || x < 1 || x > w - 2 || abs(r) > clip) continue;
      const int gxi = gray_at<CN>(rc, x + 1) - gray_at<CN>(rc, x - 1);
      const int gyi = gray_at<CN>(src.row(cur, y + 1), x) - gray_at<CN>(src.row(cur, y - 1), x);
      const double gx = (double)gxi, gy = (double)gyi, Xc = (double)(2 * x - (w - 1)), rd = (double)r;
      const double sxy = gx * Xc + gy * Yc;                 // integers below 2^53: every operation here is exact
      const double J[8] = {gx * Xc, gx * Yc, gx, gy * Xc, gy * Yc, gy, -Xc * sxy, -Yc * sxy};
      int k = 0;
#pragma unroll
      for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = i; j < 8; j++) acc[k++] += J[i] * J[j];
#pragma unroll
      for (int i = 0; i < 8; i++) acc[36 + i] += J[i] * rd;
      acc[44] += 1.0;
    }
  }
#pragma unroll
  for (int k = 0; k < EVH_REFINE_NSUMS; k++)
    for (int m = 32; m > 0; m >>= 1) acc[k] += __shfl_xor(acc[k], m);
  for (int m = 32; m > 0; m >>= 1) { cov += __shfl_xor(cov, m); ssd += __shfl_xor(ssd, m); }
  if ((threadIdx.x & 63) == 0) {
    double* o = wsum[threadIdx.x >> 6];
#pragma unroll
    for (int k = 0; k < EVH_REFINE_NSUMS; k++) o[k] = acc[k];
    o[45] = __longlong_as_double((long long)cov); o[46] = __longlong_as_double((long long)ssd);
  }
  __syncthreads();
  if (threadIdx.x < REFINE_SLOTS - 1) {
    const int k = threadIdx.x;
    double* o = part + ((int64_t)cur * gridDim.x + blockIdx.x) * REFINE_SLOTS + k;
    if (k < EVH_REFINE_NSUMS) {
      *o = ((wsum[0][k] + wsum[1][k]) + wsum[2][k]) + wsum[3][k];
    } else {
      unsigned long long u = 0;
      for (int v = 0; v < 4; v++) u += (unsigned long long)__double_as_longlong(wsum[v][k]);
      *o = __longlong_as_double((long long)u);
    }
  }
}
// A < B for the costs (ssd, covered): ssd_a * cov_b < ssd_b * cov_a in 128 bits
__device__ __forceinline__ bool refine_better(unsigned long long ssd_a, unsigned long long cov_a, unsigned long long ssd_b,
                                              unsigned long long cov_b) {
  const unsigned long long lh = __umul64hi(ssd_a, cov_b), ll = ssd_a * cov_b, rh = __umul64hi(ssd_b, cov_a), rl = ssd_b * cov_a;
  return lh < rh || (lh == rh && ll < rl);
}
__device__ __forceinline__ bool refine_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }      // NaN fails
// The step from the sums N and lambda, onto Mtry -> 0, or the reason the pair stops.  One thread; the 8x8 system sits in LDS
// (`a`, 64 doubles, and `y`, 8), where it may be indexed at run time.
__device__ int refine_step(const double* N, double lambda, const double* M, int w, int h, double* a, double* y, double* Mtry) {
  if (N[44] < (double)EVH_REFINE_MIN_PIXELS) return EVH_REFINE_TOO_FEW;
  double d[8];
  int k = 0;
  for (int i = 0; i < 8; i++)
    for (int j = i; j < 8; j++, k++) {
      a[8 * i + j] = a[8 * j + i] = N[k];
      if (i == j) d[i] = __builtin_sqrt(N[k]);
    }
  for (int i = 0; i < 8; i++) if (!(d[i] > 0.0)) return EVH_REFINE_DEGENERATE;
  for (int i = 0; i < 8; i++) {
    for (int j = 0; j < 8; j++) a[8 * i + j] = a[8 * i + j] / (d[i] * d[j]) + (i == j ? lambda : 0.0);
    y[i] = N[36 + i] / d[i];
  }
  // LDL': the lower triangle of a becomes L (unit diagonal) below D
  for (int j = 0; j < 8; j++) {
    double dj = a[8 * j + j];
    for (int q = 0; q < j; q++) dj -= a[8 * j + q] * a[8 * j + q] * a[8 * q + q];
    a[8 * j + j] = dj;
    for (int i = j + 1; i < 8; i++) {
      double v = a[8 * i + j];
      for (int q = 0; q < j; q++) v -= a[8 * i + q] * a[8 * j + q] * a[8 * q + q];
      a[8 * i + j] = v / dj;
    }
  }
  for (int i = 0; i < 8; i++) for (int q = 0; q < i; q++) y[i] -= a[8 * i + q] * y[q];
  for (int i = 0; i < 8; i++) y[i] /= a[8 * i + i];
  for (int i = 7; i >= 0; i--) for (int q = i + 1; q < 8; q++) y[i] -= a[8 * q + i] * y[q];
  double D[8];
  for (int i = 0; i < 8; i++) {
    D[i] = -4.0 * y[i] / d[i];
    if (!refine_finite(D[i])) return EVH_REFINE_DEGENERATE;
  }
  // Q = (C^-1 P) C, left to right
  const double cx = (double)(w - 1), cy = (double)(h - 1);
  const double P[9] = {1.0 + D[0], D[1], D[2], D[3], 1.0 + D[4], D[5], D[6], D[7], 1.0};
  double T[9], Q[9];
  for (int j = 0; j < 3; j++) {
    T[j] = 0.5 * P[j] + (cx / 2.0) * P[6 + j];
    T[3 + j] = 0.5 * P[3 + j] + (cy / 2.0) * P[6 + j];
    T[6 + j] = P[6 + j];
  }
  for (int i = 0; i < 3; i++) {
    Q[3 * i] = 2.0 * T[3 * i];
    Q[3 * i + 1] = 2.0 * T[3 * i + 1];
    Q[3 * i + 2] = (T[3 * i + 2] - T[3 * i] * cx) - T[3 * i + 1] * cy;
  }
  const WarpMap R = warp_map(Q, 0);
  double O[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) O[3 * i + j] = (M[3 * i] * R.a[j] + M[3 * i + 1] * R.a[3 + j]) + M[3 * i + 2] * R.a[6 + j];
  for (int i = 0; i < 9; i++) {
    Mtry[i] = O[i] / O[8];
    if (!refine_finite(Mtry[i])) return EVH_REFINE_DEGENERATE;
  }
  return 0;
}
// Launch k of the solving kernel (k = 0: behind the evaluation at M_in; last: behind the final one), one workgroup of 64 threads
// per pair: thread j adds slot j of the pair's `groups` partial sums in index order, thread 0 then judges and steps.
__global__ __launch_bounds__(64) void k_pair_refine_step(RefineState* __restrict__ state, const double* __restrict__ part, int groups,
                                                         int first, int last, int w, int h, const double* M_in, double* M_out,
                                                         unsigned long long* __restrict__ info, double* __restrict__ normal) {
  __shared__ double S[REFINE_SLOTS], a[64], y[8];
  const int pair = blockIdx.x, j = threadIdx.x;
  RefineState& st = state[pair];
  const bool active = first || !st.done;                  // the same for the whole workgroup
  if (active && j < REFINE_SLOTS - 1) {
    const double* p = part + (int64_t)pair * groups * REFINE_SLOTS + j;
    if (j < EVH_REFINE_NSUMS) {
      double v = 0.0;
      for (int g = 0; g < groups; g++) v += p[(int64_t)g * REFINE_SLOTS];
      S[j] = v;
    } else {
      unsigned long long u = 0;
      for (int g = 0; g < groups; g++) u += (unsigned long long)__double_as_longlong(p[(int64_t)g * REFINE_SLOTS]);
      S[j] = __longlong_as_double((long long)u);
    }
  }
  __syncthreads();
  if (j != 0) return;
  if (active) {
    const unsigned long long cov = (unsigned long long)__double_as_longlong(S[45]), ssd = (unsigned long long)__double_as_longlong(S[46]);
    bool take = false;
    if (first) {
      for (int i = 0; i < 9; i++) st.M[i] = M_in[9 * (int64_t)pair + i];
      st.lambda = 1e-3; st.done = 0; st.stop = 0; st.evals = 1; st.accepted = 0;
      st.cov_in = cov; st.ssd_in = ssd; st.n_in = (unsigned long long)S[44];
      if (normal) for (int i = 0; i < EVH_REFINE_NSUMS; i++) normal[(int64_t)pair * EVH_REFINE_NSUMS + i] = S[i];
      take = true;
      if (cov == 0) { st.done = 1; st.stop = EVH_REFINE_NOTHING_COVERED; }
    } else {
      st.evals += 1;
      take = cov > 0 && 10 * cov >= 9 * st.cov_in && refine_better(ssd, cov, st.ssd, st.cov);
      if (take) {
        for (int i = 0; i < 9; i++) st.M[i] = st.Mtry[i];
        st.lambda = fmax(st.lambda / 10.0, 1e-9);
        st.accepted += 1;
      } else {
        st.lambda = 10.0 * st.lambda;
      }
    }
    if (take) {
      st.cov = cov; st.ssd = ssd;
      for (int i = 0; i < EVH_REFINE_NSUMS; i++) st.N[i] = S[i];
    }
    if (!st.done && !last) {
      const int stop = refine_step(st.N, st.lambda, st.M, w, h, a, y, st.Mtry);
      if (stop) { st.done = 1; st.stop = stop; }
    }
  }
  if (last) {
    const unsigned long long* in = reinterpret_cast<const unsigned long long*>(M_in) + 9 * (int64_t)pair;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(M_out) + 9 * (int64_t)pair;
    for (int i = 0; i < 9; i++) out[i] = st.accepted ? (unsigned long long)__double_as_longlong(st.M[i]) : in[i];
    unsigned long long* o = info + (int64_t)pair * EVH_REFINE_NINFO;
    o[EVH_REFINE_STATUS] = st.accepted ? EVH_REFINE_REFINED : st.stop ? st.stop : EVH_REFINE_UNCHANGED;
    o[EVH_REFINE_EVALS] = st.evals; o[EVH_REFINE_ACCEPTED] = st.accepted;
    o[EVH_REFINE_COVERED_IN] = st.cov_in; o[EVH_REFINE_SSD_IN] = st.ssd_in;
    o[EVH_REFINE_COVERED_OUT] = st.cov; o[EVH_REFINE_SSD_OUT] = st.ssd; o[EVH_REFINE_N_IN] = st.n_in;
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
  const RunPos rp = run_pos(t, runs_per_row, dw);
  const int y = rp.y, x0 = rp.x0, n = rp.n;
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
    const int gp = gray_px<CN>(p);
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
            const int g = gray_px<CN>(v);
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
  const RunPos rp = run_pos(t, runs_per_row, w);
  const int y = rp.y, x0 = rp.x0, n = rp.n;
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

// ---- what the entries share: launch plumbing ---------------------------------------------------------------------------------------
// fn(integral_constant<int, CN>, src) with the source as the kernels take it: planes, packed BGR or packed gray
template <class Fn>
void with_source(const EvhFrames& F, Fn fn) {
  if (F.yuv) fn(std::integral_constant<int, 3>{}, yuv420_src(*F.yuv));
  else if (F.channels == 3) fn(std::integral_constant<int, 3>{}, packed_src(F));
  else fn(std::integral_constant<int, 1>{}, packed_src(F));
}
// may the rows at p move as 32-bit words?  The image stride only counts where it is used: between the images of a call.
bool words_ok(const void* p, int64_t row_stride, int64_t img_stride, int64_t nimages) {
  return (((uintptr_t)p | (uintptr_t)row_stride | (nimages > 1 ? (uintptr_t)img_stride : 0)) & 3) == 0;
}
// the runs of WARP_RUN pixels of a w x h picture (the entries have checked w * h <= INT_MAX, so they fit an unsigned)
struct Runs { int per_row; unsigned n; };
Runs runs_of(int w, int h) {
  const int per_row = (w + WARP_RUN - 1) / WARP_RUN;
  return {per_row, (unsigned)per_row * (unsigned)h};
}
// an entry: its refusals, then its launch unless there is nothing to do
template <class Args>
int run(evh_ctx* c, const Args& A) {
  if (!c) return EVH_ERR_INVALID;
  if (int rc = check(c, A)) return rc;
  return A.idle() ? EVH_SUCCESS : launch(c, A);
}

// ---- stabilised output: frames warped into the fixed plane (stabilization.py:129-172, 220-249) -------------------------------
struct WarpArgs {
  const char* who; EvhFrames F; int nframes, sw, sh; const double* M; int inverse_map, mode; const uint8_t* bg; uint8_t* out;
  int dw, dh; int64_t out_stride, out_img_stride; int ox, oy;
  bool many() const { return mode != EVH_WARP_MOSAIC && nframes > 1; }       // the canvases of out[0 .. nframes)
  bool idle() const { return nframes == 0; }
};
int check(evh_ctx* c, const WarpArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  const int cn = A.F.channels;
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.M || !A.out) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (int rc = need_channels(c, W, A.F)) return rc;
  if (A.nframes < 0 || A.sw < 1 || A.sh < 1 || A.dw < 1 || A.dh < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame or canvas");
  if (A.mode != EVH_WARP_EACH && A.mode != EVH_WARP_HISTORY && A.mode != EVH_WARP_MOSAIC) return evh_fail(c, EVH_ERR_INVALID, W + "unknown mode");
  if (int rc = need_below_2_26(c, W, "source", A.sw, A.sh)) return rc;
  if (int rc = need_area(c, W, "dw * dh", A.dw, A.dh)) return rc;
  if (A.nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  const int64_t canvas = (int64_t)(A.dh - 1) * A.out_stride + (int64_t)A.dw * cn;
  if (A.out_stride < (int64_t)A.dw * cn || (A.many() && A.out_img_stride < canvas))
    return evh_fail(c, EVH_ERR_INVALID, W + "output stride smaller than a row / canvas");
  if (int rc = need_source_stride(c, W, A.F, A.sw, A.sh, A.nframes > 1)) return rc;
  if (A.bg && !(A.mode == EVH_WARP_MOSAIC && A.bg == A.out)) {      // only a mosaic may be carried in place
    const int64_t out_bytes = canvas + (A.many() ? (A.nframes - 1) * A.out_img_stride : 0);
    if (meet({A.bg, canvas, ""}, {A.out, out_bytes, ""})) return evh_fail(c, EVH_ERR_INVALID, W + "d_background overlaps d_out");
  }
  if (A.nframes == 0) return EVH_SUCCESS;
  return need_planes(c, A.who, A.F, A.nframes, A.sw, A.sh);
}
// k_warp_fixed_plane over the canvas
int launch(evh_ctx* c, const WarpArgs& A) {
  const Runs R = runs_of(A.dw, A.dh);
  const int vec = words_ok(A.out, A.out_stride, A.out_img_stride, A.many() ? A.nframes : 1) && words_ok(A.bg, A.out_stride, 0, 1);
  const dim3 grid((R.n + 255) / 256, A.mode == EVH_WARP_EACH ? A.nframes : 1);
  with_source(A.F, [&](auto cn, const auto& S) {
    constexpr int CN = decltype(cn)::value;
    using SRC = std::decay_t<decltype(S)>;
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->stream, S, A.nframes, A.sw, A.sh, A.M, A.inverse_map, A.bg, A.out, A.dw,
                         A.out_stride, A.out_img_stride, A.ox, A.oy, R.per_row, R.n, vec);
    };
    if (A.mode == EVH_WARP_EACH) go(k_warp_fixed_plane<EVH_WARP_EACH, CN, SRC>);
    else if (A.mode == EVH_WARP_HISTORY) go(k_warp_fixed_plane<EVH_WARP_HISTORY, CN, SRC>);
    else go(k_warp_fixed_plane<EVH_WARP_MOSAIC, CN, SRC>);
  });
  return launched(c);
}

// ---- fixed surfaces: frames warped onto a canvas of viewing rays ------------------------------------------------------------------
// W: the plane entry's arguments with M = d_A, inverse_map, ox and oy unused; its refusals hold as they are
struct RayArgs {
  WarpArgs W; const double* col; const double* row;
  bool idle() const { return W.idle(); }
};
int check(evh_ctx* c, const RayArgs& A) {
  if (int rc = need_source(c, std::string(A.W.who) + ": ", A.W.F)) return rc;
  if (!A.col || !A.row) return evh_fail(c, EVH_ERR_INVALID, std::string(A.W.who) + ": NULL argument");
  return check(c, A.W);
}
// k_warp_ray_surface over the canvas
int launch(evh_ctx* c, const RayArgs& R) {
  const WarpArgs& A = R.W;
  const Runs N = runs_of(A.dw, A.dh);
  const int vec = words_ok(A.out, A.out_stride, A.out_img_stride, A.many() ? A.nframes : 1) && words_ok(A.bg, A.out_stride, 0, 1);
  const dim3 grid((N.n + 255) / 256, A.mode == EVH_WARP_EACH ? A.nframes : 1);
  with_source(A.F, [&](auto cn, const auto& S) {
    constexpr int CN = decltype(cn)::value;
    using SRC = std::decay_t<decltype(S)>;
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->stream, S, A.nframes, A.sw, A.sh, A.M, R.col, R.row, A.bg, A.out, A.dw,
                         A.out_stride, A.out_img_stride, N.per_row, N.n, vec);
    };
    if (A.mode == EVH_WARP_EACH) go(k_warp_ray_surface<EVH_WARP_EACH, CN, SRC>);
    else if (A.mode == EVH_WARP_HISTORY) go(k_warp_ray_surface<EVH_WARP_HISTORY, CN, SRC>);
    else go(k_warp_ray_surface<EVH_WARP_MOSAIC, CN, SRC>);
  });
  return launched(c);
}

// ---- the blended mosaic: feathered seams and exposure gains, on the plane or on a surface -------------------------------------------
// W: the warp entries' arguments with mode = the blend mode and out possibly NULL; col, row: the ray form's tables
struct BlendArgs {
  WarpArgs W; bool ray; const double* col; const double* row; int feather; const uint16_t* gain; uint64_t* acc; int acc_in;
  bool idle() const { return false; }       // no frames: the picture of the incoming state
};
// The refusals of a blend whose state is called `sname` (d_acc, or the band blend's d_state) and in_name (acc_in, state_in) and
// holds state_elems(dw, dh, channels) 64-bit words -- asked for only once the sizes have passed.
template <class Elems>
int check_blend(evh_ctx* c, const BlendArgs& B, const char* sname, const char* in_name, Elems state_elems) {
  const WarpArgs& A = B.W;
  const std::string W = std::string(A.who) + ": ";
  const int cn = A.F.channels;
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.M || (B.ray && (!B.col || !B.row))) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (!A.out && !B.acc) return evh_fail(c, EVH_ERR_INVALID, W + "d_out and " + sname + " are both NULL");
  if (B.acc_in && !B.acc) return evh_fail(c, EVH_ERR_INVALID, W + in_name + " without " + sname);
  if ((uintptr_t)B.acc & 7) return evh_fail(c, EVH_ERR_INVALID, W + sname + " must be 8-byte aligned");
  if (int rc = need_channels(c, W, A.F)) return rc;
  if (A.nframes < 0 || A.sw < 1 || A.sh < 1 || A.dw < 1 || A.dh < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame or canvas");
  if (A.mode != EVH_BLEND_FEATHER && A.mode != EVH_BLEND_SEAM) return evh_fail(c, EVH_ERR_INVALID, W + "unknown mode");
  if (B.feather < 0 || B.feather > 65535) return evh_fail(c, EVH_ERR_INVALID, W + "feather must lie in 0..65535");
  if (int rc = need_below_2_26(c, W, "source", A.sw, A.sh)) return rc;
  if (int rc = need_area(c, W, "dw * dh", A.dw, A.dh)) return rc;
  if (A.nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  const int64_t canvas = (int64_t)(A.dh - 1) * A.out_stride + (int64_t)A.dw * cn;
  if (A.out && A.out_stride < (int64_t)A.dw * cn) return evh_fail(c, EVH_ERR_INVALID, W + "output stride smaller than a row");
  if (int rc = need_source_stride(c, W, A.F, A.sw, A.sh, A.nframes > 1)) return rc;
  if (A.out && A.bg && A.bg != A.out && meet({A.bg, canvas, ""}, {A.out, canvas, ""}))
    return evh_fail(c, EVH_ERR_INVALID, W + "d_background overlaps d_out");
  if (A.nframes > 0)
    if (int rc = need_planes(c, A.who, A.F, A.nframes, A.sw, A.sh)) return rc;
  // the state apart from everything, the picture apart from the frames and the gains
  Span src[3];
  source_spans(A.F, A.nframes, A.sw, A.sh, src);
  const Span gain = {B.gain, (int64_t)A.nframes * 6, "d_gain"};
  const Span state[1] = {{B.acc, state_elems(A.dw, A.dh, cn) * 8, sname}};
  const Span others[9] = {{A.out, A.out ? canvas : 0, "d_out"}, {A.out ? A.bg : nullptr, canvas, "d_background"}, gain,
                          {A.M, (int64_t)A.nframes * 72, B.ray ? "d_A" : "d_M"}, {B.col, (int64_t)A.dw * 16, "d_col"},
                          {B.row, (int64_t)A.dh * 8, "d_row"}, src[0], src[1], src[2]};
  if (int rc = need_apart(c, W, state, others)) return rc;
  const Span picture[1] = {{A.out, A.out ? canvas : 0, "d_out"}};
  const Span inputs[4] = {gain, src[0], src[1], src[2]};
  return need_apart(c, W, picture, inputs);
}
int check(evh_ctx* c, const BlendArgs& B) {
  return check_blend(c, B, "d_acc", "acc_in", [](int dw, int dh, int cn) { return (int64_t)dw * dh * (cn + 1); });
}
// k_blend over the canvas; nframes may be 0, and one of out and acc NULL
int launch(evh_ctx* c, const BlendArgs& B) {
  const WarpArgs& A = B.W;
  const unsigned npix = (unsigned)A.dw * (unsigned)A.dh;
  const int vec = ((uintptr_t)B.acc & 15) == 0 ? 2 : 0;
  const BlendGeo G = {A.M, A.inverse_map, A.ox, A.oy, B.col, B.row};
  with_source(A.F, [&](auto cn, const auto& S) {
    constexpr int CN = decltype(cn)::value;
    using SRC = std::decay_t<decltype(S)>;
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((npix + 255) / 256), dim3(256), 0, c->stream, S, A.nframes, A.sw, A.sh, G, B.feather, B.gain,
                         reinterpret_cast<unsigned long long*>(B.acc), B.acc_in, A.out ? A.bg : nullptr, A.out, A.dw,
                         A.out_stride, npix, vec);
    };
    if (B.ray) {
      if (A.mode == EVH_BLEND_FEATHER) go(k_blend<EVH_BLEND_FEATHER, CN, SRC, true>);
      else go(k_blend<EVH_BLEND_SEAM, CN, SRC, true>);
    } else {
      if (A.mode == EVH_BLEND_FEATHER) go(k_blend<EVH_BLEND_FEATHER, CN, SRC, false>);
      else go(k_blend<EVH_BLEND_SEAM, CN, SRC, false>);
    }
  });
  return launched(c);
}

#include "evh_plane_bands.h"       // the multi-band blend and the seam labels: kernels, check() and launch()

// ---- the sums behind exposure gains: two frames of a batch compared where one maps onto the other ----------------------------------
struct ExposureArgs {
  const char* who; EvhFrames F; int nframes, w, h; const int32_t* pairs; int npairs; const double* M; int step, lo, hi;
  uint64_t* stats;
  bool idle() const { return npairs == 0; }
};
int check(evh_ctx* c, const ExposureArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.pairs || !A.M || !A.stats) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (int rc = need_channels(c, W, A.F)) return rc;
  if (A.nframes < 0 || A.npairs < 0 || A.w < 1 || A.h < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame or negative count");
  if (A.step < 1 || A.step > 64) return evh_fail(c, EVH_ERR_INVALID, W + "step must lie in 1..64");
  if (A.lo < 0 || A.hi > 255 || A.lo > A.hi) return evh_fail(c, EVH_ERR_INVALID, W + "lo and hi must satisfy 0 <= lo <= hi <= 255");
  if (int rc = need_below_2_26(c, W, "frame", A.w, A.h)) return rc;
  if (int rc = need_area(c, W, "w * h", A.w, A.h)) return rc;
  if (A.npairs > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 pairs per call");
  if (A.nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  if (int rc = need_source_stride(c, W, A.F, A.w, A.h, A.nframes > 1)) return rc;
  if (A.npairs == 0) return EVH_SUCCESS;
  if (A.nframes > 0)
    if (int rc = need_planes(c, A.who, A.F, A.nframes, A.w, A.h)) return rc;
  // the sums apart from everything that is read
  Span src[3];
  source_spans(A.F, A.nframes, A.w, A.h, src);
  const Span outs[1] = {{A.stats, (int64_t)A.npairs * EVH_EXPO_NSTATS * (int64_t)sizeof(uint64_t), "d_stats"}};
  const Span ins[5] = {{A.pairs, (int64_t)A.npairs * 8, "d_pairs"}, {A.M, (int64_t)A.npairs * 72, "d_M"}, src[0], src[1], src[2]};
  return need_apart(c, W, outs, ins);
}
// d_stats zeroed, then k_pair_exposure over the pairs
int launch(evh_ctx* c, const ExposureArgs& A) {
  EVH_HIP(c, hipMemsetAsync(A.stats, 0, (size_t)A.npairs * EVH_EXPO_NSTATS * sizeof(uint64_t), c->stream));
  const int gw = (A.w + A.step - 1) / A.step, gh = (A.h + A.step - 1) / A.step;
  const Runs R = runs_of(gw, gh);
  with_source(A.F, [&](auto cn, const auto& S) {
    hipLaunchKernelGGL((k_pair_exposure<decltype(cn)::value, std::decay_t<decltype(S)>>), dim3((R.n + 255) / 256, A.npairs),
                       dim3(256), 0, c->stream, S, A.nframes, A.w, A.h, A.pairs, A.M, A.step, A.lo, A.hi,
                       reinterpret_cast<unsigned long long*>(A.stats), gw, R.per_row, R.n);
  });
  return launched(c);
}

// ---- the score of a homography: the motion-compensated residual of a pair ------------------------------------------------------
struct ResidualArgs {
  const char* who; EvhFrames F; int npairs, frame_step, w, h; const double* M; int threshold; uint64_t* stats; uint8_t* out;
  int kind; int64_t out_stride, out_img_stride;
  bool idle() const { return npairs == 0; }
};
int check(evh_ctx* c, const ResidualArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.M || !A.stats) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (int rc = need_channels(c, W, A.F)) return rc;
  if (A.frame_step != 1 && A.frame_step != 2) return evh_fail(c, EVH_ERR_INVALID, W + "frame_step must be 1 or 2");
  if (A.npairs < 0 || A.w < 1 || A.h < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame or negative npairs");
  if (A.threshold < 0 || A.threshold > 255) return evh_fail(c, EVH_ERR_INVALID, W + "threshold must lie in 0..255");
  if (A.kind != EVH_RESIDUAL_ABS && A.kind != EVH_RESIDUAL_MASK) return evh_fail(c, EVH_ERR_INVALID, W + "unknown kind");
  if (int rc = need_below_2_26(c, W, "frame", A.w, A.h)) return rc;
  if (int rc = need_area(c, W, "w * h", A.w, A.h)) return rc;
  if (A.npairs > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 pairs per call");
  if (int rc = need_source_stride(c, W, A.F, A.w, A.h, true)) return rc;      // a pair takes two frames
  const int64_t picture = (A.h - 1) * A.out_stride + A.w;
  if (A.out && (A.out_stride < A.w || (A.npairs > 1 && A.out_img_stride < picture)))
    return evh_fail(c, EVH_ERR_INVALID, W + "output stride smaller than a row / picture");
  if (A.npairs == 0) return EVH_SUCCESS;
  const int64_t nframes = (int64_t)(A.npairs - 1) * A.frame_step + 2;
  if (A.F.yuv && nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  if (int rc = need_planes(c, A.who, A.F, nframes, A.w, A.h)) return rc;
  if (!A.out) return EVH_SUCCESS;
  // the pictures apart from the statistics and from the frames
  const Span outs[1] = {{A.out, picture + (A.npairs - 1) * A.out_img_stride, "d_out"}};
  Span src[3];
  source_spans(A.F, nframes, A.w, A.h, src);
  const Span ins[4] = {{A.stats, (int64_t)A.npairs * EVH_RES_NSTATS * (int64_t)sizeof(uint64_t), "d_stats"}, src[0], src[1], src[2]};
  return need_apart(c, W, outs, ins);
}
// d_stats zeroed, then k_pair_residual over the pairs; out may be NULL
int launch(evh_ctx* c, const ResidualArgs& A) {
  EVH_HIP(c, hipMemsetAsync(A.stats, 0, (size_t)A.npairs * EVH_RES_NSTATS * sizeof(uint64_t), c->stream));
  const Runs R = runs_of(A.w, A.h);
  const int vec = (A.out && words_ok(A.out, A.out_stride, A.out_img_stride, A.npairs) ? 1 : 0) |
                  (!A.F.yuv && words_ok(A.F.packed, A.F.row_stride, A.F.frame_stride, 2) ? 2 : 0);
  with_source(A.F, [&](auto cn, const auto& S) {
    hipLaunchKernelGGL((k_pair_residual<decltype(cn)::value, std::decay_t<decltype(S)>>), dim3((R.n + 255) / 256, A.npairs),
                       dim3(256), 0, c->stream, S, A.frame_step, A.w, A.h, A.M, A.threshold,
                       reinterpret_cast<unsigned long long*>(A.stats), A.out, A.kind, A.out_stride, A.out_img_stride, R.per_row,
                       R.n, vec);
  });
  return launched(c);
}

// ---- direct alignment: a pair's matrix refined on the pixels ------------------------------------------------------------------------
struct RefineArgs {
  const char* who; EvhFrames F; int npairs, frame_step, w, h; const double* M_in; int iters, clip; double* M_out; uint64_t* info;
  double* normal;
  bool idle() const { return npairs == 0; }
};
int check(evh_ctx* c, const RefineArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.M_in || !A.M_out || !A.info) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (int rc = need_channels(c, W, A.F)) return rc;
  if (A.frame_step != 1 && A.frame_step != 2) return evh_fail(c, EVH_ERR_INVALID, W + "frame_step must be 1 or 2");
  if (A.npairs < 0 || A.w < 1 || A.h < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame or negative npairs");
  if (A.iters < 0 || A.iters > EVH_REFINE_MAX_ITERS) return evh_fail(c, EVH_ERR_INVALID, W + "iters must lie in 0..64");
  if (A.clip < 0 || A.clip > 255) return evh_fail(c, EVH_ERR_INVALID, W + "clip must lie in 0..255");
  // the Jacobian's entries are exact in double up to here; this also keeps w, h below 2^26 and w * h below INT_MAX
  if (A.w > EVH_REFINE_MAX_SIZE || A.h > EVH_REFINE_MAX_SIZE) return evh_fail(c, EVH_ERR_CAPACITY, W + "w and h stay within 4096");
  if (A.npairs > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 pairs per call");
  if (int rc = need_source_stride(c, W, A.F, A.w, A.h, true)) return rc;      // a pair takes two frames
  if (A.npairs == 0) return EVH_SUCCESS;
  const int64_t nframes = (int64_t)(A.npairs - 1) * A.frame_step + 2;
  if (A.F.yuv && nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  if (int rc = need_planes(c, A.who, A.F, nframes, A.w, A.h)) return rc;
  // the outputs apart from each other, from the frames and from d_M_in, which d_M_out may only BE
  const int64_t np = A.npairs;
  const Span outs[3] = {{A.M_out, np * 72, "d_M_out"}, {A.info, np * EVH_REFINE_NINFO * 8, "d_info"},
                        {A.normal, np * EVH_REFINE_NSUMS * 8, "d_normal"}};
  Span src[3];
  source_spans(A.F, nframes, A.w, A.h, src);
  if (int rc = need_apart(c, W, outs, src)) return rc;
  const Span in{A.M_in, np * 72, "d_M_in"};
  for (int i = A.M_out == A.M_in ? 1 : 0; i < 3; i++)
    if (meet(outs[i], in)) return evh_fail(c, EVH_ERR_INVALID, W + outs[i].name + " overlaps d_M_in");
  return EVH_SUCCESS;
}
// workgroups per pair: one per 1024 runs, at most 64 -- a function of w and h only (it fixes the order of summation)
int refine_groups(const Runs& R) { return (int)std::min(64u, std::max(1u, (R.n + 1023u) / 1024u)); }
// iters + 1 times k_pair_refine_eval and k_pair_refine_step, the first evaluation at d_M_in, the others at the state's trial
int launch(evh_ctx* c, const RefineArgs& A) {
  const Runs R = runs_of(A.w, A.h);
  const int groups = refine_groups(R);
  const size_t state_bytes = ((size_t)A.npairs * sizeof(RefineState) + 255) & ~(size_t)255;
  if (int rc = grow(c, &c->d_refine_ws, &c->refine_ws_bytes, state_bytes + (size_t)A.npairs * groups * REFINE_SLOTS * sizeof(double)))
    return rc;
  RefineState* state = reinterpret_cast<RefineState*>(c->d_refine_ws);
  double* part = reinterpret_cast<double*>(c->d_refine_ws + state_bytes);
  int rc = EVH_SUCCESS;
  with_source(A.F, [&](auto cn, const auto& S) {
    for (int k = 0; k <= A.iters && rc == EVH_SUCCESS; k++) {
      hipLaunchKernelGGL((k_pair_refine_eval<decltype(cn)::value, std::decay_t<decltype(S)>>), dim3(groups, A.npairs), dim3(256), 0,
                         c->stream, S, A.frame_step, A.w, A.h, k == 0 ? A.M_in : nullptr, state, part, A.clip, R.per_row, R.n);
      hipLaunchKernelGGL(k_pair_refine_step, dim3(A.npairs), dim3(64), 0, c->stream, state, part, groups, k == 0, k == A.iters, A.w,
                         A.h, A.M_in, A.M_out, reinterpret_cast<unsigned long long*>(A.info), A.normal);
      rc = launched(c);
    }
  });
  return rc;
}

// ---- direct alignment against the mosaic: a frame's matrix refined on a canvas with holes -----------------------------------------
struct CanvasRefineArgs {
  const char* who; EvhFrames F; int nframes, w, h; const uint8_t* canvas; int dw, dh; int64_t canvas_stride; const uint8_t* count;
  int64_t count_stride; int min_cover; const double* M_in; int iters, clip; double* M_out; uint64_t* info; double* normal;
  bool idle() const { return nframes == 0; }
};
int check(evh_ctx* c, const CanvasRefineArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.canvas || !A.M_in || !A.M_out || !A.info) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (int rc = need_channels(c, W, A.F)) return rc;
  if (A.nframes < 0 || A.w < 1 || A.h < 1 || A.dw < 1 || A.dh < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame or canvas");
  if (A.iters < 0 || A.iters > EVH_REFINE_MAX_ITERS) return evh_fail(c, EVH_ERR_INVALID, W + "iters must lie in 0..64");
  if (A.clip < 0 || A.clip > 255) return evh_fail(c, EVH_ERR_INVALID, W + "clip must lie in 0..255");
  if (A.count && (A.min_cover < 1 || A.min_cover > 255)) return evh_fail(c, EVH_ERR_INVALID, W + "min_cover must lie in 1..255");
  // the frame's bounds are evh_pair_refine's (the Jacobian), the canvas's evh_warp_fixed_plane's source bounds (the positions)
  if (A.w > EVH_REFINE_MAX_SIZE || A.h > EVH_REFINE_MAX_SIZE) return evh_fail(c, EVH_ERR_CAPACITY, W + "w and h stay within 4096");
  if (int rc = need_below_2_26(c, W, "canvas", A.dw, A.dh)) return rc;
  if (int rc = need_area(c, W, "dw * dh", A.dw, A.dh)) return rc;
  if (A.nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  if (int rc = need_source_stride(c, W, A.F, A.w, A.h, A.nframes > 1)) return rc;
  if (A.canvas_stride < (int64_t)A.dw * A.F.channels) return evh_fail(c, EVH_ERR_INVALID, W + "canvas stride smaller than a row");
  if (A.count && A.count_stride < A.dw) return evh_fail(c, EVH_ERR_INVALID, W + "count stride smaller than a row");
  if (A.nframes == 0) return EVH_SUCCESS;
  if (int rc = need_planes(c, A.who, A.F, A.nframes, A.w, A.h)) return rc;
  // the outputs apart from each other, from everything that is read and from d_M_in, which d_M_out may only BE
  const int64_t nf = A.nframes;
  const Span outs[3] = {{A.M_out, nf * 72, "d_M_out"}, {A.info, nf * EVH_REFINE_NINFO * 8, "d_info"},
                        {A.normal, nf * EVH_REFINE_NSUMS * 8, "d_normal"}};
  Span src[3];
  source_spans(A.F, nf, A.w, A.h, src);
  const Span ins[5] = {src[0], src[1], src[2],
                       {A.canvas, (A.dh - 1) * A.canvas_stride + (int64_t)A.dw * A.F.channels, "the canvas"},
                       {A.count, (A.dh - 1) * A.count_stride + A.dw, "d_count"}};
  if (int rc = need_apart(c, W, outs, ins)) return rc;
  const Span in{A.M_in, nf * 72, "d_M_in"};
  for (int i = A.M_out == A.M_in ? 1 : 0; i < 3; i++)
    if (meet(outs[i], in)) return evh_fail(c, EVH_ERR_INVALID, W + outs[i].name + " overlaps d_M_in");
  return EVH_SUCCESS;
}
// evh_pair_refine's launches with k_canvas_refine_eval as the evaluation: the same groups for the same w, h, the same workspace
int launch(evh_ctx* c, const CanvasRefineArgs& A) {
  const Runs R = runs_of(A.w, A.h);
  const int groups = refine_groups(R);
  const size_t state_bytes = ((size_t)A.nframes * sizeof(RefineState) + 255) & ~(size_t)255;
  if (int rc = grow(c, &c->d_refine_ws, &c->refine_ws_bytes, state_bytes + (size_t)A.nframes * groups * REFINE_SLOTS * sizeof(double)))
    return rc;
  RefineState* state = reinterpret_cast<RefineState*>(c->d_refine_ws);
  double* part = reinterpret_cast<double*>(c->d_refine_ws + state_bytes);
  const PackedSrc canvas{A.canvas, A.F.channels, A.canvas_stride, 0};
  int rc = EVH_SUCCESS;
  with_source(A.F, [&](auto cn, const auto& S) {
    for (int k = 0; k <= A.iters && rc == EVH_SUCCESS; k++) {
      hipLaunchKernelGGL((k_canvas_refine_eval<decltype(cn)::value, std::decay_t<decltype(S)>>), dim3(groups, A.nframes), dim3(256), 0,
                         c->stream, S, canvas, A.count, A.count_stride, A.min_cover, A.w, A.h, A.dw, A.dh,
                         k == 0 ? A.M_in : nullptr, state, part, A.clip, R.per_row, R.n);
      hipLaunchKernelGGL(k_pair_refine_step, dim3(A.nframes), dim3(64), 0, c->stream, state, part, groups, k == 0, k == A.iters, A.w,
                         A.h, A.M_in, A.M_out, reinterpret_cast<unsigned long long*>(A.info), A.normal);
      rc = launched(c);
    }
  });
  return rc;
}

// ---- the trail: the fixed plane with earlier frames dimmed and the frame outlined (stabilization.py:21-97, 129-172) ----------
struct TrailArgs {
  const char* who; EvhFrames F; int nframes, sw, sh; const double* M; int inverse_map; const int32_t* rect; uint8_t* canvas;
  int64_t canvas_stride; uint8_t* out; int64_t out_stride, out_img_stride; int dw, dh, ox, oy;
  bool idle() const { return nframes == 0; }
};
int check(evh_ctx* c, const TrailArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.M || !A.canvas) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (A.nframes < 0 || A.sw < 1 || A.sh < 1 || A.dw < 1 || A.dh < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame or canvas");
  if (int rc = need_below_2_26(c, W, "source", A.sw, A.sh)) return rc;
  if (int rc = need_area(c, W, "dw * dh", A.dw, A.dh)) return rc;
  if (A.nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  const int64_t row = (int64_t)A.dw * 3;
  const int64_t canvas = (A.dh - 1) * A.canvas_stride + row, picture = (A.dh - 1) * A.out_stride + row;
  if (A.canvas_stride < row || (A.out && (A.out_stride < row || (A.nframes > 1 && A.out_img_stride < picture))))
    return evh_fail(c, EVH_ERR_INVALID, W + "canvas or output stride smaller than a row / picture");
  if (int rc = need_source_stride(c, W, A.F, A.sw, A.sh, A.nframes > 1)) return rc;
  if (A.nframes == 0) return EVH_SUCCESS;
  if (int rc = need_planes(c, A.who, A.F, A.nframes, A.sw, A.sh)) return rc;
  // canvas and pictures apart from each other, then plane by plane from the frames
  const Span outs[2] = {{A.out, A.out ? picture + (A.nframes - 1) * A.out_img_stride : 0, "d_out"}, {A.canvas, canvas, "d_canvas"}};
  Span src[3];
  source_spans(A.F, A.nframes, A.sw, A.sh, src);
  for (const Span& s : src) {
    const Span one[1] = {s};
    if (int rc = need_apart(c, W, outs, one)) return rc;
  }
  return EVH_SUCCESS;
}
// the tables of the colour step, in double on the host: S[i] = rint((255 << 12) / i), H[i] = rint((180 << 12) / (6 i)), halves
// to even; entry 0 of both is 0
const int32_t* trail_tables() {
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
// k_trail_fixed_plane over the canvas; out may be NULL.  BGR only: a packed source has three channels.
int launch(evh_ctx* c, const TrailArgs& A) {
  if (!c->trail_tab_ready) {          // once per context, stream-ordered in front of the first launch that reads it
    EVH_HIP(c, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_trail_tab), trail_tables(), 512 * sizeof(int32_t), 0, hipMemcpyHostToDevice,
                                      c->stream));
    c->trail_tab_ready = true;
  }
  const Runs R = runs_of(A.dw, A.dh);
  const int vec = (A.out && words_ok(A.out, A.out_stride, A.out_img_stride, A.nframes) ? 1 : 0) |
                  (words_ok(A.canvas, A.canvas_stride, 0, 1) ? 2 : 0);
  auto go = [&](auto kernel, const auto& S) {
    hipLaunchKernelGGL(kernel, dim3((R.n + 255) / 256), dim3(256), 0, c->stream, S, A.nframes, A.sw, A.sh, A.M, A.inverse_map,
                       A.rect, A.canvas, A.canvas_stride, A.out, A.out_stride, A.out_img_stride, A.dw, A.ox, A.oy, R.per_row, R.n, vec);
  };
  if (A.F.yuv) go(k_trail_fixed_plane<Yuv420Src>, yuv420_src(*A.F.yuv));
  else go(k_trail_fixed_plane<PackedSrc>, packed_src(A.F));
  return launched(c);
}

// ---- the background plate: the temporal median of the frames on the fixed plane, and what moves against it -------------------
struct PlateArgs {
  const char* who; EvhFrames F; int nframes, sw, sh; const double* M; int inverse_map, min_cover; const uint8_t* bg; uint8_t* plate;
  int64_t plate_stride; uint8_t* count; int64_t count_stride; uint8_t* mask; int threshold; int64_t mask_stride, mask_img_stride;
  int dw, dh, ox, oy;
  bool idle() const { return false; }       // no frames: the background goes to the plate
};
int check(evh_ctx* c, const PlateArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.M || !A.plate) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (int rc = need_channels(c, W, A.F)) return rc;
  if (A.nframes < 0 || A.sw < 1 || A.sh < 1 || A.dw < 1 || A.dh < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame or canvas");
  if (A.min_cover < 1 || A.min_cover > 255) return evh_fail(c, EVH_ERR_INVALID, W + "min_cover must lie in 1..255");
  if (A.mask && (A.threshold < 0 || A.threshold > 255)) return evh_fail(c, EVH_ERR_INVALID, W + "threshold must lie in 0..255");
  if (A.nframes > EVH_PLATE_MAX_FRAMES) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most EVH_PLATE_MAX_FRAMES = 255 frames per call");
  if (int rc = need_below_2_26(c, W, "source", A.sw, A.sh)) return rc;
  if (int rc = need_area(c, W, "dw * dh", A.dw, A.dh)) return rc;
  const int64_t row = (int64_t)A.dw * A.F.channels;
  const int64_t canvas = (A.dh - 1) * A.plate_stride + row, gray = (A.dh - 1) * A.count_stride + A.dw;
  const int64_t picture = (A.dh - 1) * A.mask_stride + A.dw;
  if (A.plate_stride < row) return evh_fail(c, EVH_ERR_INVALID, W + "plate stride smaller than a row");
  if (A.count && A.count_stride < A.dw) return evh_fail(c, EVH_ERR_INVALID, W + "count stride smaller than a row");
  if (A.mask && (A.mask_stride < A.dw || (A.nframes > 1 && A.mask_img_stride < picture)))
    return evh_fail(c, EVH_ERR_INVALID, W + "mask stride smaller than a row / picture");
  if (int rc = need_source_stride(c, W, A.F, A.sw, A.sh, A.nframes > 1)) return rc;
  if (A.nframes > 0)
    if (int rc = need_planes(c, A.who, A.F, A.nframes, A.sw, A.sh)) return rc;
  // the outputs apart from each other, from the background and from the frames
  const Span outs[3] = {{A.plate, canvas, "d_plate"}, {A.count, gray, "d_count"},
                        {A.mask, A.nframes > 0 ? picture + (A.nframes - 1) * A.mask_img_stride : 0, "d_mask"}};
  Span src[3];
  source_spans(A.F, A.nframes, A.sw, A.sh, src);
  const Span ins[4] = {{A.bg, canvas, "d_background"}, src[0], src[1], src[2]};
  return need_apart(c, W, outs, ins);
}
// k_plate_fixed_plane over the canvas (nframes <= EVH_PLATE_MAX_FRAMES, so the column of samples, 256 bytes per frame, stays
// below the 64 KiB a workgroup gets without asking); nframes may be 0, bg, count and mask may be NULL
int launch(evh_ctx* c, const PlateArgs& A) {
  const unsigned npix = (unsigned)A.dw * (unsigned)A.dh;
  const size_t lds = (size_t)A.nframes * 64 * sizeof(uint32_t);
  with_source(A.F, [&](auto cn, const auto& S) {
    hipLaunchKernelGGL((k_plate_fixed_plane<decltype(cn)::value, std::decay_t<decltype(S)>>), dim3((npix + 63) / 64), dim3(64), lds,
                       c->stream, S, A.nframes, A.sw, A.sh, A.M, A.inverse_map, A.min_cover, A.bg, A.plate, A.plate_stride, A.count,
                       A.count_stride, A.mask, A.threshold, A.mask_stride, A.mask_img_stride, A.dw, A.ox, A.oy, npix);
  });
  return launched(c);
}

// ---- match rows against the plate: rows whose points sit on what moves are dropped ------------------------------------------------
struct MovingArgs {
  const char* who; EvhFrames F; int nframes, sw, sh; const double* M; const uint8_t* plate; int64_t plate_stride;
  const uint8_t* count; int64_t count_stride; int dw, dh, ox, oy, min_cover, threshold, radius, min_hits; double row_sx, row_sy;
  const float* rows; int row_cap; const int32_t* counts; const int32_t* status1; int npairs, frame_step, min_keep;
  float* out_rows; int32_t* out_counts; int32_t* moving; uint8_t* flags;
  bool idle() const { return npairs == 0; }
};
int check(evh_ctx* c, const MovingArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.M || !A.plate || !A.count || !A.rows || !A.counts || !A.status1 || !A.out_rows || !A.out_counts)
    return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (int rc = need_channels(c, W, A.F)) return rc;
  if (A.nframes < 0 || A.sw < 1 || A.sh < 1 || A.dw < 1 || A.dh < 1 || A.row_cap < 1 || A.npairs < 0)
    return evh_fail(c, EVH_ERR_INVALID, W + "empty frame, canvas or row block");
  if (A.frame_step != 1 && A.frame_step != 2) return evh_fail(c, EVH_ERR_INVALID, W + "frame_step must be 1 or 2");
  if (A.min_cover < 1 || A.min_cover > 255) return evh_fail(c, EVH_ERR_INVALID, W + "min_cover must lie in 1..255");
  if (A.threshold < 0 || A.threshold > 255) return evh_fail(c, EVH_ERR_INVALID, W + "threshold must lie in 0..255");
  if (A.radius < 0 || A.radius > 7) return evh_fail(c, EVH_ERR_INVALID, W + "radius must lie in 0..7");
  if (A.min_hits < 1 || A.min_hits > (2 * A.radius + 1) * (2 * A.radius + 1))
    return evh_fail(c, EVH_ERR_INVALID, W + "min_hits must lie in 1..(2*radius+1)^2");
  if (A.min_keep < 0) return evh_fail(c, EVH_ERR_INVALID, W + "min_keep must not be negative");
  if (!(std::isfinite(A.row_sx) && std::isfinite(A.row_sy) && A.row_sx > 0.0 && A.row_sy > 0.0))
    return evh_fail(c, EVH_ERR_INVALID, W + "row_sx and row_sy must be finite and positive");
  if (A.npairs > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 pairs per call");
  if (int rc = need_below_2_26(c, W, "source", A.sw, A.sh)) return rc;
  if (int rc = need_area(c, W, "dw * dh", A.dw, A.dh)) return rc;
  if (A.npairs > 0 && (int64_t)(A.npairs - 1) * A.frame_step + 2 > A.nframes)
    return evh_fail(c, EVH_ERR_INVALID, W + "nframes does not reach the last pair's frames");
  const int64_t row = (int64_t)A.dw * A.F.channels;
  if (A.plate_stride < row) return evh_fail(c, EVH_ERR_INVALID, W + "plate stride smaller than a row");
  if (A.count_stride < A.dw) return evh_fail(c, EVH_ERR_INVALID, W + "count stride smaller than a row");
  if (int rc = need_source_stride(c, W, A.F, A.sw, A.sh, A.nframes > 1)) return rc;
  if (A.nframes > 0)
    if (int rc = need_planes(c, A.who, A.F, A.nframes, A.sw, A.sh)) return rc;
  if (((uintptr_t)A.rows | (uintptr_t)A.out_rows) & 15) return evh_fail(c, EVH_ERR_INVALID, W + "d_rows and d_out_rows must be 16-byte aligned");
  // every output apart from the other outputs and from every input
  const int64_t block = (int64_t)A.npairs * A.row_cap, per_pair = (int64_t)A.npairs * 4;
  const Span outs[4] = {{A.out_rows, block * 16, "d_out_rows"}, {A.out_counts, per_pair, "d_out_counts"},
                        {A.moving, per_pair, "d_moving"}, {A.flags, block, "d_flags"}};
  Span src[3];
  source_spans(A.F, A.nframes, A.sw, A.sh, src);
  const Span ins[9] = {{A.M, (int64_t)A.nframes * 72, "d_M"}, {A.plate, (A.dh - 1) * A.plate_stride + row, "d_plate"},
                       {A.count, (A.dh - 1) * A.count_stride + A.dw, "d_count"}, {A.rows, block * 16, "d_rows"},
                       {A.counts, per_pair, "d_counts"}, {A.status1, per_pair, "d_status1"}, src[0], src[1], src[2]};
  return need_apart(c, W, outs, ins);
}
// k_rows_moving_filter, one workgroup per pair (1 <= npairs <= 65535); moving and flags may be NULL
int launch(evh_ctx* c, const MovingArgs& A) {
  with_source(A.F, [&](auto cn, const auto& S) {
    hipLaunchKernelGGL((k_rows_moving_filter<decltype(cn)::value, std::decay_t<decltype(S)>>), dim3(A.npairs), dim3(MOVING_TILE), 0,
                       c->stream, S, A.sw, A.sh, A.M, A.plate, A.plate_stride, A.count, A.count_stride, A.dw, A.dh, A.ox, A.oy,
                       A.min_cover, A.threshold, A.radius, A.min_hits, A.row_sx, A.row_sy, A.rows, A.row_cap, A.counts, A.status1,
                       A.frame_step, A.min_keep, A.out_rows, A.out_counts, A.moving, A.flags);
  });
  return launched(c);
}

#include "evh_plane_components.h"  // the connected components of the masks: kernels, check() and launch()

}  // namespace

extern "C" {

int evh_warp_fixed_plane(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                         int64_t frame_stride, const double* d_M, int inverse_map, int mode, const uint8_t* d_background,
                         uint8_t* d_out, int dw, int dh, int64_t out_row_stride, int64_t out_frame_stride, int ox, int oy) {
  return run(c, WarpArgs{"evh_warp_fixed_plane", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh, d_M,
                         inverse_map, mode, d_background, d_out, dw, dh, out_row_stride, out_frame_stride, ox, oy});
}

int evh_warp_fixed_plane_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                int inverse_map, int mode, const uint8_t* d_background, uint8_t* d_out, int dw, int dh,
                                int64_t out_row_stride, int64_t out_frame_stride, int ox, int oy) {
  return run(c, WarpArgs{"evh_warp_fixed_plane_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, inverse_map, mode, d_background,
                         d_out, dw, dh, out_row_stride, out_frame_stride, ox, oy});
}

int evh_warp_ray_surface(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                         int64_t frame_stride, const double* d_A, const double* d_col, const double* d_row, int mode,
                         const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride, int64_t out_frame_stride) {
  return run(c, RayArgs{{"evh_warp_ray_surface", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh, d_A,
                         1, mode, d_background, d_out, dw, dh, out_row_stride, out_frame_stride, 0, 0}, d_col, d_row});
}

int evh_warp_ray_surface_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_A,
                                const double* d_col, const double* d_row, int mode, const uint8_t* d_background, uint8_t* d_out,
                                int dw, int dh, int64_t out_row_stride, int64_t out_frame_stride) {
  return run(c, RayArgs{{"evh_warp_ray_surface_yuv420", yuv420_frames(src), nframes, sw, sh, d_A, 1, mode, d_background, d_out,
                         dw, dh, out_row_stride, out_frame_stride, 0, 0}, d_col, d_row});
}

int evh_blend_fixed_plane(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                          int64_t frame_stride, const double* d_M, int inverse_map, int mode, int feather, const uint16_t* d_gain,
                          uint64_t* d_acc, int acc_in, const uint8_t* d_background, uint8_t* d_out, int dw, int dh,
                          int64_t out_row_stride, int ox, int oy) {
  return run(c, BlendArgs{{"evh_blend_fixed_plane", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh, d_M,
                           inverse_map, mode, d_background, d_out, dw, dh, out_row_stride, 0, ox, oy},
                          false, nullptr, nullptr, feather, d_gain, d_acc, acc_in});
}

int evh_blend_fixed_plane_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M, int inverse_map,
                                 int mode, int feather, const uint16_t* d_gain, uint64_t* d_acc, int acc_in,
                                 const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride, int ox, int oy) {
  return run(c, BlendArgs{{"evh_blend_fixed_plane_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, inverse_map, mode, d_background,
                           d_out, dw, dh, out_row_stride, 0, ox, oy},
                          false, nullptr, nullptr, feather, d_gain, d_acc, acc_in});
}

int evh_blend_ray_surface(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                          int64_t frame_stride, const double* d_A, const double* d_col, const double* d_row, int mode, int feather,
                          const uint16_t* d_gain, uint64_t* d_acc, int acc_in, const uint8_t* d_background, uint8_t* d_out, int dw,
                          int dh, int64_t out_row_stride) {
  return run(c, BlendArgs{{"evh_blend_ray_surface", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh, d_A,
                           1, mode, d_background, d_out, dw, dh, out_row_stride, 0, 0, 0},
                          true, d_col, d_row, feather, d_gain, d_acc, acc_in});
}

int evh_blend_ray_surface_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_A,
                                 const double* d_col, const double* d_row, int mode, int feather, const uint16_t* d_gain,
                                 uint64_t* d_acc, int acc_in, const uint8_t* d_background, uint8_t* d_out, int dw, int dh,
                                 int64_t out_row_stride) {
  return run(c, BlendArgs{{"evh_blend_ray_surface_yuv420", yuv420_frames(src), nframes, sw, sh, d_A, 1, mode, d_background, d_out, dw,
                           dh, out_row_stride, 0, 0, 0},
                          true, d_col, d_row, feather, d_gain, d_acc, acc_in});
}

int evh_seam_labels_fixed_plane(evh_ctx* c, int nframes, int sw, int sh, const double* d_M, int inverse_map, int feather, int dw, int dh,
                                int ox, int oy, int first_label, uint32_t* d_best, uint16_t* d_label, int state_in) {
  return run(c, LabelArgs{"evh_seam_labels_fixed_plane", nframes, sw, sh, d_M, inverse_map, false, nullptr, nullptr, feather, dw, dh, ox,
                          oy, first_label, d_best, d_label, state_in});
}

int evh_seam_labels_ray_surface(evh_ctx* c, int nframes, int sw, int sh, const double* d_A, const double* d_col, const double* d_row,
                                int feather, int dw, int dh, int first_label, uint32_t* d_best, uint16_t* d_label, int state_in) {
  return run(c, LabelArgs{"evh_seam_labels_ray_surface", nframes, sw, sh, d_A, 1, true, d_col, d_row, feather, dw, dh, 0, 0, first_label,
                          d_best, d_label, state_in});
}

int64_t evh_bands_state_elems(int dw, int dh, int channels, int levels) {
  if (dw < 1 || dh < 1 || (channels != 1 && channels != 3) || levels < 0 || levels > 8) return -1;
  return bands_state_elems(dw, dh, channels, levels);
}

int64_t evh_bands_frame_ws_bytes(int dw, int dh, int channels, int levels) {
  const int64_t elems = evh_bands_state_elems(dw, dh, channels, levels);
  return elems < 0 ? -1 : elems * 4;
}

int evh_blend_bands_fixed_plane(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                                int64_t frame_stride, const double* d_M, int inverse_map, int levels, const uint16_t* d_label,
                                int first_label, const uint16_t* d_gain, int64_t* d_state, int state_in, void* d_ws, int64_t ws_bytes,
                                const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride, int ox, int oy) {
  return run(c, BandsArgs{{{"evh_blend_bands_fixed_plane", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh,
                            d_M, inverse_map, EVH_BLEND_SEAM, d_background, d_out, dw, dh, out_row_stride, 0, ox, oy},
                           false, nullptr, nullptr, 0, d_gain, reinterpret_cast<uint64_t*>(d_state), state_in},
                          levels, d_label, first_label, d_ws, ws_bytes});
}

int evh_blend_bands_fixed_plane_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M, int inverse_map,
                                       int levels, const uint16_t* d_label, int first_label, const uint16_t* d_gain, int64_t* d_state,
                                       int state_in, void* d_ws, int64_t ws_bytes, const uint8_t* d_background, uint8_t* d_out, int dw,
                                       int dh, int64_t out_row_stride, int ox, int oy) {
  return run(c, BandsArgs{{{"evh_blend_bands_fixed_plane_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, inverse_map, EVH_BLEND_SEAM,
                            d_background, d_out, dw, dh, out_row_stride, 0, ox, oy},
                           false, nullptr, nullptr, 0, d_gain, reinterpret_cast<uint64_t*>(d_state), state_in},
                          levels, d_label, first_label, d_ws, ws_bytes});
}

int evh_blend_bands_ray_surface(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                                int64_t frame_stride, const double* d_A, const double* d_col, const double* d_row, int levels,
                                const uint16_t* d_label, int first_label, const uint16_t* d_gain, int64_t* d_state, int state_in,
                                void* d_ws, int64_t ws_bytes, const uint8_t* d_background, uint8_t* d_out, int dw, int dh,
                                int64_t out_row_stride) {
  return run(c, BandsArgs{{{"evh_blend_bands_ray_surface", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh,
                            d_A, 1, EVH_BLEND_SEAM, d_background, d_out, dw, dh, out_row_stride, 0, 0, 0},
                           true, d_col, d_row, 0, d_gain, reinterpret_cast<uint64_t*>(d_state), state_in},
                          levels, d_label, first_label, d_ws, ws_bytes});
}

int evh_blend_bands_ray_surface_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_A,
                                       const double* d_col, const double* d_row, int levels, const uint16_t* d_label, int first_label,
                                       const uint16_t* d_gain, int64_t* d_state, int state_in, void* d_ws, int64_t ws_bytes,
                                       const uint8_t* d_background, uint8_t* d_out, int dw, int dh, int64_t out_row_stride) {
  return run(c, BandsArgs{{{"evh_blend_bands_ray_surface_yuv420", yuv420_frames(src), nframes, sw, sh, d_A, 1, EVH_BLEND_SEAM,
                            d_background, d_out, dw, dh, out_row_stride, 0, 0, 0},
                           true, d_col, d_row, 0, d_gain, reinterpret_cast<uint64_t*>(d_state), state_in},
                          levels, d_label, first_label, d_ws, ws_bytes});
}

int evh_pair_exposure(evh_ctx* c, const uint8_t* d_frames, int nframes, int w, int h, int channels, int64_t row_stride,
                      int64_t frame_stride, const int32_t* d_pairs, int npairs, const double* d_M, int step, int lo, int hi,
                      uint64_t* d_stats) {
  return run(c, ExposureArgs{"evh_pair_exposure", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, w, h, d_pairs,
                             npairs, d_M, step, lo, hi, d_stats});
}

int evh_pair_exposure_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int w, int h, const int32_t* d_pairs, int npairs,
                             const double* d_M, int step, int lo, int hi, uint64_t* d_stats) {
  return run(c, ExposureArgs{"evh_pair_exposure_yuv420", yuv420_frames(src), nframes, w, h, d_pairs, npairs, d_M, step, lo, hi,
                             d_stats});
}

int evh_pair_residual(evh_ctx* c, const uint8_t* d_frames, int npairs, int frame_step, int w, int h, int channels,
                      int64_t row_stride, int64_t frame_stride, const double* d_M, int threshold, uint64_t* d_stats, uint8_t* d_out,
                      int kind, int64_t out_row_stride, int64_t out_frame_stride) {
  return run(c, ResidualArgs{"evh_pair_residual", packed_frames(d_frames, channels, row_stride, frame_stride), npairs, frame_step, w,
                             h, d_M, threshold, d_stats, d_out, kind, out_row_stride, out_frame_stride});
}

int evh_pair_residual_yuv420(evh_ctx* c, const evh_yuv420* src, int npairs, int frame_step, int w, int h, const double* d_M,
                             int threshold, uint64_t* d_stats, uint8_t* d_out, int kind, int64_t out_row_stride,
                             int64_t out_frame_stride) {
  return run(c, ResidualArgs{"evh_pair_residual_yuv420", yuv420_frames(src), npairs, frame_step, w, h, d_M, threshold, d_stats,
                             d_out, kind, out_row_stride, out_frame_stride});
}

int evh_pair_refine(evh_ctx* c, const uint8_t* d_frames, int npairs, int frame_step, int w, int h, int channels, int64_t row_stride,
                    int64_t frame_stride, const double* d_M_in, int iters, int clip, double* d_M_out, uint64_t* d_info,
                    double* d_normal) {
  return run(c, RefineArgs{"evh_pair_refine", packed_frames(d_frames, channels, row_stride, frame_stride), npairs, frame_step, w, h,
                           d_M_in, iters, clip, d_M_out, d_info, d_normal});
}

int evh_pair_refine_yuv420(evh_ctx* c, const evh_yuv420* src, int npairs, int frame_step, int w, int h, const double* d_M_in,
                           int iters, int clip, double* d_M_out, uint64_t* d_info, double* d_normal) {
  return run(c, RefineArgs{"evh_pair_refine_yuv420", yuv420_frames(src), npairs, frame_step, w, h, d_M_in, iters, clip, d_M_out,
                           d_info, d_normal});
}

int evh_canvas_refine(evh_ctx* c, const uint8_t* d_frames, int nframes, int w, int h, int channels, int64_t row_stride,
                      int64_t frame_stride, const uint8_t* d_canvas, int dw, int dh, int64_t canvas_row_stride, const uint8_t* d_count,
                      int64_t count_row_stride, int min_cover, const double* d_M_in, int iters, int clip, double* d_M_out,
                      uint64_t* d_info, double* d_normal) {
  return run(c, CanvasRefineArgs{"evh_canvas_refine", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, w, h,
                                 d_canvas, dw, dh, canvas_row_stride, d_count, count_row_stride, min_cover, d_M_in, iters, clip,
                                 d_M_out, d_info, d_normal});
}

int evh_canvas_refine_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int w, int h, const uint8_t* d_canvas, int dw, int dh,
                             int64_t canvas_row_stride, const uint8_t* d_count, int64_t count_row_stride, int min_cover,
                             const double* d_M_in, int iters, int clip, double* d_M_out, uint64_t* d_info, double* d_normal) {
  return run(c, CanvasRefineArgs{"evh_canvas_refine_yuv420", yuv420_frames(src), nframes, w, h, d_canvas, dw, dh, canvas_row_stride,
                                 d_count, count_row_stride, min_cover, d_M_in, iters, clip, d_M_out, d_info, d_normal});
}

int evh_trail_fixed_plane(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int64_t row_stride,
                          int64_t frame_stride, const double* d_M, int inverse_map, const int32_t* d_rect, uint8_t* d_canvas,
                          int64_t canvas_row_stride, uint8_t* d_out, int64_t out_row_stride, int64_t out_frame_stride, int dw,
                          int dh, int ox, int oy) {
  return run(c, TrailArgs{"evh_trail_fixed_plane", packed_frames(d_frames, 3, row_stride, frame_stride), nframes, sw, sh, d_M,
                          inverse_map, d_rect, d_canvas, canvas_row_stride, d_out, out_row_stride, out_frame_stride, dw, dh, ox, oy});
}

int evh_trail_fixed_plane_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                 int inverse_map, const int32_t* d_rect, uint8_t* d_canvas, int64_t canvas_row_stride,
                                 uint8_t* d_out, int64_t out_row_stride, int64_t out_frame_stride, int dw, int dh, int ox, int oy) {
  return run(c, TrailArgs{"evh_trail_fixed_plane_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, inverse_map, d_rect, d_canvas,
                          canvas_row_stride, d_out, out_row_stride, out_frame_stride, dw, dh, ox, oy});
}

int evh_plate_fixed_plane(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                          int64_t frame_stride, const double* d_M, int inverse_map, int min_cover, const uint8_t* d_background,
                          uint8_t* d_plate, int64_t plate_row_stride, uint8_t* d_count, int64_t count_row_stride, uint8_t* d_mask,
                          int threshold, int64_t mask_row_stride, int64_t mask_frame_stride, int dw, int dh, int ox, int oy) {
  return run(c, PlateArgs{"evh_plate_fixed_plane", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh, d_M,
                          inverse_map, min_cover, d_background, d_plate, plate_row_stride, d_count, count_row_stride, d_mask,
                          threshold, mask_row_stride, mask_frame_stride, dw, dh, ox, oy});
}

int evh_plate_fixed_plane_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                 int inverse_map, int min_cover, const uint8_t* d_background, uint8_t* d_plate,
                                 int64_t plate_row_stride, uint8_t* d_count, int64_t count_row_stride, uint8_t* d_mask, int threshold,
                                 int64_t mask_row_stride, int64_t mask_frame_stride, int dw, int dh, int ox, int oy) {
  return run(c, PlateArgs{"evh_plate_fixed_plane_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, inverse_map, min_cover,
                          d_background, d_plate, plate_row_stride, d_count, count_row_stride, d_mask, threshold, mask_row_stride,
                          mask_frame_stride, dw, dh, ox, oy});
}

size_t evh_mask_components_work_bytes(int dw, int dh, int nmasks) { return components_work_bytes(dw, dh, nmasks); }

int evh_mask_components(evh_ctx* c, const uint8_t* d_mask, int nmasks, int dw, int dh, int64_t mask_row_stride, int64_t mask_frame_stride,
                        int connectivity, int open_radius, int min_area, int32_t* d_labels, int64_t label_row_stride,
                        int64_t label_frame_stride, evh_component* d_objects, int max_objects, int32_t* d_nobjects, void* d_work,
                        size_t work_bytes) {
  return run(c, ComponentsArgs{"evh_mask_components", d_mask, nmasks, dw, dh, mask_row_stride, mask_frame_stride, connectivity,
                               open_radius, min_area, d_labels, label_row_stride, label_frame_stride, d_objects, max_objects,
                               d_nobjects, d_work, work_bytes});
}

int evh_rows_moving_filter(evh_ctx* c, const uint8_t* d_frames, int nframes, int sw, int sh, int channels, int64_t row_stride,
                           int64_t frame_stride, const double* d_M, const uint8_t* d_plate, int64_t plate_row_stride,
                           const uint8_t* d_count, int64_t count_row_stride, int dw, int dh, int ox, int oy, int min_cover,
                           int threshold, int radius, int min_hits, double row_sx, double row_sy, const float* d_rows, int row_cap,
                           const int32_t* d_counts, const int32_t* d_status1, int npairs, int frame_step, int min_keep,
                           float* d_out_rows, int32_t* d_out_counts, int32_t* d_moving, uint8_t* d_flags) {
  return run(c, MovingArgs{"evh_rows_moving_filter", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, sw, sh,
                           d_M, d_plate, plate_row_stride, d_count, count_row_stride, dw, dh, ox, oy, min_cover, threshold, radius,
                           min_hits, row_sx, row_sy, d_rows, row_cap, d_counts, d_status1, npairs, frame_step, min_keep, d_out_rows,
                           d_out_counts, d_moving, d_flags});
}

int evh_rows_moving_filter_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int sw, int sh, const double* d_M,
                                  const uint8_t* d_plate, int64_t plate_row_stride, const uint8_t* d_count,
                                  int64_t count_row_stride, int dw, int dh, int ox, int oy, int min_cover, int threshold, int radius,
                                  int min_hits, double row_sx, double row_sy, const float* d_rows, int row_cap,
                                  const int32_t* d_counts, const int32_t* d_status1, int npairs, int frame_step, int min_keep,
                                  float* d_out_rows, int32_t* d_out_counts, int32_t* d_moving, uint8_t* d_flags) {
  return run(c, MovingArgs{"evh_rows_moving_filter_yuv420", yuv420_frames(src), nframes, sw, sh, d_M, d_plate, plate_row_stride,
                           d_count, count_row_stride, dw, dh, ox, oy, min_cover, threshold, radius, min_hits, row_sx, row_sy, d_rows,
                           row_cap, d_counts, d_status1, npairs, frame_step, min_keep, d_out_rows, d_out_counts, d_moving, d_flags});
}

// ---- heat-map pictures (processing_visualization.py:336-344): one form, so the checks and the launch sit in the entry ------------
int evh_heatmap_render(evh_ctx* c, const double* d_Hsup, int n, int w, int h, const uint8_t* d_frames, int64_t row_stride,
                       int64_t frame_stride, const uint8_t* d_lut, double heatmap_constant, double alpha, int saturate,
                       uint8_t* d_out, int64_t out_row_stride, int64_t out_frame_stride) {
  if (!c) return EVH_ERR_INVALID;
  const std::string W = "evh_heatmap_render: ";
  if (!d_Hsup || !d_lut || !d_out) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (n < 0 || w < 1 || h < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty grid or negative n");
  if (!std::isfinite(heatmap_constant) || heatmap_constant <= 0) return evh_fail(c, EVH_ERR_INVALID, W + "heatmap_constant must be finite and positive");
  if (!std::isfinite(alpha) || alpha < 0) return evh_fail(c, EVH_ERR_INVALID, W + "alpha must be finite and not negative");
  if (n > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 matrices per call");
  if (int rc = need_area(c, W, "w * h", w, h)) return rc;
  const int64_t row = (int64_t)w * 3;
  if (out_row_stride < row || (d_frames && row_stride < row)) return evh_fail(c, EVH_ERR_INVALID, W + "stride smaller than a row");
  const int64_t picture = (h - 1) * out_row_stride + row, frame = d_frames ? (h - 1) * row_stride + row : 0;
  if (n > 1 && (out_frame_stride < picture || (d_frames && frame_stride < frame)))
    return evh_fail(c, EVH_ERR_INVALID, W + "stride smaller than a frame");
  if (n > 0 && meet({d_frames, frame + (n - 1) * frame_stride, ""}, {d_out, picture + (n - 1) * out_frame_stride, ""}))
    return evh_fail(c, EVH_ERR_INVALID, W + "d_frames overlaps d_out");
  if (n == 0) return EVH_SUCCESS;
  // k_heatmap_render over n frames of w x h
  const Runs R = runs_of(w, h);
  const int vec = (words_ok(d_out, out_row_stride, out_frame_stride, n) ? 1 : 0) |
                  (d_frames && words_ok(d_frames, row_stride, frame_stride, n) ? 2 : 0);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((R.n + 255) / 256, n), dim3(256), 0, c->stream, d_Hsup, w, d_frames, row_stride, frame_stride,
                       d_lut, heatmap_constant, alpha, saturate, d_out, out_row_stride, out_frame_stride, R.per_row, R.n, vec);
  };
  if (!d_frames || alpha == 0.8) go(k_heatmap_render<false>);      // the integer blend, behind the exact test for its constant
  else go(k_heatmap_render<true>);
  return launched(c);
}

// ---- matching pictures (processing_visualization.py:22-57): one form as well ------------------------------------------------------
int evh_draw_matches(evh_ctx* c, const uint8_t* d_frames, int npairs, int frame_step, int w, int h, int64_t row_stride,
                     int64_t frame_stride, const float* d_rows, int row_cap, const int32_t* d_counts, const int32_t* d_status,
                     int points, uint32_t color_bgr, uint8_t* d_out, int64_t out_row_stride, int64_t out_frame_stride) {
  if (!c) return EVH_ERR_INVALID;
  const std::string W = "evh_draw_matches: ";
  if (!d_frames || !d_rows || !d_counts || !d_out) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (npairs < 0 || w < 1 || h < 1 || row_cap < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame, no row capacity or negative npairs");
  if (frame_step != 1 && frame_step != 2) return evh_fail(c, EVH_ERR_INVALID, W + "frame_step must be 1 or 2");
  if (points != EVH_DRAW_REFERENCE && points != EVH_DRAW_OWN_FRAME) return evh_fail(c, EVH_ERR_INVALID, W + "unknown points value");
  if (color_bgr >> 24) return evh_fail(c, EVH_ERR_INVALID, W + "color_bgr has bits above 24 set");
  if (w > 16383) return evh_fail(c, EVH_ERR_CAPACITY, W + "w above 16383 (a picture's columns are held in 16 bits)");
  const int64_t row = (int64_t)w * 3;
  if (row_stride < row || out_row_stride < 2 * row) return evh_fail(c, EVH_ERR_INVALID, W + "stride smaller than a row");
  const int64_t frame = (h - 1) * row_stride + row, picture = (h - 1) * out_row_stride + 2 * row;
  if ((npairs >= 1 && frame_stride < frame) || (npairs > 1 && out_frame_stride < picture))
    return evh_fail(c, EVH_ERR_INVALID, W + "stride smaller than a frame");
  if (npairs == 0) return EVH_SUCCESS;
  const Span pictures{d_out, picture + (npairs - 1) * out_frame_stride, ""};
  if (meet({d_frames, frame + ((int64_t)(npairs - 1) * frame_step + 1) * frame_stride, ""}, pictures))
    return evh_fail(c, EVH_ERR_INVALID, W + "d_frames overlaps d_out");
  if (meet({d_rows, (int64_t)npairs * row_cap * 4 * (int64_t)sizeof(float), ""}, pictures))
    return evh_fail(c, EVH_ERR_INVALID, W + "d_rows overlaps d_out");
  // k_draw_paste, then k_draw_lines on top (w <= 16383)
  const int runs_per_half = runs_of(w, 1).per_row;
  // the frames' stride always counts: a picture takes two frames
  const bool out_words = words_ok(d_out, out_row_stride, out_frame_stride, npairs);
  const int vec = (out_words ? 1 : 0) | (words_ok(d_frames, row_stride, frame_stride, 2) ? 2 : 0) | (out_words && (w & 3) == 0 ? 4 : 0);
  const dim3 pgrid((2 * runs_per_half + 255) / 256, std::min(h, 65535), std::min(npairs, 65535));
  hipLaunchKernelGGL(k_draw_paste, pgrid, dim3(256), 0, c->stream, d_frames, npairs, frame_step, w, h, row_stride, frame_stride,
                     d_out, out_row_stride, out_frame_stride, runs_per_half, vec);
  EVH_HIP(c, hipGetLastError());
  const dim3 lgrid(std::min(64, (row_cap + 3) / 4), std::min(npairs, 65535));
  hipLaunchKernelGGL(k_draw_lines, lgrid, dim3(256), 0, c->stream, d_rows, row_cap, d_counts, d_status, npairs, points, w, h,
                     color_bgr, d_out, out_row_stride, out_frame_stride);
  return launched(c);
}

}  // extern "C"
