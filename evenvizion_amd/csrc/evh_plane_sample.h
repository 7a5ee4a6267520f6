// evh_plane_sample.h -- what the kernels of the plane unit share: the run of WARP_RUN pixels a thread owns, the map from a canvas
// pixel to a frame, the sampler, and the geometry of the blends.  Included by evh_plane.hip inside its unnamed namespace, first.

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
// ---- the sampler, in three pieces that every kernel of the unit builds on -----------------------------------------------------------
// The rows of a map at a point: tx, ty, tw as include/evhip.h states them, products and sums one IEEE operation at a time.
struct MapRows { double tx, ty, tw; };
__device__ __forceinline__ MapRows map_rows(const double* a, double X, double Y) {
  return {(a[0] * X + a[1] * Y) + a[2], (a[3] * X + a[4] * Y) + a[5], (a[6] * X + a[7] * Y) + a[8]};
}
// The position in a frame, in 1/32 pixels (INTER_BITS = 5) rounded half to even, before any test; tw for the callers that ask its
// sign.  From the rows themselves for the maps whose rows are not map_rows (the rays of evh_plane_bands.h).
struct SamplePos { double U, V, tw; };
__device__ __forceinline__ SamplePos sample_position(const MapRows& r) {
  return {__builtin_rint(r.tx / r.tw * 32.0), __builtin_rint(r.ty / r.tw * 32.0), r.tw};
}
__device__ __forceinline__ SamplePos sample_position(const WarpMap& A, double X, double Y) { return sample_position(map_rows(A.a, X, Y)); }
// Does a frame of sw x sh cover the position?  The comparisons are made in double, so NaN and +-inf (a zero, singular or NaN
// matrix, the horizon) cover nothing.
__device__ __forceinline__ bool sample_covered(const SamplePos& P, int sw, int sh) {
  return P.U >= 0.0 && P.U <= (double)(32 * (sw - 1)) && P.V >= 0.0 && P.V <= (double)(32 * (sh - 1));
}
// The four bilinear taps of frame `img` at (u, w) / 32, rounded to nearest, into v[0 .. channels).  For 0 <= u <= 32 (sw - 1) the
// column is 0 <= sx <= sw - 1, and sx + 1 is read only with fx != 0, i.e. sx <= sw - 2 (rows alike): no tap leaves the frame, and a
// tap of weight 0 is not read.  hook(dx, dy) is called beside every tap that is read.
struct NoTapHook { __device__ __forceinline__ void operator()(int, int) const {} };
template <class SRC, class HOOK = NoTapHook>
__device__ __forceinline__ void sample_taps(const SRC& src, int img, int u, int w, int (&v)[3], HOOK hook = HOOK{}) {
  const int sx = u >> 5, fx = u & 31, sy = w >> 5, fy = w & 31;
  const int cn = src.channels();
  int p00[3] = {0, 0, 0}, p01[3] = {0, 0, 0}, p10[3] = {0, 0, 0}, p11[3] = {0, 0, 0};
  const typename SRC::Row r0 = src.row(img, sy);
  r0.px(sx, p00); hook(0, 0);
  if (fx) { r0.px(sx + 1, p01); hook(1, 0); }
  if (fy) {
    const typename SRC::Row r1 = src.row(img, sy + 1);
    r1.px(sx, p10); hook(0, 1);
    if (fx) { r1.px(sx + 1, p11); hook(1, 1); }
  }
  const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
#pragma unroll
  for (int c = 0; c < 3; c++) if (c < cn) v[c] = (p00[c] * w00 + p01[c] * w01 + p10[c] * w10 + p11[c] * w11 + 512) >> 10;
}
// Frame `img` at plane point (X, Y): false = the frame does not cover it (v is left alone).
template <class SRC>
__device__ __forceinline__ bool warp_sample(const SRC& src, int img, const WarpMap& A, double X, double Y, int sw, int sh,
                                            int (&v)[3]) {
  const SamplePos P = sample_position(A, X, Y);
  if (!sample_covered(P, sw, sh)) return false;
  sample_taps(src, img, (int)P.U, (int)P.V, v);
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

// Fixed surfaces that do not end at a horizon (include/evhip.h states the contract for evh_warp_ray_surface): canvas pixel (x, y)
// is the viewing ray (a[x], b[y], c[x]) of two caller tables -- cylinder, sphere or plane is the caller's choice of tables, no
// trigonometry runs here -- and frame k's matrix takes the ray to homogeneous frame pixels as it is.  A ray and its antipode meet
// the same frame pixel: only tw > 0, the ray in front of the camera, is covered (NaN fails the comparison).
// The sampling is warp_sample's, piece by piece, handed the point (a, 1) and the map {A0, A1*b, A2*c; ...}: (a0*X + a1*Y) + a2 is then
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
  const SamplePos P = sample_position(M, a, 1.0);
  if (!(P.tw > 0.0) || !sample_covered(P, sw, sh)) return false;
  sample_taps(src, img, (int)P.U, (int)P.V, v);
  return true;
}

// A covered position's distance to the nearest frame edge, in 1/32 pixels: U and V lie inside the frame, every difference is >= 0.
__device__ __forceinline__ int edge_distance(const SamplePos& P, int sw, int sh) {
  const int u = (int)P.U, v = (int)P.V;
  return min(min(u, 32 * (sw - 1) - u), min(v, 32 * (sh - 1) - v));
}

// where the canvas pixels of a blend are: the plane entry's matrices and origin, or the ray entry's tables (col != NULL)
struct BlendGeo { const double* M; int inverse_map, ox, oy; const double* col; const double* row; };
