// evh_track.hip -- points followed from frame to frame where descriptors find nothing to match: evh_track_points (sparse pyramidal
// Lucas-Kanade in integers) and evh_track_seeds (the best-conditioned pixel of every cell), each also on decoded 4:2:0 planes.
// include/evhip.h states the arithmetic, tests/track_checks.py restates it; every result is a pure function of the inputs: the
// sums are integers (any order of addition is right), the 2x2 solve is the same double operations on every lane, and the rows
// are compacted by ballots in input order.  Kernels first, then per entry its arguments, check() -- every refusal comes before
// anything is enqueued -- and launch().
#include "evh_frame_checks.h"
#include "evh_internal.h"
#include "evh_pixels.h"
#include <cmath>
#include <type_traits>

namespace {

template <int CN> __device__ __forceinline__ int gray_value(const int (&v)[3]) { return CN == 3 ? gray_of(v[0], v[1], v[2]) : v[0]; }

// The gray pyramid of one frame: level l at off[l], rows of w[l] bytes; nlev = the levels that exist (a side < 2 ends them).
struct TrackPyr { int nlev; int w[EVH_TRACK_MAX_LEVELS], h[EVH_TRACK_MAX_LEVELS]; int64_t off[EVH_TRACK_MAX_LEVELS]; int64_t frame_bytes; };
#define PYR_TILE 32      // level-0 pixels a workgroup reduces: 16 x 16 at level 1, 8 x 8 at level 2, 4 x 4 at level 3

// Every level of every frame in one launch: a workgroup owns a PYR_TILE^2 tile of level 0, a thread its 2 x 2 pixels -- converted
// (planes) and weighted to gray as they are read -- and their mean; levels 2 and 3 come from LDS.  A 2^l x 2^l block of level-0
// pixels lies inside one tile, and a pixel of level l exists only where the whole block does (w >> l), so pixels a tile holds past
// the frame's edge feed nothing that is stored.
template <int CN, class SRC>
__global__ __launch_bounds__(256) void k_track_pyramid(SRC src, int w, int h, TrackPyr P, unsigned tiles_x, int frame0,
                                                       uint8_t* __restrict__ pyr) {
  __shared__ uint8_t L1[16][16], L2[8][8];
  const unsigned frame = (unsigned)frame0 + blockIdx.y, tile = blockIdx.x;       // grid = (tile, frame)
  const int ty0 = (int)(tile / tiles_x) * PYR_TILE, tx0 = (int)(tile % tiles_x) * PYR_TILE;
  const int t = threadIdx.x, lx = t & 15, ly = t >> 4;
  const int x = tx0 + 2 * lx, y = ty0 + 2 * ly;
  uint8_t* out = pyr + (int64_t)frame * P.frame_bytes;
  int g[2][2] = {{0, 0}, {0, 0}};
#pragma unroll
  for (int dy = 0; dy < 2; dy++) {
    if (y + dy >= h) continue;
    const typename SRC::Row row = src.row((int)frame, y + dy);
#pragma unroll
    for (int dx = 0; dx < 2; dx++) {
      if (x + dx >= w) continue;
      int v[3] = {0, 0, 0};
      row.px(x + dx, v);
      g[dy][dx] = gray_value<CN>(v);
      out[(int64_t)(y + dy) * w + (x + dx)] = (uint8_t)g[dy][dx];
    }
  }
  const int m1 = (g[0][0] + g[0][1] + g[1][0] + g[1][1] + 2) >> 2;
  L1[ly][lx] = (uint8_t)m1;
  if (P.nlev > 1 && (x >> 1) < P.w[1] && (y >> 1) < P.h[1]) out[P.off[1] + (int64_t)(y >> 1) * P.w[1] + (x >> 1)] = (uint8_t)m1;
  __syncthreads();
  if (P.nlev > 2 && t < 64) {
    const int qx = t & 7, qy = t >> 3, X = (tx0 >> 2) + qx, Y = (ty0 >> 2) + qy;
    const int m2 = (L1[2 * qy][2 * qx] + L1[2 * qy][2 * qx + 1] + L1[2 * qy + 1][2 * qx] + L1[2 * qy + 1][2 * qx + 1] + 2) >> 2;
    L2[qy][qx] = (uint8_t)m2;
    if (X < P.w[2] && Y < P.h[2]) out[P.off[2] + (int64_t)Y * P.w[2] + X] = (uint8_t)m2;
  }
  __syncthreads();
  if (P.nlev > 3 && t < 16) {
    const int qx = t & 3, qy = t >> 2, X = (tx0 >> 3) + qx, Y = (ty0 >> 3) + qy;
    const int m3 = (L2[2 * qy][2 * qx] + L2[2 * qy][2 * qx + 1] + L2[2 * qy + 1][2 * qx] + L2[2 * qy + 1][2 * qx + 1] + 2) >> 2;
    if (X < P.w[3] && Y < P.h[3]) out[P.off[3] + (int64_t)Y * P.w[3] + X] = (uint8_t)m3;
  }
}

// S(img, X, Y): the un-shifted bilinear sum at a position in 1/32 pixels; the caller has checked that it is defined, and a tap
// of weight 0 is not read (the position may sit on the last column or row).
__device__ __forceinline__ int level_sample(const uint8_t* __restrict__ img, int w, int X, int Y) {
  const int x = X >> 5, fx = X & 31, y = Y >> 5, fy = Y & 31;
  const uint8_t* r0 = img + (int64_t)y * w + x;
  int p00 = r0[0], p01 = 0, p10 = 0, p11 = 0;
  if (fx) p01 = r0[1];
  if (fy) {
    p10 = r0[w];
    if (fx) p11 = r0[w + 1];
  }
  return p00 * ((32 - fx) * (32 - fy)) + p01 * (fx * (32 - fy)) + p10 * ((32 - fx) * fy) + p11 * (fx * fy);
}
// is the (2*reach+1)^2 window of whole-pixel offsets around (X, Y) defined on a w x h level?
__device__ __forceinline__ bool window_inside(int w, int h, int X, int Y, int reach) {
  return X - 32 * reach >= 0 && X + 32 * reach <= 32 * (w - 1) && Y - 32 * reach >= 0 && Y + 32 * reach <= 32 * (h - 1);
}
// integers: any order of addition gives the sum; every lane ends with it
__device__ __forceinline__ long long wave_total(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ int level_down(int P) { return (P - 16) >> 1; }
__device__ __forceinline__ int level_up(int P) { return 2 * P + 16; }

struct TrackParams { int radius, iters, fb_max32; double eig_bar; long long err_bar; };

// One level, by one wave (the workgroup): the template with its halo goes to T, the gradient pairs of the window to G -- a lane
// keeps the window samples lane, lane + 64, ... and reads back only its own pairs --, then up to `iters` steps.  Everything that
// decides the control flow is the same on all lanes, so the barriers are met by the whole wave.  A level that fails leaves
// (Bx, By) as it got them.
__device__ int level_run(const uint8_t* __restrict__ tmpl, const uint8_t* __restrict__ search, int w, int h, int Ax, int Ay,
                         int& Bx, int& By, int r, int iters, bool level0, double eig_bar, unsigned& err, int* T, int* G, int lane) {
  if (!window_inside(w, h, Ax, Ay, r + 1)) return EVH_TRACK_NO_WINDOW;
  const int side = 2 * r + 3, win = 2 * r + 1, n = win * win;
  __syncthreads();                                     // the level or pass before this one has read T for the last time
  for (int idx = lane; idx < side * side; idx += 64) {
    const int j = idx / side, i = idx - j * side;
    T[idx] = level_sample(tmpl, w, Ax + 32 * (i - r - 1), Ay + 32 * (j - r - 1));
  }
  __syncthreads();
  long long gxx = 0, gxy = 0, gyy = 0;
  for (int idx = lane; idx < n; idx += 64) {
    const int j = idx / win, i = idx - j * win, at = (j + 1) * side + (i + 1);
    const int gx = T[at + 1] - T[at - 1], gy = T[at + side] - T[at - side];
    G[2 * idx] = gx; G[2 * idx + 1] = gy;
    gxx += (long long)gx * gx; gxy += (long long)gx * gy; gyy += (long long)gy * gy;
  }
  const double a = (double)wave_total(gxx), b = (double)wave_total(gxy), c = (double)wave_total(gyy);
  const double det = a * c - b * b;
  if (!(det > 0.0)) return EVH_TRACK_FLAT;
  if (level0) {
    const double dd = a - c;
    if (((a + c) - sqrt(dd * dd + 4.0 * (b * b))) * 0.5 < eig_bar) return EVH_TRACK_FLAT;
  }
  int bx = Bx, by = By;
  const double reach = 32.0 * (double)r;
  for (int k = 0;; k++) {
    if (!window_inside(w, h, bx, by, r)) return EVH_TRACK_LEFT_FRAME;
    long long sx = 0, sy = 0, se = 0;
    for (int idx = lane; idx < n; idx += 64) {
      const int j = idx / win, i = idx - j * win;
      const int d = level_sample(search, w, bx + 32 * (i - r), by + 32 * (j - r)) - T[(j + 1) * side + (i + 1)];
      sx += (long long)d * G[2 * idx]; sy += (long long)d * G[2 * idx + 1]; se += d < 0 ? -d : d;
    }
    sx = wave_total(sx); sy = wave_total(sy); se = wave_total(se);
    err = (unsigned)se;
    if (k == iters) break;
    const double fx = (double)sx, fy = (double)sy;
    const double dx = (c * fx - b * fy) / det, dy = (a * fy - b * fx) / det;
    const int stx = (int)fmin(fmax(rint(-64.0 * dx), -reach), reach), sty = (int)fmin(fmax(rint(-64.0 * dy), -reach), reach);
    if (stx == 0 && sty == 0) break;
    bx += stx; by += sty;
  }
  Bx = bx; By = by;
  return EVH_TRACK_TRACKED;
}

// The template around (A0x, A0y) of frame `tp` followed into frame `sp` from the guess (Bx, By): the guess goes down to the top
// level once and is carried up, the template's position comes from A0 at every level; only level 0 decides the flag.
__device__ int track_run(const uint8_t* __restrict__ tp, const uint8_t* __restrict__ sp, const TrackPyr& P, int A0x, int A0y, int& Bx,
                         int& By, const TrackParams& K, unsigned& err, int* T, int* G, int lane) {
  const int top = P.nlev - 1;
  int bx = Bx, by = By;
  for (int l = 0; l < top; l++) { bx = level_down(bx); by = level_down(by); }
  for (int l = top; l >= 1; l--) {
    int ax = A0x, ay = A0y;
    for (int t = 0; t < l; t++) { ax = level_down(ax); ay = level_down(ay); }
    unsigned e;
    level_run(tp + P.off[l], sp + P.off[l], P.w[l], P.h[l], ax, ay, bx, by, K.radius, K.iters, false, 0.0, e, T, G, lane);
    bx = level_up(bx); by = level_up(by);
  }
  const int flag = level_run(tp, sp, P.w[0], P.h[0], A0x, A0y, bx, by, K.radius, K.iters, true, K.eig_bar, err, T, G, lane);
  if (flag == EVH_TRACK_TRACKED) { Bx = bx; By = by; }
  return flag;
}

// A0 of a point, false = EVH_TRACK_BAD_POINT
__device__ __forceinline__ bool track_start(const float* __restrict__ pt, int w, int h, int& A0x, int& A0y) {
  const double x = (double)pt[0], y = (double)pt[1];
  const double ax = rint(32.0 * x), ay = rint(32.0 * y);
  if (!(ax >= 0.0 && ax <= (double)(32 * (w - 1)) && ay >= 0.0 && ay <= (double)(32 * (h - 1)))) return false;   // NaN, +-inf fail
  A0x = (int)ax; A0y = (int)ay;
  return true;
}

// grid = (point, pair), one wave per point: the forward pass, the error bar, the backward pass.  Lane 0 leaves (flag, Bx, By,
// err) in the workspace; k_track_compact writes the outputs from there.
__global__ __launch_bounds__(64) void k_track_points(const uint8_t* __restrict__ pyr, TrackPyr P, int frame_step,
                                                     const float* __restrict__ pts, const int32_t* __restrict__ npts, int pt_cap,
                                                     const double* __restrict__ M, TrackParams K, int4* __restrict__ ws) {
  extern __shared__ int lds[];
  const int p = blockIdx.y, q = blockIdx.x, lane = threadIdx.x;
  if (q >= min(max(npts[p], 0), pt_cap)) return;
  int* T = lds;
  int* G = lds + (2 * K.radius + 3) * (2 * K.radius + 3);
  const uint8_t* prev = pyr + (int64_t)p * frame_step * P.frame_bytes;
  const uint8_t* cur = prev + P.frame_bytes;
  const int64_t at = (int64_t)p * pt_cap + q;
  int A0x = 0, A0y = 0, Bx = 0, By = 0, flag = EVH_TRACK_BAD_POINT;
  unsigned err = EVH_TRACK_NO_ERR;
  if (track_start(pts + 2 * at, P.w[0], P.h[0], A0x, A0y)) {
    Bx = A0x; By = A0y;
    if (M) {                                                       // evh_warp_fixed_plane's position for A = d_M[p], inverse_map
      const double* A = M + 9 * (int64_t)p;
      const double X = (double)A0x / 32.0, Y = (double)A0y / 32.0;
      const double tx = (A[0] * X + A[1] * Y) + A[2], ty = (A[3] * X + A[4] * Y) + A[5], tw = (A[6] * X + A[7] * Y) + A[8];
      const double U = rint(tx / tw * 32.0), V = rint(ty / tw * 32.0);
      if (fabs(U) <= (double)EVH_TRACK_GUESS_MAX && fabs(V) <= (double)EVH_TRACK_GUESS_MAX) { Bx = (int)U; By = (int)V; }
    }
    flag = track_run(cur, prev, P, A0x, A0y, Bx, By, K, err, T, G, lane);
    if (flag != EVH_TRACK_TRACKED) err = EVH_TRACK_NO_ERR;
    else if (K.err_bar >= 0 && (long long)err > K.err_bar) flag = EVH_TRACK_HIGH_ERROR;
    else if (K.fb_max32 >= 0) {
      int ax = A0x, ay = A0y;
      unsigned e;
      const int back = track_run(prev, cur, P, Bx, By, ax, ay, K, e, T, G, lane);
      if (back != EVH_TRACK_TRACKED || max(abs(ax - A0x), abs(ay - A0y)) > K.fb_max32) flag = EVH_TRACK_FB_FAILED;
    }
  }
  if (lane == 0) ws[at] = make_int4(flag, Bx, By, (int)err);
}

// One workgroup per pair: flags and errors as they are, the kept points' rows moved up in input order -- per 256 points a ballot
// per wave, the waves' counts through LDS, a running offset; no atomics.
__global__ __launch_bounds__(256) void k_track_compact(const int4* __restrict__ ws, const float* __restrict__ pts,
                                                       const int32_t* __restrict__ npts, int pt_cap, int w, int h,
                                                       float* __restrict__ rows, int row_cap, int32_t* __restrict__ counts,
                                                       uint8_t* __restrict__ flags, uint32_t* __restrict__ errs) {
  __shared__ int wtot[4];
  const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int count = min(max(npts[p], 0), pt_cap);
  int running = 0;
  for (int base = 0; base < count; base += 256) {
    const int q = base + t;
    const int64_t at = (int64_t)p * pt_cap + q;
    int4 r = make_int4(EVH_TRACK_BAD_POINT, 0, 0, 0);
    if (q < count) {
      r = ws[at];
      if (flags) flags[at] = (uint8_t)r.x;
      if (errs) errs[at] = (uint32_t)r.w;
    }
    const bool keep = q < count && r.x == EVH_TRACK_TRACKED;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wtot[wv] = __popcll(m);
    __syncthreads();
    int off = running;
    for (int k = 0; k < wv; k++) off += wtot[k];
    if (keep) {
      int ax = 0, ay = 0;
      track_start(pts + 2 * at, w, h, ax, ay);
      const int64_t slot = (int64_t)p * row_cap + off + __popcll(m & ((1ull << lane) - 1ull));
      float* row = rows + 4 * slot;                      // scalar stores: the caller's rows need no more than a float's alignment
      row[0] = (float)ax / 32.0f; row[1] = (float)ay / 32.0f; row[2] = (float)r.y / 32.0f; row[3] = (float)r.z / 32.0f;
    }
    running += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (t == 0) counts[p] = running;
}

// ---- seeds ---------------------------------------------------------------------------------------------------------------------------
#define SEED_MAX_CELL 64
#define SEED_MAX_RADIUS 3
#define SEED_TILE (SEED_MAX_CELL + 2 * SEED_MAX_RADIUS + 2)     // gray with the halo of window and gradient
#define SEED_GRAD (SEED_MAX_CELL + 2 * SEED_MAX_RADIUS)        // gradients with the halo of the window

// the better of two candidates stays in (lam, idx): the larger lambda, of equals the lower raster index
__device__ __forceinline__ void seed_better(double& lam, int& idx, double lam2, int idx2) {
  const bool take = lam2 > lam || (lam2 == lam && idx2 < idx);
  lam = take ? lam2 : lam; idx = take ? idx2 : idx;
}

// grid = (cell, frame): the cell's gray with its halo to LDS, the doubled differences of the window's reach to LDS, then every
// pixel's three window sums (exact integers below 2^22), its lambda in double, and the arg-max -- ties to the lower raster index,
// whatever the order of the comparisons.  cells[frame][cell] = y << 16 | x of the kept seed, or -1.
template <int CN, class SRC>
__global__ __launch_bounds__(256) void k_track_seeds(SRC src, int w, int h, int radius, int cell, int border, double bar, int cells_x,
                                                     int32_t* __restrict__ cells) {
  __shared__ uint8_t tile[SEED_TILE * SEED_TILE];
  __shared__ short grad[2][SEED_GRAD * SEED_GRAD];
  __shared__ double best_lam[4];
  __shared__ int best_idx[4];
  const int t = threadIdx.x, frame = blockIdx.y;
  const int cy = (int)blockIdx.x / cells_x, cx = (int)blockIdx.x - cy * cells_x;
  const int x0 = border + cx * cell, y0 = border + cy * cell;
  const int cw = min(cell, w - border - x0), ch = min(cell, h - border - y0);
  const int tw = cw + 2 * radius + 2, th = ch + 2 * radius + 2, gw = cw + 2 * radius, gh = ch + 2 * radius;
  for (int idx = t; idx < tw * th; idx += 256) {          // border >= radius + 1: the halo lies inside the frame
    const int j = idx / tw, i = idx - j * tw;
    int v[3] = {0, 0, 0};
    src.row(frame, y0 - radius - 1 + j).px(x0 - radius - 1 + i, v);
    tile[j * tw + i] = (uint8_t)gray_value<CN>(v);
  }
  __syncthreads();
  for (int idx = t; idx < gw * gh; idx += 256) {
    const int j = idx / gw, i = idx - j * gw, at = (j + 1) * tw + (i + 1);
    grad[0][idx] = (short)((int)tile[at + 1] - (int)tile[at - 1]);
    grad[1][idx] = (short)((int)tile[at + tw] - (int)tile[at - tw]);
  }
  __syncthreads();
  double lam = -1.0;                                      // below every lambda that can be kept: a seed has lambda >= bar >= 0
  int best = 0x7fffffff;
  const int win = 2 * radius + 1;
  for (int idx = t; idx < cw * ch; idx += 256) {
    const int py = idx / cw, px = idx - py * cw;
    int gxx = 0, gxy = 0, gyy = 0;
    for (int j = 0; j < win; j++)
      for (int i = 0; i < win; i++) {
        const int gx = grad[0][(py + j) * gw + px + i], gy = grad[1][(py + j) * gw + px + i];
        gxx += gx * gx; gxy += gx * gy; gyy += gy * gy;
      }
    const double a = (double)gxx, b = (double)gxy, c = (double)gyy, dd = a - c;
    seed_better(lam, best, ((a + c) - sqrt(dd * dd + 4.0 * (b * b))) * 0.5, idx);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double lam2 = __shfl_xor(lam, m, 64);
    const int idx2 = __shfl_xor(best, m, 64);
    seed_better(lam, best, lam2, idx2);
  }
  if ((t & 63) == 0) { best_lam[t >> 6] = lam; best_idx[t >> 6] = best; }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 1; k < 4; k++) seed_better(lam, best, best_lam[k], best_idx[k]);
    const bool kept = best != 0x7fffffff && lam >= bar;
    const int py = kept ? best / cw : 0, px = kept ? best - py * cw : 0;
    cells[(int64_t)frame * gridDim.x + blockIdx.x] = kept ? ((y0 + py) << 16 | (x0 + px)) : -1;
  }
}

// One workgroup per frame: the kept cells in raster order, by the ballots of k_track_compact; the count is the full one.
__global__ __launch_bounds__(256) void k_seed_compact(const int32_t* __restrict__ cells, int ncells, float* __restrict__ pts, int pt_cap,
                                                      int32_t* __restrict__ npts) {
  __shared__ int wtot[4];
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int running = 0;
  for (int base = 0; base < ncells; base += 256) {
    const int q = base + t;
    const int v = q < ncells ? cells[(int64_t)f * ncells + q] : -1;
    const unsigned long long m = __ballot(v >= 0);
    if (lane == 0) wtot[wv] = __popcll(m);
    __syncthreads();
    int off = running;
    for (int k = 0; k < wv; k++) off += wtot[k];
    const int slot = off + __popcll(m & ((1ull << lane) - 1ull));
    if (v >= 0 && slot < pt_cap) {
      float* pt = pts + 2 * ((int64_t)f * pt_cap + slot);
      pt[0] = (float)(v & 0xffff); pt[1] = (float)(v >> 16);
    }
    running += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (t == 0) npts[f] = running;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
template <class Fn>
void with_source(const EvhFrames& F, Fn fn) {
  if (F.yuv) fn(std::integral_constant<int, 3>{}, yuv420_src(*F.yuv));
  else if (F.channels == 3) fn(std::integral_constant<int, 3>{}, packed_src(F));
  else fn(std::integral_constant<int, 1>{}, packed_src(F));
}
template <class Args>
int run(evh_ctx* c, const Args& A) {
  if (!c) return EVH_ERR_INVALID;
  if (int rc = check(c, A)) return rc;
  return A.idle() ? EVH_SUCCESS : launch(c, A);
}
TrackPyr pyramid_of(int w, int h, int levels) {
  TrackPyr P{};
  P.nlev = 1; P.w[0] = w; P.h[0] = h; P.off[0] = 0;
  int64_t bytes = (int64_t)w * h;
  for (int l = 1; l < levels && (P.w[l - 1] >> 1) >= 2 && (P.h[l - 1] >> 1) >= 2; l++) {
    P.w[l] = P.w[l - 1] >> 1; P.h[l] = P.h[l - 1] >> 1; P.off[l] = bytes;
    bytes += (int64_t)P.w[l] * P.h[l];
    P.nlev = l + 1;
  }
  P.frame_bytes = (bytes + 15) & ~(int64_t)15;
  return P;
}
// the size both entries stop at: positions in 1/32 pixel and the sums of a window stay well inside their integers
int check_frames(evh_ctx* c, const std::string& W, const EvhFrames& F, int w, int h) {
  if (w > EVH_TRACK_MAX_SIZE || h > EVH_TRACK_MAX_SIZE) return evh_fail(c, EVH_ERR_CAPACITY, W + "w and h stay within 4096");
  return EVH_SUCCESS;
}

// ---- evh_track_points ----
struct TrackArgs {
  const char* who; EvhFrames F; int npairs, frame_step, w, h; const float* pts; const int32_t* npts; int pt_cap; const double* M;
  int levels, radius, iters; double min_eig; int fb_max32, max_err; float* rows; int row_cap; int32_t* counts; uint8_t* flags;
  uint32_t* errs;
  bool idle() const { return npairs == 0; }
};
int check(evh_ctx* c, const TrackArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.pts || !A.npts || !A.rows || !A.counts) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (int rc = need_channels(c, W, A.F)) return rc;
  if (A.frame_step != 1 && A.frame_step != 2) return evh_fail(c, EVH_ERR_INVALID, W + "frame_step must be 1 or 2");
  if (A.npairs < 0 || A.w < 1 || A.h < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame or negative npairs");
  if (A.pt_cap < 1) return evh_fail(c, EVH_ERR_INVALID, W + "pt_cap must be at least 1");
  if (A.row_cap < A.pt_cap) return evh_fail(c, EVH_ERR_INVALID, W + "row_cap smaller than pt_cap");
  if (A.levels < 1 || A.levels > EVH_TRACK_MAX_LEVELS) return evh_fail(c, EVH_ERR_INVALID, W + "levels must lie in 1..4");
  if (A.radius < 1 || A.radius > EVH_TRACK_MAX_RADIUS) return evh_fail(c, EVH_ERR_INVALID, W + "radius must lie in 1..10");
  if (A.iters < 1 || A.iters > EVH_TRACK_MAX_ITERS) return evh_fail(c, EVH_ERR_INVALID, W + "iters must lie in 1..64");
  if (!(A.min_eig >= 0.0) || std::isinf(A.min_eig)) return evh_fail(c, EVH_ERR_INVALID, W + "min_eig must be finite and not negative");
  if (A.max_err < -1 || A.max_err > 255) return evh_fail(c, EVH_ERR_INVALID, W + "max_err must be -1 or lie in 0..255");
  if (int rc = check_frames(c, W, A.F, A.w, A.h)) return rc;
  if (A.npairs > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 pairs per call");
  if (A.pt_cap > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 points per pair");
  if (int rc = need_source_stride(c, W, A.F, A.w, A.h, true)) return rc;      // a pair takes two frames
  if (A.npairs == 0) return EVH_SUCCESS;
  const int64_t nframes = (int64_t)(A.npairs - 1) * A.frame_step + 2;
  if (A.F.yuv && nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  if (int rc = need_planes(c, A.who, A.F, nframes, A.w, A.h)) return rc;
  // the outputs apart from each other and from everything that is read
  const int64_t np = A.npairs;
  const Span outs[4] = {{A.rows, np * A.row_cap * 16, "d_out_rows"}, {A.counts, np * 4, "d_out_counts"},
                        {A.flags, np * A.pt_cap, "d_flags"}, {A.errs, np * A.pt_cap * 4, "d_err"}};
  Span src[3];
  source_spans(A.F, nframes, A.w, A.h, src);
  const Span ins[6] = {src[0], src[1], src[2], {A.pts, np * A.pt_cap * 8, "d_pts"}, {A.npts, np * 4, "d_npts"}, {A.M, np * 72, "d_M"}};
  return need_apart(c, W, outs, ins);
}
// the pyramids of every frame, the points, the compaction: three launches on one workspace
int launch(evh_ctx* c, const TrackArgs& A) {
  const TrackPyr P = pyramid_of(A.w, A.h, A.levels);
  const int64_t nframes = (int64_t)(A.npairs - 1) * A.frame_step + 2;
  const size_t pyr_bytes = (size_t)nframes * (size_t)P.frame_bytes;
  if (int rc = grow(c, &c->d_track_ws, &c->track_ws_bytes, pyr_bytes + (size_t)A.npairs * A.pt_cap * sizeof(int4))) return rc;
  uint8_t* pyr = reinterpret_cast<uint8_t*>(c->d_track_ws);
  int4* ws = reinterpret_cast<int4*>(c->d_track_ws + pyr_bytes);
  const unsigned tiles_x = (A.w + PYR_TILE - 1) / PYR_TILE, tiles = tiles_x * ((A.h + PYR_TILE - 1) / PYR_TILE);
  with_source(A.F, [&](auto cn, const auto& S) {
    for (int64_t f0 = 0; f0 < nframes; f0 += 65535)       // one launch, unless packed frames at frame_step 2 pass grid.y's range
      hipLaunchKernelGGL((k_track_pyramid<decltype(cn)::value, std::decay_t<decltype(S)>>),
                         dim3(tiles, (unsigned)std::min<int64_t>(65535, nframes - f0)), dim3(256), 0, c->stream, S, A.w, A.h, P, tiles_x,
                         (int)f0, pyr);
  });
  if (int rc = launched(c)) return rc;
  const int n = (2 * A.radius + 1) * (2 * A.radius + 1);
  const TrackParams K = {A.radius, A.iters, A.fb_max32, (A.min_eig * (double)n) * 4194304.0,
                         A.max_err < 0 ? -1ll : (long long)A.max_err * n * 1024};
  const size_t lds = ((size_t)(2 * A.radius + 3) * (2 * A.radius + 3) + 2 * (size_t)n) * sizeof(int);
  hipLaunchKernelGGL(k_track_points, dim3(A.pt_cap, A.npairs), dim3(64), lds, c->stream, pyr, P, A.frame_step, A.pts, A.npts, A.pt_cap,
                     A.M, K, ws);
  hipLaunchKernelGGL(k_track_compact, dim3(A.npairs), dim3(256), 0, c->stream, ws, A.pts, A.npts, A.pt_cap, A.w, A.h, A.rows, A.row_cap,
                     A.counts, A.flags, A.errs);
  return launched(c);
}

// ---- evh_track_seeds ----
struct SeedArgs {
  const char* who; EvhFrames F; int nframes, w, h, radius, cell, border; double min_eig; float* pts; int pt_cap; int32_t* npts;
  bool idle() const { return nframes == 0; }
};
int check(evh_ctx* c, const SeedArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.pts || !A.npts) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (int rc = need_channels(c, W, A.F)) return rc;
  if (A.nframes < 0 || A.w < 1 || A.h < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame or negative nframes");
  if (A.pt_cap < 1) return evh_fail(c, EVH_ERR_INVALID, W + "pt_cap must be at least 1");
  if (A.radius < 1 || A.radius > SEED_MAX_RADIUS) return evh_fail(c, EVH_ERR_INVALID, W + "radius must lie in 1..3");
  if (A.cell < 8 || A.cell > SEED_MAX_CELL) return evh_fail(c, EVH_ERR_INVALID, W + "cell must lie in 8..64");
  if (A.border < A.radius + 1) return evh_fail(c, EVH_ERR_INVALID, W + "border must be at least radius + 1");
  if (!(A.min_eig >= 0.0) || std::isinf(A.min_eig)) return evh_fail(c, EVH_ERR_INVALID, W + "min_eig must be finite and not negative");
  if (int rc = check_frames(c, W, A.F, A.w, A.h)) return rc;
  if (A.nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  if (A.pt_cap > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 points per frame");
  if (int rc = need_source_stride(c, W, A.F, A.w, A.h, A.nframes > 1)) return rc;
  if (A.nframes == 0) return EVH_SUCCESS;
  if (int rc = need_planes(c, A.who, A.F, A.nframes, A.w, A.h)) return rc;
  const int64_t nf = A.nframes;
  const Span outs[2] = {{A.pts, nf * A.pt_cap * 8, "d_pts"}, {A.npts, nf * 4, "d_npts"}};
  Span src[3];
  source_spans(A.F, nf, A.w, A.h, src);
  return need_apart(c, W, outs, src);
}
// the cells' arg-max, then the compaction; an empty rectangle only clears the counts
int launch(evh_ctx* c, const SeedArgs& A) {
  // [border, w - 1 - border] holds a pixel iff border <= (w - 1) / 2: compared this way because 2 * border need not fit an int
  if (A.border > (A.w - 1) / 2 || A.border > (A.h - 1) / 2) {
    EVH_HIP(c, hipMemsetAsync(A.npts, 0, (size_t)A.nframes * sizeof(int32_t), c->stream));
    return EVH_SUCCESS;
  }
  const int rw = A.w - 2 * A.border, rh = A.h - 2 * A.border;       // both >= 1 now
  const int cells_x = (rw + A.cell - 1) / A.cell, ncells = cells_x * ((rh + A.cell - 1) / A.cell);
  if (int rc = grow(c, &c->d_track_ws, &c->track_ws_bytes, (size_t)A.nframes * ncells * sizeof(int32_t))) return rc;
  int32_t* cells = reinterpret_cast<int32_t*>(c->d_track_ws);
  const int n = (2 * A.radius + 1) * (2 * A.radius + 1);
  const double bar = (A.min_eig * (double)n) * 4.0;
  with_source(A.F, [&](auto cn, const auto& S) {
    hipLaunchKernelGGL((k_track_seeds<decltype(cn)::value, std::decay_t<decltype(S)>>), dim3(ncells, A.nframes), dim3(256), 0, c->stream,
                       S, A.w, A.h, A.radius, A.cell, A.border, bar, cells_x, cells);
  });
  hipLaunchKernelGGL(k_seed_compact, dim3(A.nframes), dim3(256), 0, c->stream, cells, ncells, A.pts, A.pt_cap, A.npts);
  return launched(c);
}

}  // namespace

extern "C" {

int evh_track_points(evh_ctx* c, const uint8_t* d_frames, int npairs, int frame_step, int w, int h, int channels, int64_t row_stride,
                     int64_t frame_stride, const float* d_pts, const int32_t* d_npts, int pt_cap, const double* d_M, int levels,
                     int radius, int iters, double min_eig, int fb_max32, int max_err, float* d_out_rows, int row_cap,
                     int32_t* d_out_counts, uint8_t* d_flags, uint32_t* d_err) {
  return run(c, TrackArgs{"evh_track_points", packed_frames(d_frames, channels, row_stride, frame_stride), npairs, frame_step, w, h,
                          d_pts, d_npts, pt_cap, d_M, levels, radius, iters, min_eig, fb_max32, max_err, d_out_rows, row_cap,
                          d_out_counts, d_flags, d_err});
}

int evh_track_points_yuv420(evh_ctx* c, const evh_yuv420* src, int npairs, int frame_step, int w, int h, const float* d_pts,
                            const int32_t* d_npts, int pt_cap, const double* d_M, int levels, int radius, int iters, double min_eig,
                            int fb_max32, int max_err, float* d_out_rows, int row_cap, int32_t* d_out_counts, uint8_t* d_flags,
                            uint32_t* d_err) {
  return run(c, TrackArgs{"evh_track_points_yuv420", yuv420_frames(src), npairs, frame_step, w, h, d_pts, d_npts, pt_cap, d_M, levels,
                          radius, iters, min_eig, fb_max32, max_err, d_out_rows, row_cap, d_out_counts, d_flags, d_err});
}

int evh_track_seeds(evh_ctx* c, const uint8_t* d_frames, int nframes, int w, int h, int channels, int64_t row_stride,
                    int64_t frame_stride, int radius, int cell, int border, double min_eig, float* d_pts, int pt_cap, int32_t* d_npts) {
  return run(c, SeedArgs{"evh_track_seeds", packed_frames(d_frames, channels, row_stride, frame_stride), nframes, w, h, radius, cell,
                         border, min_eig, d_pts, pt_cap, d_npts});
}

int evh_track_seeds_yuv420(evh_ctx* c, const evh_yuv420* src, int nframes, int w, int h, int radius, int cell, int border,
                           double min_eig, float* d_pts, int pt_cap, int32_t* d_npts) {
  return run(c, SeedArgs{"evh_track_seeds_yuv420", yuv420_frames(src), nframes, w, h, radius, cell, border, min_eig, d_pts, pt_cap,
                         d_npts});
}

}  // extern "C"
