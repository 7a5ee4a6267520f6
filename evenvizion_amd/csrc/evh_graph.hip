// evh_graph.hip -- evh_graph_normal: the normal equations of one joint least-squares problem over all superposed matrices,
// from match rows of arbitrary frame pairs ("edges").  include/evhip.h states the arithmetic; tests/graph_checks.py restates it.
//
// One workgroup of 256 threads per edge.  Every entry of the 154 sums is (plus or minus) one or two sums of w times a product
// of coordinates, and only 86 such products are distinct:
//   moments   w U^a V^b, a + b <= 4, of the point in frame i, and the same of the point in frame j        15 + 15
//   cross     w p_a(P_i) p_b(P_j), p = (1, U, V, UU, UV, VV), without (UU, YY) and (VV, XX)               34
//   gradient  w ru p_a and w rv p_a for either point, a over the five monomials its Jacobian row holds    20
//   cost      rho and q                                                                                     2
// A lane keeps them in registers while it walks its rows r = tid, tid + 256, ...; they are added over the 64 lanes of a wave
// with shuffles, over the four waves in LDS in wave order, and expanded to the 154 by a table at the final store.  No atomics:
// the order of every addition is fixed by the row index alone, so an edge's sums are a pure function of that edge's inputs.
#include "evh_devmath.h"
#include "evh_internal.h"

namespace {

constexpr int NT = 256, NWAVES = NT / 64;
constexpr int EVH_GRAPH_MAX_EDGES = 1 << 22;     // 2^22 workgroups of 256 threads: 2^30 threads in the grid

// ---- accumulator slots -----------------------------------------------------------------------------------------------------------
// monomial index of a point: 0 -> 1, 1 -> U, 2 -> V, 3 -> UU, 4 -> UV, 5 -> VV
constexpr __host__ __device__ int mom(int a, int b) { return (a + b) * (a + b + 1) / 2 + b; }   // U^a V^b, a + b <= 4 -> 0..14
constexpr int MI = 0, MJ = 15, IJ = 30, GIU = 64, GIV = 69, GJU = 74, GJV = 79, RHO = 84, QQ = 85, NACC = 86;
// the slot of the cross product (a, b) among the 34 that are used: row-major without (3, 5) and (5, 3)
constexpr __host__ __device__ int ij(int a, int b) { return IJ + 6 * a + b - (6 * a + b > 23) - (6 * a + b > 33); }
// the slot of monomial a among the five a gradient's u part (0..4) and v part (0, 1, 2, 4, 5) hold
constexpr __host__ __device__ int gu(int a) { return a; }
constexpr __host__ __device__ int gv(int a) { return a < 3 ? a : a - 1; }
constexpr __host__ __device__ int exp_u(int a) { return a == 3 ? 2 : (a == 1 || a == 4) ? 1 : 0; }   // power of U in monomial a
constexpr __host__ __device__ int exp_v(int a) { return a == 5 ? 2 : (a == 2 || a == 4) ? 1 : 0; }
// the Jacobian rows as signed monomials: Ju = (U, V, 1, 0, 0, 0, -UU, -UV), Jv = (0, 0, 0, U, V, 1, -UV, -VV)
constexpr int JU_IDX[8] = {1, 2, 0, -1, -1, -1, 3, 4}, JV_IDX[8] = {-1, -1, -1, 1, 2, 0, 4, 5};
constexpr int J_SIGN[8] = {1, 1, 1, 1, 1, 1, -1, -1};

struct Entry { int8_t n, sign; uint8_t a[2]; };          // sums[k] = sign * (tot[a[0]] (+ tot[a[1]])), n = 0: structurally zero
struct Table { Entry e[EVH_GRAPH_NSUMS]; };

constexpr void add_term(Entry& t, int sign, int slot) {
  t.sign = (int8_t)sign;
  t.a[t.n] = (uint8_t)slot;
  t.n = (int8_t)(t.n + 1);
}

constexpr Table make_table() {
  Table T{};
  for (int k = 0; k < EVH_GRAPH_NSUMS; k++) T.e[k] = Entry{0, 1, {0, 0}};
  for (int comp = 0; comp < 2; comp++) {
    const int* idx = comp ? JV_IDX : JU_IDX;
    int at = 0;
    for (int r = 0; r < 8; r++)
      for (int c = r; c < 8; c++, at++) {
        if (idx[r] < 0 || idx[c] < 0) continue;
        const int m = mom(exp_u(idx[r]) + exp_u(idx[c]), exp_v(idx[r]) + exp_v(idx[c]));
        add_term(T.e[at], J_SIGN[r] * J_SIGN[c], MI + m);            // A_ii, upper triangle
        add_term(T.e[36 + at], J_SIGN[r] * J_SIGN[c], MJ + m);       // A_jj: J_j = -J(P_j), the two signs cancel
      }
    for (int r = 0; r < 8; r++)
      for (int c = 0; c < 8; c++)
        if (idx[r] >= 0 && idx[c] >= 0) add_term(T.e[72 + 8 * r + c], -J_SIGN[r] * J_SIGN[c], ij(idx[r], idx[c]));
    for (int r = 0; r < 8; r++)
      if (idx[r] >= 0) {
        add_term(T.e[136 + r], J_SIGN[r], comp ? GIV + gv(idx[r]) : GIU + gu(idx[r]));
        add_term(T.e[144 + r], -J_SIGN[r], comp ? GJV + gv(idx[r]) : GJU + gu(idx[r]));
      }
  }
  add_term(T.e[152], 1, RHO);
  add_term(T.e[153], 1, QQ);
  return T;
}
__device__ const Table g_table = make_table();

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__global__ __launch_bounds__(NT) void k_graph_normal(const double* __restrict__ S, int nframes, const int32_t* __restrict__ edges,
                                                     const float4* __restrict__ rows, int row_cap, const int32_t* __restrict__ counts,
                                                     const int32_t* __restrict__ status, const double* __restrict__ Hedge, double thr2,
                                                     double delta, double* __restrict__ sums, int32_t* __restrict__ info) {
  __shared__ double part[NWAVES][NACC];
  __shared__ double tot[NACC];
  __shared__ int cnt[NWAVES][3];
  const int e = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int fi = edges[2 * (int64_t)e], fj = edges[2 * (int64_t)e + 1];
  int flags = 0;
  if (fi < 0 || fi >= nframes || fj < 0 || fj >= nframes || fi == fj) flags |= EVH_GRAPH_BAD_INDEX;
  if (status && status[e] != EVH_PAIR_OK) flags |= EVH_GRAPH_BAD_STATUS;
  double* out = sums + (int64_t)e * EVH_GRAPH_NSUMS;
  if (flags) {                                               // uniform: the whole workgroup leaves, no row is read
    if (tid < EVH_GRAPH_NSUMS) out[tid] = 0.0;
    if (tid < 4) info[4 * (int64_t)e + tid] = tid == 3 ? flags : 0;
    return;
  }
  const int n = min(max(counts[e], 0), row_cap);
  const double* Si = S + 9 * (int64_t)fi;
  const double* Sj = S + 9 * (int64_t)fj;
  const double* He = Hedge ? Hedge + 9 * (int64_t)e : nullptr;
  const float4* my = rows + (int64_t)e * row_cap;
  const double d2 = delta * delta, twod = 2.0 * delta;

  double acc[NACC];
#pragma unroll
  for (int s = 0; s < NACC; s++) acc[s] = 0.0;
  int used = 0, gated = 0, behind = 0;

  for (int r = tid; r < n; r += NT) {
    const float4 row = my[r];
    const double ax = (double)row.x, ay = (double)row.y, bx = (double)row.z, by = (double)row.w;
    double tx, ty, tw, sx, sy, sw;
    hdot(Si, ax, ay, &tx, &ty, &tw);
    hdot(Sj, bx, by, &sx, &sy, &sw);
    if (!(isfinite(tw) && tw > 0.0 && isfinite(sw) && sw > 0.0)) { behind++; continue; }
    if (He) {
      double hx, hy, hw;
      hdot(He, ax, ay, &hx, &hy, &hw);
      const double gx = hx / hw - bx, gy = hy / hw - by;
      if (!(gx * gx + gy * gy <= thr2)) { gated++; continue; }
    }
    used++;
    const double U = tx / tw, V = ty / tw, X = sx / sw, Y = sy / sw;
    const double ru = U - X, rv = V - Y;
    const double q = ru * ru + rv * rv;
    double w = 1.0, rho = q;
    if (delta > 0.0 && !(q <= d2)) {
      const double s = sqrt(q);
      w = delta / s;
      rho = twod * s - d2;
    }
    acc[RHO] += rho;
    acc[QQ] += q;
    const double p[6] = {1.0, U, V, U * U, U * V, V * V}, pj[6] = {1.0, X, Y, X * X, X * Y, Y * Y};
    double wp[6], wq[6];
    wp[0] = wq[0] = w;
#pragma unroll
    for (int a = 1; a < 6; a++) { wp[a] = w * p[a]; wq[a] = w * pj[a]; }
    // moments: degree <= 2 are the wp themselves, degree 3 and 4 one more factor each
#pragma unroll
    for (int a = 0; a < 6; a++) {
      acc[MI + mom(exp_u(a), exp_v(a))] += wp[a];
      acc[MJ + mom(exp_u(a), exp_v(a))] += wq[a];
    }
    acc[MI + mom(3, 0)] += wp[3] * U;     acc[MJ + mom(3, 0)] += wq[3] * X;
    acc[MI + mom(2, 1)] += wp[3] * V;     acc[MJ + mom(2, 1)] += wq[3] * Y;
    acc[MI + mom(1, 2)] += wp[5] * U;     acc[MJ + mom(1, 2)] += wq[5] * X;
    acc[MI + mom(0, 3)] += wp[5] * V;     acc[MJ + mom(0, 3)] += wq[5] * Y;
    acc[MI + mom(4, 0)] += wp[3] * p[3];  acc[MJ + mom(4, 0)] += wq[3] * pj[3];
    acc[MI + mom(3, 1)] += wp[3] * p[4];  acc[MJ + mom(3, 1)] += wq[3] * pj[4];
    acc[MI + mom(2, 2)] += wp[4] * p[4];  acc[MJ + mom(2, 2)] += wq[4] * pj[4];
    acc[MI + mom(1, 3)] += wp[4] * p[5];  acc[MJ + mom(1, 3)] += wq[4] * pj[5];
    acc[MI + mom(0, 4)] += wp[5] * p[5];  acc[MJ + mom(0, 4)] += wq[5] * pj[5];
    // cross products; (UU, YY) and (VV, XX) appear in no entry
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = 0; b < 6; b++)
        if (!((a == 3 && b == 5) || (a == 5 && b == 3))) acc[ij(a, b)] += wp[a] * pj[b];
    // gradients: Ju holds the monomials 0..4, Jv the monomials 0, 1, 2, 4, 5
    const double wru = w * ru, wrv = w * rv;
#pragma unroll
    for (int a = 0; a < 6; a++) {
      if (a != 5) { acc[GIU + gu(a)] += wru * p[a]; acc[GJU + gu(a)] += wru * pj[a]; }
      if (a != 3) { acc[GIV + gv(a)] += wrv * p[a]; acc[GJV + gv(a)] += wrv * pj[a]; }
    }
  }

#pragma unroll
  for (int s = 0; s < NACC; s++) {
    const double v = wave_sum(acc[s]);
    if (lane == 0) part[wave][s] = v;
  }
  used = wave_sum(used); gated = wave_sum(gated); behind = wave_sum(behind);
  if (lane == 0) { cnt[wave][0] = used; cnt[wave][1] = gated; cnt[wave][2] = behind; }
  __syncthreads();
  if (tid < NACC) tot[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
  __syncthreads();
  if (tid < EVH_GRAPH_NSUMS) {
    const Entry t = g_table.e[tid];
    double v = 0.0;
    if (t.n >= 1) v = tot[t.a[0]];
    if (t.n == 2) v = v + tot[t.a[1]];
    out[tid] = t.sign < 0 ? 0.0 - v : v;                       // 0.0 - 0.0 = +0.0: an edge without rows stores +0.0 everywhere
  }
  if (tid < 3) info[4 * (int64_t)e + tid] = ((cnt[0][tid] + cnt[1][tid]) + cnt[2][tid]) + cnt[3][tid];
  if (tid == 3) info[4 * (int64_t)e + 3] = 0;
}

bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

int evh_graph_normal(evh_ctx* c, const double* d_S, int nframes, const int32_t* d_edges, int nedges, const float* d_rows, int row_cap,
                     const int32_t* d_counts, const int32_t* d_status, const double* d_H_edge, double inlier_thr, double huber_delta,
                     double* d_sums, int32_t* d_info) {
  const std::string W = "evh_graph_normal: ";
  if (!c) return EVH_ERR_INVALID;
  if (!d_S || !d_edges || !d_rows || !d_counts || !d_sums || !d_info) return evh_fail(c, EVH_ERR_INVALID, W + "a required pointer is NULL");
  if (nframes < 1 || nedges < 1 || row_cap < 1) return evh_fail(c, EVH_ERR_INVALID, W + "nframes, nedges and row_cap must be at least 1");
  if (nedges > EVH_GRAPH_MAX_EDGES) return evh_fail(c, EVH_ERR_INVALID, W + "more than 4 194 304 edges in one call");
  if (inlier_thr != inlier_thr || huber_delta != huber_delta) return evh_fail(c, EVH_ERR_INVALID, W + "inlier_thr or huber_delta is NaN");
  if (d_H_edge && inlier_thr < 0) return evh_fail(c, EVH_ERR_INVALID, W + "d_H_edge given with a negative inlier_thr");
  if (!aligned(d_rows, 16) || !aligned(d_S, 8) || !aligned(d_H_edge, 8) || !aligned(d_sums, 8) || !aligned(d_edges, 4) ||
      !aligned(d_counts, 4) || !aligned(d_status, 4) || !aligned(d_info, 4))
    return evh_fail(c, EVH_ERR_INVALID, W + "d_rows must be 16-byte aligned, the other buffers to their element size");
  hipLaunchKernelGGL(k_graph_normal, dim3(nedges), dim3(NT), 0, c->stream, d_S, nframes, d_edges, reinterpret_cast<const float4*>(d_rows),
                     row_cap, d_counts, d_status, d_H_edge, inlier_thr * inlier_thr, huber_delta, d_sums, d_info);
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}
