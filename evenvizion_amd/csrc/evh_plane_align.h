// evh_plane_align.h -- two frames, or a frame and the mosaic, compared where one maps onto the other: evh_pair_exposure,
// evh_pair_residual, evh_pair_refine and evh_canvas_refine, per product its kernels, arguments, check() and launch().
// Included by evh_plane.hip inside its unnamed namespace.

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
// taps and rounding -- with the count read beside each tap: a tap of non-zero weight whose count lies below min_cover makes the
// sample invalid (false; v is then of no use), a tap of weight 0 is neither read nor asked.  count == NULL: every pixel is valid.
// Unlike warp_sample, which leaves v alone when it returns false, a sample that fails on a count has its taps in v already: the counts
// are read beside the taps, and the one caller drops v.  (Holding the taps back until the counts are known is 58 to 92 instructions
// longer per instance.)
// No tap leaves the canvas (see sample_taps), so no count read does.
__device__ __forceinline__ bool canvas_sample(const PackedSrc& canvas, const uint8_t* __restrict__ count, int64_t count_stride,
                                              int min_cover, const WarpMap& A, double X, double Y, int dw, int dh, int (&v)[3]) {
  const SamplePos P = sample_position(A, X, Y);
  if (!sample_covered(P, dw, dh)) return false;
  const int u = (int)P.U, w = (int)P.V;
  int lowest = 255;                                       // the smallest count under a tap of non-zero weight
  const uint8_t* c0 = count ? count + (int64_t)(w >> 5) * count_stride + (u >> 5) : nullptr;
  sample_taps(canvas, 0, u, w, v, [&](int dx, int dy) {
    if (count) lowest = min(lowest, (int)c0[dy * count_stride + dx]);
  });
  return lowest >= min_cover || !count;
}
// grid.y = frame; the runs, the accumulation, the tree and the partial sums are k_pair_refine_eval's for the same w, h (the frame is
// the current frame there, the canvas the previous one), so k_pair_refine_step adds and judges them as they are.  The body stays
// written out a second time: folded onto one body templated on the sampler (same registers, no spills, bytes equal),
// k_pair_refine_eval<3, Yuv420Src> took 2.0 to 2.2 % longer per call on the GPU, so the copy stays (profiles/plane_second_fold.txt).
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

// ---- what the two refinements share on the host ----------------------------------------------------------------------------------------
// iters, clip, the count threshold where there is a count plane (evh_canvas_refine) and the frame's size, in the order both entries
// have always asked them.  The Jacobian's entries are exact in double up to EVH_REFINE_MAX_SIZE; the bound also keeps w, h below 2^26
// and w * h below INT_MAX.
int need_refine_bounds(evh_ctx* c, const std::string& W, int iters, int clip, const uint8_t* count, int min_cover, int w, int h) {
  if (iters < 0 || iters > EVH_REFINE_MAX_ITERS) return evh_fail(c, EVH_ERR_INVALID, W + "iters must lie in 0..64");
  if (clip < 0 || clip > 255) return evh_fail(c, EVH_ERR_INVALID, W + "clip must lie in 0..255");
  if (count && (min_cover < 1 || min_cover > 255)) return evh_fail(c, EVH_ERR_INVALID, W + "min_cover must lie in 1..255");
  if (w > EVH_REFINE_MAX_SIZE || h > EVH_REFINE_MAX_SIZE) return evh_fail(c, EVH_ERR_CAPACITY, W + "w and h stay within 4096");
  return EVH_SUCCESS;
}
// the outputs of n matrices apart from each other, from everything that is read and from d_M_in, which d_M_out may only BE
template <int NI>
int need_refine_outputs(evh_ctx* c, const std::string& W, int64_t n, const double* M_in, double* M_out, uint64_t* info, double* normal,
                        const Span (&ins)[NI]) {
  const Span outs[3] = {{M_out, n * 72, "d_M_out"}, {info, n * EVH_REFINE_NINFO * 8, "d_info"}, {normal, n * EVH_REFINE_NSUMS * 8, "d_normal"}};
  if (int rc = need_apart(c, W, outs, ins)) return rc;
  const Span in{M_in, n * 72, "d_M_in"};
  for (int i = M_out == M_in ? 1 : 0; i < 3; i++)
    if (meet(outs[i], in)) return evh_fail(c, EVH_ERR_INVALID, W + outs[i].name + " overlaps d_M_in");
  return EVH_SUCCESS;
}
// workgroups per matrix: one per 1024 runs, at most 64 -- a function of w and h only (it fixes the order of summation)
int refine_groups(const Runs& R) { return (int)std::min(64u, std::max(1u, (R.n + 1023u) / 1024u)); }
// The refinement of n matrices on frames of w x h: the workspace grown, then iters + 1 rounds of an evaluation and
// k_pair_refine_step, the first evaluation at d_M_in (M != NULL), the others at the state's trial.  eval(grid, M, state, part, R)
// launches the caller's evaluation kernel.
template <class Eval>
int refine_rounds(evh_ctx* c, int n, int w, int h, const double* M_in, int iters, double* M_out, uint64_t* info, double* normal, Eval eval) {
  const Runs R = runs_of(w, h);
  const int groups = refine_groups(R);
  const size_t state_bytes = ((size_t)n * sizeof(RefineState) + 255) & ~(size_t)255;
  if (int rc = grow(c, &c->d_refine_ws, &c->refine_ws_bytes, state_bytes + (size_t)n * groups * REFINE_SLOTS * sizeof(double))) return rc;
  RefineState* state = reinterpret_cast<RefineState*>(c->d_refine_ws);
  double* part = reinterpret_cast<double*>(c->d_refine_ws + state_bytes);
  for (int k = 0; k <= iters; k++) {
    eval(dim3(groups, n), k == 0 ? M_in : nullptr, state, part, R);
    hipLaunchKernelGGL(k_pair_refine_step, dim3(n), dim3(64), 0, c->stream, state, part, groups, k == 0, k == iters, w, h, M_in, M_out,
                       reinterpret_cast<unsigned long long*>(info), normal);
    if (int rc = launched(c)) return rc;
  }
  return EVH_SUCCESS;
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
  if (int rc = need_refine_bounds(c, W, A.iters, A.clip, nullptr, 0, A.w, A.h)) return rc;
  if (A.npairs > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 pairs per call");
  if (int rc = need_source_stride(c, W, A.F, A.w, A.h, true)) return rc;      // a pair takes two frames
  if (A.npairs == 0) return EVH_SUCCESS;
  const int64_t nframes = (int64_t)(A.npairs - 1) * A.frame_step + 2;
  if (A.F.yuv && nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  if (int rc = need_planes(c, A.who, A.F, nframes, A.w, A.h)) return rc;
  Span src[3];
  source_spans(A.F, nframes, A.w, A.h, src);
  return need_refine_outputs(c, W, A.npairs, A.M_in, A.M_out, A.info, A.normal, src);
}
// k_pair_refine_eval as the evaluation
int launch(evh_ctx* c, const RefineArgs& A) {
  int rc = EVH_SUCCESS;
  with_source(A.F, [&](auto cn, const auto& S) {
    rc = refine_rounds(c, A.npairs, A.w, A.h, A.M_in, A.iters, A.M_out, A.info, A.normal,
                       [&](dim3 grid, const double* M, const RefineState* state, double* part, const Runs& R) {
      hipLaunchKernelGGL((k_pair_refine_eval<decltype(cn)::value, std::decay_t<decltype(S)>>), grid, dim3(256), 0, c->stream, S,
                         A.frame_step, A.w, A.h, M, state, part, A.clip, R.per_row, R.n);
    });
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
  if (int rc = need_frame_and_canvas(c, W, A.nframes, A.w, A.h, A.dw, A.dh)) return rc;
  // the frame's bounds are evh_pair_refine's (the Jacobian), the canvas's evh_warp_fixed_plane's source bounds (the positions)
  if (int rc = need_refine_bounds(c, W, A.iters, A.clip, A.count, A.min_cover, A.w, A.h)) return rc;
  if (int rc = need_below_2_26(c, W, "canvas", A.dw, A.dh)) return rc;
  if (int rc = need_area(c, W, "dw * dh", A.dw, A.dh)) return rc;
  if (A.nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  if (int rc = need_source_stride(c, W, A.F, A.w, A.h, A.nframes > 1)) return rc;
  if (A.canvas_stride < (int64_t)A.dw * A.F.channels) return evh_fail(c, EVH_ERR_INVALID, W + "canvas stride smaller than a row");
  if (A.count && A.count_stride < A.dw) return evh_fail(c, EVH_ERR_INVALID, W + "count stride smaller than a row");
  if (A.nframes == 0) return EVH_SUCCESS;
  if (int rc = need_planes(c, A.who, A.F, A.nframes, A.w, A.h)) return rc;
  Span src[3];
  source_spans(A.F, A.nframes, A.w, A.h, src);
  const Span ins[5] = {src[0], src[1], src[2],
                       {A.canvas, (A.dh - 1) * A.canvas_stride + (int64_t)A.dw * A.F.channels, "the canvas"},
                       {A.count, (A.dh - 1) * A.count_stride + A.dw, "d_count"}};
  return need_refine_outputs(c, W, A.nframes, A.M_in, A.M_out, A.info, A.normal, ins);
}
// k_canvas_refine_eval as the evaluation: the same groups for the same w, h, the same workspace
int launch(evh_ctx* c, const CanvasRefineArgs& A) {
  const PackedSrc canvas{A.canvas, A.F.channels, A.canvas_stride, 0};
  int rc = EVH_SUCCESS;
  with_source(A.F, [&](auto cn, const auto& S) {
    rc = refine_rounds(c, A.nframes, A.w, A.h, A.M_in, A.iters, A.M_out, A.info, A.normal,
                       [&](dim3 grid, const double* M, const RefineState* state, double* part, const Runs& R) {
      hipLaunchKernelGGL((k_canvas_refine_eval<decltype(cn)::value, std::decay_t<decltype(S)>>), grid, dim3(256), 0, c->stream, S, canvas,
                         A.count, A.count_stride, A.min_cover, A.w, A.h, A.dw, A.dh, M, state, part, A.clip, R.per_row, R.n);
    });
  });
  return rc;
}
