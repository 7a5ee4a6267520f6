// evh_plane_steady.h -- the steady view: evh_steady_frames, kernel, arguments, check() and launch().
// Included by evh_plane.hip inside its unnamed namespace, after evh_plane_sample.h and the launch plumbing.

// The steady view (include/evhip.h states the contract for evh_steady_frames): output picture j has its own ordered list of ntaps
// candidate sources, each a frame of the chunk and a map from output pixel to frame pixel, used as it is.  A pixel takes the first
// tap that covers it; inside the feather band of tap 0 it is mixed with the next covering tap.
// A thread owns a run of WARP_RUN pixels, grid.y is the picture, and a tap's map is formed once for the run, as in
// k_warp_fixed_plane.  `open`: the pixels of the run no tap has covered yet -- the tap loop ends with it, which for a picture
// that tap 0 fills is after one tap.  `band`: the pixels that tap 0 took inside its feather band; only a run that has one goes
// through the taps again, from 1, for its second source.  vec bit 0: the picture's (and the background's) bytes move as words,
// bit 1: tap_of's do.
// counts: every pixel of the picture falls into one of ntaps + 1 buckets (0: no tap, 1 + t: first covered by tap t).  A wave
// counts a bucket with one ballot per pixel of the run, and its first lane adds the sum with one atomic -- and none for a bucket
// the wave has no pixel in.  (Threads past the last run have left: they are in no ballot, and since runs are numbered along the
// lanes, lane 0 has left only if its whole wave has.)  Bucket 1, tap 0's, is not counted here at all: it is where nearly every
// pixel of a steady view falls, so every wave of the launch would add to the same few words, the counters of all pictures
// sharing a cache line or two -- 115 200 atomics that the memory side takes one after the other, 945 us for 32 pictures of
// 1280x720 against 171 us for the same warp without counts (profiles/steady_frames.txt).  k_steady_own_count fills it in
// afterwards as what the other buckets leave of dw * dh.
template <int CN, class SRC>
__global__ __launch_bounds__(256) void k_steady_frames(SRC src, int nframes, int sw, int sh, const int32_t* __restrict__ tap_frame,
                                                       const double* __restrict__ tap_M, int ntaps, int feather, const uint8_t* bg,
                                                       uint8_t* out, int dw, int64_t out_stride, int64_t out_img_stride,
                                                       uint8_t* tap_of, int64_t of_stride, int64_t of_img_stride,
                                                       unsigned* __restrict__ counts, int runs_per_row, unsigned nruns, int vec) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nruns) return;
  const int j = (int)blockIdx.y;
  const RunPos rp = run_pos(t, runs_per_row, dw);
  const int y = rp.y, x0 = rp.x0, n = rp.n;
  const double Y = (double)y;
  double X[WARP_RUN];
#pragma unroll
  for (int p = 0; p < WARP_RUN; p++) X[p] = (double)(x0 + p);
  const int32_t* const frame_of = tap_frame + (int64_t)j * ntaps;
  const double* const M = tap_M + 9 * (int64_t)j * ntaps;
  int v[WARP_RUN][3], of[WARP_RUN][3], d[WARP_RUN];
#pragma unroll
  for (int p = 0; p < WARP_RUN; p++) { v[p][0] = v[p][1] = v[p][2] = 0; of[p][0] = of[p][1] = of[p][2] = 0; d[p] = 0; }
  unsigned open = (1u << n) - 1, band = 0;
  for (int k = 0; k < ntaps && open; k++) {
    const int f = frame_of[k];
    if ((unsigned)f >= (unsigned)nframes) continue;                 // not a frame of the chunk: covers nothing, reads nothing
    const WarpMap A = warp_map(M + 9 * k, 1);
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) {
      if (!((open >> p) & 1)) continue;
      const SamplePos P = sample_position(A, X[p], Y);
      if (!sample_covered(P, sw, sh)) continue;
      sample_taps(src, f, (int)P.U, (int)P.V, v[p]);
      of[p][0] = k + 1;
      open &= ~(1u << p);
      if (k == 0 && feather > 0) {
        d[p] = edge_distance(P, sw, sh);
        if (d[p] < feather) band |= 1u << p;
      }
    }
  }
  for (int k = 1; k < ntaps && band; k++) {                          // the second source of the pixels in tap 0's feather band
    const int f = frame_of[k];
    if ((unsigned)f >= (unsigned)nframes) continue;
    const WarpMap A = warp_map(M + 9 * k, 1);
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) {
      if (!((band >> p) & 1)) continue;
      int s[3] = {0, 0, 0};
      if (!warp_sample(src, f, A, X[p], Y, sw, sh, s)) continue;
      const unsigned w0 = (unsigned)d[p], w1 = (unsigned)(feather - d[p]), half = (unsigned)feather >> 1;
#pragma unroll
      for (int c = 0; c < CN; c++) v[p][c] = (int)(((unsigned)v[p][c] * w0 + (unsigned)s[c] * w1 + half) / (unsigned)feather);
      band &= ~(1u << p);
    }
  }
  const bool full = n == WARP_RUN;
  const int64_t at = (int64_t)y * out_stride + (int64_t)x0 * CN;
  if (open && bg) {
    int b[WARP_RUN][3];
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) b[p][0] = b[p][1] = b[p][2] = 0;
    warp_run_load<CN>(bg + at, n, (vec & 1) && full, b);
#pragma unroll
    for (int p = 0; p < WARP_RUN; p++) if ((open >> p) & 1) { v[p][0] = b[p][0]; v[p][1] = b[p][1]; v[p][2] = b[p][2]; }
  }
  warp_run_store<CN>(out + (int64_t)j * out_img_stride + at, n, (vec & 1) && full, v);
  if (tap_of) warp_run_store<1>(tap_of + (int64_t)j * of_img_stride + (int64_t)y * of_stride + x0, n, (vec & 2) && full, of);
  if (counts) {
    const bool first_lane = (threadIdx.x & 63) == 0;
    for (int b = 0; b <= ntaps; b++) {
      if (b == 1) continue;
      unsigned sum = 0;
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++) sum += (unsigned)__popcll(__ballot(p < n && of[p][0] == b));
      if (first_lane && sum) atomicAdd(counts + (int64_t)j * (ntaps + 1) + b, sum);
    }
  }
}

// counts[j, 1] = npix - the other buckets of picture j, one thread per picture
__global__ __launch_bounds__(256) void k_steady_own_count(unsigned* __restrict__ counts, int nout, int ntaps, unsigned npix) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nout) return;
  unsigned* const row = counts + (int64_t)j * (ntaps + 1);
  unsigned others = row[0];
  for (int b = 2; b <= ntaps; b++) others += row[b];
  row[1] = npix - others;
}

// ---- the steady view: every output picture from its own list of frames and maps ----------------------------------------------------
struct SteadyArgs {
  const char* who; EvhFrames F; int nframes, sw, sh; const int32_t* tap_frame; const double* tap_M; int nout, ntaps, feather;
  const uint8_t* bg; uint8_t* out; int dw, dh; int64_t out_stride, out_img_stride; uint8_t* tap_of; int64_t of_stride, of_img_stride;
  uint32_t* counts;
  bool idle() const { return nout == 0; }
};
int check(evh_ctx* c, const SteadyArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  const int cn = A.F.channels;
  if (int rc = need_source(c, W, A.F)) return rc;
  if (!A.tap_frame || !A.tap_M || !A.out) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (int rc = need_channels(c, W, A.F)) return rc;
  if (int rc = need_frame_and_canvas(c, W, A.nframes, A.sw, A.sh, A.dw, A.dh)) return rc;
  if (A.nout < 0) return evh_fail(c, EVH_ERR_INVALID, W + "negative nout");
  if (A.ntaps < 1 || A.ntaps > 16) return evh_fail(c, EVH_ERR_INVALID, W + "ntaps must lie in 1..16");
  if (A.feather < 0 || A.feather > 8160) return evh_fail(c, EVH_ERR_INVALID, W + "feather must lie in 0..8160");
  if (int rc = need_below_2_26(c, W, "source", A.sw, A.sh)) return rc;
  if (int rc = need_area(c, W, "dw * dh", A.dw, A.dh)) return rc;
  if (A.nout > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 pictures per call");
  const int64_t picture = (int64_t)(A.dh - 1) * A.out_stride + (int64_t)A.dw * cn;
  if (A.out_stride < (int64_t)A.dw * cn || (A.nout > 1 && A.out_img_stride < picture))
    return evh_fail(c, EVH_ERR_INVALID, W + "output stride smaller than a row / picture");
  const int64_t of_picture = (int64_t)(A.dh - 1) * A.of_stride + A.dw;
  if (A.tap_of && (A.of_stride < A.dw || (A.nout > 1 && A.of_img_stride < of_picture)))
    return evh_fail(c, EVH_ERR_INVALID, W + "d_tap_of stride smaller than a row / picture");
  if (int rc = need_source_stride(c, W, A.F, A.sw, A.sh, A.nframes > 1)) return rc;
  if (A.nout > 0) {
    const Span outs[3] = {{A.out, picture + (A.nout - 1) * A.out_img_stride, "d_out"},
                          {A.tap_of, of_picture + (A.nout - 1) * A.of_img_stride, "d_tap_of"},
                          {A.counts, (int64_t)A.nout * (A.ntaps + 1) * 4, "d_counts"}};
    const Span ins[1] = {{A.bg, picture, "d_background"}};
    if (int rc = need_apart(c, W, outs, ins)) return rc;
  }
  if (A.nout == 0 || A.nframes == 0) return EVH_SUCCESS;
  return need_planes(c, A.who, A.F, A.nframes, A.sw, A.sh);
}
// the counts zeroed on the stream, k_steady_frames over the nout pictures, then k_steady_own_count
int launch(evh_ctx* c, const SteadyArgs& A) {
  if (A.counts) EVH_HIP(c, hipMemsetAsync(A.counts, 0, (size_t)A.nout * (A.ntaps + 1) * sizeof(uint32_t), c->stream));
  const Runs R = runs_of(A.dw, A.dh);
  const int vec = (words_ok(A.out, A.out_stride, A.out_img_stride, A.nout) && words_ok(A.bg, A.out_stride, 0, 1) ? 1 : 0) |
                  (words_ok(A.tap_of, A.of_stride, A.of_img_stride, A.nout) ? 2 : 0);
  with_source(A.F, [&](auto cn, const auto& S) {
    hipLaunchKernelGGL((k_steady_frames<decltype(cn)::value, std::decay_t<decltype(S)>>), dim3((R.n + 255) / 256, A.nout), dim3(256), 0,
                       c->stream, S, A.nframes, A.sw, A.sh, A.tap_frame, A.tap_M, A.ntaps, A.feather, A.bg, A.out, A.dw, A.out_stride,
                       A.out_img_stride, A.tap_of, A.of_stride, A.of_img_stride, A.counts, R.per_row, R.n, vec);
  });
  if (A.counts) {
    EVH_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(k_steady_own_count, dim3((A.nout + 255) / 256), dim3(256), 0, c->stream, A.counts, A.nout, A.ntaps,
                       (unsigned)A.dw * (unsigned)A.dh);
  }
  return launched(c);
}
