// evh_plane_warp.h -- stabilised output: evh_warp_fixed_plane and evh_warp_ray_surface, kernels, arguments, check() and launch().
// Included by evh_plane.hip inside its unnamed namespace, after evh_plane_sample.h and the launch plumbing.

// The modes of a warp, for the run of n <= WARP_RUN pixels at byte `at` of a canvas.  MODE EVH_WARP_EACH: grid.y = frame, out[k] =
// frame k over the background.  EVH_WARP_HISTORY: the frames upward with the run in registers, out[k] stored at every step (the
// last covering frame wins).  EVH_WARP_MOSAIC: the frames downward, a pixel is settled by the first frame that covers it; bg may BE
// out (a thread reads only the bytes it writes, before it writes them), hence no __restrict__ on either.
// map_of(k): frame k's map, formed once for the run; sample(k, map, p, v): pixel p of the run in frame k, false = not covered.
// (Measured against the loop written out in each kernel, instance by instance, in profiles/plane_second_fold.txt section 5.)
template <int MODE, int CN, class MAP, class SAMPLE>
__device__ __forceinline__ void warp_modes(int nframes, const uint8_t* bg, uint8_t* out, int64_t at, int64_t out_img_stride, int n,
                                           bool wide, MAP map_of, SAMPLE sample) {
  int v[WARP_RUN][3];
#pragma unroll
  for (int p = 0; p < WARP_RUN; p++) v[p][0] = v[p][1] = v[p][2] = 0;
  if constexpr (MODE == EVH_WARP_HISTORY) {
    if (bg) warp_run_load<CN>(bg + at, n, wide, v);
    for (int k = 0; k < nframes; k++) {
      const auto A = map_of(k);
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++) if (p < n) sample(k, A, p, v[p]);
      warp_run_store<CN>(out + (int64_t)k * out_img_stride + at, n, wide, v);
    }
  } else {
    unsigned open = (1u << n) - 1;                      // pixels of the run no frame has covered yet
    const int first = MODE == EVH_WARP_EACH ? (int)blockIdx.y : nframes - 1, last = MODE == EVH_WARP_EACH ? first : 0;
    for (int k = first; k >= last && open; k--) {
      const auto A = map_of(k);
#pragma unroll
      for (int p = 0; p < WARP_RUN; p++)
        if (((open >> p) & 1) && sample(k, A, p, v[p])) open &= ~(1u << p);
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

// The fixed plane: a run's points are (x0 + p + ox, y + oy), a frame's map is warp_map of its matrix.
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
  warp_modes<MODE, CN>(nframes, bg, out, at, out_img_stride, n, wide,
                       [&](int k) { return warp_map(M + 9 * (int64_t)k, inverse_map); },
                       [&](int k, const WarpMap& A, int p, int (&v)[3]) { return warp_sample(src, k, A, X[p], Y, sw, sh, v); });
}

// The rays: a run's points come from two tables, a frame's map is ray_map of its matrix and the row's b.  col: f64[dw,2] = (a, c) per column,
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
  warp_modes<MODE, CN>(nframes, bg, out, at, out_img_stride, n, wide,
                       [&](int k) { return ray_map(A + 9 * (int64_t)k, b); },
                       [&](int k, const RayMap& R, int p, int (&v)[3]) { return ray_sample(src, k, R, ra[p], rc[p], sw, sh, v); });
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
  if (int rc = need_frame_and_canvas(c, W, A.nframes, A.sw, A.sh, A.dw, A.dh)) return rc;
  if (A.mode != EVH_WARP_EACH && A.mode != EVH_WARP_HISTORY && A.mode != EVH_WARP_MOSAIC) return evh_fail(c, EVH_ERR_INVALID, W + "unknown mode");
  if (int rc = need_canvas_bounds(c, W, A.nframes, A.sw, A.sh, A.dw, A.dh)) return rc;
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
// The launch the plane and the ray warps share: the runs, vec, the grid and the three modes.  go(mode, cn, S, grid, R, vec) launches
// the caller's kernel for that mode (an integral_constant, as cn is) and source.
template <class Go>
int launch_warp(evh_ctx* c, const WarpArgs& A, Go go) {
  const Runs R = runs_of(A.dw, A.dh);
  const int vec = words_ok(A.out, A.out_stride, A.out_img_stride, A.many() ? A.nframes : 1) && words_ok(A.bg, A.out_stride, 0, 1);
  const dim3 grid((R.n + 255) / 256, A.mode == EVH_WARP_EACH ? A.nframes : 1);
  with_source(A.F, [&](auto cn, const auto& S) {
    if (A.mode == EVH_WARP_EACH) go(std::integral_constant<int, EVH_WARP_EACH>{}, cn, S, grid, R, vec);
    else if (A.mode == EVH_WARP_HISTORY) go(std::integral_constant<int, EVH_WARP_HISTORY>{}, cn, S, grid, R, vec);
    else go(std::integral_constant<int, EVH_WARP_MOSAIC>{}, cn, S, grid, R, vec);
  });
  return launched(c);
}
// k_warp_fixed_plane over the canvas
int launch(evh_ctx* c, const WarpArgs& A) {
  return launch_warp(c, A, [&](auto mode, auto cn, const auto& S, dim3 grid, const Runs& R, int vec) {
    hipLaunchKernelGGL((k_warp_fixed_plane<decltype(mode)::value, decltype(cn)::value, std::decay_t<decltype(S)>>), grid, dim3(256), 0,
                       c->stream, S, A.nframes, A.sw, A.sh, A.M, A.inverse_map, A.bg, A.out, A.dw, A.out_stride, A.out_img_stride, A.ox,
                       A.oy, R.per_row, R.n, vec);
  });
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
int launch(evh_ctx* c, const RayArgs& A) {
  return launch_warp(c, A.W, [&](auto mode, auto cn, const auto& S, dim3 grid, const Runs& R, int vec) {
    hipLaunchKernelGGL((k_warp_ray_surface<decltype(mode)::value, decltype(cn)::value, std::decay_t<decltype(S)>>), grid, dim3(256), 0,
                       c->stream, S, A.W.nframes, A.W.sw, A.W.sh, A.W.M, A.col, A.row, A.W.bg, A.W.out, A.W.dw, A.W.out_stride,
                       A.W.out_img_stride, R.per_row, R.n, vec);
  });
}
