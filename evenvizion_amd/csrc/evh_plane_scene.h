// evh_plane_scene.h -- what the fixed plane shows over time: evh_trail_fixed_plane, evh_plate_fixed_plane and
// evh_rows_moving_filter, per product its kernel, arguments, check() and launch().  Included by evh_plane.hip inside its unnamed
// namespace; evh_plane_components.h follows it.

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
  if (int rc = need_frame_and_canvas(c, W, A.nframes, A.sw, A.sh, A.dw, A.dh)) return rc;
  if (int rc = need_canvas_bounds(c, W, A.nframes, A.sw, A.sh, A.dw, A.dh)) return rc;
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
  if (int rc = need_frame_and_canvas(c, W, A.nframes, A.sw, A.sh, A.dw, A.dh)) return rc;
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
      const MapRows r = map_rows(s_fwd[s], px, py);
      const double cx = __builtin_rint(r.tx / r.tw), cy = __builtin_rint(r.ty / r.tw);
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
