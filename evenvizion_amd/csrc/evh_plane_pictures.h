// evh_plane_pictures.h -- the kernels of the pictures drawn from a batch's results: evh_heatmap_render and evh_draw_matches.  Each
// has one form, so its checks and its launch sit in the entry (evh_plane.hip).  Included inside the unit's unnamed namespace.

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
