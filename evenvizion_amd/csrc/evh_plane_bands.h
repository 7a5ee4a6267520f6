// evh_plane_bands.h -- multi-band blending of the mosaic and the seam labels it blends under (include/evhip.h states the contract
// for evh_seam_labels_* and evh_blend_bands_*).  Included by evh_plane.hip inside its unnamed namespace, after the blend entries:
// it uses their geometry (BlendGeo, warp_map), their checks and the launch plumbing.
//
// Level 0 continues a frame past its border, so it takes the sampler of evh_plane_sample.h by its pieces: the position before the
// coverage test, clamped here, then the taps.  A covered position gives warp_sample's integers.
//
// Per group of frames that the workspace holds:   k_bands_level0     G^0 = s * g and W^0 = 65536 [label == frame], frames on grid.z
//                                                 k_bands_reduce     G^{l+1}, W^{l+1} from G^l, W^l, one launch per level for the group
//                                                 k_bands_accumulate every level of the state in one launch, the frames looped in the
//                                                                    thread with the state in registers (no atomics)
// and once, after the last group:                 k_bands_collapse   R^l = q^l + E(R^{l+1}), one launch per level, top down
// A frame's slot of the workspace holds, per level, G^l as u32[dh_l][dw_l][cn] and then W^l as u32[dh_l][dw_l]; the collapse keeps
// R^l as i32 where slot 0 kept G^l.

// the levels of a canvas: sizes, and the number of pixels in front of each level (off[n + 1]: all of them)
struct BandsGeo { int n; int w[10], h[10]; int64_t off[10]; };
BandsGeo bands_geo(int dw, int dh, int levels) {
  BandsGeo P = {};
  P.n = levels;
  int w = dw, h = dh;
  int64_t at = 0;
  for (int l = 0; l <= levels; l++) {
    P.w[l] = w; P.h[l] = h; P.off[l] = at;
    at += (int64_t)w * h;
    w = (w + 1) >> 1; h = (h + 1) >> 1;
  }
  for (int l = levels + 1; l < 10; l++) { P.w[l] = P.h[l] = 1; P.off[l] = at; }
  return P;
}

// the position of a canvas pixel in frame k, in 1/32 pixels before any test: the plane's through its map, a ray's from the
// header's tx, ty, tw, whose third term is a product
template <bool RAY>
__device__ __forceinline__ SamplePos bands_position(const BlendGeo& G, int k, double X, double Y, double rc) {
  if constexpr (RAY) {
    const double* A = G.M + 9 * (int64_t)k;
    return sample_position(MapRows{(A[0] * X + A[1] * Y) + A[2] * rc, (A[3] * X + A[4] * Y) + A[5] * rc, (A[6] * X + A[7] * Y) + A[8] * rc});
  } else {
    return sample_position(warp_map(G.M + 9 * (int64_t)k, G.inverse_map), X, Y);
  }
}
// canvas pixel (x, y) as the position takes it: the plane point, or the ray (a, b, c)
template <bool RAY>
__device__ __forceinline__ void bands_pixel(const BlendGeo& G, int x, int y, double& X, double& Y, double& rc) {
  if constexpr (RAY) {
    X = G.col[2 * (int64_t)x]; rc = G.col[2 * (int64_t)x + 1]; Y = G.row[y];
  } else {
    X = (double)((int64_t)x + G.ox); Y = (double)((int64_t)y + G.oy); rc = 0.0;
  }
}

// SEAM's partition of the canvas from the geometry alone: one pixel per thread, the frames in order, no frame read.
template <bool RAY>
__global__ __launch_bounds__(256) void k_seam_labels(int nframes, int sw, int sh, BlendGeo G, int feather, int first_label,
                                                     uint32_t* __restrict__ best, uint16_t* __restrict__ label, int state_in,
                                                     int dw, unsigned npix) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npix) return;
  const int y = (int)(t / (unsigned)dw), x = (int)t - y * dw;
  double X, Y, rc;
  bands_pixel<RAY>(G, x, y, X, Y, rc);
  uint32_t b = state_in ? best[t] : 0u;
  uint32_t lab = state_in ? label[t] : 65535u;
  for (int k = 0; k < nframes; k++) {
    const SamplePos P = bands_position<RAY>(G, k, X, Y, rc);
    if (RAY && !(P.tw > 0.0)) continue;
    if (!sample_covered(P, sw, sh)) continue;
    const uint32_t w = (uint32_t)min(edge_distance(P, sw, sh), feather) + 1u;
    if (w > b) { b = w; lab = (uint32_t)(first_label + k); }
  }
  best[t] = b;
  label[t] = (uint16_t)lab;
}

// Level 0 of frame f0 + blockIdx.z: the frame continued past its border by its edge pixels, times its gain, at every canvas pixel,
// and the frame's mask.  A clamped position lies in 0 .. 32 (sw - 1), 0 .. 32 (sh - 1): no tap leaves the frame (sample_taps).
template <int CN, class SRC, bool RAY>
__global__ __launch_bounds__(256) void k_bands_level0(SRC src, int f0, int sw, int sh, BlendGeo G, const uint16_t* __restrict__ gain,
                                                      const uint16_t* __restrict__ label, int first_label, uint32_t* __restrict__ ws,
                                                      int64_t frame_elems, int dw, unsigned npix) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npix) return;
  const int k = f0 + (int)blockIdx.z;
  const int y = (int)(t / (unsigned)dw), x = (int)t - y * dw;
  double X, Y, rc;
  bands_pixel<RAY>(G, x, y, X, Y, rc);
  const SamplePos P = bands_position<RAY>(G, k, X, Y, rc);
  int s[3] = {0, 0, 0};
  if (P.U == P.U && P.V == P.V && (!RAY || P.tw > 0.0)) {
    const double umax = (double)(32 * (sw - 1)), vmax = (double)(32 * (sh - 1));
    const double Uc = P.U < 0.0 ? 0.0 : (P.U > umax ? umax : P.U), Vc = P.V < 0.0 ? 0.0 : (P.V > vmax ? vmax : P.V);
    sample_taps(src, k, (int)Uc, (int)Vc, s);
  }
  uint32_t* o = ws + (int64_t)blockIdx.z * frame_elems;
#pragma unroll
  for (int c = 0; c < CN; c++) o[(int64_t)t * CN + c] = (uint32_t)s[c] * (gain ? (uint32_t)gain[3 * (int64_t)k + c] : 4096u);
  o[(int64_t)npix * CN + t] = (int)label[t] == first_label + k ? 65536u : 0u;
}

// One level down, frame slot blockIdx.z: (1,4,6,4,1) in both directions with clamped indices, G rounded to nearest, W rounded up.
// in / out: element offsets of the two levels inside a slot.
template <int CN>
__global__ __launch_bounds__(256) void k_bands_reduce(uint32_t* __restrict__ ws, int64_t frame_elems, int64_t in, int w0, int h0,
                                                      int64_t out, int w1, unsigned npix1) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npix1) return;
  const int y = (int)(t / (unsigned)w1), x = (int)t - y * w1;
  uint32_t* slot = ws + (int64_t)blockIdx.z * frame_elems;
  const uint32_t* g = slot + in;
  const uint32_t* m = g + (int64_t)w0 * h0 * CN;
  int64_t xs[5];
#pragma unroll
  for (int i = 0; i < 5; i++) xs[i] = min(max(2 * x + i - 2, 0), w0 - 1);
  uint32_t acc[CN + 1];
#pragma unroll
  for (int c = 0; c <= CN; c++) acc[c] = 0;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const int64_t row = (int64_t)min(max(2 * y + j - 2, 0), h0 - 1) * w0;
    const uint32_t kj = j == 0 || j == 4 ? 1u : (j == 2 ? 6u : 4u);
    uint32_t r[CN + 1];
#pragma unroll
    for (int c = 0; c <= CN; c++) r[c] = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      const uint32_t ki = i == 0 || i == 4 ? 1u : (i == 2 ? 6u : 4u);
#pragma unroll
      for (int c = 0; c < CN; c++) r[c] += ki * g[(row + xs[i]) * CN + c];
      r[CN] += ki * m[row + xs[i]];
    }
#pragma unroll
    for (int c = 0; c <= CN; c++) acc[c] += kj * r[c];
  }
  uint32_t* go = slot + out;
#pragma unroll
  for (int c = 0; c < CN; c++) go[(int64_t)t * CN + c] = (acc[c] + 128u) >> 8;
  go[(int64_t)npix1 * CN + t] = (acc[CN] + 255u) >> 8;
}

// E(g)(x, y) before its shift: g is a level of w1 x h1 with CN interleaved channels (stride CN, channel c), expanded to the level
// above.  Along an axis, with j = i >> 1: even i takes (1, 6, 1) of g[j-1 .. j+1], odd i (0, 4, 4); indices clamped.  Rows and
// columns are sums of integers, so their order does not matter.
template <int CN, class T>
__device__ __forceinline__ int64_t bands_expand(const T* __restrict__ g, int w1, int h1, int x, int y, int c) {
  const int xj = x >> 1, yj = y >> 1;
  const int cx0 = (x & 1) ? 0 : 1, cx1 = (x & 1) ? 4 : 6, cx2 = (x & 1) ? 4 : 1;
  const int cy0 = (y & 1) ? 0 : 1, cy1 = (y & 1) ? 4 : 6, cy2 = (y & 1) ? 4 : 1;
  const int64_t x0 = max(xj - 1, 0), x1 = xj, x2 = min(xj + 1, w1 - 1);
  const int64_t r0 = (int64_t)max(yj - 1, 0) * w1, r1 = (int64_t)yj * w1, r2 = (int64_t)min(yj + 1, h1 - 1) * w1;
  const int64_t a = cx0 * (int64_t)g[(r0 + x0) * CN + c] + cx1 * (int64_t)g[(r0 + x1) * CN + c] + cx2 * (int64_t)g[(r0 + x2) * CN + c];
  const int64_t b = cx0 * (int64_t)g[(r1 + x0) * CN + c] + cx1 * (int64_t)g[(r1 + x1) * CN + c] + cx2 * (int64_t)g[(r1 + x2) * CN + c];
  const int64_t d = cx0 * (int64_t)g[(r2 + x0) * CN + c] + cx1 * (int64_t)g[(r2 + x1) * CN + c] + cx2 * (int64_t)g[(r2 + x2) * CN + c];
  return cy0 * a + cy1 * b + cy2 * d;
}

// which level pixel t of the concatenated levels lies in, without an indexed read of P (indexed by a lane, the table would go to
// scratch): l, the level's size, the next level's size, and the pixels in front of both
struct BandsAt { int l, w, h, w1, h1; int64_t off, off1; };
__device__ __forceinline__ BandsAt bands_at(const BandsGeo& P, int64_t t) {
  BandsAt a = {0, P.w[0], P.h[0], P.w[1], P.h[1], P.off[0], P.off[1]};
#pragma unroll
  for (int j = 1; j <= 8; j++)
    if (j <= P.n && t >= P.off[j]) a = {j, P.w[j], P.h[j], P.w[j + 1], P.h[j + 1], P.off[j], P.off[j + 1]};
  return a;
}

// A^l += W^l * L^l and D^l += W^l for the nfr frames of the group, every level in one launch: one state pixel (of any level) per
// thread, its CN + 1 words in registers over the frames.  A frame whose mask is 0 at the pixel adds nothing and is not read further.
template <int CN>
__global__ __launch_bounds__(256) void k_bands_accumulate(const uint32_t* __restrict__ ws, int64_t frame_elems, int nfr, BandsGeo P,
                                                          long long* __restrict__ state, int state_in, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const BandsAt a = bands_at(P, t);
  const int64_t p = t - a.off;
  const int y = (int)(p / a.w), x = (int)(p - (int64_t)y * a.w);
  long long st[CN + 1];
  long long* sp = state + t * (CN + 1);
#pragma unroll
  for (int c = 0; c <= CN; c++) st[c] = state_in ? sp[c] : 0;
  const int64_t npl = (int64_t)a.w * a.h;
  for (int f = 0; f < nfr; f++) {
    const uint32_t* slot = ws + (int64_t)f * frame_elems;
    const uint32_t* g = slot + a.off * (CN + 1);
    const long long W = g[npl * CN + p];
    if (W == 0) continue;
    const uint32_t* g1 = slot + a.off1 * (CN + 1);
#pragma unroll
    for (int c = 0; c < CN; c++) {
      long long L = g[p * CN + c];
      if (a.l < P.n) L -= (bands_expand<CN>(g1, a.w1, a.h1, x, y, c) + 32) >> 6;
      st[c] += W * L;
    }
    st[CN] += W;
  }
#pragma unroll
  for (int c = 0; c <= CN; c++) sp[c] = st[c];
}

// floor((2 A + D) / (2 D)) for D > 0: the quotient has at most 27 bits and both operands are exact doubles under the header's
// bounds (|2 A + D| < 2^53), so one float64 division is within one of it and a multiplication back settles which -- against the
// general 64-bit division, which works out 64 bits.
__device__ __forceinline__ long long bands_quotient(long long A, long long D) {
  const long long num = 2 * A + D, den = 2 * D;
  long long q = (long long)__builtin_floor((double)num / (double)den);
  const long long r = num - q * den;
  if (r < 0) q--;
  else if (r >= den) q++;
  return q;
}

// Level l of the picture, top down: R^l = q^l + E(R^{l+1}) into r (i32, where slot 0 of the workspace kept G^l), or for l == 0 the
// bytes of the picture.  bg may BE out: a pixel reads its bytes before it writes them.
template <int CN>
__global__ __launch_bounds__(256) void k_bands_collapse(const long long* __restrict__ state, int32_t* r, int l, BandsGeo P,
                                                        const uint8_t* bg, uint8_t* out, int64_t out_stride, unsigned npix) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npix) return;
  int w = P.w[0], h1 = P.h[1], w1 = P.w[1];
  int64_t off = 0, off1 = P.off[1];
#pragma unroll
  for (int j = 1; j <= 8; j++) if (j == l) { w = P.w[j]; w1 = P.w[j + 1]; h1 = P.h[j + 1]; off = P.off[j]; off1 = P.off[j + 1]; }
  const int y = (int)(t / (unsigned)w), x = (int)t - y * w;
  const long long* sp = state + (off + t) * (CN + 1);
  const long long D = sp[CN];
  long long R[CN];
#pragma unroll
  for (int c = 0; c < CN; c++) {
    R[c] = D > 0 ? bands_quotient(sp[c], D) : 0;
    if (l < P.n) R[c] += (bands_expand<CN>(r + off1 * (CN + 1), w1, h1, x, y, c) + 32) >> 6;
  }
  if (l > 0) {
#pragma unroll
    for (int c = 0; c < CN; c++) r[off * (CN + 1) + (int64_t)t * CN + c] = (int32_t)R[c];
    return;
  }
  const int64_t at = (int64_t)y * out_stride + (int64_t)x * CN;
#pragma unroll
  for (int c = 0; c < CN; c++) {
    int v;
    if (D > 0) v = (int)min(max((R[c] + 2048) >> 12, 0ll), 255ll);
    else v = bg ? bg[at + c] : 0;
    out[at + c] = (uint8_t)v;
  }
}

// ---- the seam labels ------------------------------------------------------------------------------------------------------------------
struct LabelArgs {
  const char* who; int nframes, sw, sh; const double* M; int inverse_map; bool ray; const double* col; const double* row; int feather;
  int dw, dh, ox, oy, first_label; uint32_t* best; uint16_t* label; int state_in;
  bool idle() const { return false; }       // no frames: the start state is still written
};
// what the label and band entries ask of first_label
int need_labels(evh_ctx* c, const std::string& W, int first_label, int nframes) {
  if (first_label < 0 || (int64_t)first_label + std::max(nframes, 1) - 1 > 65534)
    return evh_fail(c, EVH_ERR_INVALID, W + "labels first_label .. first_label + nframes - 1 must lie in 0..65534");
  return EVH_SUCCESS;
}
int check(evh_ctx* c, const LabelArgs& A) {
  const std::string W = std::string(A.who) + ": ";
  if (!A.M || (A.ray && (!A.col || !A.row)) || !A.best || !A.label) return evh_fail(c, EVH_ERR_INVALID, W + "NULL argument");
  if (((uintptr_t)A.best & 3) || ((uintptr_t)A.label & 1))
    return evh_fail(c, EVH_ERR_INVALID, W + "d_best must be 4-byte and d_label 2-byte aligned");
  if (int rc = need_frame_and_canvas(c, W, A.nframes, A.sw, A.sh, A.dw, A.dh)) return rc;
  if (A.feather < 0 || A.feather > 65535) return evh_fail(c, EVH_ERR_INVALID, W + "feather must lie in 0..65535");
  if (int rc = need_canvas_bounds(c, W, A.nframes, A.sw, A.sh, A.dw, A.dh)) return rc;
  if (int rc = need_labels(c, W, A.first_label, A.nframes)) return rc;
  const int64_t npix = (int64_t)A.dw * A.dh;
  const Span outs[2] = {{A.best, npix * 4, "d_best"}, {A.label, npix * 2, "d_label"}};
  const Span ins[3] = {{A.M, (int64_t)A.nframes * 72, A.ray ? "d_A" : "d_M"}, {A.col, (int64_t)A.dw * 16, "d_col"},
                       {A.row, (int64_t)A.dh * 8, "d_row"}};
  return need_apart(c, W, outs, ins);
}
int launch(evh_ctx* c, const LabelArgs& A) {
  const unsigned npix = (unsigned)A.dw * (unsigned)A.dh;
  const BlendGeo G = {A.M, A.inverse_map, A.ox, A.oy, A.col, A.row};
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((npix + 255) / 256), dim3(256), 0, c->stream, A.nframes, A.sw, A.sh, G, A.feather, A.first_label,
                       A.best, A.label, A.state_in, A.dw, npix);
  };
  if (A.ray) go(k_seam_labels<true>); else go(k_seam_labels<false>);
  return launched(c);
}

// ---- the band blend --------------------------------------------------------------------------------------------------------------------
int64_t bands_state_elems(int dw, int dh, int cn, int levels) {
  const BandsGeo P = bands_geo(dw, dh, levels);
  return P.off[levels + 1] * (cn + 1);
}
// B: the blend entries' arguments with acc = d_state, acc_in = state_in and no mode or feather
struct BandsArgs {
  BlendArgs B; int levels; const uint16_t* label; int first_label; void* ws; int64_t ws_bytes;
  bool idle() const { return false; }       // no frames: the picture of the incoming state
};
int check(evh_ctx* c, const BandsArgs& A) {
  const WarpArgs& Wa = A.B.W;
  const std::string W = std::string(Wa.who) + ": ";
  const int levels = A.levels;
  if (levels < 0 || levels > 8) return evh_fail(c, EVH_ERR_INVALID, W + "levels must lie in 0..8");
  if (!A.label) return evh_fail(c, EVH_ERR_INVALID, W + "d_label is NULL");
  if (int rc = check_blend(c, A.B, "d_state", "state_in", [levels](int dw, int dh, int cn) { return bands_state_elems(dw, dh, cn, levels); }))
    return rc;
  if (int rc = need_labels(c, W, A.first_label, Wa.nframes)) return rc;
  if ((uintptr_t)A.label & 1) return evh_fail(c, EVH_ERR_INVALID, W + "d_label must be 2-byte aligned");
  const int cn = Wa.F.channels;
  const int64_t elems = bands_state_elems(Wa.dw, Wa.dh, cn, levels), held = A.B.acc ? 0 : elems * 8;
  if (!A.ws || ((uintptr_t)A.ws & 7)) return evh_fail(c, EVH_ERR_INVALID, W + "d_ws must be given and 8-byte aligned");
  if (A.ws_bytes < held + elems * 4)
    return evh_fail(c, EVH_ERR_INVALID, W + "ws_bytes holds less than one frame's pyramids (and the state, where d_state is NULL)");
  // the workspace apart from everything, the labels apart from what is written
  Span src[3];
  source_spans(Wa.F, Wa.nframes, Wa.sw, Wa.sh, src);
  const int64_t canvas = (int64_t)(Wa.dh - 1) * Wa.out_stride + (int64_t)Wa.dw * cn, npix = (int64_t)Wa.dw * Wa.dh;
  const Span label = {A.label, npix * 2, "d_label"};
  const Span work[1] = {{A.ws, A.ws_bytes, "d_ws"}};
  const Span others[11] = {{A.B.acc, elems * 8, "d_state"}, {Wa.out, Wa.out ? canvas : 0, "d_out"},
                           {Wa.out ? Wa.bg : nullptr, canvas, "d_background"}, {A.B.gain, (int64_t)Wa.nframes * 6, "d_gain"},
                           {Wa.M, (int64_t)Wa.nframes * 72, A.B.ray ? "d_A" : "d_M"}, {A.B.col, (int64_t)Wa.dw * 16, "d_col"},
                           {A.B.row, (int64_t)Wa.dh * 8, "d_row"}, src[0], src[1], src[2], label};
  if (int rc = need_apart(c, W, work, others)) return rc;
  const Span written[2] = {{A.B.acc, elems * 8, "d_state"}, {Wa.out, Wa.out ? canvas : 0, "d_out"}};
  for (const Span& o : written)
    if (meet(o, label)) return evh_fail(c, EVH_ERR_INVALID, W + o.name + " overlaps d_label");
  return EVH_SUCCESS;
}
int launch(evh_ctx* c, const BandsArgs& A) {
  const BlendArgs& B = A.B;
  const WarpArgs& Wa = B.W;
  const int cn = Wa.F.channels, n = A.levels;
  const BandsGeo P = bands_geo(Wa.dw, Wa.dh, n);
  const int64_t total = P.off[n + 1], elems = total * (cn + 1);
  // without d_state the state lives at the head of the workspace
  long long* state = B.acc ? reinterpret_cast<long long*>(B.acc) : static_cast<long long*>(A.ws);
  uint32_t* slots = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(A.ws) + (B.acc ? 0 : elems * 8));
  const int64_t room = (A.ws_bytes - (B.acc ? 0 : elems * 8)) / (elems * 4);
  const int group = (int)std::min<int64_t>(std::min<int64_t>(room, 65535), std::max(Wa.nframes, 1));
  const unsigned npix = (unsigned)Wa.dw * (unsigned)Wa.dh;
  const BlendGeo G = {Wa.M, Wa.inverse_map, Wa.ox, Wa.oy, B.col, B.row};
  const dim3 all((unsigned)((total + 255) / 256));
  with_source(Wa.F, [&](auto cnc, const auto& S) {
    constexpr int CN = decltype(cnc)::value;
    using SRC = std::decay_t<decltype(S)>;
    int carried = B.acc_in;
    for (int f0 = 0; f0 < Wa.nframes || (f0 == 0 && !carried); f0 += group) {     // no frames and no state: zeros are written
      const int g = std::min(group, Wa.nframes - f0);
      if (g > 0) {
        auto level0 = [&](auto kernel) {
          hipLaunchKernelGGL(kernel, dim3((npix + 255) / 256, 1, g), dim3(256), 0, c->stream, S, f0, Wa.sw, Wa.sh, G, B.gain, A.label,
                             A.first_label, slots, elems, Wa.dw, npix);
        };
        if (B.ray) level0(k_bands_level0<CN, SRC, true>); else level0(k_bands_level0<CN, SRC, false>);
        for (int l = 0; l < n; l++) {
          const unsigned np1 = (unsigned)P.w[l + 1] * (unsigned)P.h[l + 1];
          hipLaunchKernelGGL(k_bands_reduce<CN>, dim3((np1 + 255) / 256, 1, g), dim3(256), 0, c->stream, slots, elems,
                             P.off[l] * (CN + 1), P.w[l], P.h[l], P.off[l + 1] * (CN + 1), P.w[l + 1], np1);
        }
      }
      hipLaunchKernelGGL(k_bands_accumulate<CN>, all, dim3(256), 0, c->stream, slots, elems, g, P, state, carried, total);
      carried = 1;
      if (g <= 0) break;
    }
    if (Wa.out)
      for (int l = n; l >= 0; l--) {
        const unsigned npl = (unsigned)P.w[l] * (unsigned)P.h[l];
        hipLaunchKernelGGL(k_bands_collapse<CN>, dim3((npl + 255) / 256), dim3(256), 0, c->stream, state,
                           reinterpret_cast<int32_t*>(slots), l, P, Wa.bg, Wa.out, Wa.out_stride, npl);
      }
  });
  return launched(c);
}
