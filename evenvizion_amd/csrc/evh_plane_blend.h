// evh_plane_blend.h -- the blended mosaic: evh_blend_fixed_plane and evh_blend_ray_surface, kernel, arguments, checks and launch().
// Included by evh_plane.hip inside its unnamed namespace, after evh_plane_warp.h (BlendArgs holds a WarpArgs); evh_plane_bands.h
// follows it and uses check_blend.

// The blended mosaic (include/evhip.h states the contract for evh_blend_fixed_plane and evh_blend_ray_surface): every covering
// frame enters a canvas pixel's state u64[CN + 1] -- FEATHER: the sums of w * s * g and of w; SEAM: s * g of the frame with the
// largest w, and that w -- where w = min(d, F) + 1 and d is the sample's distance to the nearest frame edge in 1/32 pixels.

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
    const uint32_t w = (uint32_t)min(edge_distance(sample_position(A, X, Y), sw, sh), feather) + 1u;
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
  if (int rc = need_frame_and_canvas(c, W, A.nframes, A.sw, A.sh, A.dw, A.dh)) return rc;
  if (A.mode != EVH_BLEND_FEATHER && A.mode != EVH_BLEND_SEAM) return evh_fail(c, EVH_ERR_INVALID, W + "unknown mode");
  if (B.feather < 0 || B.feather > 65535) return evh_fail(c, EVH_ERR_INVALID, W + "feather must lie in 0..65535");
  if (int rc = need_canvas_bounds(c, W, A.nframes, A.sw, A.sh, A.dw, A.dh)) return rc;
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
