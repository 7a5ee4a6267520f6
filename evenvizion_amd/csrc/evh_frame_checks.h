// evh_frame_checks.h -- the refusals shared by the entries that read frames and compare byte ranges (evh_plane.hip,
// evh_track.hip).  Host code only.  Everything sits in an unnamed namespace, as in evh_pixels.h: each unit keeps its own copy.
#pragma once
#include "evh_internal.h"
#include <climits>

namespace {

// ---- what the entries share: checks ------------------------------------------------------------------------------------------------
// Each refuses with W = "<entry>: " in front.  The ORDER of the refusals is the entry's own: an entry calls these where it has
// always made the check, and what only some entries word differently comes in as a parameter.
int need_source(evh_ctx* c, const std::string& W, const EvhFrames& F) {
  if (F.planes ? (!F.yuv || !F.yuv->d_y || !F.yuv->d_cb || !F.yuv->d_cr) : !F.packed)
    return evh_fail(c, EVH_ERR_INVALID, W + "NULL source");
  return EVH_SUCCESS;
}
int need_channels(evh_ctx* c, const std::string& W, const EvhFrames& F) {
  if (F.channels != 1 && F.channels != 3) return evh_fail(c, EVH_ERR_INVALID, W + "channels must be 1 or 3");
  return EVH_SUCCESS;
}
// warp_sample's positions; `what`: "source" or "frame"
int need_below_2_26(evh_ctx* c, const std::string& W, const char* what, int w, int h) {
  if (w >= (1 << 26) || h >= (1 << 26))
    return evh_fail(c, EVH_ERR_CAPACITY, W + what + " sizes stay below 2^26 (positions are held in 1/32 pixels)");
  return EVH_SUCCESS;
}
// the pixels (or runs) of a picture are numbered in 32 bits; `what`: "dw * dh" or "w * h"
int need_area(evh_ctx* c, const std::string& W, const char* what, int w, int h) {
  if ((int64_t)w * h > INT_MAX) return evh_fail(c, EVH_ERR_CAPACITY, W + what + " above INT_MAX");
  return EVH_SUCCESS;
}
// nframes frames of sw x sh onto a canvas of dw x dh: nothing empty
int need_frame_and_canvas(evh_ctx* c, const std::string& W, int nframes, int sw, int sh, int dw, int dh) {
  if (nframes < 0 || sw < 1 || sh < 1 || dw < 1 || dh < 1) return evh_fail(c, EVH_ERR_INVALID, W + "empty frame or canvas");
  return EVH_SUCCESS;
}
// ... and nothing too large, for the entries that ask these three in this order (the warps, the blends, the seam labels, the trail)
int need_canvas_bounds(evh_ctx* c, const std::string& W, int nframes, int sw, int sh, int dw, int dh) {
  if (int rc = need_below_2_26(c, W, "source", sw, sh)) return rc;
  if (int rc = need_area(c, W, "dw * dh", dw, dh)) return rc;
  if (nframes > 65535) return evh_fail(c, EVH_ERR_CAPACITY, W + "at most 65535 frames per call");
  return EVH_SUCCESS;
}
// packed frames only; `apart`: the frame stride is used (more than one frame, or pairs of frames)
int need_source_stride(evh_ctx* c, const std::string& W, const EvhFrames& F, int w, int h, bool apart) {
  const int64_t row = (int64_t)w * F.channels;
  if (!F.planes && (F.row_stride < row || (apart && F.frame_stride < (h - 1) * F.row_stride + row)))
    return evh_fail(c, EVH_ERR_INVALID, W + "source stride smaller than a row / frame");
  return EVH_SUCCESS;
}
int need_planes(evh_ctx* c, const char* who, const EvhFrames& F, int64_t nframes, int w, int h) {
  return F.yuv ? evh_check_yuv420(c, who, F.yuv, (int)nframes, w, h) : EVH_SUCCESS;
}

// A byte range a launch reads or writes.  A NULL or empty span meets nothing.
struct Span { const void* p; int64_t n; const char* name; };
bool meet(const Span& a, const Span& b) {
  const uint8_t* x = (const uint8_t*)a.p; const uint8_t* y = (const uint8_t*)b.p;
  return x && y && a.n > 0 && b.n > 0 && x < y + b.n && y < x + a.n;
}
// the byte ranges of nframes frames: the packed rows, or the three planes; nothing for nframes < 1
void source_spans(const EvhFrames& F, int64_t nframes, int sw, int sh, Span (&out)[3]) {
  out[0] = out[1] = out[2] = {nullptr, 0, "the frames"};
  if (nframes < 1) return;
  if (F.yuv) {
    const evh_yuv420& s = *F.yuv;
    const int64_t cw = (sw + 1) / 2, ch = (sh + 1) / 2, crow = (cw - 1) * s.c_pixel_stride + 1;
    const int64_t yb = (sh - 1) * s.y_stride + sw + (nframes - 1) * s.y_frame_stride;
    const int64_t cb = (ch - 1) * s.c_stride + crow + (nframes - 1) * s.c_frame_stride;
    out[0].p = s.d_y; out[0].n = yb; out[1].p = s.d_cb; out[1].n = cb; out[2].p = s.d_cr; out[2].n = cb;
  } else {
    out[0].p = F.packed; out[0].n = (sh - 1) * F.row_stride + (int64_t)sw * F.channels + (nframes - 1) * F.frame_stride;
  }
}
// every output against every later output and every input
template <int NO, int NI>
int need_apart(evh_ctx* c, const std::string& W, const Span (&outs)[NO], const Span (&ins)[NI]) {
  for (int i = 0; i < NO; i++) {
    for (int j = i + 1; j < NO; j++)
      if (meet(outs[i], outs[j])) return evh_fail(c, EVH_ERR_INVALID, W + outs[i].name + " overlaps " + outs[j].name);
    for (const Span& in : ins)
      if (meet(outs[i], in)) return evh_fail(c, EVH_ERR_INVALID, W + outs[i].name + " overlaps " + in.name);
  }
  return EVH_SUCCESS;
}
int launched(evh_ctx* c) {
  EVH_HIP(c, hipGetLastError());
  return EVH_SUCCESS;
}

}  // namespace
