// evh_pixels.h -- where a kernel's source pixels come from, for the units whose kernels read frames (evh_image.hip,
// evh_plane.hip): packed rows or decoded 4:2:0 planes, the conversion of the latter, and cvtColor's gray weights.
// Everything sits in an unnamed namespace on purpose: the kernels templated on these types are local to their unit, and
// their names stay what they were when the types lived in evh_image.hip.
#pragma once
#include "evh_internal.h"

namespace {

__device__ __forceinline__ uint8_t gray_of(int b, int g, int r) { return (uint8_t)((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14); }
__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

// The kernels are templated on where a source pixel's channel bytes come from: SRC::row(img, y) hands out a row,
// Row::px(x, v) the pixel's bytes v[0 .. channels).
struct PackedSrc {       // rows of cn bytes per pixel (BGR or gray)
  const uint8_t* p; int cn; int64_t stride, img_stride;
  struct Row {
    const uint8_t* r; int cn;
    __device__ __forceinline__ void px(int x, int (&v)[3]) const {
      const uint8_t* q = r + (int64_t)x * cn;
#pragma unroll
      for (int c = 0; c < 3; c++) if (c < cn) v[c] = q[c];
    }
  };
  __device__ __forceinline__ int channels() const { return cn; }
  __device__ __forceinline__ Row row(int img, int y) const { return {p + (int64_t)img * img_stride + (int64_t)y * stride, cn}; }
};

// yuv420p -> bgr24 as capture.read() delivers it (video_processing.py:58,70; EVCAP_BGR_SWSCALE_X86 of include/evcap.h,
// SwsX86::px in capture/evcap_api.cpp): 13-bit BT.601 limited-range coefficients, arithmetic shifts, one saturation per
// channel (the 16-bit saturations of the original never act).  The chroma terms are shared by the luma pixels of a sample.
struct ChromaTerms { int b, g, r; };
__device__ __forceinline__ ChromaTerms chroma_terms(int u, int v) {
  const int cu = (u << 3) - 1024, cv = (v << 3) - 1024;
  return {(cu * 16525) >> 16, ((cu * -3209) >> 16) + ((cv * -6660) >> 16), (cv * 13075) >> 16};
}
__device__ __forceinline__ void yuv_px(int y, const ChromaTerms& t, int (&v)[3]) {
  const int Y = (((y << 3) - 128) * 9539) >> 16;
  v[0] = sat8(Y + t.b); v[1] = sat8(Y + t.g); v[2] = sat8(Y + t.r);
}
struct Yuv420Src {       // 4:2:0 planes, chroma pixel stride cps = 1 (I420 / YV12) or 2 (NV12 / NV21)
  const uint8_t* y; const uint8_t* cb; const uint8_t* cr;
  int64_t ys, cs, yfs, cfs; int cps;
  struct Row {
    const uint8_t* y; const uint8_t* cb; const uint8_t* cr; int cps;
    __device__ __forceinline__ void px(int x, int (&v)[3]) const {
      const int cx = (x >> 1) * cps;
      yuv_px(y[x], chroma_terms(cb[cx], cr[cx]), v);
    }
  };
  __device__ __forceinline__ int channels() const { return 3; }
  __device__ __forceinline__ Row row(int img, int yy) const {
    const int64_t co = (int64_t)img * cfs + (int64_t)(yy >> 1) * cs;
    return {y + (int64_t)img * yfs + (int64_t)yy * ys, cb + co, cr + co, cps};
  }
};

// the host's descriptions as the kernels take them
inline Yuv420Src yuv420_src(const evh_yuv420& s) {
  return {s.d_y, s.d_cb, s.d_cr, s.y_stride, s.c_stride, s.y_frame_stride, s.c_frame_stride, s.c_pixel_stride};
}
inline PackedSrc packed_src(const EvhFrames& F) { return {F.packed, F.channels, F.row_stride, F.frame_stride}; }

}  // namespace
