// Per-pixel integer arithmetic of the image I/O kernels (t2o_image_io.hip): OpenCV's 8-bit INTER_LINEAR resize as
// t2onet_amd/data.py:resize_linear_u8 restates it (what the reference's loaders call: utils/visual_utils.py:6-47), the
// /255 conversion behind it, and the * 255 truncation of utils/visual_utils.py:50-58 in the other direction.
//
// Like t2o_pixel_math.h every function is `__host__ __device__`: tests/host_emul/emul_image.cpp compiles the SAME
// functions with g++, so the arithmetic is held to the numpy statement bit for bit on a machine without a GPU.  The
// fp64 tap expression is evaluated in numpy's operation order, one rounding per step (-ffp-contract=off).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define T2O_IMG_HD __host__ __device__ __forceinline__
#else
#define T2O_IMG_HD static inline
#endif

namespace t2o {

enum : int {
  RESIZE_ZERO = 0,     // descriptor with h = w = 0: an absent image, the output is zero
  RESIZE_COPY = 1,     // source size == output size: plain convert
  RESIZE_MEAN2 = 2,    // exact 2x shrink both ways: rounded mean of each 2x2 block
  RESIZE_LINEAR = 3    // everything else
};

struct ResizeTap {
  int i0, i1;          // the two source indices
  int c0, c1;          // their 11-bit fixed-point weights, c0 + c1 == 2048
};

T2O_IMG_HD int resize_mode(int H, int W, int out_h, int out_w) {
  if (H <= 0 || W <= 0) return RESIZE_ZERO;
  if (H == out_h && W == out_w) return RESIZE_COPY;
  if (H == 2 * out_h && W == 2 * out_w) return RESIZE_MEAN2;
  return RESIZE_LINEAR;
}

// taps() of resize_linear_u8 for destination index d: half-pixel centres in fp64, both clamps set the fraction to 0,
// rint = round half to even (cvRound).
T2O_IMG_HD ResizeTap resize_tap(int d, int n_src, int n_dst) {
  const double scale = (double)n_src / (double)n_dst;
  double f = ((double)d + 0.5) * scale - 0.5;
  const double fl = floor(f);
  long long i0 = (long long)fl;
  f = f - fl;
  if (i0 < 0) { f = 0.0; i0 = 0; }
  if (i0 >= n_src - 1) { f = 0.0; i0 = n_src - 1; }
  ResizeTap t;
  t.i0 = (int)i0;
  t.i1 = t.i0 + 1 < n_src - 1 ? t.i0 + 1 : n_src - 1;
  t.c1 = (int)rint(f * 2048.0);
  t.c0 = (int)rint((1.0 - f) * 2048.0);
  return t;
}

// horizontal pass in int32, then ((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2, for the 3 channels of one pixel
T2O_IMG_HD void resize_linear_px(const unsigned char* src, int W, const ResizeTap& ty, const ResizeTap& tx, int rgb[3]) {
  const unsigned char* r0 = src + (size_t)ty.i0 * W * 3;
  const unsigned char* r1 = src + (size_t)ty.i1 * W * 3;
  const size_t x0 = (size_t)tx.i0 * 3, x1 = (size_t)tx.i1 * 3;
  for (int c = 0; c < 3; ++c) {
    const int S0 = (int)r0[x0 + c] * tx.c0 + (int)r0[x1 + c] * tx.c1;
    const int S1 = (int)r1[x0 + c] * tx.c0 + (int)r1[x1 + c] * tx.c1;
    int v = (((ty.c0 * (S0 >> 4)) >> 16) + ((ty.c1 * (S1 >> 4)) >> 16) + 2) >> 2;
    v = v < 0 ? 0 : v;
    rgb[c] = v > 255 ? 255 : v;
  }
}

T2O_IMG_HD void resize_mean2_px(const unsigned char* src, int W, int y, int x, int rgb[3]) {
  const unsigned char* r0 = src + ((size_t)(2 * y) * W + 2 * x) * 3;
  const unsigned char* r1 = r0 + (size_t)W * 3;
  for (int c = 0; c < 3; ++c) rgb[c] = ((int)r0[c] + (int)r0[3 + c] + (int)r1[c] + (int)r1[3 + c] + 2) >> 2;
}

T2O_IMG_HD void resize_copy_px(const unsigned char* src, int W, int y, int x, int rgb[3]) {
  const unsigned char* p = src + ((size_t)y * W + x) * 3;
  for (int c = 0; c < 3; ++c) rgb[c] = p[c];
}

// astype(float32) / 255.0: the correctly rounded fp32 quotient (IEEE division on both sides of the build)
T2O_IMG_HD float u8_to_unit(int v) { return (float)v / 255.0f; }

// (t * 255).astype(uint8) for t in [0, 1]: one fp32 product, truncated
T2O_IMG_HD unsigned char unit_to_u8(float v) { return (unsigned char)(int)(v * 255.0f); }

// one output pixel (y, x) of an (H, W, 3) source resized to (out_h, out_w): the whole per-pixel program
T2O_IMG_HD void resize_pixel(const unsigned char* src, int H, int W, int out_h, int out_w, int y, int x, float out[3]) {
  int rgb[3] = {0, 0, 0};
  const int mode = resize_mode(H, W, out_h, out_w);
  if (mode == RESIZE_COPY) {
    resize_copy_px(src, W, y, x, rgb);
  } else if (mode == RESIZE_MEAN2) {
    resize_mean2_px(src, W, y, x, rgb);
  } else if (mode == RESIZE_LINEAR) {
    resize_linear_px(src, W, resize_tap(y, H, out_h), resize_tap(x, W, out_w), rgb);
  }
  for (int c = 0; c < 3; ++c) out[c] = u8_to_unit(rgb[c]);
}

}  // namespace t2o
