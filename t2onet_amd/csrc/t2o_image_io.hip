// t2o_image_io.hip -- the data step's pixel work on the device, in both directions.
//
//   k_resize_u8_f32   N decoded uint8 HWC images of DIFFERING sizes, packed back to back in one byte buffer, to one
//                     (N,3,out_h,out_w) fp32 planar tensor in [0,1]: cv2.resize's 8-bit INTER_LINEAR followed by
//                     astype(float32).transpose(2,0,1) / 255 (utils/visual_utils.py:6-47), bit for bit what
//                     data.resize_linear_u8 + the numpy conversion give.  ONE launch for the whole batch: the grid runs
//                     over output tiles x images, a device-side descriptor table says where each image lies.  No atomics,
//                     no host synchronisation; every output element is written exactly once.
//   k_f32_u8_hwc      (N,3,H,W) fp32 in [0,1] to (N,H,W,3) uint8, * 255 truncated (utils/visual_utils.py:50-58): what an
//                     image writer needs, so that bytes and not floats cross the bus.
//
// Thread-to-pixel mapping of the resize: a workgroup owns a 64 x 16 output tile, lane = x.  The three plane stores of a
// wave are 256 contiguous bytes each (the coalesced side).  The source side is a gather of single bytes at arbitrary
// byte offsets -- byte loads only, nothing is assumed about alignment; neighbouring lanes read neighbouring (when
// shrinking: strided) source pixels of the same two rows, which the cache serves.  A thread evaluates its column's fp64
// tap once and walks 4 rows with it.
#include <hip/hip_runtime.h>

#include "t2o_image_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

namespace {

constexpr int kTileW = 64, kTileH = 16, kResizeThreads = 256;
constexpr int kRowsPerThread = kTileH / (kResizeThreads / kTileW);     // 4

__global__ __launch_bounds__(kResizeThreads) void k_resize_u8_f32(const unsigned char* __restrict__ src,
                                                                   const t2o_image_desc_t* __restrict__ descs, int tiles_x,
                                                                   int tiles, int out_h, int out_w, float* __restrict__ out) {
  const int n = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const t2o_image_desc_t d = descs[n];
  const int H = d.h, W = d.w;
  const unsigned char* img = src + d.offset;
  const int x = (tile % tiles_x) * kTileW + (threadIdx.x & (kTileW - 1));
  const int y_first = (tile / tiles_x) * kTileH + (threadIdx.x / kTileW);
  if (x >= out_w) return;
  const size_t plane = (size_t)out_h * out_w;
  float* o = out + (size_t)n * 3 * plane + x;
  const int mode = resize_mode(H, W, out_h, out_w);                     // (uniform over the workgroup)
  ResizeTap tx = {};
  if (mode == RESIZE_LINEAR) tx = resize_tap(x, W, out_w);
#pragma unroll
  for (int r = 0; r < kRowsPerThread; ++r) {
    const int y = y_first + r * (kResizeThreads / kTileW);
    if (y >= out_h) break;
    int rgb[3] = {0, 0, 0};
    if (mode == RESIZE_LINEAR) resize_linear_px(img, W, resize_tap(y, H, out_h), tx, rgb);
    else if (mode == RESIZE_MEAN2) resize_mean2_px(img, W, y, x, rgb);
    else if (mode == RESIZE_COPY) resize_copy_px(img, W, y, x, rgb);
    float* p = o + (size_t)y * out_w;
    p[0] = u8_to_unit(rgb[0]);
    p[plane] = u8_to_unit(rgb[1]);
    p[2 * plane] = u8_to_unit(rgb[2]);
  }
}

constexpr int kPackThreads = 256;

// The (image, channel, pixel) position of flat output byte j = ((n * hw + p) * 3 + c), stepped byte by byte.
struct PackPos {
  size_t n, p;
  unsigned c;
};

__device__ __forceinline__ PackPos pack_pos(size_t j, size_t hw) {
  const size_t px = j / 3;
  PackPos q;
  q.c = (unsigned)(j - px * 3);
  q.n = px / hw;
  q.p = px - q.n * hw;
  return q;
}

__device__ __forceinline__ unsigned pack_next(const float* __restrict__ img, PackPos& q, size_t hw) {
  const unsigned b = unit_to_u8(img[(q.n * 3 + q.c) * hw + q.p]);
  if (++q.c == 3) {
    q.c = 0;
    if (++q.p == hw) { q.p = 0; ++q.n; }
  }
  return b;
}

// One thread per 4 output bytes.  ALIGNED (the output address is a multiple of 4): one dword store per thread;
// otherwise, and for the last total % 4 bytes, byte stores.
template <bool ALIGNED>
__global__ __launch_bounds__(kPackThreads) void k_f32_u8_hwc(const float* __restrict__ img, size_t hw, size_t total,
                                                             unsigned char* __restrict__ out) {
  const size_t j = ((size_t)blockIdx.x * kPackThreads + threadIdx.x) * 4;
  if (j >= total) return;
  PackPos q = pack_pos(j, hw);
  if (j + 4 <= total) {
    const unsigned b0 = pack_next(img, q, hw), b1 = pack_next(img, q, hw), b2 = pack_next(img, q, hw), b3 = pack_next(img, q, hw);
    if (ALIGNED) {
      *reinterpret_cast<unsigned*>(out + j) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    } else {
      out[j] = (unsigned char)b0;
      out[j + 1] = (unsigned char)b1;
      out[j + 2] = (unsigned char)b2;
      out[j + 3] = (unsigned char)b3;
    }
  } else {
    for (size_t k = j; k < total; ++k) out[k] = (unsigned char)pack_next(img, q, hw);
  }
}

}  // namespace

extern "C" {

int t2o_resize_u8_to_f32(const unsigned char* src, const t2o_image_desc_t* descs, int n, int out_h, int out_w, float* out,
                         void* stream) {
  if (!src || !descs || !out) return set_error(T2O_EINVAL, "resize_u8_to_f32: null pointer");
  if (n <= 0) return set_error(T2O_EINVAL, "resize_u8_to_f32: n must be positive");
  if (out_h <= 0 || out_w <= 0) return set_error(T2O_EINVAL, "resize_u8_to_f32: out_h and out_w must be positive");
  if ((size_t)descs & 7) return set_error(T2O_EINVAL, "resize_u8_to_f32: descriptor table must be 8-byte aligned");
  const long long tiles_x = (out_w + kTileW - 1) / kTileW, tiles_y = (out_h + kTileH - 1) / kTileH;
  const long long tiles = tiles_x * tiles_y;
  if (tiles * n > 0x7fffffffll) return set_error(T2O_EINVAL, "resize_u8_to_f32: more than 2^31 - 1 output tiles");
  k_resize_u8_f32<<<(unsigned)(tiles * n), kResizeThreads, 0, (hipStream_t)stream>>>(src, descs, (int)tiles_x, (int)tiles, out_h,
                                                                                    out_w, out);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "resize_u8_to_f32 launch failed");
}

int t2o_f32_to_u8_hwc(const float* img, int n, int h, int w, unsigned char* out, void* stream) {
  if (!img || !out) return set_error(T2O_EINVAL, "f32_to_u8_hwc: null pointer");
  if (n <= 0) return set_error(T2O_EINVAL, "f32_to_u8_hwc: n must be positive");
  if (h <= 0 || w <= 0) return set_error(T2O_EINVAL, "f32_to_u8_hwc: h and w must be positive");
  const size_t hw = (size_t)h * w, total = hw * 3 * (size_t)n;
  const size_t blocks = (total + (size_t)kPackThreads * 4 - 1) / ((size_t)kPackThreads * 4);
  if (blocks > 0x7fffffffull) return set_error(T2O_EINVAL, "f32_to_u8_hwc: batch too large");
  if (((size_t)out & 3) == 0)
    k_f32_u8_hwc<true><<<(unsigned)blocks, kPackThreads, 0, (hipStream_t)stream>>>(img, hw, total, out);
  else
    k_f32_u8_hwc<false><<<(unsigned)blocks, kPackThreads, 0, (hipStream_t)stream>>>(img, hw, total, out);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "f32_to_u8_hwc launch failed");
}

}  // extern "C"
