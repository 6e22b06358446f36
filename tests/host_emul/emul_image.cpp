// Host emulation of the image I/O kernels' per-pixel program (t2onet_amd/csrc/t2o_image_math.h), compiled with g++ by
// tests/test_image_io_cpu.py.  TEST HARNESS ONLY: the same functions the HIP kernels run, looped over the pixels here.
#include "../../t2onet_amd/csrc/t2o_image_math.h"

extern "C" {

// out (3, out_h, out_w) fp32 planar from src (H, W, 3) uint8: k_resize_u8_f32 for one image
int emul_resize_u8_f32(const unsigned char* src, int H, int W, int out_h, int out_w, float* out) {
  for (int y = 0; y < out_h; ++y)
    for (int x = 0; x < out_w; ++x) {
      float px[3];
      t2o::resize_pixel(src, H, W, out_h, out_w, y, x, px);
      for (int c = 0; c < 3; ++c) out[((size_t)c * out_h + y) * out_w + x] = px[c];
    }
  return 0;
}

// out (n) uint8 from values (n) fp32: k_f32_u8_hwc's conversion, element by element
int emul_unit_to_u8(const float* v, long long n, unsigned char* out) {
  for (long long i = 0; i < n; ++i) out[i] = t2o::unit_to_u8(v[i]);
  return 0;
}

}  // extern "C"
