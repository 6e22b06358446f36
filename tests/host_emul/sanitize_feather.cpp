// Stand-alone memory check of the feather tile programs (t2onet_amd/csrc/t2o_feather_math.h), built by
// tests/test_feather_cpu.py with g++ -fsanitize=address,undefined and run as a program of its own.  TEST HARNESS ONLY.
// Source and destination are heap buffers that end with the plane (and start `offset` bytes in front of it), the
// intermediate and the column pass' LDS image are heap buffers of exactly the sizes the library asks for, the row
// pass' LDS a static object: an index outside any of them is a redzone hit, a misaligned or overflowing operation a
// run-time error.
#include <stdio.h>

#include <vector>

#include "emul_feather.cpp"

int main() {
  const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 9}, {33, 65}, {2 * kFeatherColH + 1, 2 * kFeatherRowW + 1}, {70, 300}, {9, 260}};
  const double sigmas[] = {0, 0.1, 0.5, 2.5, 7, 20, 64};
  unsigned seed = 1;
  for (const auto& s : sizes)
    for (const double sigma : sigmas)
      for (int so = 0; so < 4; ++so) {
        const int h = s[0], w = s[1], oo = (3 * so + 1) % 4;
        std::vector<unsigned char> src(so + (size_t)h * w), out(oo + (size_t)h * w);
        for (auto& b : src) b = (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
        const long long src_offset = so, out_offset = oo;
        if (emul_feather_u8(src.data(), out.data(), &src_offset, &out_offset, &h, &w, &sigma, 1)) return 1;
      }
  printf("feather tile programs: clean\n");
  return 0;
}
