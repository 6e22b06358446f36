// Stand-alone memory check of the morph tile programs (t2onet_amd/csrc/t2o_morph_math.h), built by
// tests/test_morph_cpu.py with g++ -fsanitize=address,undefined and run as a program of its own.  TEST HARNESS ONLY.
// Source and destination are heap buffers that end with the plane (and start `offset` bytes in front of it), the fields a
// heap buffer of exactly the size the library asks for, the two LDS images static objects: an index outside any of them
// is a redzone hit, a misaligned or overflowing operation a run-time error.
#include <stdio.h>

#include <vector>

#include "emul_morph.cpp"

int main() {
  const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {5, 9}, {63, 65}, {65, 63}, {2 * kMorphColH + 1, kMorphRowW + 3}, {9, 2 * kMorphRowW + 1}};
  const int radii[] = {0, 1, 2, 5, 25, 63, 64};
  unsigned seed = 1;
  for (const auto& s : sizes)
    for (const int radius : radii)
      for (int mode = kMorphGrow; mode <= kMorphBorder; ++mode)
        for (int so = 0; so < 4; ++so) {
          const int h = s[0], w = s[1], oo = (3 * so + 1) % 4;
          std::vector<unsigned char> src(so + (size_t)h * w), out(oo + (size_t)h * w);
          for (auto& b : src) b = (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
          const long long src_offset = so, out_offset = oo;
          if (emul_morph_u8(src.data(), out.data(), &src_offset, &out_offset, &h, &w, &radius, &mode, 1, so & 1)) return 1;
        }
  printf("morph tile programs: clean\n");
  return 0;
}
