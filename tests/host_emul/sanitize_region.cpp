// Stand-alone memory check of the region programs (t2onet_amd/csrc/t2o_region_math.h), built by
// tests/test_region_cpu.py with g++ -fsanitize=address,undefined and run as a program of its own.  TEST HARNESS ONLY.
// The photo is a heap buffer that starts `po` bytes in front of the photo and ends with it, the destination one that
// starts `oo` bytes in front of the plane and ends with it; the workspace has exactly the size the library asks for: an
// index outside any of them is a redzone hit, a misaligned or overflowing operation a run-time error.  Every size meets
// every residue of the two offsets, both connectivities and three tolerances, on two-colour noise near the percolation
// threshold, in the three lane orders, which must agree byte for byte.
#include <stdio.h>

#include <vector>

#include "emul_region.cpp"

int main() {
  const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 6}, {37, 53}, {64, 64}, {kRegionTile + 1, kRegionTile + 3}, {2 * kRegionTile + 1, kRegionTile - 1},
                          {3, 4 * kRegionTile + 5}};
  const int tols[] = {0, 10, 255};
  unsigned seed = 1;
  int run = 0;
  for (const auto& s : sizes)
    for (int k = 0; k < 4; ++k)
      for (int c = 4; c <= 8; c += 4, ++run) {
        const int h = s[0], w = s[1];
        const long long n = (long long)h * w;
        const long long po = k, oo = (3 * k + run / 4 + 1) & 3;
        std::vector<unsigned char> photo(po + 3 * (size_t)n);
        for (size_t i = 0; i < (size_t)n; ++i) {
          const bool on = ((seed = seed * 1664525u + 1013904223u) >> 24) < (run & 1 ? 150u : 128u);
          for (int ch = 0; ch < 3; ++ch) photo[po + 3 * i + ch] = (unsigned char)(on ? 200 - 40 * ch + (int)((seed >> (8 + 2 * ch)) & 3) : 20 + 30 * ch);
        }
        const int hh[1] = {h}, ww[1] = {w}, sx[1] = {(int)((seed >> 8) % (unsigned)w)}, sy[1] = {(int)((seed >> 16) % (unsigned)h)};
        const int tt[1] = {tols[run % 3]}, cc[1] = {c};
        std::vector<unsigned char> first;
        for (int order = 0; order < 3; ++order) {
          std::vector<unsigned char> out(oo + (size_t)n);
          if (emul_region_u8(photo.data(), out.data(), &po, &oo, hh, ww, sx, sy, tt, cc, 1, order, nullptr)) return 1;
          if (out[oo + (size_t)sy[0] * w + sx[0]] != 255) { printf("the seed is not selected\n"); return 2; }
          if (order == 0) first = out;
          for (size_t i = 0; i < (size_t)n; ++i)
            if (out[oo + i] != first[oo + i]) { printf("the lane orders differ\n"); return 2; }
        }
      }
  printf("region programs: clean\n");
  return 0;
}
