// Stand-alone memory check of the fill programs (t2onet_amd/csrc/t2o_fill_math.h), built by tests/test_fill_cpu.py with
// g++ -fsanitize=address,undefined and run as a program of its own.  TEST HARNESS ONLY.
// The photo is a heap buffer that starts `po` bytes in front of the photo and ends with it, the plane one that starts `mo`
// bytes in front of the plane and ends with it, the destination likewise with `oo`; the workspace has exactly the size the
// arrays take: an index outside any of them is a redzone hit, a misaligned or overflowing operation a run-time error.
// Every size meets every residue of the three offsets and four kinds of plane (scattered, a hole, one known pixel, none),
// out of place and in place, in both thread orders, which must agree byte for byte; kept pixels must come out as they were.
#include <stdio.h>

#include <vector>

#include "emul_fill.cpp"

int main() {
  const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {5, 6}, {37, 53}, {64, 64}, {kFillTile + 1, kFillTile + 3}, {2 * kFillTile + 1, kFillTile - 1},
                          {3, 4 * kFillTile + 5}, {4 * kFillTile + 2, 2}, {2 * kFillTile + 7, 2 * kFillTile + 2}};
  unsigned seed = 1;
  int run = 0;
  for (const auto& s : sizes)
    for (int k = 0; k < 4; ++k)
      for (int kind = 0; kind < 4; ++kind, ++run) {
        const int h = s[0], w = s[1];
        const size_t n = (size_t)h * w;
        const long long po = k, mo = (k + kind + 1) & 3, oo = (3 * k + run / 4 + 1) & 3;
        std::vector<unsigned char> photo(po + 3 * n), plane(mo + n);
        for (size_t i = 0; i < 3 * n; ++i) photo[po + i] = (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
        for (size_t i = 0; i < n; ++i) {
          const unsigned r = (seed = seed * 1664525u + 1013904223u) >> 16;
          const int y = (int)(i / w), x = (int)(i % w);
          unsigned char m = 0;
          if (kind == 0) m = (r & 15) == 0 ? (unsigned char)(r >> 8) : 0;
          if (kind == 1) m = (y >= h / 3 && x >= w / 4) ? 255 : 0;
          if (kind == 2) m = i == n - 1 ? 0 : (unsigned char)(1 + (r >> 8) % 255);
          if (kind == 3) m = (unsigned char)(1 + (r >> 8) % 255);
          plane[mo + i] = m;
        }
        const int hh[1] = {h}, ww[1] = {w};
        std::vector<unsigned char> first;
        for (int order = 0; order < 2; ++order) {
          std::vector<unsigned char> out(oo + 3 * n, 0xA5);
          if (emul_fill_u8(photo.data(), plane.data(), out.data(), &po, &mo, &oo, hh, ww, 1, order)) return 1;
          for (size_t i = 0; i < n; ++i)
            if (plane[mo + i] == 0 || kind == 3)
              for (int c = 0; c < 3; ++c)
                if (out[oo + 3 * i + c] != photo[po + 3 * i + c]) { printf("a kept pixel changed\n"); return 2; }
          if (order == 0) first = out;
          if (out != first) { printf("the thread orders differ\n"); return 2; }
        }
        std::vector<unsigned char> same(photo);                       // in place: the photo is its own destination
        if (emul_fill_u8(same.data(), plane.data(), same.data(), &po, &mo, &po, hh, ww, 1, 1)) return 1;
        for (size_t i = 0; i < 3 * n; ++i)
          if (same[po + i] != first[oo + i]) { printf("in place differs\n"); return 2; }
      }
  printf("fill programs: clean\n");
  return 0;
}
