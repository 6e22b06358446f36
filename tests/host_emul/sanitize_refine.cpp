// Stand-alone memory check of the refine programs (t2onet_amd/csrc/t2o_refine_math.h), built by
// tests/test_refine_cpu.py with g++ -fsanitize=address,undefined and run as a program of its own.  TEST HARNESS ONLY.
// The photo is a heap buffer that starts `po` bytes in front of the photo and ends with it, the plane one that starts
// `so` bytes in front of the plane and ends with it, the destination likewise with `oo`; the workspace has exactly the
// size the library asks for: an index outside any of them is a redzone hit, a misaligned or overflowing operation a
// run-time error.  Every size meets every residue of the three offsets (rotating together), every radius and both ends of
// E, on random bytes and on the plane that falls where the guide rises (negative numerators).
#include <stdio.h>

#include <vector>

#include "emul_refine.cpp"

int main() {
  const int sizes[][2] = {{1, 1}, {1, 5}, {3, 1}, {5, 7}, {37, 53}, {64, 64}, {kRefineRowH + 1, kRefineRowW + 1}, {kRefineColH + 1, kRefineColW + 1}};
  const int radii[] = {0, 1, 2, 7, 64};
  const int eps2[] = {1, 26, 65025};
  unsigned seed = 1;
  int run = 0;
  for (const auto& s : sizes)
    for (int r : radii)
      for (int k = 0; k < 4; ++k, ++run) {
        const int h = s[0], w = s[1];
        const long long n = (long long)h * w;
        const long long po = k, so = (k + run) & 3, oo = (3 * k + run / 4 + 1) & 3;
        std::vector<unsigned char> photo(po + 3 * (size_t)n), src(so + (size_t)n), out(oo + (size_t)n);
        for (auto& b : photo) b = (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
        for (size_t i = 0; i < (size_t)n; ++i) {
          const int L = select_lum(photo[po + 3 * i], photo[po + 3 * i + 1], photo[po + 3 * i + 2]);
          src[so + i] = run & 1 ? (unsigned char)(255 - L) : (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
        }
        const int hh[1] = {h}, ww[1] = {w}, rr[1] = {r}, ee[1] = {eps2[run % 3]};
        if (emul_refine_u8(photo.data(), src.data(), out.data(), &po, &so, &oo, hh, ww, rr, ee, 1)) return 1;
        if (run % 5 == 0) {                                            // in place
          std::vector<unsigned char> buf(src);
          if (emul_refine_u8(photo.data(), buf.data(), buf.data(), &po, &so, &so, hh, ww, rr, ee, 1)) return 1;
          for (size_t i = 0; i < (size_t)n; ++i)
            if (buf[so + i] != out[oo + i]) { printf("in place differs\n"); return 2; }
        }
      }
  printf("refine programs: clean\n");
  return 0;
}
