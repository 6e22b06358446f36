// Stand-alone memory check of the selection programs (t2onet_amd/csrc/t2o_select_math.h), built by
// tests/test_select_cpu.py with g++ -fsanitize=address,undefined and run as a program of its own.  TEST HARNESS ONLY.
// The source is a heap buffer that holds `so` bytes, the photo and, straight behind it, one plane, and ends there; the
// destination is a heap buffer that starts `oo` bytes in front of the plane and ends with it: an index outside either is
// a redzone hit, a misaligned or overflowing operation a run-time error.  Every size meets every residue of both
// offsets, every term kind, inversion, and a four-term selection.
#include <stdio.h>

#include <vector>

#include "emul_select.cpp"

static SelectTerm term(int kind, int invert, int a, int b, int c, int d, long long plane_offset = 0) {
  SelectTerm t;
  memset(&t, 0, sizeof(t));
  t.kind = kind; t.invert = invert;
  t.p[0] = a; t.p[1] = b; t.p[2] = c; t.p[3] = d;
  t.plane_offset = plane_offset;
  return t;
}

int main() {
  const int sizes[][2] = {{1, 1}, {1, 5}, {3, 1}, {5, 7}, {37, 53}, {64, 64}, {1, kSelectTilePx + 1}, {kSelectTilePx + 1, 1}, {65, 127}};
  unsigned seed = 1;
  for (const auto& s : sizes)
    for (int so = 0; so < 4; ++so)
      for (int oo = 0; oo < 4; ++oo) {
        const int h = s[0], w = s[1];
        const long long n = (long long)h * w;
        std::vector<unsigned char> src(so + 4 * (size_t)n), out(oo + (size_t)n);
        for (auto& b : src) b = (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
        const long long plane = so + 3 * n;
        const SelectTerm all[] = {term(SELECT_LUM, 0, 128, 255, 32, 0),      term(SELECT_SAT, 1, 0, 96, 48, 0),
                                  term(SELECT_HUE, 0, 1365, 171, 128, 0),    term(SELECT_LINEAR, 0, 0, 0, w - 1, h, 0),
                                  term(SELECT_LINEAR, 1, -70000, 3, 90000, -5), term(SELECT_RADIAL, 0, w / 2, h / 2, 0, (h < w ? h : w) / 2 + 1),
                                  term(SELECT_RADIAL, 0, -100000, 131070, 5000, 131070), term(SELECT_PLANE, 1, 0, 0, 0, 0, plane),
                                  term(SELECT_LUM, 0, 0, 255, 0, 0)};
        const int count = (int)(sizeof(all) / sizeof(all[0]));
        for (int first = 0; first < count; ++first) {
          SelectJob j;
          memset(&j, 0, sizeof(j));
          j.src_offset = so; j.out_offset = oo; j.h = h; j.w = w;
          j.n_terms = first % 3 == 2 ? 4 : 1;                                // every third job multiplies four terms
          for (int t = 0; t < j.n_terms; ++t) j.terms[t] = all[(first + 2 * t) % count];
          if (emul_select_u8(src.data(), out.data(), &j, 1)) return 1;
        }
      }
  printf("select programs: clean\n");
  return 0;
}
