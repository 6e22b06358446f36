// Stand-alone memory check of the stencils replay tile program (t2onet_amd/csrc/t2o_replay_stencils_math.h), built by
// tests/test_replay_stencils_cpu.py with g++ -fsanitize=address,undefined and run as a program of its own.  TEST HARNESS
// ONLY.  The LDS structs (both instances) are heap objects of exactly their size; source, destination and mask planes are heap buffers that
// start `offset` bytes in front of the picture and end with it: an index outside any of them is a redzone hit, a
// misaligned or overflowing operation a run-time error.
#include <stdio.h>

#include <memory>
#include <vector>

#include "emul_replay_stencils.cpp"

int main() {
  const int sizes[][2] = {{1, 1}, {3, 3}, {33, 65}};
  const int eight[8] = {6, 6, 6, 6, 6, 6, 6, 6};
  const int masked[8] = {1, 6, 6, 0, 0, 0, 0, 0}, masked_of[8] = {0, 1, 0, -1, -1, -1, -1, -1};
  std::unique_ptr<ReplayStLds> lds(new ReplayStLds);
  std::unique_ptr<ReplayStLdsSmall> small(new ReplayStLdsSmall);
  unsigned seed = 1;
  for (const auto& s : sizes)
    for (int so = 0; so < 4; ++so) {
      const int h = s[0], w = s[1], oo = (3 * so + 1) % 4, mo = (so + 2) % 4;
      const size_t n = (size_t)h * w;
      std::vector<unsigned char> src(so + 3 * n), out(oo + 3 * n), masks(mo + n + 1 + n);
      for (auto& b : src) b = (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
      for (auto& b : masks) b = (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
      std::vector<float> params(8 * 24, 0.0f);
      for (int k = 0; k < 8; ++k) params[24 * k] = 0.1f + 0.05f * k;
      if (replay_stencils_run(*lds, src.data(), so, out.data(), oo, h, w, 8, eight, nullptr, params.data(), nullptr, nullptr, 0)) return 1;
      const long long offs[2] = {mo, mo + (long long)n + 1};
      if (replay_stencils_run(*lds, src.data(), so, out.data(), oo, h, w, 4, masked, masked_of, params.data(), masks.data(), offs, 2)) return 1;
      if (replay_stencils_run(*small, src.data(), so, out.data(), oo, h, w, 4, masked, masked_of, params.data(), masks.data(), offs, 2)) return 1;
      if (replay_stencils_run(*small, src.data(), so, out.data(), oo, h, w, 2, eight, nullptr, params.data(), nullptr, nullptr, 0)) return 1;
    }
  printf("replay stencils tile program: clean\n");
  return 0;
}
