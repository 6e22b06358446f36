// Host emulation of the resident-set gather (t2onet_amd/csrc/t2o_resident.hip), compiled with g++ by
// tests/test_resident_cpu.py.  TEST HARNESS ONLY: the thread program of t2o_resident_math.h -- the one the kernel runs --
// for every thread of every workgroup of the grid the entry point launches (threads past a picture's end included: they
// must return without a store), behind the entry point's own argument check.
#include "../../t2onet_amd/csrc/t2o_resident_math.h"

using namespace t2o;

extern "C" int emul_gather_u8_to_f32(const unsigned char* store, const long long* slot_offsets, const long long* index, int N, int K,
                                     int B, int h, int w, float* out_x, float* out_ys) {
  long long per_image = 0;
  const char* why = "";
  if (gather_check(store, slot_offsets, index, N, K, B, h, w, out_x, out_ys, &per_image, &why)) return 1;
  GatherArgs a;
  a.store = store; a.slots = slot_offsets; a.index = index; a.out_x = out_x; a.out_ys = out_ys;
  a.hw = (long long)h * w; a.blocks_per_image = (unsigned)per_image; a.N = N; a.K = K; a.B = B;
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < K; ++k)
      for (long long t = 0; t < per_image * kGatherThreads; ++t) gather_thread(a, b, k, t);
  return 0;
}
