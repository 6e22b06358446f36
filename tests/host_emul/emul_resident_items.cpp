// Host emulation of the resident-item gather (t2onet_amd/csrc/t2o_resident_items.hip), compiled with g++ by
// tests/test_resident_gier_cpu.py.  TEST HARNESS ONLY: items_thread of t2o_resident_items_math.h -- the one the kernel runs
// -- for every thread of every workgroup of the flat grid the entry point launches (picture workgroups, then the row
// workgroups; threads past a picture's or the table's end included: they must return without a store), behind the entry
// point's own argument check.  Returns 0, or 1 when the check refuses; *grid (may be NULL) receives the workgroup count.
#include "../../t2onet_amd/csrc/t2o_resident_items_math.h"

using namespace t2o;

extern "C" int emul_gather_items_u8_to_f32(const unsigned char* store, const long long* slot_offsets, const long long* index, int N,
                                           int K, int B, int h, int w, float* out_x, float* out_ys, const int* rows, int V,
                                           int* out_rows, long long* grid) {
  ItemsArgs a;
  const char* why = "";
  if (items_check(store, slot_offsets, index, N, K, B, h, w, out_x, out_ys, rows, V, out_rows, &a, &why)) return 1;
  const unsigned blocks = a.picture_blocks + a.row_blocks;
  if (grid) *grid = blocks;
  for (unsigned block = 0; block < blocks; ++block)
    for (unsigned thread = 0; thread < (unsigned)kGatherThreads; ++thread) items_thread(a, block, thread);
  return 0;
}

// The workgroup count the entry point would launch for these sizes, or -1 where its check refuses them (no thread runs).
extern "C" long long emul_items_grid(int N, int K, int B, int h, int w, int V) {
  alignas(16) static unsigned char some[16];
  ItemsArgs a;
  const char* why = "";
  const int* rows = V > 0 ? reinterpret_cast<const int*>(some) : nullptr;
  if (items_check(some, reinterpret_cast<const long long*>(some), reinterpret_cast<const long long*>(some), N, K, B, h, w,
                  reinterpret_cast<float*>(some), reinterpret_cast<float*>(some), rows, V, const_cast<int*>(rows), &a, &why))
    return -1;
  return (long long)a.picture_blocks + a.row_blocks;
}
