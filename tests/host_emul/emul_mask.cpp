// Host emulation of the mask kernels (t2onet_amd/csrc/t2o_mask.hip), compiled with g++ by tests/test_mask_cpu.py.
// TEST HARNESS ONLY: the thread programs of t2o_mask_math.h -- the ones the kernels run -- for every thread of every
// workgroup of the grid the entry points launch (threads past a plane's end included: they must return without a store).
#include <string.h>

#include "../../t2onet_amd/csrc/t2o_mask_math.h"

using namespace t2o;

extern "C" {

// t2o_rle_union_u8 with host memory throughout: `tables` laid out as the entry point expects them
int emul_rle_union_u8(const void* tables, int n_jobs, int n_masks, int n_sel, long long n_ends, unsigned char* out, long long out_bytes) {
  if (!tables || !out || n_jobs <= 0 || n_masks < 0 || n_sel < 0 || n_ends < 0 || out_bytes <= 0) return 1;
  const size_t at_masks = sizeof(UnionJob) * (size_t)n_jobs, at_sel = at_masks + sizeof(RleMask) * (size_t)n_masks,
               at_ends = at_sel + sizeof(int) * (size_t)n_sel;
  const char* h = (const char*)tables;
  UnionArgs a;
  a.jobs = (const UnionJob*)h; a.masks = (const RleMask*)(h + at_masks); a.sel = (const int*)(h + at_sel);
  a.ends = (const unsigned*)(h + at_ends); a.out = out;
  const char* why = "";
  if (union_check(a.jobs, n_jobs, a.masks, n_masks, a.sel, n_sel, a.ends, n_ends, out_bytes, &why)) return 1;
  long long most = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const long long n = union_job_dwords(a.jobs[i], (size_t)out);
    most = n > most ? n : most;
  }
  const long long blocks = (most + kMaskThreads - 1) / kMaskThreads;
  for (int job = 0; job < n_jobs; ++job)
    for (long long t = 0; t < blocks * kMaskThreads; ++t) union_thread(a, job, t);
  return 0;
}

int emul_mask_select(const unsigned char* planes, const int* slot, const long long* pred_op, float* out, int N, int B, int V, int H, int W) {
  if (!slot || !pred_op || !out || N < 0 || (N > 0 && !planes) || B <= 0 || V <= 0 || H <= 0 || W <= 0 || ((size_t)out & 3)) return 1;
  SelectArgs a;
  a.planes = planes; a.slot = slot; a.op = pred_op; a.out = out;
  a.hw = (long long)H * W; a.N = N; a.B = B; a.V = V;
  const long long blocks = (((a.hw + 6) >> 2) + kMaskThreads - 1) / kMaskThreads;
  for (int b = 0; b < B; ++b)
    for (long long t = 0; t < blocks * kMaskThreads; ++t) select_thread(a, b, t);
  return 0;
}

}  // extern "C"
