// t2o_mask.hip -- the local-edit masks of the GIER half of the reference on the device (programs: t2o_mask_math.h).
//
//   k_rle_union_u8   grid (max dwords of a plane / 256, J): resize_and_union_mask (data/GIER/GIER.py:288-307) for every
//                    plane of a batch in ONE launch, from the masks' run lengths: no native-size plane exists anywhere.
//                    A thread owns an aligned dword of the output buffer = four neighbouring pixels of a row (lanes walk
//                    x: the stores coalesce); per selected mask each pixel's source position is searched in the mask's
//                    cumulative run ends (an upper-bound search, ~log2(runs) cached loads), a pixel that falls into the
//                    run found for its left neighbour is not searched.  The three tables (jobs, masks, selection) and the
//                    run ends lie in ONE device buffer, filled by one upload; the entry point checks the HOST copy of the
//                    same bytes before the launch, so the kernel never reads or writes outside what it was given.
//   k_mask_select    grid (groups of a sample / 256, B): get_gt_mask (models/actor.py:78-98) for the operator each sample
//                    chose, read from the device: (B,1,H,W) fp32 = the chosen plane's bytes as floats, or all ones.
//                    16-byte stores on aligned groups, single floats at a sample's unaligned ends.
// No allocation, no host synchronisation, capturable, deterministic (every output element has one writer).
#include <hip/hip_runtime.h>
#include <string.h>

#include "t2o_mask_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

static_assert(sizeof(RleMask) == sizeof(t2o_rle_mask_t) && sizeof(UnionJob) == sizeof(t2o_union_job_t), "table records as the header declares them");
static_assert(sizeof(RleMask) == 16 && sizeof(UnionJob) == 24, "table records as functional.py packs them");

namespace {

__global__ __launch_bounds__(kMaskThreads) void k_rle_union_u8(const UnionArgs a) {
  union_thread(a, (int)blockIdx.y, (long long)blockIdx.x * kMaskThreads + threadIdx.x);
}

__global__ __launch_bounds__(kMaskThreads) void k_mask_select(const SelectArgs a) {
  select_thread(a, (int)blockIdx.y, (long long)blockIdx.x * kMaskThreads + threadIdx.x);
}

}  // namespace

extern "C" int t2o_rle_union_u8(const void* host_tables, const void* dev_tables, int n_jobs, int n_masks, int n_sel, long long n_ends,
                                unsigned char* out, long long out_bytes, void* stream) {
  if (!host_tables || !dev_tables || !out) return set_error(T2O_EINVAL, "rle_union_u8: null pointer");
  if (n_jobs <= 0 || n_jobs > 65535) return set_error(T2O_EINVAL, "rle_union_u8: 1 <= jobs <= 65535 per launch");
  if (n_masks < 0 || n_sel < 0 || n_ends < 0 || n_ends > 0xffffffffll || out_bytes <= 0)
    return set_error(T2O_EINVAL, "rle_union_u8: table sizes must not be negative and the output must not be empty");
  if (((size_t)host_tables | (size_t)dev_tables) & 7) return set_error(T2O_EINVAL, "rle_union_u8: the tables must be 8-byte aligned");
  // the layout of the packed buffer: jobs, masks, selection, run ends
  const size_t at_masks = sizeof(UnionJob) * (size_t)n_jobs, at_sel = at_masks + sizeof(RleMask) * (size_t)n_masks,
               at_ends = at_sel + sizeof(int) * (size_t)n_sel;
  const char* h = (const char*)host_tables;
  const char* why = "";
  if (union_check((const UnionJob*)h, n_jobs, (const RleMask*)(h + at_masks), n_masks, (const int*)(h + at_sel), n_sel,
                  (const unsigned*)(h + at_ends), n_ends, out_bytes, &why))
    return set_error(T2O_EINVAL, why);
  const char* d = (const char*)dev_tables;
  UnionArgs a;
  a.jobs = (const UnionJob*)d; a.masks = (const RleMask*)(d + at_masks); a.sel = (const int*)(d + at_sel);
  a.ends = (const unsigned*)(d + at_ends); a.out = out;
  long long most = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const long long n = union_job_dwords(((const UnionJob*)h)[i], (size_t)out);
    most = n > most ? n : most;
  }
  const long long blocks = (most + kMaskThreads - 1) / kMaskThreads;
  k_rle_union_u8<<<dim3((unsigned)blocks, (unsigned)n_jobs), kMaskThreads, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "rle_union_u8 launch failed");
}

extern "C" int t2o_mask_select(const unsigned char* planes, const int* slot, const long long* pred_op, float* out, int N, int B, int V,
                               int H, int W, void* stream) {
  if (!slot || !pred_op || !out) return set_error(T2O_EINVAL, "mask_select: null pointer");
  if (N < 0 || (N > 0 && !planes)) return set_error(T2O_EINVAL, "mask_select: null plane buffer");
  if (B <= 0 || B > 65535 || V <= 0 || H <= 0 || W <= 0) return set_error(T2O_EINVAL, "mask_select: sizes must be positive (B <= 65535)");
  if ((long long)H * W >= 0x80000000ll) return set_error(T2O_EINVAL, "mask_select: a plane of 2^31 pixels or more");
  if ((size_t)out & 3) return set_error(T2O_EINVAL, "mask_select: the output must be 4-byte aligned");
  SelectArgs a;
  a.planes = planes; a.slot = slot; a.op = pred_op; a.out = out;
  a.hw = (long long)H * W; a.N = N; a.B = B; a.V = V;
  const long long groups = (a.hw + 3 + 3) >> 2;                       // the most a sample can touch, whatever its alignment
  const long long blocks = (groups + kMaskThreads - 1) / kMaskThreads;
  k_mask_select<<<dim3((unsigned)blocks, (unsigned)B), kMaskThreads, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "mask_select launch failed");
}
