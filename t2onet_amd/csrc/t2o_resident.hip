// t2o_resident.hip -- a training batch out of a device-resident set of 8-bit pictures (program: t2o_resident_math.h).
//
//   k_gather_u8_f32   grid = B x K x workgroups of a picture, flat: for sample b the pictures of item index[b] -- the
//                     index is read on the device -- converted from (h,w,3) uint8 to (3,h,w) fp32 in [0,1].  A workgroup
//                     serves one picture, so the index and the slot are one scalar load each; a lane owns four
//                     neighbouring pixels: 12 bytes in as three dwords, one 16-byte store per plane out.  3 bytes read and
//                     12 written per pixel, nothing else: the kernel is bound by the stores.
// No atomics, no allocation, no host synchronisation; deterministic (every output element has one writer) and
// capturable: a captured launch serves a new batch once the index buffer has been overwritten.
// Host side: gather_check of t2o_resident_math.h checks the arguments and fills GatherArgs, here and (through items_check)
// for t2o_resident_items.hip.
#include <hip/hip_runtime.h>

#include "t2o_resident_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

namespace {

__global__ __launch_bounds__(kGatherThreads) void k_gather_u8_f32(const GatherArgs a) {
  const unsigned image = blockIdx.x / a.blocks_per_image, block = blockIdx.x - image * a.blocks_per_image;
  const unsigned b = image / (unsigned)a.K;
  gather_thread(a, (int)b, (int)(image - b * (unsigned)a.K), (long long)block * kGatherThreads + threadIdx.x);
}

}  // namespace

extern "C" int t2o_gather_u8_to_f32(const unsigned char* store, const long long* slot_offsets, const long long* index, int N, int K,
                                    int B, int h, int w, float* out_x, float* out_ys, void* stream) {
  GatherArgs a;
  long long per_image = 0;
  const char* why = "";
  if (gather_check(store, slot_offsets, index, N, K, B, h, w, out_x, out_ys, &per_image, &why, &a)) return set_error(T2O_EINVAL, why);
  k_gather_u8_f32<<<(unsigned)(per_image * K * B), kGatherThreads, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "gather_u8_to_f32 launch failed");
}
