// t2o_resident_items.hip -- a training batch out of a device-resident set of ITEMS: up to 16 pictures per item whose slots
// may be shared between items, and one row of an int32 table per sample (program: t2o_resident_items_math.h).
//
//   k_gather_items_u8_f32   grid = B x K x workgroups of a picture, then ceil(B V / 256) row workgroups, flat.  The picture
//                           workgroups run gather_thread exactly as k_gather_u8_f32 does (t2o_resident.hip: one picture
//                           per workgroup, four pixels per lane, 3 bytes read and 12 written per pixel); the row
//                           workgroups copy rows[index[b]] to out_rows[b], one int per lane.  The branch between the two
//                           is uniform over a workgroup.
// No atomics, no allocation, no host synchronisation; deterministic (every output element has one writer) and
// capturable: a captured launch serves a new batch, rows included, once the index buffer has been overwritten.
// Host side: items_check checks the row table and leaves the pictures to gather_check (t2o_resident_math.h), as t2o_resident.hip.
#include <hip/hip_runtime.h>

#include "t2o_resident_items_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

namespace {

__global__ __launch_bounds__(kGatherThreads) void k_gather_items_u8_f32(const ItemsArgs a) {
  items_thread(a, blockIdx.x, threadIdx.x);
}

}  // namespace

extern "C" int t2o_gather_items_u8_to_f32(const unsigned char* store, const long long* slot_offsets, const long long* index, int N,
                                          int K, int B, int h, int w, float* out_x, float* out_ys, const int* rows, int V,
                                          int* out_rows, void* stream) {
  ItemsArgs a;
  const char* why = "";
  if (items_check(store, slot_offsets, index, N, K, B, h, w, out_x, out_ys, rows, V, out_rows, &a, &why)) return set_error(T2O_EINVAL, why);
  k_gather_items_u8_f32<<<a.picture_blocks + a.row_blocks, kGatherThreads, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "gather_items_u8_to_f32 launch failed");
}
