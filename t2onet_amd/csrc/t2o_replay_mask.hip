// t2o_replay_mask.hip -- t2o_replay.hip's 8-bit replay with Operator.execute's mask operand: a LOCAL edit ("brighten the
// sky") applied to 8-bit pictures at their native size, 8-bit in and 8-bit out, ONE launch for up to 64 jobs that share
// up to 4 uint8 mask planes.
//
//   k_replay_u8_masked   grid (max tiles over the jobs, J); a workgroup owns a 32 x 32 tile of one job and runs the phase
//                        functions of t2o_replay_mask_math.h with a barrier between them.  Global traffic is the 3 source
//                        and the 3 output bytes of a pixel plus 1 byte per distinct mask the job's list names (plus the
//                        1-pixel ring of a sharpness list), all moved as aligned dwords whatever the byte alignment.  A
//                        step whose mask is zero over the workgroup's window is skipped (same bytes, see the header).
//                        The job table, the mask offsets and the per-step mask indices travel in the kernel arguments:
//                        no allocation, no host synchronisation, capturable, deterministic.
// Host side, shared by the three replay entry points: replay_launch_prepare (t2o_replay_mask_math.h) checks the arguments
// and fills the job table through replay_job_fill (t2o_replay_math.h).
#include <hip/hip_runtime.h>

#include "t2o_replay_mask_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

static_assert(sizeof(ReplayMaskArgs) <= 4096, "the job table must fit the kernel arguments");
static_assert(sizeof(ReplayMaskLds) <= 32 * 1024, "LDS budget of the masked replay");

namespace {

__global__ __launch_bounds__(kReplayThreads) void k_replay_u8_masked(const ReplayMaskArgs a) {
  __shared__ ReplayMaskLds lds;
  const ReplayMaskJob mj = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= replay_tiles(mj.j)) return;
  const ReplayTile t = replay_tile(mj.j, (int)blockIdx.x);
  const float* params = a.params + (size_t)blockIdx.y * kReplayMaxSteps * kMaxParam;
  const int tid = (int)threadIdx.x;
  replay_phase_load(mj.j, a.src, t, tid, lds.base);
  replay_phase_mask_clear(tid, lds);
  __syncthreads();
  replay_phase_mask_load(mj, a.masks, a.mask_offsets, t, tid, lds);
  __syncthreads();
  if (mj.j.sharp >= 0) {
    replay_mask_phase_pre(mj, a.src, params, a.masks, a.mask_offsets, t, tid, lds);
    __syncthreads();
  }
  replay_mask_phase_main(mj, a.src, a.out, params, a.masks, a.mask_offsets, t, tid, lds);
  __syncthreads();
  replay_phase_store(mj.j, a.out, t, tid, lds.base);
}

}  // namespace

extern "C" int t2o_replay_u8_masked(const unsigned char* src, unsigned char* out, const t2o_replay_job_t* jobs, const int* mask_of,
                                    int J, const float* params, const unsigned char* masks, const long long* mask_offsets,
                                    int n_masks, void* stream) {
  if (!mask_of) return set_error(T2O_EINVAL, "replay_u8_masked: null pointer");      // its own: required even without masks
  ReplayMaskArgs a;
  const char* why = "";
  unsigned tiles = 0;
  int ring = 0;
  if (const int rc = replay_launch_prepare(a, "replay_u8_masked", kReplaySharpIndex, src, out, jobs, mask_of, J, params, masks,
                                           mask_offsets, n_masks, &tiles, &ring, &why))
    return set_error(rc, why);
  k_replay_u8_masked<<<dim3(tiles, (unsigned)J), kReplayThreads, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "replay_u8_masked launch failed");
}
