// t2o_replay.hip -- a known (operator, parameter) list applied to 8-bit pictures at their native size, 8-bit in and
// 8-bit out, ONE launch for up to 64 jobs (the prefixes of one list on one photo: the per-step pictures of an edit).
//
//   k_replay_u8   grid (max tiles over the jobs, J); a workgroup owns a 32 x 32 tile of one job and runs the phase
//                 functions of t2o_replay_math.h with a barrier between them; workgroups beyond a job's tile count
//                 return.  Global traffic is the 3 source and the 3 output bytes of a pixel (plus the 1-pixel ring of a
//                 sharpness list), moved as aligned dwords whatever the pictures' byte alignment; everything between the
//                 two conversions lives in registers, with one LDS exchange for the stencil.  The job table travels in
//                 the kernel arguments: no allocation, no host synchronisation, capturable, deterministic.
// Host side, shared by the three replay entry points: replay_launch_prepare (t2o_replay_mask_math.h) checks the arguments
// and fills the job table through replay_job_fill (t2o_replay_math.h); the entry point copies the jobs into the plain kernel's form.
#include <hip/hip_runtime.h>
#include <string.h>

#include "t2o_replay_mask_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

namespace {

__global__ __launch_bounds__(kReplayThreads) void k_replay_u8(const ReplayArgs a) {
  __shared__ ReplayLds lds;
  const ReplayJob j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= replay_tiles(j)) return;
  const ReplayTile t = replay_tile(j, (int)blockIdx.x);
  const float* params = a.params + (size_t)blockIdx.y * kReplayMaxSteps * kMaxParam;
  const int tid = (int)threadIdx.x;
  replay_phase_load(j, a.src, t, tid, lds);
  __syncthreads();
  if (j.sharp >= 0) {
    replay_phase_pre(j, a.src, params, t, tid, lds);
    __syncthreads();
  }
  replay_phase_main(j, a.src, a.out, params, t, tid, lds);
  __syncthreads();
  replay_phase_store(j, a.out, t, tid, lds);
}

}  // namespace

extern "C" int t2o_replay_u8(const unsigned char* src, unsigned char* out, const t2o_replay_job_t* jobs, int J, const float* params,
                             void* stream) {
  ReplayMaskArgs m;
  const char* why = "";
  unsigned tiles = 0;
  int ring = 0;
  if (const int rc = replay_launch_prepare(m, "replay_u8", kReplaySharpIndex, src, out, jobs, nullptr, J, params, nullptr, nullptr, 0,
                                           &tiles, &ring, &why))
    return set_error(rc, why);
  ReplayArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src; a.out = out; a.params = params;
  for (int i = 0; i < J; ++i) a.jobs[i] = m.jobs[i].j;               // no step names a mask: the plain kernel's job form
  k_replay_u8<<<dim3(tiles, (unsigned)J), kReplayThreads, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "replay_u8 launch failed");
}
