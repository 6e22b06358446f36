// t2o_replay_stencils.hip -- the 8-bit replay for operator lists with ANY number of sharpness steps, with or without
// masks: what t2o_replay_u8 / t2o_replay_u8_masked refuse (their 1-pixel halo serves one sharpness).  8-bit in and 8-bit
// out at the pictures' native size, ONE launch for up to 64 jobs that share up to 4 uint8 mask planes.  Added BESIDE the
// two existing entry points, which behave and refuse as before; t2o_abi_version() stays 4 although an entry point is
// added (the version is pinned by the tests of the existing entry points, whose form does not change).
//
//   k_replay_u8_stencils  grid (max tiles over the jobs, J); a workgroup owns a 32 x 32 tile of one job and runs the phase
//                         functions of t2o_replay_stencils_math.h with a barrier between them: the window of tile + R
//                         pixels (R = the job's number of sharpness steps, sized at run time) is staged once, the list
//                         runs in segments -- per-pixel steps in registers, the intermediate image into ONE LDS float
//                         tile with zeros outside the picture, the stencil -- and the correct region shrinks by a pixel
//                         per sharpness down to the tile.  The float tile is updated in place (register hold, barrier).
//                         Global traffic is the 3 source and 3 output bytes of a pixel plus 1 byte per distinct mask the
//                         list names, plus the ring; no intermediate image ever reaches memory.  The per-pixel work is
//                         recomputed on the ring: up to (32 + 2R)^2 / 32^2 of it (1.27 at R = 2, 2.25 at R = 8).
//                         TWO INSTANCES of the one program, chosen per launch by the largest R among its jobs, because
//                         the window sizes the LDS and the pixels a thread holds across a barrier size the registers:
//                           R <= 2  36 x 36 window, 28 992 B of static LDS (float tile 15 984, source rows 4 032, four
//                                   mask windows 5 760, output rows 3 200, flags), at most 5 held pixels: 132 VGPRs, no
//                                   scratch -> 3 workgroups = 12 waves per CU (the registers bind; LDS has room for 5)
//                           R <= 8  48 x 48 window, 48 528 B (28 224 + 7 104 + 9 984 + 3 200, flags), at most 9 held
//                                   pixels: 194 VGPRs, no scratch -> 2 workgroups = 8 waves per CU (LDS has room for 3)
//                         (ROCm 7.2 hipcc; capping the registers for one more workgroup spills in both, so it is not
//                         done.)  t2o_replay_u8 runs 4 workgroups per CU at 106 VGPRs and 21 KB: lists with at most one
//                         sharpness are served here too, but the callers keep the older kernels for them.
//                         TILE SKIP kept in its conservative form: a step whose mask is zero over the whole staged
//                         window is not run (same bytes, see the header).
//                         The job table, the mask offsets and the per-step mask indices travel in the kernel arguments
//                         (ReplayMaskArgs, under 4 KB): no allocation, no host synchronisation, capturable, deterministic.
// Measured on one synthetic 4000 x 6000 picture (profiles/replay_u8_stencils.txt, medians of 20): [0,6,1,6,5] 0.537 ms
// against 0.771 ms of the materialised path (0.70 of it); [0,6,1,2,5] 0.442 ms against 0.312 ms of t2o_replay_u8 (1.42x).
// Not measured: real photos through the decoder, R > 2 (the large instance), the kernel's share of peak.
// Host side, shared by the three replay entry points: replay_launch_prepare (t2o_replay_mask_math.h) checks the arguments
// and fills the job table through replay_job_fill (t2o_replay_math.h) (here in the mode that counts the sharpness steps).
#include <hip/hip_runtime.h>

#include "t2o_replay_stencils_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

static_assert(sizeof(ReplayMaskArgs) <= 4096, "the job table must fit the kernel arguments");
static_assert(sizeof(ReplayStLds) <= 52 * 1024, "LDS budget of the stencils replay: three workgroups per CU");
static_assert(sizeof(ReplayStLdsSmall) <= 32 * 1024, "LDS budget of the stencils replay for R <= 2: five workgroups per CU");

namespace {

// one chunk of `first` for the thread that stands for pixel slot tid0 = tid + base: NP pixels, then their `put` (a
// sharpness follows) or `out` (none does: region = tile, NP = 4, base = 0).  No barrier inside.
template <int NP, class L>
__device__ __forceinline__ void first_chunk(const ReplayMaskArgs& a, const ReplayMaskJob& mj, const float* params, const ReplayTile& t,
                                            int E, int tid0, L& lds) {
  if (tid0 >= E * E) return;                       // its later pixels lie outside the region as well
  Rgb hold[NP];
  replay_st_phase_first<NP>(mj, a.src, params, a.masks, a.mask_offsets, t, E, tid0, lds, hold);
  if (mj.j.sharp > 0) replay_st_phase_put<NP>(mj.j, t, E, tid0, lds, hold);
  else if constexpr (NP == kReplayPix) replay_st_phase_out(mj.j, a.out, t, tid0, lds, hold);
}

// the n-th sharpness (step s) on the region of edge E, then `put` when a sharpness follows, else `out`.  NP pixels per
// thread; the held values stay in registers across the barrier.
template <int NP, class L>
__device__ __forceinline__ void segment(const ReplayMaskArgs& a, const ReplayMaskJob& mj, const float* params, const ReplayTile& t,
                                        int E, int n, int s, int tid, L& lds) {
  Rgb hold[NP];
  replay_st_phase_stencil<NP>(mj, params, a.masks, a.mask_offsets, t, E, s, tid, lds, hold);
  if (n + 1 < mj.j.sharp) {
    __syncthreads();                               // every stencil has read the tile that is about to change
    replay_st_phase_put<NP>(mj.j, t, E, tid, lds, hold);
    __syncthreads();
  } else if constexpr (NP == kReplayPix) {
    replay_st_phase_out(mj.j, a.out, t, tid, lds, hold);
  }
}

// RMAX = the largest R among the launch's jobs that this instance serves: it sizes the LDS and bounds the pixels a thread
// holds across a barrier (5 at RMAX = 2, 9 at RMAX = 8), and with them the registers
template <int RMAX>
__global__ __launch_bounds__(kReplayThreads) void k_replay_u8_stencils(const ReplayMaskArgs a) {
  __shared__ ReplayStLdsT<RMAX> lds;
  const ReplayMaskJob mj = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= replay_tiles(mj.j)) return;
  const ReplayTile t = replay_st_tile(mj.j, (int)blockIdx.x);
  const float* params = a.params + (size_t)blockIdx.y * kReplayMaxSteps * kMaxParam;
  const int tid = (int)threadIdx.x;
  replay_st_phase_load(mj.j, a.src, t, tid, lds);
  __syncthreads();
  if (replay_masks_used(mj)) {                     // the same in every thread of the workgroup
    replay_st_phase_mask_load(mj, a.masks, a.mask_offsets, t, tid, lds);
    __syncthreads();
  }
  const int R = mj.j.sharp, W = kReplayTile + 2 * R;
  for (int base = 0; base < W * W;) {              // `first` on the window, chunk by chunk
    const int np = replay_st_first_np(W * W - base);
    if (np == 4) first_chunk<4>(a, mj, params, t, W, tid + base, lds);
    else if (np == 2) first_chunk<2>(a, mj, params, t, W, tid + base, lds);
    else first_chunk<1>(a, mj, params, t, W, tid + base, lds);
    base += np * kReplayThreads;
  }
  if (R > 0) __syncthreads();
  int s = -1;
  for (int n = 0; n < R; ++n) {                    // the last segment's region is the tile: E = 32, NP = 4
    const int E = kReplayTile + 2 * (R - n - 1);
    s = replay_st_next_sharp(mj.j, s + 1);
    const int np = replay_st_np(E);
    if (np == 4) segment<4>(a, mj, params, t, E, n, s, tid, lds);
    else if (np == 5) segment<5>(a, mj, params, t, E, n, s, tid, lds);
    else if constexpr (RMAX > kStSmallRing) {
      if (np == 6) segment<6>(a, mj, params, t, E, n, s, tid, lds);
      else segment<9>(a, mj, params, t, E, n, s, tid, lds);
    }
  }
  __syncthreads();
  replay_st_phase_store(mj.j, a.out, t, tid, lds);
}

}  // namespace

extern "C" int t2o_replay_u8_stencils(const unsigned char* src, unsigned char* out, const t2o_replay_job_t* jobs, const int* mask_of,
                                      int J, const float* params, const unsigned char* masks, const long long* mask_offsets,
                                      int n_masks, void* stream) {
  ReplayMaskArgs a;
  const char* why = "";
  unsigned tiles = 0;
  int max_ring = 0;
  if (const int rc = replay_launch_prepare(a, "replay_u8_stencils", kReplaySharpCount, src, out, jobs, mask_of, J, params, masks,
                                           mask_offsets, n_masks, &tiles, &max_ring, &why))
    return set_error(rc, why);
  const dim3 grid(tiles, (unsigned)J);
  if (max_ring <= kStSmallRing) k_replay_u8_stencils<kStSmallRing><<<grid, kReplayThreads, 0, (hipStream_t)stream>>>(a);
  else k_replay_u8_stencils<kStMaxRing><<<grid, kReplayThreads, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "replay_u8_stencils launch failed");
}
