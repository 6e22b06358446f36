// Host emulation of the masked 8-bit replay kernel (t2onet_amd/csrc/t2o_replay_mask.hip), compiled with g++ by
// tests/test_replay_mask_cpu.py.  TEST HARNESS ONLY: the phase functions of t2o_replay_mask_math.h -- the ones the kernel
// runs -- for every tile of a picture, thread by thread, a loop over the threads standing in for each barrier.
#include "../../t2onet_amd/csrc/t2o_replay_mask_math.h"

using namespace t2o;

extern "C" {

int emul_replay_mask_tile(void) { return kReplayTile; }
int emul_replay_mask_lds_bytes(void) { return (int)sizeof(ReplayMaskLds); }
int emul_replay_mask_args_bytes(void) { return (int)sizeof(ReplayMaskArgs); }

// one job of t2o_replay_u8_masked: (h, w, 3) uint8 at src + src_offset -> out + out_offset; params (8, 24); mask_of: 8
// indices into mask_offsets (n_masks entries, counted from masks), -1 = none.  Returns the status of the job check.
int emul_replay_u8_masked(const unsigned char* src, long long src_offset, unsigned char* out, long long out_offset, int h, int w,
                          int steps, const int* ops, const int* mask_of, const float* params, const unsigned char* masks,
                          const long long* mask_offsets, int n_masks) {
  if (n_masks < 0 || n_masks > kReplayMaxMasks) return 1;
  ReplayMaskJob mj;
  const char* why = "";
  if (const int rc = replay_mask_job_make(mj, src_offset, out_offset, h, w, steps, ops, mask_of, n_masks, &why)) return rc;
  long long offs[kReplayMaxMasks] = {0, 0, 0, 0};
  for (int i = 0; i < n_masks; ++i) offs[i] = mask_offsets[i];
  static ReplayMaskLds lds;
  for (int tile = 0; tile < replay_tiles(mj.j); ++tile) {
    const ReplayTile t = replay_tile(mj.j, tile);
    unsigned char* fill = reinterpret_cast<unsigned char*>(&lds);
    for (size_t i = 0; i < sizeof(lds); ++i) fill[i] = 0xFF;          // nothing may rest on what a previous tile left
    for (int tid = 0; tid < kReplayThreads; ++tid) {
      replay_phase_load(mj.j, src, t, tid, lds.base);
      replay_phase_mask_clear(tid, lds);
    }
    for (int tid = 0; tid < kReplayThreads; ++tid) replay_phase_mask_load(mj, masks, offs, t, tid, lds);
    if (mj.j.sharp >= 0)
      for (int tid = 0; tid < kReplayThreads; ++tid) replay_mask_phase_pre(mj, src, params, masks, offs, t, tid, lds);
    for (int tid = 0; tid < kReplayThreads; ++tid) replay_mask_phase_main(mj, src, out, params, masks, offs, t, tid, lds);
    for (int tid = 0; tid < kReplayThreads; ++tid) replay_phase_store(mj.j, out, t, tid, lds.base);
  }
  return 0;
}

}  // extern "C"
