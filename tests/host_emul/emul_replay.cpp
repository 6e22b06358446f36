// Host emulation of the 8-bit replay kernel (t2onet_amd/csrc/t2o_replay.hip), compiled with g++ by tests/test_replay_cpu.py.
// TEST HARNESS ONLY: the phase functions of t2o_replay_math.h -- the ones the kernel runs -- for every tile of a picture,
// thread by thread, a loop over the threads standing in for each barrier.
#include "../../t2onet_amd/csrc/t2o_replay_math.h"

using namespace t2o;

extern "C" {

int emul_replay_tile(void) { return kReplayTile; }

// one job of t2o_replay_u8: (h, w, 3) uint8 at src + src_offset -> out + out_offset; params (8, 24).  Returns the status
// of the job check (0 = ran).
int emul_replay_u8(const unsigned char* src, long long src_offset, unsigned char* out, long long out_offset, int h, int w,
                   int steps, const int* ops, const float* params) {
  ReplayJob j;
  const char* why = "";
  if (const int rc = replay_job_make(j, src_offset, out_offset, h, w, steps, ops, &why)) return rc;
  static ReplayLds lds;
  for (int tile = 0; tile < replay_tiles(j); ++tile) {
    const ReplayTile t = replay_tile(j, tile);
    unsigned char* fill = reinterpret_cast<unsigned char*>(&lds);
    for (size_t i = 0; i < sizeof(lds); ++i) fill[i] = 0xFF;          // (NaN floats) nothing may rest on what a previous tile left
    for (int tid = 0; tid < kReplayThreads; ++tid) replay_phase_load(j, src, t, tid, lds);
    if (j.sharp >= 0)
      for (int tid = 0; tid < kReplayThreads; ++tid) replay_phase_pre(j, src, params, t, tid, lds);
    for (int tid = 0; tid < kReplayThreads; ++tid) replay_phase_main(j, src, out, params, t, tid, lds);
    for (int tid = 0; tid < kReplayThreads; ++tid) replay_phase_store(j, out, t, tid, lds);
  }
  return 0;
}

}  // extern "C"
