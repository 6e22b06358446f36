// Host emulation of the selection kernel (t2onet_amd/csrc/t2o_select.hip), compiled with g++ by
// tests/test_select_cpu.py.  TEST HARNESS ONLY: select_thread of t2o_select_math.h -- what the kernel runs -- for every
// thread of every workgroup of the grid (max tiles over the jobs, J).
#include "../../t2onet_amd/csrc/t2o_select_math.h"

using namespace t2o;

extern "C" {

int emul_select_tile_px(void) { return kSelectTilePx; }
int emul_select_args_bytes(void) { return (int)sizeof(SelectArgs); }
int emul_select_job_bytes(void) { return (int)sizeof(SelectJob); }

// select_ramp(dist, soft) for dist = 0 .. count - 1, with the reciprocal select_prepare hands the kernel
void emul_select_ramp(int soft, int count, int* out) {
  for (int dist = 0; dist < count; ++dist) out[dist] = select_ramp(dist, soft, select_magic(soft));
}

// t2o_select_u8 on a job table laid out as t2o_select_job_t.  Returns 1 for J, n_terms or sizes the library refuses (its
// other checks are not repeated here).
int emul_select_u8(const unsigned char* src, unsigned char* out, const SelectJob* jobs, int J) {
  if (J <= 0 || J > kSelectMaxJobs) return 1;
  static SelectArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src; a.out = out;
  int tiles = 0;
  for (int i = 0; i < J; ++i) {
    if (jobs[i].h <= 0 || jobs[i].w <= 0 || jobs[i].n_terms <= 0 || jobs[i].n_terms > kSelectMaxTerms) return 1;
    a.jobs[i] = jobs[i];
    select_prepare(a.jobs[i]);
    tiles = select_tiles(a.jobs[i], out) > tiles ? select_tiles(a.jobs[i], out) : tiles;
  }
  for (int by = 0; by < J; ++by)
    for (int bx = 0; bx < tiles; ++bx)
      for (int tid = 0; tid < kSelectThreads; ++tid) select_thread(a, bx, by, tid);
  return 0;
}

}  // extern "C"
