// Host emulation of the mask refine kernels (t2onet_amd/csrc/t2o_refine.hip), compiled with g++ by
// tests/test_refine_cpu.py.  TEST HARNESS ONLY: the phase functions of t2o_refine_math.h -- the ones the kernels run --
// for every workgroup of the four grids, thread by thread, a loop over the threads standing in for each barrier, every
// launch complete for every job before the next starts.
#include <stdlib.h>

#include "../../t2onet_amd/csrc/t2o_refine_math.h"

using namespace t2o;

extern "C" {

int emul_refine_row_tile_w(void) { return kRefineRowW; }
int emul_refine_row_tile_h(void) { return kRefineRowH; }
int emul_refine_col_tile_w(void) { return kRefineColW; }
int emul_refine_col_tile_h(void) { return kRefineColH; }
int emul_refine_max_radius(void) { return kRefineMaxRadius; }
int emul_refine_launches(void) { return kRefineLaunches; }
int emul_refine_ws_per_pixel(void) { return kRefineWsPerPixel; }
int emul_refine_lds_bytes(int pass) {
  return pass == 1 ? (int)sizeof(RefineRowLds) : pass == 3 ? (int)sizeof(RefineRow3Lds) : pass == 4 ? (int)sizeof(RefineOutLds) : 0;
}
int emul_refine_args_bytes(void) { return (int)sizeof(RefineArgs); }

// t2o_refine_u8 for J jobs given as parallel arrays; the workspace lives in a buffer of this call, of exactly the size
// the library asks for.  Returns 1 for a table the library refuses for its values (the overlap checks are not repeated
// here), 3 when the workspace cannot be had.
int emul_refine_u8(const unsigned char* photo, const unsigned char* src, unsigned char* out, const long long* photo_offset,
                   const long long* src_offset, const long long* out_offset, const int* h, const int* w, const int* radius, const int* eps2,
                   int J) {
  if (J <= 0 || J > kRefineMaxJobs) return 1;
  static RefineArgs a;
  memset(&a, 0, sizeof(a));
  long long at = 0;
  for (int i = 0; i < J; ++i) {
    if (refine_prepare(a.jobs[i], photo_offset[i], src_offset[i], out_offset[i], h[i], w[i], radius[i], eps2[i], at)) return 1;
    at += refine_ws_bytes(a.jobs[i]);
  }
  unsigned char* ws = static_cast<unsigned char*>(aligned_alloc(16, (size_t)at));
  if (!ws) return 3;
  memset(ws, 0xEE, (size_t)at);
  static RefineRowLds l1;
  static RefineRow3Lds l3;
  static RefineOutLds l4;
  for (int i = 0; i < J; ++i)
    for (int tile = 0; tile < refine_row_tiles(a.jobs[i]); ++tile) {
      memset(&l1, 0xFF, sizeof(l1));                                  // nothing may rest on what a previous tile left
      for (int tid = 0; tid < kRefineThreads; ++tid) refine_rows1_stage(a.jobs[i], photo, src, tile, tid, l1);
      for (int tid = 0; tid < kRefineThreads; ++tid) refine_rows1_main(a.jobs[i], ws, tile, tid, l1);
    }
  for (int i = 0; i < J; ++i)
    for (int tile = 0; tile < refine_col_tiles(a.jobs[i]); ++tile)
      for (int tid = 0; tid < kRefineThreads; ++tid) refine_cols2(a.jobs[i], ws, tile, tid);
  for (int i = 0; i < J; ++i)
    for (int tile = 0; tile < refine_row_tiles(a.jobs[i]); ++tile) {
      memset(&l3, 0xFF, sizeof(l3));
      for (int tid = 0; tid < kRefineThreads; ++tid) refine_rows3_stage(a.jobs[i], ws, tile, tid, l3);
      for (int tid = 0; tid < kRefineThreads; ++tid) refine_rows3_main(a.jobs[i], ws, tile, tid, l3);
    }
  for (int i = 0; i < J; ++i)
    for (int tile = 0; tile < refine_col_tiles(a.jobs[i]); ++tile) {
      memset(&l4, 0xFF, sizeof(l4));
      for (int tid = 0; tid < kRefineThreads; ++tid) refine_cols4_main(a.jobs[i], photo, out, ws, tile, tid, l4);
      for (int tid = 0; tid < kRefineThreads; ++tid) refine_cols4_store(a.jobs[i], out, tile, tid, l4);
    }
  free(ws);
  return 0;
}

}  // extern "C"
