// Host emulation of the fill kernels (t2onet_amd/csrc/t2o_fill.hip), compiled with g++ by tests/test_fill_cpu.py.
// TEST HARNESS ONLY: the programs of t2o_fill_math.h -- the ones the kernels run -- for every workgroup of the three
// grids, thread by thread, a loop over the threads standing in for each barrier, every launch complete for every job
// before the next starts.  order 1 runs the threads (and the tiles) backwards.
#include <stdlib.h>
#include <string.h>

#include "../../t2onet_amd/csrc/t2o_fill_math.h"

using namespace t2o;

extern "C" {

int emul_fill_tile(void) { return kFillTile; }
int emul_fill_launches(void) { return kFillLaunches; }
int emul_fill_lds_bytes(void) { return (int)(sizeof(FillPullLds) > sizeof(FillPushLds) ? sizeof(FillPullLds) : sizeof(FillPushLds)); }
int emul_fill_args_bytes(void) { return (int)sizeof(FillArgs); }
long long emul_fill_ws_bytes(int h, int w) {
  FillJob j;
  return fill_prepare(j, 0, 0, 0, h, w, 0) ? 0 : fill_ws_bytes(j);
}

// t2o_fill_u8 for J jobs given as parallel arrays; the workspace lives in a buffer of this call, of exactly the size the
// arrays take.  Returns 1 for a table the library refuses for its values (the overlap checks are not repeated here), 3
// when the workspace cannot be had.
int emul_fill_u8(const unsigned char* photo, const unsigned char* plane, unsigned char* out, const long long* photo_offset,
                 const long long* plane_offset, const long long* out_offset, const int* h, const int* w, int J, int order) {
  if (J <= 0 || J > kFillMaxJobs) return 1;
  static FillArgs a;
  memset(&a, 0, sizeof(a));
  long long at = 0;
  for (int i = 0; i < J; ++i) {
    if (fill_prepare(a.jobs[i], photo_offset[i], plane_offset[i], out_offset[i], h[i], w[i], at)) return 1;
    at += fill_ws_bytes(a.jobs[i]);
  }
  unsigned char* ws = static_cast<unsigned char*>(aligned_alloc(kFillLine, (size_t)at));
  if (!ws) return 3;
  memset(ws, 0xEE, (size_t)at);
  a.photo = photo; a.plane = plane; a.out = out; a.ws = ws;
  const auto T = [order](int tid, int n) { return order == 1 ? n - 1 - tid : tid; };
  static FillPullLds pull;
  for (int i = 0; i < J; ++i)
    for (int t = 0; t < fill_tiles_x(a.jobs[i]) * fill_tiles_y(a.jobs[i]); ++t) {
      const int tile = T(t, fill_tiles_x(a.jobs[i]) * fill_tiles_y(a.jobs[i]));
      const int tx = tile % fill_tiles_x(a.jobs[i]), ty = tile / fill_tiles_x(a.jobs[i]);
      memset(&pull, 0x7F, sizeof(pull));                              // nothing may rest on what a previous tile left
      for (int tid = 0; tid < kFillThreads; ++tid) fill_pull_stage(a.jobs[i], photo, plane, tx, ty, T(tid, kFillThreads), pull);
      for (int k = 1; k < kFillTileLevels; ++k)
        for (int tid = 0; tid < kFillThreads; ++tid) fill_pull_level(k, T(tid, kFillThreads), pull);
      for (int tid = 0; tid < kFillThreads; ++tid) fill_pull_store(a.jobs[i], ws, tx, ty, T(tid, kFillThreads), pull);
    }
  for (int i = 0; i < J; ++i) {
    const FillJob& j = a.jobs[i];
    for (int k = kFillTileLevels; k < j.K; ++k)
      for (int tid = 0; tid < kFillTopThreads; ++tid) fill_top_pull(j, ws, k, T(tid, kFillTopThreads));
    for (int tid = 0; tid < kFillTopThreads; ++tid) fill_top_seed(j, ws, T(tid, kFillTopThreads));
    for (int k = j.K - 1; k >= kFillTileLevels; --k)
      for (int tid = 0; tid < kFillTopThreads; ++tid) fill_top_push(j, ws, k, T(tid, kFillTopThreads));
  }
  static FillPushLds push;
  for (int i = 0; i < J; ++i)
    for (int t = 0; t < fill_tiles_x(a.jobs[i]) * fill_tiles_y(a.jobs[i]); ++t) {
      const FillJob& j = a.jobs[i];
      const int tile = T(t, fill_tiles_x(j) * fill_tiles_y(j));
      const int tx = tile % fill_tiles_x(j), ty = tile / fill_tiles_x(j);
      memset(&push, 0x7F, sizeof(push));
      push.any = 0;
      for (int tid = 0; tid < kFillThreads; ++tid) fill_push_plane(j, plane, tx, ty, T(tid, kFillThreads), push);
      const bool plain = !push.any || fill_empty(j, ws);
      if (plain && fill_in_place(a, j)) continue;
      if (!plain)
        for (int k = fill_tile_top(j); k >= 1; --k)
          for (int tid = 0; tid < kFillThreads; ++tid) fill_push_level(j, ws, k, tx, ty, T(tid, kFillThreads), push);
      for (int tid = 0; tid < kFillThreads; ++tid) fill_push_blend(a, j, tx, ty, T(tid, kFillThreads), plain, push);
      for (int tid = 0; tid < kFillThreads; ++tid) fill_push_store(a, j, tx, ty, T(tid, kFillThreads), push);
    }
  free(ws);
  return 0;
}

}  // extern "C"
