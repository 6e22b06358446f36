// Host emulation of the mask morph kernels (t2onet_amd/csrc/t2o_morph.hip), compiled with g++ by tests/test_morph_cpu.py.
// TEST HARNESS ONLY: the phase functions of t2o_morph_math.h -- the ones the kernels run -- for every workgroup of both
// grids, thread by thread, a loop over the threads standing in for each barrier, the first launch complete for every job
// before the second starts.  `reverse` runs the threads of every phase from the last to the first.
#include <stdlib.h>

#include "../../t2onet_amd/csrc/t2o_morph_math.h"

using namespace t2o;

extern "C" {

int emul_morph_col_tile_w(void) { return kMorphColW; }
int emul_morph_col_tile_h(void) { return kMorphColH; }
int emul_morph_row_tile_w(void) { return kMorphRowW; }
int emul_morph_row_tile_h(void) { return kMorphRowH; }
int emul_morph_max_radius(void) { return kMorphMaxRadius; }
int emul_morph_col_lds_bytes(void) { return (int)sizeof(MorphColLds); }
int emul_morph_row_lds_bytes(void) { return (int)sizeof(MorphRowLds); }
int emul_morph_args_bytes(void) { return (int)sizeof(MorphArgs); }

int emul_morph_thresholds(int radius, unsigned char* c) { return morph_thresholds(radius, c); }

// t2o_morph_u8 for J jobs given as parallel arrays; the fields live in a buffer of this call, of exactly the size the
// library asks for.  Returns 1 for J, sizes, a radius or a mode the library refuses (its other checks are not repeated
// here), 3 when the buffer cannot be had.
int emul_morph_u8(const unsigned char* src, unsigned char* out, const long long* src_offset, const long long* out_offset,
                  const int* h, const int* w, const int* radius, const int* mode, int J, int reverse) {
  if (J <= 0 || J > kMorphMaxJobs) return 1;
  static MorphArgs a;
  memset(&a, 0, sizeof(a));
  long long at = 0;
  for (int i = 0; i < J; ++i) {
    MorphJob& d = a.jobs[i];
    if (h[i] <= 0 || w[i] <= 0 || mode[i] < kMorphGrow || mode[i] > kMorphBorder || morph_thresholds(radius[i], a.c[i])) return 1;
    d.src_offset = src_offset[i]; d.out_offset = out_offset[i];
    d.h = h[i]; d.w = w[i];
    d.radius = radius[i]; d.mode = mode[i];
    d.pitch = morph_pitch(w[i]);
    d.fields = mode[i] == kMorphBorder ? 2 : 1;
    d.ws_offset = at;
    at += (long long)d.fields * d.h * d.pitch;
  }
  unsigned char* ws = static_cast<unsigned char*>(malloc((size_t)at));
  if (!ws) return 3;
  memset(ws, 0xEE, (size_t)at);
  const int first = reverse ? kMorphThreads - 1 : 0, step = reverse ? -1 : 1;
  static MorphColLds cl;
  for (int i = 0; i < J; ++i)
    for (int tile = 0; tile < morph_col_tiles(a.jobs[i]); ++tile) {
      memset(&cl, 0xFF, sizeof(cl));                                  // nothing may rest on what a previous tile left
      for (int n = 0, tid = first; n < kMorphThreads; ++n, tid += step) morph_col_stage(a.jobs[i], src, tile, tid, cl);
      for (int n = 0, tid = first; n < kMorphThreads; ++n, tid += step) morph_col_main(a.jobs[i], ws, tile, tid, cl);
    }
  static MorphRowLds rl;
  for (int i = 0; i < J; ++i)
    for (int tile = 0; tile < morph_row_tiles(a.jobs[i]); ++tile) {
      memset(&rl, 0xFF, sizeof(rl));
      for (int n = 0, tid = first; n < kMorphThreads; ++n, tid += step) morph_row_stage(a.jobs[i], a.c[i], ws, tile, tid, rl);
      for (int n = 0, tid = first; n < kMorphThreads; ++n, tid += step) morph_row_main(a.jobs[i], out, tile, tid, rl);
      for (int n = 0, tid = first; n < kMorphThreads; ++n, tid += step) morph_row_store(a.jobs[i], out, tile, tid, rl);
    }
  free(ws);
  return 0;
}

}  // extern "C"
