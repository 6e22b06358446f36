// Host emulation of the mask feather kernels (t2onet_amd/csrc/t2o_feather.hip), compiled with g++ by
// tests/test_feather_cpu.py.  TEST HARNESS ONLY: the phase functions of t2o_feather_math.h -- the ones the kernels run --
// for every workgroup of both grids, thread by thread, a loop over the threads standing in for each barrier, the first
// launch complete for every job before the second starts.
#include <stdlib.h>

#include "../../t2onet_amd/csrc/t2o_feather_math.h"

using namespace t2o;

extern "C" {

int emul_feather_row_tile_w(void) { return kFeatherRowW; }
int emul_feather_row_tile_h(void) { return kFeatherRowH; }
int emul_feather_col_tile_w(void) { return kFeatherColW; }
int emul_feather_col_tile_h(void) { return kFeatherColH; }
int emul_feather_max_radius(void) { return kFeatherMaxRadius; }
int emul_feather_row_lds_bytes(void) { return (int)sizeof(FeatherRowLds); }
int emul_feather_col_lds_bytes(int radius) { return (int)feather_col_lds_bytes(radius); }
int emul_feather_args_bytes(void) { return (int)sizeof(FeatherArgs); }

int emul_feather_weights(double sigma, unsigned short* w, int* radius) { return feather_weights(sigma, w, radius); }

// t2o_feather_u8 for J jobs given as parallel arrays; the intermediate lives in a buffer of this call.  The arithmetic
// is unsigned 32-bit as on the device.  Returns 1 for J, sizes or a sigma the library refuses (its other checks are not
// repeated here), 3 when the buffers cannot be had.
int emul_feather_u8(const unsigned char* src, unsigned char* out, const long long* src_offset, const long long* out_offset,
                    const int* h, const int* w, const double* sigma, int J) {
  if (J <= 0 || J > kFeatherMaxJobs) return 1;
  static FeatherArgs a;
  memset(&a, 0, sizeof(a));
  long long at = 0;
  int max_radius = 0;
  for (int i = 0; i < J; ++i) {
    FeatherJob& d = a.jobs[i];
    if (h[i] <= 0 || w[i] <= 0 || feather_weights(sigma[i], a.w[i], &d.radius)) return 1;
    d.src_offset = src_offset[i]; d.out_offset = out_offset[i];
    d.h = h[i]; d.w = w[i];
    d.pitch = feather_pitch(w[i]);
    d.ws_offset = at;
    at += (long long)d.h * d.pitch;
    max_radius = d.radius > max_radius ? d.radius : max_radius;
  }
  unsigned short* ws = static_cast<unsigned short*>(malloc((size_t)at * sizeof(unsigned short)));
  unsigned char* smem = static_cast<unsigned char*>(malloc(feather_col_lds_bytes(max_radius)));
  if (!ws || !smem) { free(ws); free(smem); return 3; }
  memset(ws, 0xEE, (size_t)at * sizeof(unsigned short));
  static FeatherRowLds rl;
  for (int i = 0; i < J; ++i)
    for (int tile = 0; tile < feather_row_tiles(a.jobs[i]); ++tile) {
      memset(&rl, 0xFF, sizeof(rl));                                  // nothing may rest on what a previous tile left
      for (int tid = 0; tid < kFeatherThreads; ++tid) feather_row_stage(a.jobs[i], a.w[i], src, tile, tid, rl);
      for (int tid = 0; tid < kFeatherThreads; ++tid) feather_row_main(a.jobs[i], ws, tile, tid, rl);
    }
  const FeatherColLds cl = feather_col_lds(smem, max_radius);
  for (int i = 0; i < J; ++i)
    for (int tile = 0; tile < feather_col_tiles(a.jobs[i]); ++tile) {
      memset(smem, 0xFF, feather_col_lds_bytes(max_radius));
      for (int tid = 0; tid < kFeatherThreads; ++tid) feather_col_stage(a.jobs[i], a.w[i], ws, tile, tid, cl);
      for (int tid = 0; tid < kFeatherThreads; ++tid) feather_col_main(a.jobs[i], out, tile, tid, cl);
      for (int tid = 0; tid < kFeatherThreads; ++tid) feather_col_store(a.jobs[i], out, tile, tid, cl);
    }
  free(ws);
  free(smem);
  return 0;
}

}  // extern "C"
