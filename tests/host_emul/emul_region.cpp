// Host emulation of the region kernels (t2onet_amd/csrc/t2o_region.hip), compiled with g++ by tests/test_region_cpu.py.
// TEST HARNESS ONLY: the programs of t2o_region_math.h -- the ones the kernels run -- for every workgroup of the three
// grids, thread by thread, a loop over the threads standing in for each barrier, every launch complete for every job
// before the next starts.  The lanes of the border pass run in one of three ORDERS (ascending, descending, a fixed
// shuffle): the host stand-in for the order in which workgroups arrive.
#include <stdlib.h>

#include <vector>

#include "../../t2onet_amd/csrc/t2o_region_math.h"

using namespace t2o;

extern "C" {

int emul_region_tile(void) { return kRegionTile; }
int emul_region_launches(void) { return kRegionLaunches; }
int emul_region_lds_bytes(void) { return (int)sizeof(RegionLds); }
int emul_region_args_bytes(void) { return (int)sizeof(RegionArgs); }
int emul_region_ws_align(void) { return kRegionWsAlign; }

// t2o_region_u8 for J jobs given as parallel arrays; the workspace lives in a buffer of this call, of exactly the size the
// library asks for.  order: 0 ascending, 1 descending, 2 shuffled border lanes.  roots: null, or room for the final root
// of every pixel of every job, one job after the other (-1 where a pixel does not pass).  Returns 1 for a table the
// library refuses for its values (the overlap checks are not repeated here), 3 when the workspace cannot be had.
int emul_region_u8(const unsigned char* photo, unsigned char* out, const long long* photo_offset, const long long* out_offset, const int* h,
                   const int* w, const int* seed_x, const int* seed_y, const int* tol, const int* conn, int J, int order, int* roots) {
  if (J <= 0 || J > kRegionMaxJobs) return 1;
  static RegionArgs a;
  memset(&a, 0, sizeof(a));
  long long at = 0;
  for (int i = 0; i < J; ++i) {
    if (region_prepare(a.jobs[i], photo_offset[i], out_offset[i], h[i], w[i], seed_x[i], seed_y[i], tol[i], conn[i], at)) return 1;
    at += region_ws_bytes(a.jobs[i]);
  }
  unsigned char* ws = static_cast<unsigned char*>(aligned_alloc(kRegionWsAlign, (size_t)at));
  if (!ws) return 3;
  memset(ws, 0xEE, (size_t)at);
  a.photo = photo; a.out = out; a.ws = ws;
  static RegionLds lds;
  for (int i = 0; i < J; ++i)
    for (int tile = 0; tile < region_tiles(a.jobs[i]); ++tile) {
      memset(&lds, 0x7F, sizeof(lds));                                // nothing may rest on what a previous tile left
      for (int tid = 0; tid < kRegionThreads; ++tid) region_tile_stage(a.jobs[i], photo, tile, tid, lds);
      for (int tid = 0; tid < kRegionThreads; ++tid) region_tile_link(a.jobs[i], order == 1 ? kRegionThreads - 1 - tid : tid, lds);
      for (int tid = 0; tid < kRegionThreads; ++tid) region_tile_store(a.jobs[i], ws, tile, tid, lds);
    }
  for (int i = 0; i < J; ++i) {
    const long long lanes = (long long)region_tiles(a.jobs[i]) * kRegionBorderThreads;
    std::vector<long long> seq((size_t)lanes);
    for (long long k = 0; k < lanes; ++k) seq[(size_t)k] = order == 1 ? lanes - 1 - k : k;
    if (order == 2) {
      unsigned long long s = 0x9E3779B97F4A7C15ull;
      for (long long k = lanes - 1; k > 0; --k) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const long long r = (long long)((s >> 33) % (unsigned long long)(k + 1));
        const long long t = seq[(size_t)k]; seq[(size_t)k] = seq[(size_t)r]; seq[(size_t)r] = t;
      }
    }
    for (long long k = 0; k < lanes; ++k)
      region_border_lane(a.jobs[i], ws, (int)(seq[(size_t)k] / kRegionBorderThreads), (int)(seq[(size_t)k] % kRegionBorderThreads));
  }
  for (int i = 0; i < J; ++i) {
    const int root = region_seed_root(a.jobs[i], ws);
    for (int block = 0; block < region_out_tiles(a.jobs[i], out); ++block)
      for (int tid = 0; tid < kRegionThreads; ++tid) region_resolve_thread(a, block, i, order == 1 ? kRegionThreads - 1 - tid : tid, root);
  }
  if (roots)
    for (int i = 0; i < J; ++i) {
      const int* L = region_parents(a.jobs[i], ws);
      const int n = a.jobs[i].h * a.jobs[i].w;
      for (int p = 0; p < n; ++p) *roots++ = L[p] < 0 ? -1 : region_find<RegionGlobal>(L, p);
    }
  free(ws);
  return 0;
}

}  // extern "C"
