// t2o_region.hip -- the magic wand of a local edit: the connected region around a seed pixel as a hard 0/255 uint8 plane,
// labelled where the photo already lies by union-find over an int32 parent array, in THREE launches that cover every
// job of the call (at most 4), whatever the pictures hold.
//
//   k_region_tile      grid (max tiles over the jobs, J); a workgroup owns 64 x 64 pixels: photo bytes at any alignment ->
//                      pass against the seed's bytes (read here, on the device) -> runs, then unions with the row above on
//                      16 KB of LDS -> each pixel's parent = the global index of its tile-local root.  3 bytes read and 4
//                      written per pixel, plain stores.
//   k_region_border    the same grid, 128 lanes: a tile's top row and left column joined with the passing neighbours across
//                      the tile edge by lock-free min-index unions in the global array.
//   k_region_resolve   grid (max 4096-pixel tiles of the destination streams, J): one lane finds the seed's root, LDS hands
//                      it to the others; a lane owns four neighbouring pixels, finds their roots and stores one aligned
//                      dword -- single bytes at the two ends of a misaligned plane.
// The programs are t2o_region_math.h's, where the visibility rule (every access to the parent array in the last two launches
// is an agent-scope relaxed atomic) and the progress argument (no workgroup waits for another; every loop follows strictly
// falling indices) are written out.  The job table travels in the kernel arguments: no allocation, no host
// synchronisation, no float; the output bytes and the final roots are deterministic; capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "t2o_region_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

static_assert(sizeof(RegionArgs) <= 2048, "the job table must fit the kernel arguments");
static_assert(sizeof(RegionLds) <= 16 * 1024, "LDS budget");
static_assert(kRegionMaxJobs == T2O_REGION_MAX_JOBS, "header and kernels agree");

namespace {

__global__ __launch_bounds__(kRegionThreads) void k_region_tile(const RegionArgs a) {
  __shared__ RegionLds lds;
  const RegionJob j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= region_tiles(j)) return;
  region_tile_stage(j, a.photo, (int)blockIdx.x, (int)threadIdx.x, lds);
  __syncthreads();
  region_tile_link(j, (int)threadIdx.x, lds);
  __syncthreads();
  region_tile_store(j, a.ws, (int)blockIdx.x, (int)threadIdx.x, lds);
}

__global__ __launch_bounds__(kRegionBorderThreads) void k_region_border(const RegionArgs a) {
  const RegionJob j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= region_tiles(j)) return;
  region_border_lane(j, a.ws, (int)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(kRegionThreads) void k_region_resolve(const RegionArgs a) {
  __shared__ int root;
  const RegionJob& j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= region_out_tiles(j, a.out)) return;
  if (threadIdx.x == 0) root = region_seed_root(j, a.ws);
  __syncthreads();
  region_resolve_thread(a, (int)blockIdx.x, (int)blockIdx.y, (int)threadIdx.x, root);
}

bool overlap(uintptr_t a, long long na, uintptr_t b, long long nb) { return a < b + (uintptr_t)nb && b < a + (uintptr_t)na; }

// the checks of the C ABI that need no pointer; fills the jobs and the workspace layout.  Returns nullptr or the reason.
const char* region_make(RegionArgs& a, const t2o_region_job_t* jobs, int J, size_t* bytes) {
  if (!jobs) return "region_u8: null job table";
  if (J <= 0 || J > kRegionMaxJobs) return "region_u8: 1 <= J <= 4 jobs per call";
  memset(&a, 0, sizeof(a));
  long long at = 0;
  for (int i = 0; i < J; ++i) {
    const t2o_region_job_t& s = jobs[i];
    if (const char* why = region_prepare(a.jobs[i], s.photo_offset, s.out_offset, s.h, s.w, s.seed_x, s.seed_y, s.tol, s.conn, at)) return why;
    at += region_ws_bytes(a.jobs[i]);
  }
  *bytes = (size_t)at;
  return nullptr;
}

}  // namespace

extern "C" size_t t2o_region_workspace_bytes(const t2o_region_job_t* jobs, int J) {
  RegionArgs a;
  size_t bytes = 0;
  return region_make(a, jobs, J, &bytes) ? 0 : bytes;
}

extern "C" int t2o_region_u8(const unsigned char* photo, unsigned char* out, const t2o_region_job_t* jobs, int J,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!photo || !out || !jobs) return set_error(T2O_EINVAL, "region_u8: null pointer");
  RegionArgs a;
  size_t need = 0;
  if (const char* why = region_make(a, jobs, J, &need)) return set_error(T2O_EINVAL, why);
  // one writer per byte, and no destination on a photo: the first launch of another job may still read it
  for (int i = 0; i < J; ++i) {
    const long long n = (long long)jobs[i].h * jobs[i].w;
    const uintptr_t dst = (uintptr_t)out + (uintptr_t)jobs[i].out_offset;
    for (int k = 0; k < i; ++k)
      if (overlap(dst, n, (uintptr_t)out + (uintptr_t)jobs[k].out_offset, (long long)jobs[k].h * jobs[k].w))
        return set_error(T2O_EINVAL, "region_u8: two jobs' destinations overlap");
    for (int k = 0; k < J; ++k)
      if (overlap(dst, n, (uintptr_t)photo + (uintptr_t)jobs[k].photo_offset, 3ll * jobs[k].h * jobs[k].w))
        return set_error(T2O_EINVAL, "region_u8: a destination overlaps a photo of the call");
  }
  if (!workspace || workspace_bytes < need) return set_error(T2O_EWORKSPACE, "region_u8: workspace too small (t2o_region_workspace_bytes)");
  if ((size_t)workspace & (kRegionWsAlign - 1)) return set_error(T2O_EWORKSPACE, "region_u8: the workspace must be 16-byte aligned");
  a.photo = photo; a.out = out; a.ws = static_cast<unsigned char*>(workspace);
  int tiles = 0, out_tiles = 0;
  for (int i = 0; i < J; ++i) {
    tiles = region_tiles(a.jobs[i]) > tiles ? region_tiles(a.jobs[i]) : tiles;
    out_tiles = region_out_tiles(a.jobs[i], out) > out_tiles ? region_out_tiles(a.jobs[i], out) : out_tiles;
  }
  hipStream_t s = (hipStream_t)stream;
  k_region_tile<<<dim3((unsigned)tiles, (unsigned)J), kRegionThreads, 0, s>>>(a);
  if (hipGetLastError() != hipSuccess) return set_error(T2O_ELAUNCH, "region_u8: tile pass launch failed");
  k_region_border<<<dim3((unsigned)tiles, (unsigned)J), kRegionBorderThreads, 0, s>>>(a);
  if (hipGetLastError() != hipSuccess) return set_error(T2O_ELAUNCH, "region_u8: border pass launch failed");
  k_region_resolve<<<dim3((unsigned)out_tiles, (unsigned)J), kRegionThreads, 0, s>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "region_u8: resolve pass launch failed");
}
