// t2o_fill.hip -- a region of a photo removed on the device: the pixels under a plane replaced by a push-pull fill from the
// pixels around them, in THREE launches that cover every job of the call (at most 4), whatever the pictures hold.
//
//   k_fill_pull   grid (max tiles across, max tiles down, J); a workgroup owns 64 x 64 pixels: photo and plane bytes at any
//                 alignment -> levels 1..6 of the pull pyramid on 11 KB of LDS -> the workspace, 8 bytes per cell.
//   k_fill_top    grid (J): ONE workgroup per job pulls levels 7..K and pushes K..6 through the workspace, a level per
//                 phase, __threadfence() and __syncthreads() between two phases.
//   k_fill_push   the first grid again: a tile without a plane byte > 0 (or of a job without a kept pixel) copies its photo
//                 bytes, or returns when the job runs in place; another reads F_6 around it and C_5..C_1 with one cell of
//                 halo, pushes down on LDS and stores the blended bytes as aligned dwords -- single bytes at the two ends
//                 of a misaligned row range.
// The programs are t2o_fill_math.h's, where the halo, visibility and progress arguments are written out.  The job table
// travels in the kernel arguments: no allocation, no host synchronisation, no float, no atomics; deterministic; capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "t2o_fill_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

static_assert(sizeof(FillArgs) <= 2048, "the job table must fit the kernel arguments");
static_assert(sizeof(FillPullLds) <= 16 * 1024 && sizeof(FillPushLds) <= 32 * 1024, "LDS budget");
static_assert(kFillMaxJobs == T2O_FILL_MAX_JOBS && kFillLaunches == T2O_FILL_LAUNCHES, "header and kernels agree");

namespace {

__global__ __launch_bounds__(kFillThreads) void k_fill_pull(const FillArgs a) {
  __shared__ FillPullLds lds;
  const FillJob j = a.jobs[blockIdx.z];
  const int tx = (int)blockIdx.x, ty = (int)blockIdx.y;
  if (tx >= fill_tiles_x(j) || ty >= fill_tiles_y(j)) return;
  fill_pull_stage(j, a.photo, a.plane, tx, ty, (int)threadIdx.x, lds);
  for (int k = 1; k < kFillTileLevels; ++k) {
    __syncthreads();
    fill_pull_level(k, (int)threadIdx.x, lds);
  }
  __syncthreads();
  fill_pull_store(j, a.ws, tx, ty, (int)threadIdx.x, lds);
}

__global__ __launch_bounds__(kFillTopThreads) void k_fill_top(const FillArgs a) {
  const FillJob j = a.jobs[blockIdx.x];
  // every bound below is the same for all threads: it follows from h and w alone
  for (int k = kFillTileLevels; k < j.K; ++k) {
    fill_top_pull(j, a.ws, k, (int)threadIdx.x);
    __threadfence();
    __syncthreads();
  }
  fill_top_seed(j, a.ws, (int)threadIdx.x);
  __threadfence();
  __syncthreads();
  for (int k = j.K - 1; k >= kFillTileLevels; --k) {
    fill_top_push(j, a.ws, k, (int)threadIdx.x);
    __threadfence();
    __syncthreads();
  }
}

__global__ __launch_bounds__(kFillThreads) void k_fill_push(const FillArgs a) {
  __shared__ FillPushLds lds;
  const FillJob j = a.jobs[blockIdx.z];
  const int tx = (int)blockIdx.x, ty = (int)blockIdx.y, tid = (int)threadIdx.x;
  if (tx >= fill_tiles_x(j) || ty >= fill_tiles_y(j)) return;
  if (tid == 0) lds.any = 0;
  __syncthreads();
  fill_push_plane(j, a.plane, tx, ty, tid, lds);
  __syncthreads();
  const bool plain = !lds.any || fill_empty(j, a.ws);       // the same for every thread
  if (plain && fill_in_place(a, j)) return;
  if (!plain)
    for (int k = fill_tile_top(j); k >= 1; --k) {
      fill_push_level(j, a.ws, k, tx, ty, tid, lds);
      __syncthreads();
    }
  fill_push_blend(a, j, tx, ty, tid, plain, lds);
  __syncthreads();                                          // every read of the tile's photo bytes lies in front of it
  fill_push_store(a, j, tx, ty, tid, lds);
}

bool overlap(uintptr_t a, long long na, uintptr_t b, long long nb) { return a < b + (uintptr_t)nb && b < a + (uintptr_t)na; }

// the checks of the C ABI that need no pointer; fills the jobs and the workspace layout.  Returns nullptr or the reason.
const char* fill_make(FillArgs& a, const t2o_fill_job_t* jobs, int J, size_t* bytes) {
  if (!jobs) return "fill_u8: null job table";
  if (J <= 0 || J > kFillMaxJobs) return "fill_u8: 1 <= J <= 4 jobs per call";
  memset(&a, 0, sizeof(a));
  long long at = 0;
  for (int i = 0; i < J; ++i) {
    const t2o_fill_job_t& s = jobs[i];
    if (const char* why = fill_prepare(a.jobs[i], s.photo_offset, s.plane_offset, s.out_offset, s.h, s.w, at)) return why;
    at += fill_ws_bytes(a.jobs[i]);
  }
  *bytes = (size_t)at + (kFillLine - kFillWsAlign);         // room to round a 16-byte aligned base up to a line
  return nullptr;
}

}  // namespace

extern "C" size_t t2o_fill_workspace_bytes(const t2o_fill_job_t* jobs, int J) {
  FillArgs a;
  size_t bytes = 0;
  return fill_make(a, jobs, J, &bytes) ? 0 : bytes;
}

extern "C" int t2o_fill_u8(const unsigned char* photo, const unsigned char* plane, unsigned char* out, const t2o_fill_job_t* jobs, int J,
                           void* workspace, size_t workspace_bytes, void* stream) {
  if (!photo || !plane || !out || !jobs) return set_error(T2O_EINVAL, "fill_u8: null pointer");
  FillArgs a;
  size_t need = 0;
  if (const char* why = fill_make(a, jobs, J, &need)) return set_error(T2O_EINVAL, why);
  // one writer per byte; no destination on a plane; on a photo only a job's own, at exactly its own address: the push pass
  // reads level-0 bytes of its own tile alone, but another job's may read this photo while this one writes it
  for (int i = 0; i < J; ++i) {
    const long long n = 3ll * jobs[i].h * jobs[i].w;
    const uintptr_t dst = (uintptr_t)out + (uintptr_t)jobs[i].out_offset;
    for (int k = 0; k < i; ++k)
      if (overlap(dst, n, (uintptr_t)out + (uintptr_t)jobs[k].out_offset, 3ll * jobs[k].h * jobs[k].w))
        return set_error(T2O_EINVAL, "fill_u8: two jobs' destinations overlap");
    for (int k = 0; k < J; ++k) {
      if (overlap(dst, n, (uintptr_t)plane + (uintptr_t)jobs[k].plane_offset, (long long)jobs[k].h * jobs[k].w))
        return set_error(T2O_EINVAL, "fill_u8: a destination overlaps a plane of the call");
      const uintptr_t src = (uintptr_t)photo + (uintptr_t)jobs[k].photo_offset;
      if (!(k == i && src == dst) && overlap(dst, n, src, 3ll * jobs[k].h * jobs[k].w))
        return set_error(T2O_EINVAL, "fill_u8: a destination overlaps a photo of the call (only a job's own photo, at its own address, may be its destination)");
    }
  }
  if (!workspace || workspace_bytes < need) return set_error(T2O_EWORKSPACE, "fill_u8: workspace too small (t2o_fill_workspace_bytes)");
  if ((size_t)workspace & (kFillWsAlign - 1)) return set_error(T2O_EWORKSPACE, "fill_u8: the workspace must be 16-byte aligned");
  a.photo = photo; a.plane = plane; a.out = out;
  a.ws = reinterpret_cast<unsigned char*>(((uintptr_t)workspace + kFillLine - 1) & ~(uintptr_t)(kFillLine - 1));
  int tiles_x = 0, tiles_y = 0;                             // the grid: the largest job's tiles; a workgroup outside its job's returns
  for (int i = 0; i < J; ++i) {
    tiles_x = fill_tiles_x(a.jobs[i]) > tiles_x ? fill_tiles_x(a.jobs[i]) : tiles_x;
    tiles_y = fill_tiles_y(a.jobs[i]) > tiles_y ? fill_tiles_y(a.jobs[i]) : tiles_y;
  }
  hipStream_t s = (hipStream_t)stream;
  k_fill_pull<<<dim3((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)J), kFillThreads, 0, s>>>(a);
  if (hipGetLastError() != hipSuccess) return set_error(T2O_ELAUNCH, "fill_u8: pull pass launch failed");
  k_fill_top<<<dim3((unsigned)J), kFillTopThreads, 0, s>>>(a);
  if (hipGetLastError() != hipSuccess) return set_error(T2O_ELAUNCH, "fill_u8: top pass launch failed");
  k_fill_push<<<dim3((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)J), kFillThreads, 0, s>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "fill_u8: push pass launch failed");
}
