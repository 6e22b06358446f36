// t2o_refine.hip -- the mask planes of a local edit snapped to the photo's own edges where they already lie: up to 4 uint8
// planes through the guided filter (guide = the photo's luminance, radius <= 64, replicated borders) in exact INTEGER
// arithmetic, in FOUR launches that cover every job of the call.
//
//   k_refine_rows1   grid (max row tiles over the jobs, J); a workgroup owns 256 x 8 pixels: photo and plane bytes at any byte
//                    offset -> luminance and plane bytes in LDS -> the row sums of I, p, I I, I p as three uint32 planes
//                    (aligned 16-byte stores).  4 bytes read and 12 written per pixel, plus the 2r-pixel apron of a tile row.
//   k_refine_cols2   grid (max column tiles, J); a workgroup owns 64 x 256 pixels, lane = x, a wave 64 rows: running sums down
//                    the column, no LDS; the two 64-bit floor divisions that give A and B.  12 bytes read twice (the row
//                    that enters, the row that leaves) and 8 written per pixel, plus the apron.
//   k_refine_rows3   as rows1 on A and B (24.5 KB of LDS); T_A rows int32, T_B rows int64, over the dead row-sum planes.
//   k_refine_cols4   as cols2 on those; the luminance again from the photo; bytes staged with the destination's address
//                    modulo 4 and stored as dwords with single bytes at a row's two ends.
// The phase functions are t2o_refine_math.h's.  Every plane byte is read by the first launch and every destination byte
// written by the last, so a job may run in place.  The job table travels in the kernel arguments: no allocation, no host
// synchronisation, no float, no atomics; deterministic, capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "t2o_refine_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

static_assert(sizeof(RefineArgs) <= 2048, "the job table must fit the kernel arguments");
static_assert(sizeof(RefineRowLds) <= 8 * 1024 && sizeof(RefineRow3Lds) <= 32 * 1024 && sizeof(RefineOutLds) <= 32 * 1024, "LDS budgets");
static_assert(kRefineMaxJobs == T2O_REFINE_MAX_JOBS && kRefineMaxRadius == T2O_REFINE_MAX_RADIUS && kRefineMaxEps2 == T2O_REFINE_MAX_EPS2,
              "header and kernels agree");

namespace {

__global__ __launch_bounds__(kRefineThreads) void k_refine_rows1(const RefineArgs a) {
  __shared__ RefineRowLds lds;
  const RefineJob j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= refine_row_tiles(j)) return;
  refine_rows1_stage(j, a.photo, a.src, (int)blockIdx.x, (int)threadIdx.x, lds);
  __syncthreads();
  refine_rows1_main(j, a.ws, (int)blockIdx.x, (int)threadIdx.x, lds);
}

__global__ __launch_bounds__(kRefineThreads) void k_refine_cols2(const RefineArgs a) {
  const RefineJob j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= refine_col_tiles(j)) return;
  refine_cols2(j, a.ws, (int)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(kRefineThreads) void k_refine_rows3(const RefineArgs a) {
  __shared__ RefineRow3Lds lds;
  const RefineJob j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= refine_row_tiles(j)) return;
  refine_rows3_stage(j, a.ws, (int)blockIdx.x, (int)threadIdx.x, lds);
  __syncthreads();
  refine_rows3_main(j, a.ws, (int)blockIdx.x, (int)threadIdx.x, lds);
}

__global__ __launch_bounds__(kRefineThreads) void k_refine_cols4(const RefineArgs a) {
  __shared__ RefineOutLds lds;
  const RefineJob j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= refine_col_tiles(j)) return;
  refine_cols4_main(j, a.photo, a.out, a.ws, (int)blockIdx.x, (int)threadIdx.x, lds);
  __syncthreads();
  refine_cols4_store(j, a.out, (int)blockIdx.x, (int)threadIdx.x, lds);
}

bool overlap(uintptr_t a, long long na, uintptr_t b, long long nb) { return a < b + (uintptr_t)nb && b < a + (uintptr_t)na; }

// the checks of the C ABI that need no pointer; fills the jobs and the workspace layout.  Returns nullptr or the reason.
const char* refine_make(RefineArgs& a, const t2o_refine_job_t* jobs, int J, size_t* bytes) {
  if (!jobs) return "refine_u8: null job table";
  if (J <= 0 || J > kRefineMaxJobs) return "refine_u8: 1 <= J <= 4 jobs per call";
  memset(&a, 0, sizeof(a));
  long long at = 0;
  for (int i = 0; i < J; ++i) {
    const t2o_refine_job_t& s = jobs[i];
    if (const char* why = refine_prepare(a.jobs[i], s.photo_offset, s.src_offset, s.out_offset, s.h, s.w, s.radius, s.eps2, at)) return why;
    at += refine_ws_bytes(a.jobs[i]);
  }
  *bytes = (size_t)at;
  return nullptr;
}

}  // namespace

extern "C" size_t t2o_refine_workspace_bytes(const t2o_refine_job_t* jobs, int J) {
  RefineArgs a;
  size_t bytes = 0;
  return refine_make(a, jobs, J, &bytes) ? 0 : bytes;
}

extern "C" int t2o_refine_u8(const unsigned char* photo, const unsigned char* src, unsigned char* out, const t2o_refine_job_t* jobs, int J,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!photo || !src || !out || !jobs) return set_error(T2O_EINVAL, "refine_u8: null pointer");
  RefineArgs a;
  size_t need = 0;
  if (const char* why = refine_make(a, jobs, J, &need)) return set_error(T2O_EINVAL, why);
  // one writer per byte, and no destination on a photo: the last launch reads the photos while it writes
  for (int i = 0; i < J; ++i) {
    const long long n = (long long)jobs[i].h * jobs[i].w;
    const uintptr_t dst = (uintptr_t)out + (uintptr_t)jobs[i].out_offset;
    for (int k = 0; k < i; ++k)
      if (overlap(dst, n, (uintptr_t)out + (uintptr_t)jobs[k].out_offset, (long long)jobs[k].h * jobs[k].w))
        return set_error(T2O_EINVAL, "refine_u8: two jobs' destinations overlap");
    for (int k = 0; k < J; ++k)
      if (overlap(dst, n, (uintptr_t)photo + (uintptr_t)jobs[k].photo_offset, 3ll * jobs[k].h * jobs[k].w))
        return set_error(T2O_EINVAL, "refine_u8: a destination overlaps a photo of the call");
  }
  if (!workspace || workspace_bytes < need) return set_error(T2O_EWORKSPACE, "refine_u8: workspace too small (t2o_refine_workspace_bytes)");
  if ((size_t)workspace & 15) return set_error(T2O_EWORKSPACE, "refine_u8: the workspace must be 16-byte aligned");
  int row_tiles = 0, col_tiles = 0;
  for (int i = 0; i < J; ++i) {
    row_tiles = refine_row_tiles(a.jobs[i]) > row_tiles ? refine_row_tiles(a.jobs[i]) : row_tiles;
    col_tiles = refine_col_tiles(a.jobs[i]) > col_tiles ? refine_col_tiles(a.jobs[i]) : col_tiles;
  }
  a.photo = photo; a.src = src; a.out = out; a.ws = static_cast<unsigned char*>(workspace);
  const dim3 rows((unsigned)row_tiles, (unsigned)J), cols((unsigned)col_tiles, (unsigned)J);
  hipStream_t s = (hipStream_t)stream;
  k_refine_rows1<<<rows, kRefineThreads, 0, s>>>(a);
  if (hipGetLastError() != hipSuccess) return set_error(T2O_ELAUNCH, "refine_u8: first row pass launch failed");
  k_refine_cols2<<<cols, kRefineThreads, 0, s>>>(a);
  if (hipGetLastError() != hipSuccess) return set_error(T2O_ELAUNCH, "refine_u8: first column pass launch failed");
  k_refine_rows3<<<rows, kRefineThreads, 0, s>>>(a);
  if (hipGetLastError() != hipSuccess) return set_error(T2O_ELAUNCH, "refine_u8: second row pass launch failed");
  k_refine_cols4<<<cols, kRefineThreads, 0, s>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "refine_u8: second column pass launch failed");
}
