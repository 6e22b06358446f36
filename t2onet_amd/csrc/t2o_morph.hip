// t2o_morph.hip -- moving the boundary of a local edit's plane by a number of pixels, where the plane already lies: up to 4
// uint8 planes grown, shrunk or turned into a border band by the EXACT Euclidean distance R <= 64 (pixels inside the frame
// only; include/t2onet_hip.h has the definition) in TWO launches that cover every job of the call.
//
//   k_morph_cols   grid (max column tiles over the jobs, J); a workgroup owns 64 x 64 pixels, lane = x: source bytes at any
//                  byte offset plus R rows above and below -> LDS through aligned dwords (12 KB) -> the vertical distance
//                  fields (one byte per pixel and field, capped at R + 1) in the workspace.  1 byte read and 1 written per
//                  pixel (2 for BORDER), plus the 2R-row apron of a tile.
//   k_morph_rows   grid (max row tiles, J); a workgroup owns 256 x 8 pixels: the fields' bytes from R columns left of the
//                  tile on as aligned dwords in LDS (8.9 KB with the thresholds and the output rows), per pixel 2R + 1 byte
//                  compares against c[|dx|] = floor(sqrt(R^2 - dx^2)), bytes staged with the destination's address modulo 4
//                  and stored as dwords with single bytes at a row's two ends.  1 byte read (2 for BORDER) and 1 written per
//                  pixel, plus the apron.
// The phase functions are t2o_morph_math.h's.  Every source byte is read by the first launch before the second writes any
// destination byte, so a job may run in place.  The job table and the threshold tables travel in the kernel arguments: no
// allocation, no host synchronisation, no float, no atomics, no workgroup waits for another; deterministic, capturable.
#include <hip/hip_runtime.h>
#include <string.h>

#include "t2o_morph_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

static_assert(sizeof(MorphArgs) <= 1024, "the job table and the thresholds must fit the kernel arguments");
static_assert(sizeof(MorphColLds) <= 12 * 1024 && sizeof(MorphRowLds) <= 9 * 1024, "LDS budgets of the two passes");
static_assert(kMorphMaxJobs == T2O_MORPH_MAX_JOBS && kMorphMaxRadius == T2O_MORPH_MAX_RADIUS, "header and kernels agree");
static_assert(kMorphGrow == T2O_MORPH_GROW && kMorphShrink == T2O_MORPH_SHRINK && kMorphBorder == T2O_MORPH_BORDER, "header and kernels agree");

namespace {

__global__ __launch_bounds__(kMorphThreads) void k_morph_cols(const MorphArgs a) {
  __shared__ MorphColLds lds;
  const MorphJob j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= morph_col_tiles(j)) return;
  const int tid = (int)threadIdx.x;
  morph_col_stage(j, a.src, (int)blockIdx.x, tid, lds);
  __syncthreads();
  morph_col_main(j, a.ws, (int)blockIdx.x, tid, lds);
}

__global__ __launch_bounds__(kMorphThreads) void k_morph_rows(const MorphArgs a) {
  __shared__ MorphRowLds lds;
  const MorphJob j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= morph_row_tiles(j)) return;
  const int tid = (int)threadIdx.x;
  morph_row_stage(j, a.c[blockIdx.y], a.ws, (int)blockIdx.x, tid, lds);
  __syncthreads();
  morph_row_main(j, a.out, (int)blockIdx.x, tid, lds);
  __syncthreads();
  morph_row_store(j, a.out, (int)blockIdx.x, tid, lds);
}

// the checks of the C ABI; fills the jobs, the thresholds and the workspace layout.  Returns 0 or T2O_EINVAL with *why.
int morph_make(MorphArgs& a, const t2o_morph_job_t* jobs, int J, size_t* bytes, const char** why) {
  if (!jobs) { *why = "morph_u8: null job table"; return T2O_EINVAL; }
  if (J <= 0 || J > kMorphMaxJobs) { *why = "morph_u8: 1 <= J <= 4 jobs per call"; return T2O_EINVAL; }
  memset(&a, 0, sizeof(a));
  long long at = 0;
  for (int i = 0; i < J; ++i) {
    const t2o_morph_job_t& s = jobs[i];
    MorphJob& d = a.jobs[i];
    if (s.h <= 0 || s.w <= 0) { *why = "morph_u8: h and w must be positive"; return T2O_EINVAL; }
    if ((long long)s.h * s.w >= (1ll << 31)) { *why = "morph_u8: h * w must stay below 2^31"; return T2O_EINVAL; }
    if (s.src_offset < 0 || s.out_offset < 0) { *why = "morph_u8: negative offset"; return T2O_EINVAL; }
    if (s.mode != T2O_MORPH_GROW && s.mode != T2O_MORPH_SHRINK && s.mode != T2O_MORPH_BORDER) { *why = "morph_u8: unknown mode"; return T2O_EINVAL; }
    if (morph_thresholds(s.radius, a.c[i])) { *why = "morph_u8: the radius must lie in 0..64"; return T2O_EINVAL; }
    d.src_offset = s.src_offset; d.out_offset = s.out_offset;
    d.h = s.h; d.w = s.w;
    d.radius = s.radius; d.mode = s.mode;
    d.pitch = morph_pitch(s.w);
    d.fields = s.mode == T2O_MORPH_BORDER ? 2 : 1;
    d.ws_offset = at;
    at += (long long)d.fields * s.h * d.pitch;
    for (int k = 0; k < i; ++k) {
      const long long lo = jobs[k].out_offset, hi = lo + (long long)jobs[k].h * jobs[k].w;
      if (s.out_offset < hi && lo < s.out_offset + (long long)s.h * s.w) { *why = "morph_u8: two jobs' destinations overlap"; return T2O_EINVAL; }
    }
  }
  *bytes = (size_t)at;
  return T2O_OK;
}

}  // namespace

extern "C" size_t t2o_morph_workspace_bytes(const t2o_morph_job_t* jobs, int J) {
  MorphArgs a;
  size_t bytes = 0;
  const char* why = "";
  return morph_make(a, jobs, J, &bytes, &why) == T2O_OK ? bytes : 0;
}

extern "C" int t2o_morph_u8(const unsigned char* src, unsigned char* out, const t2o_morph_job_t* jobs, int J, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!src || !out || !jobs) return set_error(T2O_EINVAL, "morph_u8: null pointer");
  MorphArgs a;
  size_t need = 0;
  const char* why = "";
  if (const int rc = morph_make(a, jobs, J, &need, &why)) return set_error(rc, why);
  if (!workspace || workspace_bytes < need) return set_error(T2O_EWORKSPACE, "morph_u8: workspace too small (t2o_morph_workspace_bytes)");
  if ((size_t)workspace & 7) return set_error(T2O_EINVAL, "morph_u8: the workspace must be 8-byte aligned");
  int col_tiles = 0, row_tiles = 0;
  for (int i = 0; i < J; ++i) {
    col_tiles = morph_col_tiles(a.jobs[i]) > col_tiles ? morph_col_tiles(a.jobs[i]) : col_tiles;
    row_tiles = morph_row_tiles(a.jobs[i]) > row_tiles ? morph_row_tiles(a.jobs[i]) : row_tiles;
  }
  a.src = src; a.out = out; a.ws = static_cast<unsigned char*>(workspace);
  k_morph_cols<<<dim3((unsigned)col_tiles, (unsigned)J), kMorphThreads, 0, (hipStream_t)stream>>>(a);
  if (hipGetLastError() != hipSuccess) return set_error(T2O_ELAUNCH, "morph_u8: column pass launch failed");
  k_morph_rows<<<dim3((unsigned)row_tiles, (unsigned)J), kMorphThreads, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "morph_u8: row pass launch failed");
}
