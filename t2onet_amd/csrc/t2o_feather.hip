// t2o_feather.hip -- the soft edge of a local edit, made where the mask already lies: up to 4 uint8 planes blurred by an
// exact integer separable Gaussian (sigma <= 64, replicated borders) in TWO launches that cover every job of the call.
//
//   k_feather_rows   grid (max row tiles over the jobs, J); a workgroup owns 256 x 8 pixels of one plane: source bytes at
//                    any byte offset -> LDS through aligned dwords -> uint16 intermediate in the workspace (aligned 8-byte
//                    stores).  1 byte read and 2 written per pixel, plus the 2R-pixel apron of a tile row.
//   k_feather_cols   grid (max column tiles, J); a workgroup owns 64 x 64 pixels, lane = x: tile + 2R apron rows of the
//                    intermediate in LDS (dynamic, sized by the call's largest radius: 16 KB at R = 6, 62 KB at R = 192),
//                    a register window per thread, bytes staged with the destination's address modulo 4 and stored as
//                    dwords with single bytes at a row's two ends.  2 bytes read and 1 written per pixel, plus the apron.
// The phase functions are t2o_feather_math.h's.  Every source byte is read by the first launch before the second writes
// any destination byte, so a job may run in place.  The job table and the weights travel in the kernel arguments: no
// allocation, no host synchronisation, no float, no atomics; deterministic, capturable.
#include <hip/hip_runtime.h>
#include <string.h>

#include "t2o_feather_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

static_assert(sizeof(FeatherArgs) <= 2048, "the job table and the weights must fit the kernel arguments");
static_assert(sizeof(FeatherRowLds) <= 8 * 1024, "LDS budget of the row pass");
static_assert(kFeatherMaxJobs == T2O_FEATHER_MAX_JOBS && kFeatherMaxRadius == T2O_FEATHER_MAX_RADIUS, "header and kernels agree");

namespace {

__global__ __launch_bounds__(kFeatherThreads) void k_feather_rows(const FeatherArgs a) {
  __shared__ FeatherRowLds lds;
  const FeatherJob j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= feather_row_tiles(j)) return;
  const int tid = (int)threadIdx.x;
  feather_row_stage(j, a.w[blockIdx.y], a.src, (int)blockIdx.x, tid, lds);
  __syncthreads();
  feather_row_main(j, a.ws, (int)blockIdx.x, tid, lds);
}

__global__ __launch_bounds__(kFeatherThreads) void k_feather_cols(const FeatherArgs a, const int max_radius) {
  extern __shared__ __align__(16) unsigned char smem[];
  const FeatherJob j = a.jobs[blockIdx.y];
  if ((int)blockIdx.x >= feather_col_tiles(j)) return;
  const FeatherColLds lds = feather_col_lds(smem, max_radius);
  const int tid = (int)threadIdx.x;
  feather_col_stage(j, a.w[blockIdx.y], a.ws, (int)blockIdx.x, tid, lds);
  __syncthreads();
  feather_col_main(j, a.out, (int)blockIdx.x, tid, lds);
  __syncthreads();
  feather_col_store(j, a.out, (int)blockIdx.x, tid, lds);
}

// the checks of the C ABI; fills the jobs, the weights and the workspace layout.  Returns 0 or T2O_EINVAL with *why.
int feather_make(FeatherArgs& a, const t2o_feather_job_t* jobs, int J, size_t* bytes, const char** why) {
  if (!jobs) { *why = "feather_u8: null job table"; return T2O_EINVAL; }
  if (J <= 0 || J > kFeatherMaxJobs) { *why = "feather_u8: 1 <= J <= 4 jobs per call"; return T2O_EINVAL; }
  memset(&a, 0, sizeof(a));
  long long at = 0;
  for (int i = 0; i < J; ++i) {
    const t2o_feather_job_t& s = jobs[i];
    FeatherJob& d = a.jobs[i];
    if (s.h <= 0 || s.w <= 0) { *why = "feather_u8: h and w must be positive"; return T2O_EINVAL; }
    if ((long long)s.h * s.w >= (1ll << 31)) { *why = "feather_u8: h * w must stay below 2^31"; return T2O_EINVAL; }
    if (s.src_offset < 0 || s.out_offset < 0) { *why = "feather_u8: negative offset"; return T2O_EINVAL; }
    if (feather_weights(s.sigma, a.w[i], &d.radius)) { *why = "feather_u8: sigma must lie in [0, 64]"; return T2O_EINVAL; }
    d.src_offset = s.src_offset; d.out_offset = s.out_offset;
    d.h = s.h; d.w = s.w;
    d.pitch = feather_pitch(s.w);
    d.ws_offset = at;
    at += (long long)s.h * d.pitch;
    for (int k = 0; k < i; ++k) {
      const long long lo = jobs[k].out_offset, hi = lo + (long long)jobs[k].h * jobs[k].w;
      if (s.out_offset < hi && lo < s.out_offset + (long long)s.h * s.w) { *why = "feather_u8: two jobs' destinations overlap"; return T2O_EINVAL; }
    }
  }
  *bytes = (size_t)at * sizeof(unsigned short);
  return T2O_OK;
}

}  // namespace

extern "C" int t2o_feather_weights(double sigma, unsigned short* w, int* radius) {
  if (!w || !radius) return set_error(T2O_EINVAL, "feather_weights: null pointer");
  if (feather_weights(sigma, w, radius)) return set_error(T2O_EINVAL, "feather_weights: sigma must lie in [0, 64]");
  return T2O_OK;
}

extern "C" size_t t2o_feather_workspace_bytes(const t2o_feather_job_t* jobs, int J) {
  FeatherArgs a;
  size_t bytes = 0;
  const char* why = "";
  return feather_make(a, jobs, J, &bytes, &why) == T2O_OK ? bytes : 0;
}

extern "C" int t2o_feather_u8(const unsigned char* src, unsigned char* out, const t2o_feather_job_t* jobs, int J, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!src || !out || !jobs) return set_error(T2O_EINVAL, "feather_u8: null pointer");
  FeatherArgs a;
  size_t need = 0;
  const char* why = "";
  if (const int rc = feather_make(a, jobs, J, &need, &why)) return set_error(rc, why);
  if (!workspace || workspace_bytes < need) return set_error(T2O_EWORKSPACE, "feather_u8: workspace too small (t2o_feather_workspace_bytes)");
  if ((size_t)workspace & 7) return set_error(T2O_EINVAL, "feather_u8: the workspace must be 8-byte aligned");
  int row_tiles = 0, col_tiles = 0, max_radius = 0;
  for (int i = 0; i < J; ++i) {
    row_tiles = feather_row_tiles(a.jobs[i]) > row_tiles ? feather_row_tiles(a.jobs[i]) : row_tiles;
    col_tiles = feather_col_tiles(a.jobs[i]) > col_tiles ? feather_col_tiles(a.jobs[i]) : col_tiles;
    max_radius = a.jobs[i].radius > max_radius ? a.jobs[i].radius : max_radius;
  }
  a.src = src; a.out = out; a.ws = static_cast<unsigned short*>(workspace);
  k_feather_rows<<<dim3((unsigned)row_tiles, (unsigned)J), kFeatherThreads, 0, (hipStream_t)stream>>>(a);
  if (hipGetLastError() != hipSuccess) return set_error(T2O_ELAUNCH, "feather_u8: row pass launch failed");
  k_feather_cols<<<dim3((unsigned)col_tiles, (unsigned)J), kFeatherThreads, feather_col_lds_bytes(max_radius), (hipStream_t)stream>>>(a, max_radius);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "feather_u8: column pass launch failed");
}
