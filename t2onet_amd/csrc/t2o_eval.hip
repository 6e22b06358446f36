// t2o_eval.hip -- the metrics of the test loop (experiments/t2onet/test_seq2seqL1.py) as two fused launches each, so that
// nothing between two images of an evaluation depends on a device value.
//
//   k_eval_metrics    grid B * C * tiles (XCD-remapped like the other tile kernels); a workgroup owns a 32 x 32 tile of a
//                     (b, c) plane and runs the phase functions of t2o_eval_math.h with a barrier between them: the input,
//                     the target and sample b's END image (read where it lies, through the pointer table in the kernel
//                     arguments) are each read ONCE with their 5-pixel halo; both L1 sums and both SSIM sums come out of
//                     the same LDS tile (66 KB); four partials per workgroup.
//   k_eval_finalize   grid 4 (one workgroup per output slot): the partials added in a fixed order -- per sample, then
//                     over the samples -- so the four numbers are the same bits from run to run.
//   k_var_mean        the unbiased variance over the N = R B END images of a batch, element by element in two passes, the
//                     END image of every (request, sample) read where it lies; one partial per workgroup.
//   k_var_finalize    one workgroup: the partials in a fixed order, over `row`.
// No float atomics, no allocation, no host synchronisation: capturable.
#include <hip/hip_runtime.h>
#include <string.h>

#include "t2o_chain_kernels.h"
#include "t2o_eval_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

namespace {

// the sum of v over the workgroup in a fixed order, valid in thread 0; `cell` = kThreads / 64 floats of LDS.  Ends with
// a barrier, so the cells can be used again at once.
__device__ __forceinline__ float block_sum(float v, float* cell) {
  const float s = wave_sum(v);
  if ((threadIdx.x & 63) == 0) cell[threadIdx.x >> 6] = s;
  __syncthreads();
  const float total = ((cell[0] + cell[1]) + cell[2]) + cell[3];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(kThreads) void k_eval_metrics(const EvalArgs s) {
  __shared__ __attribute__((aligned(16))) float lds[kEvalLdsFloats];
  __shared__ float cell[kThreads / 64];
  int plane, tile;
  wg_coords(s.tiles, plane, tile);
  eval_phase_load(s, plane, tile, threadIdx.x, lds);
  __syncthreads();
  if (s.with_ssim) {
    eval_phase_rows(s, threadIdx.x, lds);
    __syncthreads();
  }
  float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  eval_phase_cols(s, tile, threadIdx.x, lds, sum);
  const size_t per_slot = (size_t)s.B * s.C * s.tiles, at = (size_t)plane * s.tiles + tile;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= 2 && !s.with_ssim) break;
    const float total = block_sum(sum[k], cell);
    if (threadIdx.x == 0) s.partials[k * per_slot + at] = total;
  }
}

// slot k = blockIdx.x: out4[k] = the mean over the samples of (sample sum / (C H W)); slots 2, 3 without SSIM: 0
__global__ __launch_bounds__(kThreads) void k_eval_finalize(const float* partials, int B, int per_sample, float inv, int with_ssim,
                                                            float* out4) {
  __shared__ float cell[kThreads / 64];
  const int k = blockIdx.x;
  if (k >= 2 && !with_ssim) {
    if (threadIdx.x == 0) out4[k] = 0.0f;
    return;
  }
  const float* p = partials + (size_t)k * B * per_sample;
  float total = 0.0f;
  for (int b = 0; b < B; ++b) {
    float acc = 0.0f;
    for (int i = threadIdx.x; i < per_sample; i += kThreads) acc += p[(size_t)b * per_sample + i];
    total += block_sum(acc, cell) * inv;
  }
  if (threadIdx.x == 0) out4[k] = total / (float)B;
}

template <int V>
__global__ __launch_bounds__(kThreads) void k_var_mean(const VarArgs a) {
  __shared__ float cell[kThreads / 64];
  const float total = block_sum(var_thread<V>(a, blockIdx.x, threadIdx.x), cell);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void k_var_finalize(const float* partials, size_t nblk, float inv_row, float* out) {
  __shared__ float cell[kThreads / 64];
  float acc = 0.0f;
  for (size_t i = threadIdx.x; i < nblk; i += kThreads) acc += partials[i];
  const float total = block_sum(acc, cell);
  if (threadIdx.x == 0) out[0] = total * inv_row;
}

long long eval_tiles(int H, int W) { return (long long)((W + kSsimTile - 1) / kSsimTile) * ((H + kSsimTile - 1) / kSsimTile); }

// the widest load every (request, step) image and the row length allow: 4, 2 or 1 floats
int var_width(const float* const* imgs, int n, size_t row) {
  size_t bits = row * sizeof(float);
  for (int i = 0; i < n; ++i) bits |= (size_t)imgs[i];
  return bits % 16 == 0 ? 4 : bits % 8 == 0 ? 2 : 1;
}

}  // namespace

extern "C" size_t t2o_eval_metrics_workspace_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)4 * B * C * (size_t)eval_tiles(H, W) * sizeof(float);
}

extern "C" int t2o_eval_metrics(const float* input, const float* const* imgs, int T, const long long* first, const float* target,
                                float* out4, int with_ssim, void* workspace, size_t workspace_bytes, int B, int C, int H, int W,
                                void* stream) {
  if (!input || !imgs || !first || !target || !out4) return set_error(T2O_EINVAL, "eval_metrics: null pointer");
  if (T < 1 || T > kEvalMaxT) return set_error(T2O_EINVAL, "eval_metrics: 1 <= T <= 8 step images");
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return set_error(T2O_EINVAL, "eval_metrics: sizes must be positive");
  EvalArgs s;
  memset(&s, 0, sizeof(s));
  for (int t = 0; t < T; ++t) {
    if (!imgs[t]) return set_error(T2O_EINVAL, "eval_metrics: null step image");
    s.img[t] = imgs[t];
  }
  const long long tiles = eval_tiles(H, W);
  const long long planes = (long long)B * C;
  if (planes > 0x7fffffffll || tiles > 0x7fffffffll / planes) return set_error(T2O_EUNSUPPORTED, "eval_metrics: 2^31 tiles or more");
  if (!workspace || workspace_bytes < t2o_eval_metrics_workspace_bytes(B, C, H, W)) return set_error(T2O_EWORKSPACE, "eval_metrics: workspace too small");
  s.input = input; s.target = target; s.first = first; s.partials = (float*)workspace;
  ssim_window(s.g);
  s.T = T; s.B = B; s.C = C; s.H = H; s.W = W;
  s.tiles_x = (W + kSsimTile - 1) / kSsimTile;
  s.tiles = (int)tiles;
  s.with_ssim = with_ssim ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  k_eval_metrics<<<(unsigned)(B * C * s.tiles), kThreads, 0, st>>>(s);
  k_eval_finalize<<<4, kThreads, 0, st>>>(s.partials, B, C * s.tiles, 1.0f / ((float)C * (float)H * (float)W), s.with_ssim, out4);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "eval_metrics launch failed");
}

extern "C" size_t t2o_end_select_var_mean_workspace_bytes(size_t row) {
  return var_blocks(row, 1) * sizeof(float);       // the narrowest loads make the most workgroups
}

extern "C" int t2o_end_select_var_mean(const float* const* imgs, const long long* const* first, int R, int T, int B, size_t row,
                                       float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!imgs || !first || !out) return set_error(T2O_EINVAL, "end_select_var_mean: null pointer");
  if (R < 1 || R > kEvalMaxR) return set_error(T2O_EINVAL, "end_select_var_mean: 1 <= R <= 16 requests");
  if (T < 1 || T > kEvalMaxT) return set_error(T2O_EINVAL, "end_select_var_mean: 1 <= T <= 8 step images");
  if (B <= 0 || row == 0) return set_error(T2O_EINVAL, "end_select_var_mean: sizes must be positive");
  if ((long long)R * B < 2) return set_error(T2O_EINVAL, "end_select_var_mean: the variance over fewer than two samples is undefined");
  if ((long long)R * B > 0x7fffffffll) return set_error(T2O_EUNSUPPORTED, "end_select_var_mean: 2^31 samples or more");
  VarArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < R * T; ++i) {
    if (!imgs[i]) return set_error(T2O_EINVAL, "end_select_var_mean: null step image");
    a.img[i] = imgs[i];
  }
  for (int r = 0; r < R; ++r) {
    if (!first[r]) return set_error(T2O_EINVAL, "end_select_var_mean: null step table");
    a.first[r] = first[r];
  }
  const int V = var_width(imgs, R * T, row);
  const size_t nblk = var_blocks(row, V);
  if (nblk > 0x7fffffffull) return set_error(T2O_EUNSUPPORTED, "end_select_var_mean: 2^31 workgroups or more");
  if (!workspace || workspace_bytes < nblk * sizeof(float)) return set_error(T2O_EWORKSPACE, "end_select_var_mean: workspace too small");
  a.partials = (float*)workspace;
  a.row = row; a.R = R; a.T = T; a.B = B;
  hipStream_t st = (hipStream_t)stream;
  if (V == 4) k_var_mean<4><<<(unsigned)nblk, kThreads, 0, st>>>(a);
  else if (V == 2) k_var_mean<2><<<(unsigned)nblk, kThreads, 0, st>>>(a);
  else k_var_mean<1><<<(unsigned)nblk, kThreads, 0, st>>>(a);
  k_var_finalize<<<1, kThreads, 0, st>>>(a.partials, nblk, 1.0f / (float)row, out);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "end_select_var_mean launch failed");
}
