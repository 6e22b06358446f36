// t2o_planner_fit.hip -- the planner's multi-parameter fits as ONE device-resident batched solve
// (utils/beam_search.py:65-91,148-167: one scipy minimisation per candidate step, every objective evaluation an
// executor call plus a host sync).  Up to 64 jobs -- (image, target, operator) triples -- run Adam side by side on
//     mean |clamp(process(img, p)) - target|
// with two launches per iteration and no host synchronisation:
//   k_fit_eval<true>   grid (pixel chunks, jobs): forward, L1 sign, closed-form parameter derivative of every pixel;
//                      one partial sum per (job, slot, chunk), written -- never accumulated -- to the workspace
//                      (k_fit_eval<GRAD, true>: the same under a per-job local-edit mask plane, see FitMaskArgs)
//   k_fit_adam         one wave per job: the chunk partials summed in index order, the curve raw sums turned into
//                      gradients, torch.optim.Adam's update, and the stop rule of the serial fit evaluated per job
// and a closing k_fit_eval<false> + k_fit_dist pair that leaves the loss at the returned parameters.
// Determinism: partials are summed in a fixed order, there are no atomics and nothing waits on another workgroup.  A
// job reads and writes only its own rows (blockIdx.y = job), so its result does not depend on its neighbours.
// Partial sums are kept in fp64 from the wave reduction on: the per-pixel terms are the fp32 ones of the single-operator
// kernels, their sum carries no further rounding.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <type_traits>

#include "t2o_pixel_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

namespace {

constexpr int kFitThreads = 256;
constexpr int kFitPix = 2;                     // pixels per thread: 512 per workgroup, 32 workgroups per job at 128 x 128
constexpr int kFitMaxJobs = 64;
constexpr int kFitLossSlot = kMaxParam;        // slots 0..23: raw parameter-gradient sums; slot 24: sum |out - target|
constexpr int kFitSlots = kMaxParam + 1;
constexpr int kFitHasPrev = 1, kFitFrozen = 2; // per-job flag bits

struct FitArgs {
  const float* imgs;      // (n_img, 3, H, W)
  const float* targets;   // (n_target, 3, H, W)
  float* params;          // (J, 24), updated in place
  double* partials;       // (J, kFitSlots, nblk)
  float* m;               // (J, 24) Adam first moment
  float* v;               // (J, 24) Adam second moment
  float* prev;            // (J) loss at the job's last check
  int* flags;             // (J)
  int op[kFitMaxJobs];
  int img_index[kFitMaxJobs];
  int target_index[kFitMaxJobs];
  int H, W, nblk;
  float inv_n;            // 1 / (3 H W)
};

// The masked form's arguments: job j blends its operator with planes (n_mask, H, W) uint8, packed -- plane k starts at
// byte k H W, any alignment, read byte by byte -- under mask_index[j]; -1 = no mask (m = 1).  The unmasked kernels keep
// FitArgs as their argument, so their code does not change.
struct FitMaskArgs : FitArgs {
  const unsigned char* masks;
  int mask_index[kFitMaxJobs];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);     // fixed butterfly: the same order every run
  return v;
}

__device__ __forceinline__ float fit_sign(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }

// one input pixel value with the stencil's zero padding (models/operators.py:351-358: conv2d(padding=1))
__device__ __forceinline__ float fit_at(const float* plane, int y, int x, int H, int W) {
  return (y >= 0 && y < H && x >= 0 && x < W) ? plane[(size_t)y * W + x] : 0.0f;
}

template <bool GRAD, bool MASKED>
__global__ __launch_bounds__(kFitThreads) void k_fit_eval(typename std::conditional<MASKED, FitMaskArgs, FitArgs>::type a) {
  __shared__ double wsum[kFitSlots][kFitThreads / 64];
  const int job = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  if (GRAD && (a.flags[job] & kFitFrozen)) return;                         // (uniform over the workgroup)
  const int op = a.op[job];
  const unsigned hw = (unsigned)a.H * (unsigned)a.W;
  const float* img = a.imgs + (size_t)a.img_index[job] * 3 * hw;
  const float* tgt = a.targets + (size_t)a.target_index[job] * 3 * hw;
  const float* prow = a.params + (size_t)job * kMaxParam;
  const unsigned char* mplane = nullptr;                                   // (uniform; stays null for a job without a mask)
  if constexpr (MASKED) {
    if (a.mask_index[job] >= 0) mplane = a.masks + (size_t)a.mask_index[job] * hw;
  }
  const bool curve = op == OP_COLOR || op == OP_TONE;
  Curve cv = {};
  if (curve) curve_load(cv, prow, op == OP_COLOR);
  const float p0[1] = {prow[0]};
  float red[kMaxParam];
  T2O_UNROLL
  for (int k = 0; k < kMaxParam; ++k) red[k] = 0.0f;
  float loss = 0.0f;
  T2O_UNROLL
  for (int i = 0; i < kFitPix; ++i) {
    const unsigned px = ((unsigned)blk * kFitPix + i) * kFitThreads + tid;
    if (px >= hw) continue;
    Rgb x, z;
    float t[3], d[3] = {0.0f, 0.0f, 0.0f};
    T2O_UNROLL
    for (int c = 0; c < 3; ++c) { x.c[c] = img[c * (size_t)hw + px]; t[c] = tgt[c * (size_t)hw + px]; }
    if (op == OP_SHARPNESS) {
      const int y = (int)(px / (unsigned)a.W), xx = (int)(px % (unsigned)a.W);
      T2O_UNROLL
      for (int c = 0; c < 3; ++c) {
        const float* plane = img + c * (size_t)hw;
        d[c] = sharp_delta(x.c[c], fit_at(plane, y - 1, xx, a.H, a.W), fit_at(plane, y, xx - 1, a.H, a.W),
                           fit_at(plane, y, xx + 1, a.H, a.W), fit_at(plane, y + 1, xx, a.H, a.W));
        z.c[c] = x.c[c] + p0[0] * d[c];
      }
    } else {
      z = pointwise_fwd(op, x, p0, cv);
    }
    Rgb go;
    if constexpr (MASKED) {
      const float m = mplane ? (float)mplane[px] : 1.0f;                   // one byte per pixel, shared by the three channels
      T2O_UNROLL
      for (int c = 0; c < 3; ++c) loss += masked_l1_term(z.c[c], x.c[c], m, t[c], a.inv_n, go.c[c]);
    } else {
      T2O_UNROLL
      for (int c = 0; c < 3; ++c) {
        const float diff = clamp01(z.c[c]) - t[c];
        loss += fabsf(diff);
        const float gz = fit_sign(diff) * a.inv_n;
        go.c[c] = (z.c[c] >= 0.0f && z.c[c] <= 1.0f) ? gz : 0.0f;         // clamp(0,1) backward, inclusive
      }
    }
    if (!GRAD) continue;
    if (op == OP_SHARPNESS) {
      T2O_UNROLL
      for (int c = 0; c < 3; ++c) red[0] += go.c[c] * d[c];
    } else if (curve) {
      // raw sums red[8 kc + j] += g * clamp(x - j/8, 0, 1/8); curve_param_grad turns them into gradients
      T2O_UNROLL
      for (int c = 0; c < 3; ++c) {
        T2O_UNROLL
        for (int j = 0; j < kCurveSteps; ++j) {
          const float tj = fminf(fmaxf(x.c[c] - (float)j / kCurveSteps, 0.0f), 1.0f / kCurveSteps);
          if (op == OP_COLOR) red[c * kCurveSteps + j] += go.c[c] * tj;
          else red[j] += go.c[c] * tj;
        }
      }
    } else {
      pointwise_bwd(op, x, p0, cv, go, red);                               // brightness / contrast / saturation: red[0]
    }
  }
  // workgroup sums: wave butterfly, then the four waves in index order
  const int n = GRAD ? op_num_params(op) : 0;
  T2O_UNROLL
  for (int k = 0; k < kFitSlots; ++k) {
    if (k != kFitLossSlot && k >= n) continue;                             // (uniform)
    const double s = wave_sum_f64(k == kFitLossSlot ? (double)loss : (double)red[k]);
    if ((tid & 63) == 0) wsum[k][tid >> 6] = s;
  }
  __syncthreads();
  if (tid < kFitSlots && (tid == kFitLossSlot || tid < n))
    a.partials[((size_t)job * kFitSlots + tid) * a.nblk + blk] = ((wsum[tid][0] + wsum[tid][1]) + wsum[tid][2]) + wsum[tid][3];
}

__device__ __forceinline__ double fit_sum_partials(const FitArgs& a, int job, int slot) {
  const double* p = a.partials + ((size_t)job * kFitSlots + slot) * a.nblk;
  double s = 0.0;
  for (int b = 0; b < a.nblk; ++b) s += p[b];
  return s;
}

// One wave per job.  step arithmetic of torch.optim.Adam (no weight decay, no amsgrad), per element:
//   m = m + (g - m) (1 - b1);  v = v b2 + g g (1 - b2);  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
// check != 0 on iterations check_every, 2 check_every, ...: the serial fit's stop rule on this iteration's loss.
__global__ __launch_bounds__(64) void k_fit_adam(FitArgs a, float lr_c, float b2, float om1, float om2, float sq_bc2, float eps,
                                                 int check, float tol) {
  __shared__ float A[kFitSlots];
  const int job = blockIdx.x, tid = threadIdx.x;
  const int flags = a.flags[job];
  if (flags & kFitFrozen) return;                                          // (uniform)
  const int op = a.op[job], n = op_num_params(op);
  if (tid < n) A[tid] = (float)fit_sum_partials(a, job, tid);
  if (tid == kFitLossSlot) A[tid] = (float)(fit_sum_partials(a, job, tid) / (3.0 * (double)a.H * (double)a.W));
  __syncthreads();
  float* prow = a.params + (size_t)job * kMaxParam;
  float g = 0.0f;
  if (tid < n) {
    if (op == OP_COLOR || op == OP_TONE) {
      const int row = tid / kCurveSteps, col = tid % kCurveSteps;
      float gk[kCurveSteps];
      curve_param_grad(prow + row * kCurveSteps, A + row * kCurveSteps, gk);
      T2O_UNROLL
      for (int i = 0; i < kCurveSteps; ++i) g = (i == col) ? gk[i] : g;
    } else {
      g = A[0];
    }
  }
  __syncthreads();                                                         // every row read before any element moves
  if (tid < n) {
    const size_t e = (size_t)job * kMaxParam + tid;
    const float m = a.m[e] + (g - a.m[e]) * om1;
    const float v = a.v[e] * b2 + (g * g) * om2;
    a.m[e] = m;
    a.v[e] = v;
    prow[tid] = prow[tid] - lr_c * (m / (sqrtf(v) / sq_bc2 + eps));
  }
  if (tid == 0 && check) {
    const float cur = A[kFitLossSlot];
    int f = flags;
    if ((f & kFitHasPrev) && (double)a.prev[job] - (double)cur < (double)tol) f |= kFitFrozen;
    a.prev[job] = cur;
    a.flags[job] = f | kFitHasPrev;
  }
}

__global__ __launch_bounds__(64) void k_fit_dist(FitArgs a, float* dist) {
  if (threadIdx.x == 0)
    dist[blockIdx.x] = (float)(fit_sum_partials(a, blockIdx.x, kFitLossSlot) / (3.0 * (double)a.H * (double)a.W));
}

// Adam moments, last-check losses and flags to zero (a kernel, not a memset node: see t2o_optim.hip)
__global__ __launch_bounds__(256) void k_fit_init(unsigned* state, int words) {
  for (int i = threadIdx.x; i < words; i += 256) state[i] = 0u;
}

int fit_nblk(int H, int W) {
  return (int)(((size_t)H * W + (size_t)kFitThreads * kFitPix - 1) / ((size_t)kFitThreads * kFitPix));
}

constexpr int kFitStateWords = 2 * kMaxParam + 2;   // per job: m, v, prev, flags

}  // namespace

extern "C" {

size_t t2o_fit_multi_workspace_bytes(int J, int H, int W) {
  if (J <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)J * ((size_t)kFitSlots * fit_nblk(H, W) * sizeof(double) + (size_t)kFitStateWords * sizeof(float));
}

}  // extern "C"

namespace {

// mask_index == nullptr: the unmasked entry point.  Otherwise the masked one; a call whose indices are all -1 runs the
// unmasked kernels (the same numbers: m = 1 is exact), any other the masked instantiation.
int fit_multi_impl(const int* ops, const int* img_index, const int* target_index, const int* mask_index, bool masked_entry, int J,
                   const float* imgs, int n_img, const float* targets, int n_target, const unsigned char* masks, int n_mask,
                   float* params, float* dist, void* workspace, size_t workspace_bytes, int H, int W, int steps, double lr,
                   double beta1, double beta2, double eps, int check_every, double tol, void* stream) {
  if (masked_entry && !mask_index) return set_error(T2O_EINVAL, "fit_multi_l1_adam: null pointer");
  if (!ops || !img_index || !target_index || !imgs || !targets || !params || !dist)
    return set_error(T2O_EINVAL, "fit_multi_l1_adam: null pointer");
  if (J <= 0 || J > kFitMaxJobs) return set_error(T2O_EINVAL, "fit_multi_l1_adam: 1 <= J <= 64 jobs per call");
  if (H <= 0 || W <= 0 || n_img <= 0 || n_target <= 0) return set_error(T2O_EINVAL, "fit_multi_l1_adam: H, W, n_img, n_target must be positive");
  if ((size_t)H * W > 0x7fffffffull / 3) return set_error(T2O_EINVAL, "fit_multi_l1_adam: image too large");
  if (steps < 0) return set_error(T2O_EINVAL, "fit_multi_l1_adam: steps < 0");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
    return set_error(T2O_EINVAL, "fit_multi_l1_adam: betas must lie in [0, 1)");
  if (masked_entry && n_mask < 0) return set_error(T2O_EINVAL, "fit_multi_l1_adam: n_mask < 0");
  FitMaskArgs a;
  memset(&a, 0, sizeof(a));
  bool any_mask = false;
  for (int j = 0; j < J; ++j) {
    const int op = ops[j];
    if (!(op == OP_BRIGHTNESS || op == OP_CONTRAST || op == OP_SATURATION || op == OP_COLOR || op == OP_TONE || op == OP_SHARPNESS))
      return set_error(T2O_EUNSUPPORTED, "fit_multi_l1_adam: operators 0, 1, 2, 3, 5, 6 (an operator with parameters to fit)");
    if (img_index[j] < 0 || img_index[j] >= n_img) return set_error(T2O_EINVAL, "fit_multi_l1_adam: img_index out of range");
    if (target_index[j] < 0 || target_index[j] >= n_target) return set_error(T2O_EINVAL, "fit_multi_l1_adam: target_index out of range");
    a.op[j] = op;
    a.img_index[j] = img_index[j];
    a.target_index[j] = target_index[j];
    a.mask_index[j] = -1;
    if (masked_entry) {
      const int mk = mask_index[j];
      if (mk < -1 || mk >= n_mask) return set_error(T2O_EINVAL, "fit_multi_l1_adam: mask_index out of range (-1 = no mask, 0 .. n_mask - 1)");
      if (mk >= 0 && !masks) return set_error(T2O_EINVAL, "fit_multi_l1_adam: null pointer (masks) with a mask_index >= 0");
      a.mask_index[j] = mk;
      any_mask = any_mask || mk >= 0;
    }
  }
  if (!workspace || workspace_bytes < t2o_fit_multi_workspace_bytes(J, H, W)) return set_error(T2O_EWORKSPACE, "fit_multi_l1_adam: workspace too small");
  if ((size_t)workspace & 7) return set_error(T2O_EINVAL, "fit_multi_l1_adam: workspace must be 8-byte aligned");
  a.imgs = imgs; a.targets = targets; a.params = params; a.masks = masks;
  a.H = H; a.W = W; a.nblk = fit_nblk(H, W);
  a.inv_n = 1.0f / (3.0f * (float)H * (float)W);
  a.partials = (double*)workspace;
  float* state = (float*)(a.partials + (size_t)J * kFitSlots * a.nblk);
  a.m = state;
  a.v = state + (size_t)J * kMaxParam;
  a.prev = state + (size_t)2 * J * kMaxParam;
  a.flags = (int*)(state + (size_t)2 * J * kMaxParam + J);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)a.nblk, (unsigned)J);
  k_fit_init<<<1, 256, 0, st>>>((unsigned*)state, J * kFitStateWords);
  for (int t = 1; t <= steps; ++t) {
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    if (any_mask) k_fit_eval<true, true><<<grid, kFitThreads, 0, st>>>(a);
    else k_fit_eval<true, false><<<grid, kFitThreads, 0, st>>>(a);
    k_fit_adam<<<(unsigned)J, 64, 0, st>>>(a, (float)(lr / bc1), (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)sqrt(bc2),
                                           (float)eps, (check_every > 0 && t % check_every == 0) ? 1 : 0, (float)tol);
  }
  if (any_mask) k_fit_eval<false, true><<<grid, kFitThreads, 0, st>>>(a);
  else k_fit_eval<false, false><<<grid, kFitThreads, 0, st>>>(a);
  k_fit_dist<<<(unsigned)J, 64, 0, st>>>(a, dist);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "fit_multi_l1_adam launch failed");
}

}  // namespace

extern "C" {

int t2o_fit_multi_l1_adam(const int* ops, const int* img_index, const int* target_index, int J, const float* imgs, int n_img,
                          const float* targets, int n_target, float* params, float* dist, void* workspace,
                          size_t workspace_bytes, int H, int W, int steps, double lr, double beta1, double beta2, double eps,
                          int check_every, double tol, void* stream) {
  return fit_multi_impl(ops, img_index, target_index, nullptr, false, J, imgs, n_img, targets, n_target, nullptr, 0, params, dist,
                        workspace, workspace_bytes, H, W, steps, lr, beta1, beta2, eps, check_every, tol, stream);
}

size_t t2o_fit_multi_masked_workspace_bytes(int J, int H, int W) { return t2o_fit_multi_workspace_bytes(J, H, W); }

int t2o_fit_multi_l1_adam_masked(const int* ops, const int* img_index, const int* target_index, const int* mask_index, int J,
                                 const float* imgs, int n_img, const float* targets, int n_target, const unsigned char* masks,
                                 int n_mask, float* params, float* dist, void* workspace, size_t workspace_bytes, int H, int W,
                                 int steps, double lr, double beta1, double beta2, double eps, int check_every, double tol,
                                 void* stream) {
  return fit_multi_impl(ops, img_index, target_index, mask_index, true, J, imgs, n_img, targets, n_target, masks, n_mask, params,
                        dist, workspace, workspace_bytes, H, W, steps, lr, beta1, beta2, eps, check_every, tol, stream);
}

}  // extern "C"
