// t2o_apply_planes.hip -- per-sample operators under the uint8 mask planes of a gier.MaskTable: t2o_mask_select +
// t2o_apply_fwd / t2o_apply_bwd as one call that reads the planes where they lie (programs: t2o_plane_programs.h).
//
// Every kernel here is the masked per-sample (OP_DYNAMIC) kernel of t2o_kernels.hip with the mask fetch replaced: the same
// block programs, launch geometry, partials layout and finalisation kernel, so out, gimg and gparam carry the same bits
// as the two-launch path -- the parameter sums add in the same order.  What changes is the traffic: one byte of mask per
// pixel instead of a 4-byte store plus a 4-byte load, no fp32 mask kept for the backward, one launch less per step.
//
//   k_planes_point_fwd / _bwd <V>      pointwise operators, V = 4 (H*W % 4 == 0) or 1
//   k_planes_strip_fwd / _bwd <WIDE>   sharpness, W % 4 == 0: LDS-free strips, one or several 256-column segments
//   k_planes_tile_fwd / _bwd           sharpness, ragged widths: LDS tiles, bytes converted while the tile is filled
// The slot lookup is uniform per workgroup and done once, before the pixel loop.  Enqueue only: no allocation, no
// synchronisation, capturable; deterministic two-stage parameter sums as in t2o_kernels.hip.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/t2onet_hip.h"
#include "t2o_plane_programs.h"
#include "t2o_strip_kernels.h"

namespace t2o {
int set_error(int code, const char* msg);
bool stencil_uses_strips(const Geometry& g);
void launch_finalize_params(const OpArgs& a, float* gparam, int gparam_stride, int nblk_point, int nblk_sharp, void* stream);
}
using namespace t2o;

namespace {

__device__ __forceinline__ PlaneU8 plane_fetch(const OpArgs& a, const PlaneArgs& pa, int b) {
  return PlaneU8{plane_of(pa, b, (size_t)a.H * (size_t)a.W)};
}

template <int V>
__global__ __launch_bounds__(kThreads) void k_planes_point_fwd(OpArgs a, PlaneArgs pa, int nblk) {
  int b, blk;
  wg_coords(nblk, b, blk);
  const int op = a.op_id[b];
  if (op == OP_SHARPNESS) return;                          // handled by the stencil kernel
  const PlaneU8 mf = plane_fetch(a, pa, b);
  switch (op) {                                            // one specialised body per operator, as k_point_fwd
#define T2O_CASE(K) case K: pointwise_fwd_thread<V, true, false>(a, K, b, blk, threadIdx.x, mf); break;
    T2O_CASE(OP_BRIGHTNESS) T2O_CASE(OP_CONTRAST) T2O_CASE(OP_SATURATION) T2O_CASE(OP_COLOR)
    T2O_CASE(OP_TONE) T2O_CASE(OP_WHITE)
#undef T2O_CASE
    default: pointwise_fwd_thread<V, true, false>(a, OP_IDENTITY, b, blk, threadIdx.x, mf); break;
  }
}

template <int V>
__global__ __launch_bounds__(kThreads) void k_planes_point_bwd(OpArgs a, PlaneArgs pa, int nblk) {
  int b, blk;
  wg_coords(nblk, b, blk);
  const int op = a.op_id[b];
  if (op == OP_SHARPNESS) return;
  const PlaneU8 mf = plane_fetch(a, pa, b);
  float red[kRedSlots];
#pragma unroll
  for (int i = 0; i < kRedSlots; ++i) red[i] = 0.0f;
  __shared__ float tab[kTabStride];                        // curve lookup table of this sample (curve operators only)
  if ((op == OP_COLOR || op == OP_TONE) && threadIdx.x == 0)
    curve_table_build(a.param + (size_t)b * a.param_stride, op == OP_COLOR, tab);
  __syncthreads();
  switch (op) {
#define T2O_CASE(K) case K: pointwise_bwd_thread<V, true, false>(a, K, b, blk, threadIdx.x, red, tab, mf); break;
    T2O_CASE(OP_BRIGHTNESS) T2O_CASE(OP_CONTRAST) T2O_CASE(OP_SATURATION) T2O_CASE(OP_COLOR)
    T2O_CASE(OP_TONE) T2O_CASE(OP_WHITE)
#undef T2O_CASE
    default: pointwise_bwd_thread<V, true, false>(a, OP_IDENTITY, b, blk, threadIdx.x, red, tab, mf); break;
  }
  if (op == OP_IDENTITY || op == OP_WHITE) return;         // no parameter gradient (uniform per block)
  block_reduce_store(red, nred_of(op), a.partials + ((size_t)b * a.nblk_max + blk) * kRedSlots);
}

// (sample of this workgroup: the bodies below derive it again from the same mapping)
__device__ __forceinline__ int wg_sample(int per_sample) {
  int b, blk;
  wg_coords(per_sample, b, blk);
  return b;
}

template <bool WIDE>
__global__ __launch_bounds__(kThreads) void k_planes_strip_fwd(OpArgs a, PlaneArgs pa, int nblk, int nseg) {
  const int b = wg_sample(nblk);
  if (a.op_id[b] != OP_SHARPNESS) return;
  strip_fwd_body<true, WIDE, kFwdStripRows>(a, nblk, nseg, plane_fetch(a, pa, b));
}

template <bool WIDE>
__global__ __launch_bounds__(kThreads) void k_planes_strip_bwd(OpArgs a, PlaneArgs pa, int nblk, int nseg) {
  const int b = wg_sample(nblk);
  if (a.op_id[b] != OP_SHARPNESS) return;
  strip_bwd_body<true, WIDE, true, false>(a, nblk, nseg, plane_fetch(a, pa, b));
}

__global__ __launch_bounds__(kThreads) void k_planes_tile_fwd(OpArgs a, PlaneArgs pa, int tiles) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int b, tile;
  wg_coords(tiles, b, tile);
  if (a.op_id[b] != OP_SHARPNESS) return;
  const PlaneU8 mf = plane_fetch(a, pa, b);
  sharp_fwd_phase_load<1>(a, b, tile, threadIdx.x, lds);
  __syncthreads();
  sharp_fwd_phase_compute<1>(a, b, tile, threadIdx.x, lds, mf);
}

__global__ __launch_bounds__(kThreads) void k_planes_tile_bwd(OpArgs a, PlaneArgs pa, int tiles) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int b, tile;
  wg_coords(tiles, b, tile);
  if (a.op_id[b] != OP_SHARPNESS) return;
  sharp_bwd_phase_load_planes(a, plane_fetch(a, pa, b), b, tile, threadIdx.x, lds);
  __syncthreads();
  float red0 = 0.0f;
  sharp_bwd_phase_dz<1>(a, b, tile, threadIdx.x, lds, red0);
  __syncthreads();
  sharp_bwd_phase_out<1>(a, b, tile, threadIdx.x, lds);
  block_reduce_store1(red0, a.partials + ((size_t)b * a.nblk_max + tile) * kRedSlots);
}

// the checks of t2o_apply_* (check_common of t2o_kernels.hip, per-sample form) and of t2o_mask_select, same codes
int check_planes(const char*& why, const int* op_id, const long long* pred_op, const unsigned char* planes, const int* slot, int N,
                 int V, const float* img, const float* param, int param_stride, int B, int H, int W) {
  why = nullptr;
  if (B <= 0 || H <= 0 || W <= 0) why = "apply_planes: B, H, W must be positive";
  else if (!img) why = "apply_planes: img is null";
  else if (!op_id) why = "apply_planes: op_id is null";
  else if (!param || param_stride < kMaxParam) why = "apply_planes: param rows must be padded to >= 24 floats";
  else if (!slot || !pred_op) why = "apply_planes: slot or pred_op is null";
  else if (N < 0 || (N > 0 && !planes)) why = "apply_planes: null plane buffer";
  else if (V <= 0) why = "apply_planes: V must be positive";
  else if ((size_t)B * (size_t)sharp_num_tiles(H, W) > 0x7fffffffull || (size_t)H * W > 0x7fffffffull)
    why = "apply_planes: image too large for the launch grid";
  return why ? T2O_EINVAL : T2O_OK;
}

void fill(OpArgs& a, PlaneArgs& pa, const Geometry& g, const int* op_id, const long long* pred_op, const unsigned char* planes,
          const int* slot, int N, int V, const float* img, const float* param, int param_stride, int B, int H, int W) {
  memset(&a, 0, sizeof(a));
  a.img = img; a.param = param; a.op_id = op_id;
  a.op = OP_DYNAMIC; a.param_stride = param_stride; a.B = B; a.H = H; a.W = W;
  a.mask_ch = 1;                                           // the masked programs, one mask channel; a.mask stays null: the
  a.iters = g.iters; a.nblk_max = g.nblk_max;              // fetch (PlaneU8) never reads it
  a.inv_n = 1.0f / ((float)B * 3.0f * (float)H * (float)W);
  pa.planes = planes; pa.slot = slot; pa.pred_op = pred_op; pa.N = N; pa.V = V;
}

int launched(const char* what) {
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, what);
}

}  // namespace

extern "C" int t2o_apply_planes_fwd(const int* op_id, const long long* pred_op, const unsigned char* planes, const int* slot, int N,
                                    int V, const float* img, const float* param, int param_stride, float* out, int B, int H,
                                    int W, void* stream) {
  const char* why;
  if (check_planes(why, op_id, pred_op, planes, slot, N, V, img, param, param_stride, B, H, W)) return set_error(T2O_EINVAL, why);
  if (!out) return set_error(T2O_EINVAL, "apply_planes: out is null");
  const Geometry g = geometry(B, H, W);                    // (launch_geometry of t2o_kernels.hip)
  OpArgs a;
  PlaneArgs pa;
  fill(a, pa, g, op_id, pred_op, planes, slot, N, V, img, param, param_stride, B, H, W);
  a.out = out;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)B * g.nblk_point;
  if (g.vec == 4) k_planes_point_fwd<4><<<grid, kThreads, 0, st>>>(a, pa, g.nblk_point);
  else k_planes_point_fwd<1><<<grid, kThreads, 0, st>>>(a, pa, g.nblk_point);
  if (stencil_uses_strips(g)) {
    const int nseg = (W + 255) / 256, nblk = g.nblk_strip_fwd;
    if (nseg > 1) k_planes_strip_fwd<true><<<(unsigned)B * nblk, kThreads, 0, st>>>(a, pa, nblk, nseg);
    else k_planes_strip_fwd<false><<<(unsigned)B * nblk, kThreads, 0, st>>>(a, pa, nblk, nseg);
  } else {
    k_planes_tile_fwd<<<(unsigned)B * g.nblk_sharp, kThreads, sizeof(float) * sharp_fwd_lds_floats(), st>>>(a, pa, g.nblk_sharp);
  }
  return launched("apply_planes forward launch failed");
}

extern "C" int t2o_apply_planes_bwd(const int* op_id, const long long* pred_op, const unsigned char* planes, const int* slot, int N,
                                    int V, const float* img, const float* param, int param_stride, const float* gout,
                                    float* gimg, float* gparam, int gparam_stride, void* workspace, size_t workspace_bytes, int B,
                                    int H, int W, void* stream) {
  const char* why;
  if (check_planes(why, op_id, pred_op, planes, slot, N, V, img, param, param_stride, B, H, W)) return set_error(T2O_EINVAL, why);
  if (!gout) return set_error(T2O_EINVAL, "apply_planes: gout is null");
  if (!workspace || workspace_bytes < t2o_workspace_bytes(B, H, W)) return set_error(T2O_EWORKSPACE, "apply_planes: workspace too small");
  if (gparam && gparam_stride < kMaxParam) return set_error(T2O_EINVAL, "apply_planes: gparam_stride too small");
  const Geometry g = geometry(B, H, W);
  OpArgs a;
  PlaneArgs pa;
  fill(a, pa, g, op_id, pred_op, planes, slot, N, V, img, param, param_stride, B, H, W);
  a.gout = gout; a.gimg = gimg; a.partials = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)B * g.nblk_point;
  if (g.vec == 4) k_planes_point_bwd<4><<<grid, kThreads, 0, st>>>(a, pa, g.nblk_point);
  else k_planes_point_bwd<1><<<grid, kThreads, 0, st>>>(a, pa, g.nblk_point);
  int nblk_sharp = g.nblk_sharp;
  if (stencil_uses_strips(g)) {
    const int nseg = strip_bwd_segments(W);
    nblk_sharp = g.nblk_strip_bwd;
    if (nseg > 1) k_planes_strip_bwd<true><<<(unsigned)B * nblk_sharp, kThreads, 0, st>>>(a, pa, nblk_sharp, nseg);
    else k_planes_strip_bwd<false><<<(unsigned)B * nblk_sharp, kThreads, 0, st>>>(a, pa, nblk_sharp, nseg);
  } else {
    k_planes_tile_bwd<<<(unsigned)B * nblk_sharp, kThreads, sizeof(float) * sharp_bwd_lds_floats(1), st>>>(a, pa, nblk_sharp);
  }
  if (gparam) launch_finalize_params(a, gparam, gparam_stride, g.nblk_point, nblk_sharp, stream);
  return launched("apply_planes backward launch failed");
}
