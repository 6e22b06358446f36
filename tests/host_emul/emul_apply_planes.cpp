// Host emulation of the per-sample operator kernels under a mask, with either mask fetch -- TEST HARNESS ONLY (see
// emul.cpp).
//
// g++ compiles the block programs and this file walks them workgroup by workgroup, thread by thread, the way the
// OP_DYNAMIC kernels of t2o_kernels.hip (fetch MaskF32: a (B,1,H,W) fp32 mask) and of t2o_apply_planes.hip (fetch PlaneU8:
// the uint8 planes of a MaskTable, read in place) do: pointwise forward and backward with the launch geometry's vector
// width, the LDS-tile sharpness forward and backward.  The caller compares the two walks bit for bit.  (The LDS-free strip
// kernels exchange neighbours by DPP and have no host form; their mask fetch is PlaneU8::group<4>, which the V = 4
// pointwise walk exercises at every alignment.)  Never shipped, never a fallback.
#include <string.h>

#include <vector>

#include "../../t2onet_amd/csrc/t2o_plane_programs.h"

using namespace t2o;

namespace {

template <int V, class MF>
void walk_point(const OpArgs& a, const Geometry& g, int op, int b, const MF& mf) {
  float tab[kTabStride];
  memset(tab, 0, sizeof(tab));
  if (op == OP_COLOR || op == OP_TONE) curve_table_build(a.param + (size_t)b * a.param_stride, op == OP_COLOR, tab);
  for (int blk = 0; blk < g.nblk_point; ++blk) {
    float sum[kRedSlots];
    for (int i = 0; i < kRedSlots; ++i) sum[i] = 0.0f;
    for (int tid = 0; tid < kThreads; ++tid) {
      pointwise_fwd_thread<V, true, false>(a, op, b, blk, tid, mf);
      float red[kRedSlots];
      for (int i = 0; i < kRedSlots; ++i) red[i] = 0.0f;
      pointwise_bwd_thread<V, true, false>(a, op, b, blk, tid, red, tab, mf);
      for (int i = 0; i < kRedSlots; ++i) sum[i] += red[i];            // (thread order: the same for both fetches)
    }
    memcpy(a.partials + ((size_t)b * a.nblk_max + blk) * kRedSlots, sum, sizeof(sum));
  }
}

void tile_bwd_load(const OpArgs& a, const MaskF32&, int b, int tile, int tid, float* lds) { sharp_bwd_phase_load<1>(a, b, tile, tid, lds); }
void tile_bwd_load(const OpArgs& a, const PlaneU8& mf, int b, int tile, int tid, float* lds) { sharp_bwd_phase_load_planes(a, mf, b, tile, tid, lds); }

template <class MF>
void walk_tiles(const OpArgs& a, const Geometry& g, int b, const MF& mf) {
  std::vector<float> lds((size_t)sharp_bwd_lds_floats(1));
  for (int tile = 0; tile < g.nblk_sharp; ++tile) {
    for (int tid = 0; tid < kThreads; ++tid) sharp_fwd_phase_load<1>(a, b, tile, tid, lds.data());
    for (int tid = 0; tid < kThreads; ++tid) sharp_fwd_phase_compute<1>(a, b, tile, tid, lds.data(), mf);
    for (int tid = 0; tid < kThreads; ++tid) tile_bwd_load(a, mf, b, tile, tid, lds.data());
    float sum = 0.0f;
    for (int tid = 0; tid < kThreads; ++tid) {
      float red0 = 0.0f;
      sharp_bwd_phase_dz<1>(a, b, tile, tid, lds.data(), red0);
      sum += red0;
    }
    for (int tid = 0; tid < kThreads; ++tid) sharp_bwd_phase_out<1>(a, b, tile, tid, lds.data());
    a.partials[((size_t)b * a.nblk_max + tile) * kRedSlots] = sum;
  }
}

template <class MF>
void walk_sample(const OpArgs& a, const Geometry& g, int op, int b, const MF& mf) {
  if (op == OP_SHARPNESS) walk_tiles(a, g, b, mf);
  else if (g.vec == 4) walk_point<4>(a, g, op, b, mf);
  else walk_point<1>(a, g, op, b, mf);
}

}  // namespace

extern "C" {

// block rows per sample of the partials array
int emul_apply_planes_rows(int B, int H, int W) { return geometry(B, H, W).nblk_max; }

// One masked per-sample call, forward and backward.  mask_f32 null: the byte-plane fetch on (planes, slot, pred_op); else
// the fp32 fetch on mask_f32 (B,1,H,W).  out, gimg: (B,3,H,W); partials: (B, rows, 24) zero-filled by the caller.
int emul_apply_planes(const int* op_id, const long long* pred_op, const unsigned char* planes, const int* slot, int N, int V,
                      const float* mask_f32, const float* img, const float* param, const float* gout, float* out, float* gimg,
                      float* partials, int B, int H, int W) {
  const Geometry g = geometry(B, H, W);
  OpArgs a;
  memset(&a, 0, sizeof(a));
  a.img = img; a.param = param; a.op_id = op_id; a.gout = gout; a.out = out; a.gimg = gimg; a.partials = partials;
  a.op = OP_DYNAMIC; a.param_stride = kMaxParam; a.mask_ch = 1; a.mask = mask_f32; a.B = B; a.H = H; a.W = W;
  a.iters = g.iters; a.nblk_max = g.nblk_max;
  a.inv_n = 1.0f / ((float)B * 3.0f * (float)H * (float)W);
  PlaneArgs pa;
  pa.planes = planes; pa.slot = slot; pa.pred_op = pred_op; pa.N = N; pa.V = V;
  for (int b = 0; b < B; ++b) {
    int op = op_id[b];
    if (op < 0 || op > 7 || op == OP_INPAINT) op = OP_IDENTITY;            // the kernels' `default:` branch
    if (mask_f32) walk_sample(a, g, op, b, MaskF32());
    else walk_sample(a, g, op, b, PlaneU8{plane_of(pa, b, (size_t)H * W)});
  }
  return 0;
}

}  // extern "C"
