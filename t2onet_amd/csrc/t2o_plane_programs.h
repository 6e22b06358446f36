// Byte-plane mask fetch for the per-sample operator programs (t2o_apply_planes.hip): the masked programs of
// t2o_block_programs.h / t2o_strip_kernels.h run unchanged, only the place their mask values come from differs -- the uint8
// plane the sample's chosen operator points at (gier.MaskTable), read where it lies, instead of a (B,1,H,W) fp32 tensor
// that t2o_mask_select expanded it to.  float(byte) is exact, so both give the same floats and, with the same programs
// behind them, the same bits.
//
// `__host__ __device__` programs, as the other block programs: tests/host_emul/emul_apply_planes.cpp walks them next to
// the fp32-mask forms (a test harness, never a fallback).
#pragma once
#include "t2o_block_programs.h"

namespace t2o {

struct PlaneArgs {
  const unsigned char* planes;   // (N, H*W) uint8, packed: plane k starts at byte k * H*W, whatever its alignment
  const int* slot;               // (B, V): a plane number, anything else = no plane
  const long long* pred_op;      // (B) int64: the operator vocabulary id each sample chose
  int N, V;
};

// The plane of sample b, or null for "all ones" (select_plane of t2o_mask_math.h: pred_op outside [0, V) or a slot that is
// not a plane number means a global edit).  Uniform per workgroup: looked up once, before the pixel loop.
T2O_HD const unsigned char* plane_of(const PlaneArgs& p, int b, size_t hw) {
  const long long op = p.pred_op[b];
  if (op < 0 || op >= (long long)p.V) return nullptr;
  const int k = p.slot[(size_t)b * p.V + (size_t)op];
  return (k < 0 || k >= p.N) ? nullptr : p.planes + (size_t)k * hw;
}

// The mask fetch (see MaskF32): p = the sample's plane or null.
struct PlaneU8 {
  const unsigned char* p;

  // V consecutive mask values from pixel px on.  Four bytes are ONE 32-bit load when their address is 4-aligned -- a
  // run-time test: for odd H*W every second plane starts at an odd byte -- else four byte loads.
  template <int V>
  T2O_HD_MEMBER void group(const float*, unsigned px, float (&r)[V]) const {
    if (!p) {
      T2O_UNROLL
      for (int i = 0; i < V; ++i) r[i] = 1.0f;
      return;
    }
    const unsigned char* q = p + px;
    if (V == 4 && ((size_t)q & 3) == 0) {
      const unsigned word = *reinterpret_cast<const unsigned*>(q);
      T2O_UNROLL
      for (int i = 0; i < V; ++i) r[i] = (float)((word >> (8 * i)) & 255u);
      return;
    }
    T2O_UNROLL
    for (int i = 0; i < V; ++i) r[i] = (float)q[i];
  }

  T2O_HD_MEMBER float at(const OpArgs&, int, int, size_t px) const { return p ? (float)p[px] : 1.0f; }
};

// LDS-tile stencil backward (ragged widths): the mask tile [1 plane, halo 1] filled from the bytes, converted while it is
// filled, zero outside the image as tile_load leaves it -- phases dz and out then run as they are.
template <int HALO>
T2O_HD void tile_load_u8(const PlaneU8& mf, int H, int W, int y0, int x0, float* lds, int tid) {
  constexpr int rows = kTileH + 2 * HALO, cols = kTileW + 2 * HALO;
  for (int i = tid; i < rows * cols; i += kThreads) {
    const int r = i / cols, j = i % cols - HALO;
    const int gy = y0 - HALO + r, gx = x0 + j;
    float v = 0.0f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = mf.p ? (float)mf.p[(unsigned)gy * (unsigned)W + (unsigned)gx] : 1.0f;
    lds[r * kRowStride + kIntOff + j] = v;
  }
}

// sharp_bwd_phase_load<1> with the mask tile from the plane (a.mask_ch == 1, a.mask unused)
T2O_HD void sharp_bwd_phase_load_planes(const OpArgs& a, const PlaneU8& mf, int b, int tile, int tid, float* lds) {
  int y0, x0;
  tile_origin(a, tile, y0, x0);
  const unsigned hw = (unsigned)a.H * (unsigned)a.W;
  tile_load<1, 2>(a.img + plane_off(a, b, 0), hw, 3, a.H, a.W, y0, x0, lds + sharp_bwd_x_off(), tid);
  tile_load<1, 1>(a.gout + plane_off(a, b, 0), hw, 3, a.H, a.W, y0, x0, lds + sharp_bwd_g_off(), tid);
  tile_load_u8<1>(mf, a.H, a.W, y0, x0, lds + sharp_bwd_m_off(), tid);
}

}  // namespace t2o
