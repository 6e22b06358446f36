// The LDS-free stencil (sharpness) kernels' bodies: what one thread of a strip workgroup does.  Device code only (DPP
// lane shifts): the kernels of t2o_kernels.hip and t2o_apply_planes.hip are one-line wrappers that differ in the mask fetch
// (t2o_block_programs.h: MaskF32; t2o_plane_programs.h: PlaneU8).
#pragma once
#include "t2o_chain_kernels.h"

namespace t2o {

// ---- stencil kernels without LDS (W % 4 == 0) ----
// A thread owns a column strip of kStripRows rows x one aligned quad; a wave = 64 consecutive quads
// (a 256-pixel segment) x kStripRows rows; the workgroup = 4 strips stacked (16 rows).  Every row a strip
// needs is loaded up front with independent 16-byte loads, rows above / below are simply more registers,
// left / right neighbours come from the adjacent lanes by wave-wide DPP shifts (wave_shr:1 / wave_shl:1);
// only lane 0 / lane 63 of a segment that does not touch the image border read their outside column
// from global memory.  No LDS staging pass, no barrier, no item arithmetic: these kernels stream.
// (The LDS-tile kernels of t2o_kernels.hip remain for W % 4 != 0.  Measured at bs=64
// 256x256 inside the benchmark step: backward 48.6 -> 31.0 us.  The tile kernels were issue-bound, ~170
// vector + ~90 scalar instructions per pixel mostly for window addressing and predication, and their
// load / compute / store phases added up exactly, with or without a register prefetch of the next tile.)
// blocks per sample = ceil(H / 16) * ceil(W / 256).

__device__ __forceinline__ float dpp_wave_shr1(float v) {   // lane i <- lane i-1 (lane 0 <- 0)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_wave_shl1(float v) {   // lane i <- lane i+1 (lane 63 <- 0)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xF, 0xF, true));
}

// WIDE = the image is wider than one 256-pixel segment (outside-column code compiled in).
template <bool DYN, bool WIDE, int ROWS, class MF = MaskF32>
__device__ __forceinline__ void strip_fwd_body(OpArgs a, int nblk, int nseg, const MF& mf = MF()) {
  int b, blk;
  wg_coords(nblk, b, blk);
  if (DYN && a.op_id[b] != OP_SHARPNESS) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y0 = (blk / nseg) * (4 * ROWS) + wave * ROWS, gx0 = (blk % nseg) * 256 + 4 * lane;
  const bool col_live = gx0 < a.W;
  const unsigned hw = (unsigned)a.H * (unsigned)a.W;
  const float p = a.param[(size_t)b * a.param_stride];
  const bool ext_l = WIDE && lane == 0 && gx0 > 0 && col_live, ext_r = WIDE && lane == 63 && gx0 + 4 < a.W;
  float l1 = 0.0f;
#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    const float* xp = a.img + ((size_t)b * 3 + c) * hw;
    float xr[ROWS + 2][4], tg[ROWS][4];
#pragma unroll
    for (int k = 0; k < ROWS + 2; ++k) {
      const int y = y0 - 1 + k;
      xr[k][0] = xr[k][1] = xr[k][2] = xr[k][3] = 0.0f;
      if (col_live && y >= 0 && y < a.H) load_vec<4>(xp + (unsigned)y * (unsigned)a.W + (unsigned)gx0, xr[k]);
    }
    if (a.target) {
#pragma unroll
      for (int k = 0; k < ROWS; ++k) {
        const int y = y0 + k;
        tg[k][0] = tg[k][1] = tg[k][2] = tg[k][3] = 0.0f;
        if (col_live && y < a.H) load_vec<4>(a.target + ((size_t)b * 3 + c) * hw + (unsigned)y * (unsigned)a.W + (unsigned)gx0, tg[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
      const int y = y0 + k;
      const bool live = col_live && y < a.H;
      const float* ce = xr[k + 1];
      float L = dpp_wave_shr1(ce[3]), R = dpp_wave_shl1(ce[0]);
      if (ext_l && live) L = xp[(unsigned)y * (unsigned)a.W + (unsigned)gx0 - 1];
      if (ext_r && live) R = xp[(unsigned)y * (unsigned)a.W + (unsigned)gx0 + 4];
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float left = i == 0 ? L : ce[i > 0 ? i - 1 : 0], right = i == 3 ? R : ce[i < 3 ? i + 1 : 3];
        o[i] = ce[i] + p * sharp_delta(ce[i], xr[k][i], left, right, xr[k + 2][i]);
      }
      if (!live) continue;
      const unsigned off = (unsigned)y * (unsigned)a.W + (unsigned)gx0;
      if (a.mask_ch) {
        float m[4];
        mf.template group<4>(a.mask + ((size_t)b * a.mask_ch + (a.mask_ch == 3 ? c : 0)) * hw, off, m);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = blend(o[i], ce[i], m[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = clamp01(o[i]);
      store_vec<4>(a.out + ((size_t)b * 3 + c) * hw + off, o);
      if (a.target) {
#pragma unroll
        for (int i = 0; i < 4; ++i) l1 += fabsf(o[i] - tg[k][i]);
      }
    }
  }
  if (a.target) block_reduce_store1(l1, a.loss_partials + (size_t)b * a.nblk_max + blk);
}

// Backward, strip layout as above: x rows y0-2..y0+5 and gradient (or L1 target) rows y0-1..y0+4
// are loaded up front (14 independent 16-byte loads per plane), dz is computed once per window row in
// registers (in place of the gradient rows), then the symmetric stencil is applied to it.
// WIDE (W > 256): segments OVERLAP by one quad on each side -- lanes 0 and 63 only compute the dz column
// their neighbours need (their own outer columns may be wrong and are never used) and store nothing, so a
// wave outputs 62 quads = kStripWideCols pixels and no lane ever needs a dz from outside its wave.

// MASKED: out = clamp(blend(x + p * Lap(x), x, m)): with do = dz * m the input gradient is
// dz * (1 - m) + do + p * Lap(do) and d loss / d p sums do * Lap(x); the mask rows ride along in registers.
// VAL (fused-L1 calls only): the launch also emits |out - target| partial sums (a.loss_partials) and, when a.out is set,
// the output image -- a value-and-gradient call needs no forward launch.  A separate instantiation: the plain kernels keep
// their register count (119 / 173 VGPRs; +29 with the value outputs).
template <bool DYN, bool WIDE, bool MASKED, bool VAL = false, class MF = MaskF32>
__device__ __forceinline__ void strip_bwd_body(OpArgs a, int nblk, int nseg, const MF& mf = MF()) {
  int b, blk;
  wg_coords(nblk, b, blk);
  if (DYN && a.op_id[b] != OP_SHARPNESS) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y0 = (blk / nseg) * (4 * kStripRows) + wave * kStripRows;
  const int gx0 = WIDE ? (blk % nseg) * kStripWideCols - 4 + 4 * lane : 4 * lane;
  const bool col_live = gx0 >= 0 && gx0 < a.W;
  const bool own = !WIDE || (lane >= 1 && lane <= 62);      // this lane's quad is output (not an overlap lane)
  const unsigned hw = (unsigned)a.H * (unsigned)a.W;
  const float p = a.param[(size_t)b * a.param_stride];
  const float gs = a.target ? a.gloss[0] * a.inv_n : 0.0f;
  float red0 = 0.0f;
  float l1 = 0.0f;                  // L1 form: sum |out - target| over this thread's output pixels (value-and-gradient calls)
#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    const float* xp = a.img + ((size_t)b * 3 + c) * hw;
    const float* gp = (a.target ? a.target : a.gout) + ((size_t)b * 3 + c) * hw;
    const float* mp = MASKED ? a.mask + ((size_t)b * a.mask_ch + (a.mask_ch == 3 ? c : 0)) * hw : nullptr;
    float xr[kStripRows + 4][4], g[kStripRows + 2][4], mk[MASKED ? kStripRows + 2 : 1][4], pass[MASKED ? kStripRows : 1][4];
#pragma unroll
    for (int k = 0; k < kStripRows + 4; ++k) {
      const int y = y0 - 2 + k;
      xr[k][0] = xr[k][1] = xr[k][2] = xr[k][3] = 0.0f;
      if (col_live && y >= 0 && y < a.H) load_vec<4>(xp + (unsigned)y * (unsigned)a.W + (unsigned)gx0, xr[k]);
    }
#pragma unroll
    for (int k = 0; k < kStripRows + 2; ++k) {
      const int y = y0 - 1 + k;
      g[k][0] = g[k][1] = g[k][2] = g[k][3] = 0.0f;
      if (MASKED) mk[k][0] = mk[k][1] = mk[k][2] = mk[k][3] = 0.0f;
      if (col_live && y >= 0 && y < a.H) {
        load_vec<4>(gp + (unsigned)y * (unsigned)a.W + (unsigned)gx0, g[k]);
        if (MASKED) mf.template group<4>(mp, (unsigned)y * (unsigned)a.W + (unsigned)gx0, mk[k]);
      }
    }
    // dz for window rows y0-1 .. y0+kStripRows (in place of g)
#pragma unroll
    for (int k = 0; k < kStripRows + 2; ++k) {
      const int y = y0 - 1 + k;
      const bool in = col_live && y >= 0 && y < a.H;
      const float* ce = xr[k + 1];
      const float L = dpp_wave_shr1(ce[3]), R = dpp_wave_shl1(ce[0]);
      const bool mine = VAL && k >= 1 && k <= kStripRows && own && in;        // an output pixel of this thread
      float oz[VAL ? 4 : 1];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float left = i == 0 ? L : ce[i > 0 ? i - 1 : 0], right = i == 3 ? R : ce[i < 3 ? i + 1 : 3];
        const float d = sharp_delta(ce[i], xr[k][i], left, right, xr[k + 2][i]);
        const float m = MASKED ? mk[k][i] : 1.0f;
        float z = ce[i] + p * d;
        if (MASKED) z = blend(z, ce[i], m);
        if constexpr (VAL) {
          oz[i] = clamp01(z);
          if (mine) l1 += fabsf(oz[i] - g[k][i]);
        }
        const float gz = a.target ? sign_of(clamp01(z) - g[k][i]) * gs : g[k][i];
        const float dz = (in && z >= 0.0f && z <= 1.0f) ? gz : 0.0f;
        g[k][i] = MASKED ? dz * m : dz;                                   // do
        if (MASKED && k >= 1 && k <= kStripRows) pass[k - 1][i] = dz * (1.0f - m);
        if (k >= 1 && k <= kStripRows && own) red0 += dz * m * d;
      }
      if constexpr (VAL) {
        if (a.out && mine) store_vec<4>(a.out + ((size_t)b * 3 + c) * hw + (unsigned)y * (unsigned)a.W + (unsigned)gx0, oz);
      }
    }
    // gimg rows y0 .. y0+kStripRows-1
#pragma unroll
    for (int k = 1; k <= kStripRows; ++k) {
      const int y = y0 - 1 + k;
      const float* ce = g[k];
      const float L = dpp_wave_shr1(ce[3]), R = dpp_wave_shl1(ce[0]);
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float left = i == 0 ? L : ce[i > 0 ? i - 1 : 0], right = i == 3 ? R : ce[i < 3 ? i + 1 : 3];
        o[i] = ce[i] + p * sharp_delta(ce[i], g[k - 1][i], left, right, g[k + 1][i]);
        if (MASKED) o[i] = pass[k - 1][i] + o[i];
      }
      if (a.gimg && own && col_live && y < a.H)
        store_vec<4>(a.gimg + ((size_t)b * 3 + c) * hw + (unsigned)y * (unsigned)a.W + (unsigned)gx0, o);
    }
  }
  block_reduce_store1(red0, a.partials + ((size_t)b * a.nblk_max + blk) * kRedSlots);
  if constexpr (VAL) {
    __syncthreads();                                           // (block_reduce_store1's staging cells are reused)
    block_reduce_store1(l1, a.loss_partials + (size_t)b * a.nblk_max + blk);
  }
}

}  // namespace t2o
