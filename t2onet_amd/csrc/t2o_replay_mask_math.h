// The per-tile program of the MASKED 8-bit replay kernel (t2o_replay_mask.hip): t2o_replay_math.h's program with
// Operator.execute's mask operand (models/operators.py:112-131) -- step k of a job may name an (h,w) uint8 plane m_k, and
//   x = clamp01(blend(process(op_k, x, p_k), x, m_k / 255))     where it names one,
//   x = clamp01(process(op_k, x, p_k))                          where it names none.
// 0 leaves a pixel as it is, 255 applies the operator, values between feather the edge.  The bytes are those of
// resize (same size) -> t2o_op_fwd with the mask as (1,1,h,w) fp32 per step -> f32_to_u8_hwc: the same device functions
// (pointwise_fwd, sharp_delta, blend, clamp01, u8_to_unit, unit_to_u8) in the same order.
//
// The source load, the output staging and the store are t2o_replay_math.h's phases, used as they are (ReplayMaskLds
// starts with a ReplayLds).  What is new:
//   mask   every distinct mask the job's list names is staged like the source: the window's rows (tile + the 1-pixel
//          ring of a sharpness list) as ALIGNED dwords with the row's address modulo 4 as a lead-in, 1 byte per pixel.
//          While staging, two flags per mask are raised: "a byte of the window is not 0" and "a byte of the TILE is
//          not 0".  They are cleared one barrier earlier (in the source load's phase).
//   pre    as before, with the masked steps in front of the sharpness blended on tile + ring (the stencil reads the
//          blended neighbours); the zero padding of the intermediate image at the picture's border is unchanged
//   main   a masked sharpness blends the stencil's result with the stencil's INPUT at the centre pixel
// TILE SKIP: a step whose mask is all zero over the pixels this phase computes (window flag in pre, tile flag in main)
// is not run.  With m = 0, blend(o, x, 0) = o * 0 + x * 1 = x for every finite o (x lies in [0,1], so clamp01 keeps it),
// and process() is finite for finite parameters: the bytes do not change.  The flags are the same for every thread of
// the workgroup, so the branch is wave-uniform.
#pragma once
#include "t2o_replay_math.h"

namespace t2o {

constexpr int kReplayMaxMasks = 4;
constexpr int kReplayMaskDw = (3 + kReplayWin + 3) / 4;      // 10 dwords per staged mask row (lead-in + 34 pixels)

// one job as the masked kernel sees it: 48 bytes, 64 of them + the mask table stay under the 4 KB of kernel arguments
struct ReplayMaskJob {
  ReplayJob j;
  unsigned long long mask_of;    // step k's mask index as a signed byte at bits [8k, 8k+8), -1 = none (as ReplayJob::ops)
};

T2O_HD int replay_mask_of(const ReplayMaskJob& m, int k) { return (int)(signed char)(unsigned char)(m.mask_of >> (8 * k)); }

// bit i set: some applied step of the job names mask i
T2O_HD unsigned replay_masks_used(const ReplayMaskJob& m) {
  unsigned used = 0;
  for (int k = 0; k < m.j.steps; ++k) {
    const int i = replay_mask_of(m, k);
    if (i >= 0 && replay_op(m.j, k) >= 0) used |= 1u << i;
  }
  return used;
}

// Host side: the job check, replay_job_fill of t2o_replay_math.h, under the name this kernel's host emulation calls
static inline int replay_mask_job_make(ReplayMaskJob& d, long long src_offset, long long out_offset, int h, int w, int steps,
                                       const int* ops, const int* mask_of, int n_masks, const char** why) {
  return replay_job_fill(d.j, d.mask_of, "replay_u8_masked", kReplaySharpIndex, src_offset, out_offset, h, w, steps, ops, mask_of, n_masks, why);
}

struct ReplayMaskArgs {
  const unsigned char* src;
  unsigned char* out;
  const float* params;           // (J, 8, 24)
  const unsigned char* masks;
  long long mask_offsets[kReplayMaxMasks];     // first byte of mask i, counted from masks
  ReplayMaskJob jobs[kReplayMaxJobs];
};

// Host side: what the three entry points do alike in front of their launch: the checks in their order and `a` filled in.
// AbiJob = t2o_replay_job_t; mask_of: (J, 8) or NULL; *grid_x, *max_ring = the largest tile count and ReplayJob::sharp.
template <class AbiJob>
static inline int replay_launch_prepare(ReplayMaskArgs& a, const char* who, ReplaySharp mode, const unsigned char* src,
                                        unsigned char* out, const AbiJob* jobs, const int* mask_of, int J, const float* params,
                                        const unsigned char* masks, const long long* mask_offsets, int n_masks,
                                        unsigned* grid_x, int* max_ring, const char** why) {
  if (!src || !out || !jobs) return replay_refuse(why, 1, who, "null pointer");
  if (J <= 0 || J > kReplayMaxJobs) return replay_refuse(why, 1, who, "1 <= J <= 64 jobs per launch");
  if (n_masks < 0 || n_masks > kReplayMaxMasks) return replay_refuse(why, 1, who, "at most 4 masks per launch");
  if (n_masks > 0 && (!masks || !mask_offsets || !mask_of))
    return replay_refuse(why, 1, who, mode == kReplaySharpIndex ? "null mask buffer or offset table"
                                                                : "null mask buffer, offset table or mask index table");
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n_masks; ++i) {
    if (mask_offsets[i] < 0) return replay_refuse(why, 1, who, "negative mask offset");
    a.mask_offsets[i] = mask_offsets[i];
  }
  long long max_tiles = 0;
  bool any_step = false;
  *max_ring = 0;
  for (int i = 0; i < J; ++i) {
    const AbiJob& s = jobs[i];
    if (const int rc = replay_job_fill(a.jobs[i].j, a.jobs[i].mask_of, who, mode, s.src_offset, s.out_offset, s.h, s.w, s.steps, s.ops,
                                       mask_of ? mask_of + (size_t)i * kReplayMaxSteps : nullptr, n_masks, why))
      return rc;
    for (int k = 0; k < s.steps; ++k) any_step = any_step || s.ops[k] >= 0;
    const long long tiles = (long long)((s.w + kReplayTile - 1) / kReplayTile) * ((s.h + kReplayTile - 1) / kReplayTile);
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
    *max_ring = a.jobs[i].j.sharp > *max_ring ? a.jobs[i].j.sharp : *max_ring;
  }
  if (any_step && !params) return replay_refuse(why, 1, who, "null parameter table");
  if (max_tiles > 0x7fffffffll) return replay_refuse(why, 1, who, "more than 2^31 - 1 tiles in a picture");
  a.src = src; a.out = out; a.params = params; a.masks = masks;
  *grid_x = (unsigned)max_tiles;
  return 0;
}

struct ReplayMaskLds {
  ReplayLds base;
  unsigned mraw[kReplayMaxMasks][kReplayWin * kReplayMaskDw];      // mask rows, each with its lead-in
  int nz_win[kReplayMaxMasks];                                      // a byte of the staged window is not 0
  int nz_tile[kReplayMaxMasks];                                     // a byte of the tile itself is not 0
};

// a value that is the same in every thread, told to the compiler (scalar branch instead of a masked one)
T2O_HD int replay_uniform(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_readfirstlane(v);
#else
  return v;
#endif
}

// ---------------------------------------------------------------- phase: clear (runs beside the source load)
T2O_HD void replay_phase_mask_clear(int tid, ReplayMaskLds& lds) {
  if (tid < kReplayMaxMasks) lds.nz_win[tid] = lds.nz_tile[tid] = 0;
}

// ---------------------------------------------------------------- phase: mask load
T2O_HD void replay_phase_mask_load(const ReplayMaskJob& mj, const unsigned char* masks, const long long* mask_offsets,
                                   const ReplayTile& t, int tid, ReplayMaskLds& lds) {
  const ReplayJob& j = mj.j;
  const unsigned used = replay_masks_used(mj);
  const int rows = t.ry1 - t.ry0, nb = t.cx1 - t.cx0;
  for (int i = 0; i < kReplayMaxMasks; ++i) {
    if (!(used >> i & 1)) continue;
    const unsigned char* plane = masks + mask_offsets[i];
    const unsigned char* end = plane + (size_t)j.h * j.w;
    bool win = false, tile = false;
    for (int id = tid; id < rows * kReplayMaskDw; id += kReplayThreads) {
      const int r = id / kReplayMaskDw, d = id - r * kReplayMaskDw;
      const unsigned char* a = plane + (size_t)(t.ry0 + r) * j.w + t.cx0;
      const int m = (int)replay_misalign(a);
      if (4 * d >= m + nb) continue;
      const unsigned v = replay_load_dword(a - m + 4 * d, plane, end);
      lds.mraw[i][id] = v;
      const int y = t.ry0 + r;
      const bool row_in_tile = y >= t.y0 && y < t.y0 + kReplayTile;
      T2O_UNROLL
      for (int b = 0; b < 4; ++b) {
        const int col = 4 * d + b - m;                               // this byte's column, counted from the window's first
        if (col < 0 || col >= nb || !((v >> (8 * b)) & 0xffu)) continue;
        win = true;
        const int x = t.cx0 + col;
        tile = tile || (row_in_tile && x >= t.x0 && x < t.x0 + kReplayTile);
      }
    }
    if (win) lds.nz_win[i] = 1;                                       // every writer stores the same value
    if (tile) lds.nz_tile[i] = 1;
  }
}

// mask i at pixel (y, x) of the picture (inside the staged window), converted as the picture's bytes are
T2O_HD float replay_mask_fetch(const ReplayJob& j, const unsigned char* masks, const long long* mask_offsets, const ReplayTile& t,
                               const ReplayMaskLds& lds, int i, int y, int x) {
  const unsigned char* a = masks + mask_offsets[i] + (size_t)y * j.w + t.cx0;
  const unsigned char* b = reinterpret_cast<const unsigned char*>(lds.mraw[i]) + (y - t.ry0) * (kReplayMaskDw * 4) +
                           replay_misalign(a) + (x - t.cx0);
  return u8_to_unit((int)b[0]);
}

// x[i] = clamp01(blend(process(op, x[i], prow), x[i], m[i])): replay_apply with Operator.execute's mask operand
template <int NP>
T2O_HD void replay_apply_masked(int op, const float* prow, Rgb (&x)[NP], const float (&m)[NP]) {
  Curve cv;
  if (op == OP_COLOR || op == OP_TONE) curve_load(cv, prow, op == OP_COLOR);
  const float p0[1] = {prow[0]};
  switch (op) {
#define T2O_REPLAY_CASE(K)                                                                  \
  case K:                                                                                   \
    T2O_UNROLL                                                                              \
    for (int i = 0; i < NP; ++i) {                                                          \
      const Rgb r = pointwise_fwd(K, x[i], p0, cv);                                         \
      T2O_UNROLL                                                                            \
      for (int c = 0; c < 3; ++c) x[i].c[c] = clamp01(blend(r.c[c], x[i].c[c], m[i]));      \
    }                                                                                       \
    break;
    T2O_REPLAY_CASE(OP_BRIGHTNESS) T2O_REPLAY_CASE(OP_CONTRAST) T2O_REPLAY_CASE(OP_SATURATION)
    T2O_REPLAY_CASE(OP_COLOR) T2O_REPLAY_CASE(OP_TONE) T2O_REPLAY_CASE(OP_WHITE)
#undef T2O_REPLAY_CASE
    default: break;              // -1 (END): identity
  }
}

// ---------------------------------------------------------------- phase: pre (lists with a sharpness)
T2O_HD void replay_mask_phase_pre(const ReplayMaskJob& mj, const unsigned char* src, const float* params, const unsigned char* masks,
                                  const long long* mask_offsets, const ReplayTile& t, int tid, ReplayMaskLds& lds) {
  const ReplayJob& j = mj.j;
  Rgb x[kReplayPrePix];
  bool in[kReplayPrePix];
  T2O_UNROLL
  for (int i = 0; i < kReplayPrePix; ++i) {
    const int idx = tid + i * kReplayThreads, ry = idx / kReplayWin, rx = idx - ry * kReplayWin;
    const int y = t.y0 - 1 + ry, xx = t.x0 - 1 + rx;
    in[i] = idx < kReplayWin * kReplayWin && y >= 0 && y < j.h && xx >= 0 && xx < j.w;
    x[i].c[0] = x[i].c[1] = x[i].c[2] = 0.0f;
    if (in[i]) x[i] = replay_fetch(j, src, t, lds.base, y, xx);
  }
  for (int k = 0; k < j.sharp; ++k) {
    const int op = replay_op(j, k), mi = replay_mask_of(mj, k);
    if (op < 0) continue;
    const float* prow = params + k * kMaxParam;
    if (mi < 0) { replay_apply<kReplayPrePix>(op, prow, x); continue; }
    if (!replay_uniform(lds.nz_win[mi])) continue;                   // tile skip: the mask is 0 on tile + ring
    float m[kReplayPrePix];
    T2O_UNROLL
    for (int i = 0; i < kReplayPrePix; ++i) {
      const int idx = tid + i * kReplayThreads, ry = idx / kReplayWin, rx = idx - ry * kReplayWin;
      m[i] = in[i] ? replay_mask_fetch(j, masks, mask_offsets, t, lds, mi, t.y0 - 1 + ry, t.x0 - 1 + rx) : 0.0f;
    }
    replay_apply_masked<kReplayPrePix>(op, prow, x, m);
  }
  T2O_UNROLL
  for (int i = 0; i < kReplayPrePix; ++i) {
    const int idx = tid + i * kReplayThreads, ry = idx / kReplayWin, rx = idx - ry * kReplayWin;
    if (idx >= kReplayWin * kReplayWin) continue;
    T2O_UNROLL
    for (int c = 0; c < 3; ++c) lds.base.f[c][ry][rx] = in[i] ? x[i].c[c] : 0.0f;      // zero padding of the INTERMEDIATE image
  }
}

// ---------------------------------------------------------------- phase: main
T2O_HD void replay_mask_phase_main(const ReplayMaskJob& mj, const unsigned char* src, unsigned char* out, const float* params,
                                   const unsigned char* masks, const long long* mask_offsets, const ReplayTile& t, int tid,
                                   ReplayMaskLds& lds) {
  const ReplayJob& j = mj.j;
  Rgb x[kReplayPix];
  bool live[kReplayPix];
  float m[kReplayPix];
  const float p = j.sharp >= 0 ? params[j.sharp * kMaxParam] : 0.0f;
  const int ms = j.sharp >= 0 ? replay_mask_of(mj, j.sharp) : -1;
  // a masked sharpness whose mask is 0 on the tile leaves the centre pixel as it is: no stencil
  const bool stencil = j.sharp >= 0 && (ms < 0 || replay_uniform(lds.nz_tile[ms]));
  T2O_UNROLL
  for (int i = 0; i < kReplayPix; ++i) {
    const int idx = tid + i * kReplayThreads, iy = idx / kReplayTile, ix = idx - iy * kReplayTile;
    const int y = t.y0 + iy, xx = t.x0 + ix;
    live[i] = y < j.h && xx < j.w;
    x[i].c[0] = x[i].c[1] = x[i].c[2] = 0.0f;
    if (stencil) {
      m[i] = ms >= 0 && live[i] ? replay_mask_fetch(j, masks, mask_offsets, t, lds, ms, y, xx) : 0.0f;
      T2O_UNROLL
      for (int c = 0; c < 3; ++c) {
        const float ce = lds.base.f[c][iy + 1][ix + 1];
        float z = ce + p * sharp_delta(ce, lds.base.f[c][iy][ix + 1], lds.base.f[c][iy + 1][ix], lds.base.f[c][iy + 1][ix + 2],
                                       lds.base.f[c][iy + 2][ix + 1]);
        if (ms >= 0) z = blend(z, ce, m[i]);
        x[i].c[c] = clamp01(z);
      }
    } else if (j.sharp >= 0) {
      T2O_UNROLL
      for (int c = 0; c < 3; ++c) x[i].c[c] = lds.base.f[c][iy + 1][ix + 1];
    } else if (live[i]) {
      x[i] = replay_fetch(j, src, t, lds.base, y, xx);
    }
  }
  for (int k = j.sharp + 1; k < j.steps; ++k) {
    const int op = replay_op(j, k), mi = replay_mask_of(mj, k);
    if (op < 0 || op == OP_SHARPNESS) continue;
    const float* prow = params + k * kMaxParam;
    if (mi < 0) { replay_apply<kReplayPix>(op, prow, x); continue; }
    if (!replay_uniform(lds.nz_tile[mi])) continue;                  // tile skip: the mask is 0 on the tile
    T2O_UNROLL
    for (int i = 0; i < kReplayPix; ++i) {
      const int idx = tid + i * kReplayThreads, iy = idx / kReplayTile, ix = idx - iy * kReplayTile;
      m[i] = live[i] ? replay_mask_fetch(j, masks, mask_offsets, t, lds, mi, t.y0 + iy, t.x0 + ix) : 0.0f;
    }
    replay_apply_masked<kReplayPix>(op, prow, x, m);
  }
  unsigned char* ob = reinterpret_cast<unsigned char*>(lds.base.ob);
  T2O_UNROLL
  for (int i = 0; i < kReplayPix; ++i) {
    const int idx = tid + i * kReplayThreads, iy = idx / kReplayTile, ix = idx - iy * kReplayTile;
    if (!live[i]) continue;
    const unsigned char* a = out + j.out_offset + ((size_t)(t.y0 + iy) * j.w + t.x0) * 3;
    unsigned char* b = ob + iy * (kReplayOutDw * 4) + replay_misalign(a) + ix * 3;
    T2O_UNROLL
    for (int c = 0; c < 3; ++c) b[c] = unit_to_u8(x[i].c[c]);
  }
}

}  // namespace t2o
