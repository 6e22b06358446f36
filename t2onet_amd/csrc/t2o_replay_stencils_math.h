// The per-tile program of the 8-bit replay kernel for lists with ANY number of sharpness steps (t2o_replay_stencils.hip):
// t2o_replay_mask_math.h's semantics -- per step x = clamp01(blend(process(op, x, p), x, m / 255)) where the step names a
// mask, clamp01(process(op, x, p)) where it names none, bytes -> floats by / 255 and back by * 255 truncated -- with every
// sharpness reading the four neighbours of the image in front of it, that INTERMEDIATE image counting as zero outside the
// picture.  The bytes are those of resize (same size) -> t2o_op_fwd per step -> f32_to_u8_hwc: the same device functions
// (pointwise_fwd, curve_load, sharp_delta, blend, clamp01, u8_to_unit, unit_to_u8) in the same order.
//
// Taken from t2o_replay_math.h / t2o_replay_mask_math.h as they are: the job form (ReplayMaskJob; ReplayJob::sharp holds
// R, the NUMBER of sharpness steps the job applies, instead of an index), replay_op / replay_mask_of / replay_masks_used,
// the tile count, replay_misalign, replay_load_dword / replay_store_dword with their aligned-dword rule, replay_apply and
// replay_apply_masked, replay_uniform, and the argument struct ReplayMaskArgs.  The staging phases are restated here
// because the window is wider (their LDS structs fix a 34-pixel window); the store is the same dword / byte split.
//
// A workgroup owns a 32 x 32 tile.  Its WINDOW is the tile plus an R-pixel ring, (32 + 2R)^2 <= 48 x 48 pixels, sized at
// run time by the job's own R.  A REGION of edge E is the window shrunk by (W - E) / 2 on every side; a thread computes
// the pixels tid, tid + 256, ... of a region, NP = 4, 5, 6 or 9 of them (E <= 32, <= 34, <= 38, <= 46).  Phases, a barrier between:
//   load      the window's source rows (the part inside the picture) as ALIGNED dwords into LDS, each row with its
//             address modulo 4 as a lead-in; the mask flags are cleared
//   mask      every distinct mask the list names, staged the same way, 1 byte per pixel; flag i is raised when a byte of
//             the staged window of mask i is not 0
//   first     region = window: bytes -> floats, the steps in front of the first sharpness in registers; in chunks of
//             4, 2 or 1 pixels per thread, each followed by its own `put` (or `out`): nothing is held across a barrier
//   put       the held values of a region into the float tile, ZERO wherever the region leaves the picture: the padding
//             of the intermediate image, which is not process(0) (white turns 0 into 1, brightness can lift it)
//   stencil   sharpness number n, region E = W - 2 (n + 1): the stencil from the float tile, blended with the stencil's
//             input at the centre where the step names a mask, then the steps up to the next sharpness in registers.
//             Its reads stay inside the region the last `put` wrote.  The tile is updated IN PLACE: the results are held
//             in registers across a barrier, then `put`.
//   out       region = tile (after the last sharpness, or `first` when R = 0): floats -> bytes into an LDS row buffer
//             laid out with the OUTPUT rows' address modulo 4
//   store     whole aligned dwords wherever all four bytes belong to this tile's row, single bytes at the two ends
// What is still correct shrinks by one pixel per sharpness and ends at the tile: after n sharpness steps the values of
// region W - 2n equal the whole-image chain's, because each one's neighbours lay in region W - 2n + 2, and positions
// outside the picture were forced to 0 by `put` before any stencil read them.
// TILE SKIP, conservative form: a step whose mask is all zero over the WHOLE staged window is not run (for a sharpness:
// the centre value is kept).  blend(o, x, 0) = o * 0 + x * 1 = x for finite o and x in [0, 1] stays under clamp01, so the
// bytes do not change.  The flag is the same for every thread: a wave-uniform branch.
#pragma once
#include "t2o_replay_mask_math.h"

namespace t2o {

constexpr int kStMaxRing = kReplayMaxSteps;                       // every step a sharpness
constexpr int kStSmallRing = 2;                                   // what the smaller of the two kernels serves

// LDS of a workgroup whose jobs apply at most RMAX sharpness steps: window edge 32 + 2 RMAX
//   RMAX = 8: float tile 28 224 B, source rows 7 104 B, four mask windows 9 984 B, output rows 3 200 B: 48 528 B
//   RMAX = 2: float tile 15 984 B, source rows 4 032 B, four mask windows 5 760 B, output rows 3 200 B: 28 992 B
template <int RMAX>
struct ReplayStLdsT {
  static constexpr int kRing = RMAX;
  static constexpr int kWin = kReplayTile + 2 * RMAX;
  static constexpr int kRawDw = (3 + 3 * kWin + 3) / 4;           // dwords per staged source row (lead-in + kWin pixels)
  static constexpr int kMaskDw = (3 + kWin + 3) / 4;              // dwords per staged mask row
  float f[3][kWin][kWin + 1];                                     // the intermediate image, updated in place
  unsigned raw[kWin * kRawDw];                                    // source rows, each with its lead-in
  unsigned mraw[kReplayMaxMasks][kWin * kMaskDw];                 // mask rows, each with its lead-in
  unsigned ob[kReplayTile * kReplayOutDw];                        // output rows, each with its lead-in
  int nz[kReplayMaxMasks];                                        // a byte of mask i's staged window is not 0
};
using ReplayStLds = ReplayStLdsT<kStMaxRing>;
using ReplayStLdsSmall = ReplayStLdsT<kStSmallRing>;

// pixels per thread of a stencil segment on a region of edge E: all of a thread's pixels are held across a barrier
T2O_HD int replay_st_np(int E) { return E <= kReplayTile ? 4 : E <= 34 ? 5 : E <= 38 ? 6 : 9; }

// `first` holds nothing across a barrier (its `put` or `out` follows in the same thread), so it runs in CHUNKS of few
// pixels per thread, which bounds its registers: pixels per thread of the next chunk when `remaining` pixels of the
// region are left (4, 2 or 1; 256 threads).  A chunk starts at pixel index `base`: thread tid stands for tid + base.
T2O_HD int replay_st_first_np(int remaining) { return remaining > 3 * kReplayThreads ? 4 : remaining > kReplayThreads ? 2 : 1; }

// the first sharpness at or behind step k, or steps
T2O_HD int replay_st_next_sharp(const ReplayJob& j, int k) {
  while (k < j.steps && replay_op(j, k) != OP_SHARPNESS) ++k;
  return k;
}

// Host side: replay_job_fill counting the sharpness steps, d.j.sharp = R (the host emulation's name); mask_of may be NULL
static inline int replay_st_job_make(ReplayMaskJob& d, long long src_offset, long long out_offset, int h, int w, int steps,
                                     const int* ops, const int* mask_of, int n_masks, const char** why) {
  return replay_job_fill(d.j, d.mask_of, "replay_u8_stencils", kReplaySharpCount, src_offset, out_offset, h, w, steps, ops, mask_of, n_masks, why);
}

// the tile's origin and the part of the window (tile + R) that lies inside the picture
T2O_HD ReplayTile replay_st_tile(const ReplayJob& j, int tile) {
  const int tx = tile % replay_tiles_x(j), ty = tile / replay_tiles_x(j), R = j.sharp;
  ReplayTile t;
  t.y0 = ty * kReplayTile;
  t.x0 = tx * kReplayTile;
  t.ry0 = t.y0 - R < 0 ? 0 : t.y0 - R;
  t.cx0 = t.x0 - R < 0 ? 0 : t.x0 - R;
  t.ry1 = t.y0 + kReplayTile + R > j.h ? j.h : t.y0 + kReplayTile + R;
  t.cx1 = t.x0 + kReplayTile + R > j.w ? j.w : t.x0 + kReplayTile + R;
  return t;
}

// pixel i of thread tid in the region of edge E: window coordinates (wy, wx), picture coordinates (y, x)
struct ReplayStPos {
  int wy, wx, y, x;
  bool in;                       // belongs to the region and lies inside the picture
  bool any;                      // belongs to the region
};

T2O_HD ReplayStPos replay_st_pos(const ReplayJob& j, const ReplayTile& t, int E, int tid, int i) {
  const int R = j.sharp, off = (kReplayTile + 2 * R - E) / 2;
  const int idx = tid + i * kReplayThreads, ry = idx / E, rx = idx - ry * E;
  ReplayStPos p;
  p.wy = off + ry; p.wx = off + rx;
  p.y = t.y0 - R + p.wy; p.x = t.x0 - R + p.wx;
  p.any = idx < E * E;
  p.in = p.any && p.y >= 0 && p.y < j.h && p.x >= 0 && p.x < j.w;
  return p;
}

// ---------------------------------------------------------------- phase: load
template <class L>
T2O_HD void replay_st_phase_load(const ReplayJob& j, const unsigned char* src, const ReplayTile& t, int tid, L& lds) {
  const unsigned char* img = src + j.src_offset;
  const unsigned char* end = img + (size_t)j.h * j.w * 3;
  const int rows = t.ry1 - t.ry0, nb = (t.cx1 - t.cx0) * 3;
  for (int id = tid; id < rows * L::kRawDw; id += kReplayThreads) {
    const int r = id / L::kRawDw, d = id - r * L::kRawDw;
    const unsigned char* a = img + ((size_t)(t.ry0 + r) * j.w + t.cx0) * 3;
    const int m = (int)replay_misalign(a);
    if (4 * d < m + nb) lds.raw[id] = replay_load_dword(a - m + 4 * d, img, end);
  }
  if (tid < kReplayMaxMasks) lds.nz[tid] = 0;
}

// ---------------------------------------------------------------- phase: mask load
template <class L>
T2O_HD void replay_st_phase_mask_load(const ReplayMaskJob& mj, const unsigned char* masks, const long long* mask_offsets,
                                      const ReplayTile& t, int tid, L& lds) {
  const ReplayJob& j = mj.j;
  const unsigned used = replay_masks_used(mj);
  const int rows = t.ry1 - t.ry0, nb = t.cx1 - t.cx0;
  for (int i = 0; i < kReplayMaxMasks; ++i) {
    if (!(used >> i & 1)) continue;
    const unsigned char* plane = masks + mask_offsets[i];
    const unsigned char* end = plane + (size_t)j.h * j.w;
    bool win = false;
    for (int id = tid; id < rows * L::kMaskDw; id += kReplayThreads) {
      const int r = id / L::kMaskDw, d = id - r * L::kMaskDw;
      const unsigned char* a = plane + (size_t)(t.ry0 + r) * j.w + t.cx0;
      const int m = (int)replay_misalign(a);
      if (4 * d >= m + nb) continue;
      const unsigned v = replay_load_dword(a - m + 4 * d, plane, end);
      lds.mraw[i][id] = v;
      T2O_UNROLL
      for (int b = 0; b < 4; ++b) {
        const int col = 4 * d + b - m;                               // this byte's column, counted from the window's first
        win = win || (col >= 0 && col < nb && ((v >> (8 * b)) & 0xffu));
      }
    }
    if (win) lds.nz[i] = 1;                                           // every writer stores the same value
  }
}

// pixel (y, x) of the picture (inside the staged window) from the staged bytes, as the loaders convert it
template <class L>
T2O_HD Rgb replay_st_fetch(const ReplayJob& j, const unsigned char* src, const ReplayTile& t, const L& lds, int y, int x) {
  const unsigned char* a = src + j.src_offset + ((size_t)y * j.w + t.cx0) * 3;
  const unsigned char* b = reinterpret_cast<const unsigned char*>(lds.raw) + (y - t.ry0) * (L::kRawDw * 4) +
                           replay_misalign(a) + (x - t.cx0) * 3;
  Rgb v;
  T2O_UNROLL
  for (int c = 0; c < 3; ++c) v.c[c] = u8_to_unit((int)b[c]);
  return v;
}

// mask i at pixel (y, x) of the picture (inside the staged window), converted as the picture's bytes are
template <class L>
T2O_HD float replay_st_mask_fetch(const ReplayJob& j, const unsigned char* masks, const long long* mask_offsets, const ReplayTile& t,
                                  const L& lds, int i, int y, int x) {
  const unsigned char* a = masks + mask_offsets[i] + (size_t)y * j.w + t.cx0;
  const unsigned char* b = reinterpret_cast<const unsigned char*>(lds.mraw[i]) + (y - t.ry0) * (L::kMaskDw * 4) +
                           replay_misalign(a) + (x - t.cx0);
  return u8_to_unit((int)b[0]);
}

// steps [k0, k1) of the list on a region's pixels in registers; no sharpness among them
template <int NP, class L>
T2O_HD void replay_st_steps(const ReplayMaskJob& mj, const float* params, const unsigned char* masks, const long long* mask_offsets,
                            const ReplayTile& t, int E, int tid, const L& lds, int k0, int k1, Rgb (&x)[NP]) {
  const ReplayJob& j = mj.j;
  for (int k = k0; k < k1; ++k) {
    const int op = replay_op(j, k), mi = replay_mask_of(mj, k);
    if (op < 0 || op == OP_SHARPNESS) continue;
    const float* prow = params + k * kMaxParam;
    if (mi < 0) { replay_apply<NP>(op, prow, x); continue; }
    if (!replay_uniform(lds.nz[mi])) continue;                       // tile skip: the mask is 0 on the whole window
    float m[NP];
    T2O_UNROLL
    for (int i = 0; i < NP; ++i) {
      const ReplayStPos p = replay_st_pos(j, t, E, tid, i);
      m[i] = p.in ? replay_st_mask_fetch(j, masks, mask_offsets, t, lds, mi, p.y, p.x) : 0.0f;
    }
    replay_apply_masked<NP>(op, prow, x, m);
  }
}

// ---------------------------------------------------------------- phase: first (region = window, E = 32 + 2R)
// params = this job's (8, 24) rows; hold = the thread's NP pixels, kept in registers for `put` or `out`
template <int NP, class L>
T2O_HD void replay_st_phase_first(const ReplayMaskJob& mj, const unsigned char* src, const float* params, const unsigned char* masks,
                                  const long long* mask_offsets, const ReplayTile& t, int E, int tid, const L& lds,
                                  Rgb (&hold)[NP]) {
  const ReplayJob& j = mj.j;
  T2O_UNROLL
  for (int i = 0; i < NP; ++i) {
    const ReplayStPos p = replay_st_pos(j, t, E, tid, i);
    hold[i].c[0] = hold[i].c[1] = hold[i].c[2] = 0.0f;
    if (p.in) hold[i] = replay_st_fetch(j, src, t, lds, p.y, p.x);
  }
  replay_st_steps<NP>(mj, params, masks, mask_offsets, t, E, tid, lds, 0, replay_st_next_sharp(j, 0), hold);
}

// ---------------------------------------------------------------- phase: put
template <int NP, class L>
T2O_HD void replay_st_phase_put(const ReplayJob& j, const ReplayTile& t, int E, int tid, L& lds, const Rgb (&hold)[NP]) {
  T2O_UNROLL
  for (int i = 0; i < NP; ++i) {
    const ReplayStPos p = replay_st_pos(j, t, E, tid, i);
    if (!p.any) continue;
    T2O_UNROLL
    for (int c = 0; c < 3; ++c) lds.f[c][p.wy][p.wx] = p.in ? hold[i].c[c] : 0.0f;      // zero padding of the INTERMEDIATE image
  }
}

// ---------------------------------------------------------------- phase: stencil (the sharpness at step s, region E)
template <int NP, class L>
T2O_HD void replay_st_phase_stencil(const ReplayMaskJob& mj, const float* params, const unsigned char* masks,
                                    const long long* mask_offsets, const ReplayTile& t, int E, int s, int tid, const L& lds,
                                    Rgb (&hold)[NP]) {
  const ReplayJob& j = mj.j;
  const float p = params[s * kMaxParam];
  const int ms = replay_mask_of(mj, s);
  // a masked sharpness whose mask is 0 on the whole window leaves the centre pixel as it is: no stencil
  const bool stencil = ms < 0 || replay_uniform(lds.nz[ms]);
  T2O_UNROLL
  for (int i = 0; i < NP; ++i) {
    const ReplayStPos q = replay_st_pos(j, t, E, tid, i);
    hold[i].c[0] = hold[i].c[1] = hold[i].c[2] = 0.0f;
    if (!q.any) continue;                                            // the neighbours of the others lie in the last region
    const float m = ms >= 0 && stencil && q.in ? replay_st_mask_fetch(j, masks, mask_offsets, t, lds, ms, q.y, q.x) : 0.0f;
    T2O_UNROLL
    for (int c = 0; c < 3; ++c) {
      const float ce = lds.f[c][q.wy][q.wx];
      if (stencil) {
        float z = ce + p * sharp_delta(ce, lds.f[c][q.wy - 1][q.wx], lds.f[c][q.wy][q.wx - 1], lds.f[c][q.wy][q.wx + 1],
                                       lds.f[c][q.wy + 1][q.wx]);
        if (ms >= 0) z = blend(z, ce, m);
        hold[i].c[c] = clamp01(z);
      } else {
        hold[i].c[c] = ce;
      }
    }
  }
  replay_st_steps<NP>(mj, params, masks, mask_offsets, t, E, tid, lds, s + 1, replay_st_next_sharp(j, s + 1), hold);
}

// ---------------------------------------------------------------- phase: out (region = tile, 4 pixels per thread)
template <class L>
T2O_HD void replay_st_phase_out(const ReplayJob& j, unsigned char* out, const ReplayTile& t, int tid, L& lds,
                                const Rgb (&hold)[kReplayPix]) {
  unsigned char* ob = reinterpret_cast<unsigned char*>(lds.ob);
  T2O_UNROLL
  for (int i = 0; i < kReplayPix; ++i) {
    const int idx = tid + i * kReplayThreads, iy = idx / kReplayTile, ix = idx - iy * kReplayTile;
    if (t.y0 + iy >= j.h || t.x0 + ix >= j.w) continue;
    const unsigned char* a = out + j.out_offset + ((size_t)(t.y0 + iy) * j.w + t.x0) * 3;
    unsigned char* b = ob + iy * (kReplayOutDw * 4) + replay_misalign(a) + ix * 3;
    T2O_UNROLL
    for (int c = 0; c < 3; ++c) b[c] = unit_to_u8(hold[i].c[c]);
  }
}

// ---------------------------------------------------------------- phase: store (replay_phase_store on this LDS struct)
template <class L>
T2O_HD void replay_st_phase_store(const ReplayJob& j, unsigned char* out, const ReplayTile& t, int tid, const L& lds) {
  const int rows = j.h - t.y0 < kReplayTile ? j.h - t.y0 : kReplayTile;
  const int cols = j.w - t.x0 < kReplayTile ? j.w - t.x0 : kReplayTile;
  const int nb = cols * 3;
  for (int id = tid; id < rows * kReplayOutDw; id += kReplayThreads) {
    const int r = id / kReplayOutDw, d = id - r * kReplayOutDw;
    unsigned char* a = out + j.out_offset + ((size_t)(t.y0 + r) * j.w + t.x0) * 3;
    const int lo = 4 * d - (int)replay_misalign(a);          // this dword's first byte, counted from the row's first
    if (lo + 4 <= 0 || lo >= nb) continue;
    const unsigned v = lds.ob[id];
    if (lo >= 0 && lo + 4 <= nb) {
      replay_store_dword(a + lo, v);
    } else {
      for (int b = 0; b < 4; ++b)
        if (lo + b >= 0 && lo + b < nb) a[lo + b] = (unsigned char)(v >> (8 * b));
    }
  }
}

}  // namespace t2o
