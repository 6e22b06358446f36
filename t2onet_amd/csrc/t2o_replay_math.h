// The per-tile program of the 8-bit replay kernel (t2o_replay.hip): a known (operator, parameter) list applied to an
// (h,w,3) uint8 RGB picture, 8-bit in, 8-bit out -- Operator.execute with specified_param and no mask
// (models/operators.py:112-131) between the loaders' / 255 (utils/visual_utils.py:6-31) and the writers' * 255 truncated
// (utils/visual_utils.py:50-58).
//
// Like t2o_block_programs.h these are `__host__ __device__` phase functions -- what ONE thread of ONE workgroup does
// between two barriers -- so that tests/host_emul/emul_replay.cpp runs the same program thread by thread with g++ (a test
// harness, never a fallback).  All arithmetic is t2o_pixel_math.h's (pointwise_fwd, curve_load, sharp_delta, clamp01) and
// t2o_image_math.h's two conversions: the bytes are those of resize (same size) -> t2o_op_fwd per step -> f32_to_u8_hwc.
//
// A workgroup owns a kReplayTile^2 tile.  Phases:
//   load   the tile's source bytes (plus a 1-pixel ring when the list holds a sharpness), row by row, as ALIGNED dwords
//          into LDS: a row starts at any byte address, so each staged row keeps its address modulo 4 as a lead-in
//   pre    (sharpness lists only) tile + ring: bytes -> floats, the steps in front of the sharpness in registers, then
//          the intermediate image into an LDS float tile, ZERO outside the picture (the stencil pads what it is given)
//   main   the tile's pixels: the stencil from the float tile (or bytes -> floats), the remaining steps in registers,
//          floats -> bytes into an LDS row buffer laid out with the OUTPUT rows' address modulo 4
//   store  whole aligned dwords wherever all four bytes belong to this tile's row, single bytes at the two ends
// The aligned dword that holds a picture's first or last byte may reach up to 3 bytes outside the picture; it lies in
// the same 4-byte word of the same allocation as a valid byte, and those bytes are never used.  Stores never touch a
// byte outside the tile's own rows.
#pragma once
#ifndef __HIPCC_RTC__
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#endif

#include "t2o_image_math.h"
#include "t2o_pixel_math.h"

namespace t2o {

constexpr int kReplayTile = 32;                          // tile edge T
constexpr int kReplayThreads = 256;
constexpr int kReplayMaxSteps = 8, kReplayMaxJobs = 64;
constexpr int kReplayWin = kReplayTile + 2;              // tile + ring
constexpr int kReplayRawDw = (3 + 3 * kReplayWin + 3) / 4;    // 27 dwords per staged source row (lead-in + 34 pixels)
constexpr int kReplayOutDw = (3 + 3 * kReplayTile + 3) / 4;   // 25 dwords per staged output row
constexpr int kReplayFStride = kReplayWin + 1;           // floats per row of the intermediate tile
constexpr int kReplayPrePix = (kReplayWin * kReplayWin + kReplayThreads - 1) / kReplayThreads;    // 5 window pixels per thread
constexpr int kReplayPix = kReplayTile * kReplayTile / kReplayThreads;                           // 4 tile pixels per thread

// one job as the kernel sees it (t2o_replay_job_t after validation): 40 bytes, 64 of them fit the kernel arguments
struct ReplayJob {
  long long src_offset, out_offset;
  int h, w;
  int steps;
  int sharp;                     // index of the sharpness step among the applied ones, -1 = none
  unsigned long long ops;        // step k's operator as a signed byte at bits [8k, 8k+8): one register pair, no indexed array
};

T2O_HD int replay_op(const ReplayJob& j, int k) { return (int)(signed char)(unsigned char)(j.ops >> (8 * k)); }

// ---- host side: ONE job check for t2o_replay_u8, t2o_replay_u8_masked and t2o_replay_u8_stencils.  A refusal leaves
// "<entry point>: reason" in *why: a thread's buffer, good until its next refusal (t2o::set_error copies it). ----
static inline int replay_refuse(const char** why, int rc, const char* who, const char* reason) {
  static thread_local char text[160];
  snprintf(text, sizeof(text), "%s: %s", who, reason);
  *why = text;
  return rc;
}

// ReplayJob::sharp holds the index of the sharpness step (-1 = none) and a second one is refused, or their number R
enum ReplaySharp { kReplaySharpIndex, kReplaySharpCount };

// Check one job of the C ABI and bring it into the kernel's form: d, and mask_bits = ReplayMaskJob::mask_of (step k's mask
// index as a signed byte at bits [8k, 8k+8)).  mask_of: 8 ints, NULL = none.  Returns 0, 1 (T2O_EINVAL) or 2 (T2O_EUNSUPPORTED).
// Kept as they were: the kReplaySharpIndex entry points call a job's refusals "replay_u8" and look at every operator first.
static inline int replay_job_fill(ReplayJob& d, unsigned long long& mask_bits, const char* who, ReplaySharp mode, long long src_offset,
                                  long long out_offset, int h, int w, int steps, const int* ops, const int* mask_of, int n_masks,
                                  const char** why) {
  const char* job_who = mode == kReplaySharpIndex ? "replay_u8" : who;
  if (h <= 0 || w <= 0) return replay_refuse(why, 1, job_who, "h and w must be positive");
  if (src_offset < 0 || out_offset < 0) return replay_refuse(why, 1, job_who, "negative offset");
  if (steps < 0 || steps > kReplayMaxSteps) return replay_refuse(why, 1, job_who, "0 <= steps <= 8");
  d.src_offset = src_offset; d.out_offset = out_offset;
  d.h = h; d.w = w; d.steps = steps; d.sharp = mode == kReplaySharpIndex ? -1 : 0;
  d.ops = mask_bits = ~0ull;                       // every step the identity (-1) and without a mask until set
  bool bad_mask = false;
  for (int k = 0; k < steps; ++k) {
    const int op = ops[k];
    if (op == OP_INPAINT) return replay_refuse(why, 2, job_who, "operator 4 (inpaint) is not supported");
    if (op < OP_IDENTITY || op > OP_WHITE) return replay_refuse(why, 1, job_who, "operator index outside -1, 0..7");
    if (op == OP_SHARPNESS) {
      if (mode == kReplaySharpCount) ++d.sharp;
      else if (d.sharp >= 0) return replay_refuse(why, 2, job_who, "more than one sharpness in a job's list (the 1-pixel halo serves one)");
      else d.sharp = k;
    }
    d.ops = (d.ops & ~(0xffull << (8 * k))) | ((unsigned long long)(unsigned char)(signed char)op << (8 * k));
    const int i = mask_of ? mask_of[k] : -1;
    bad_mask = bad_mask || i < -1 || i >= n_masks;
    if (bad_mask && mode == kReplaySharpCount) break;      // (kReplaySharpIndex: reported behind the later steps' operators)
    mask_bits = (mask_bits & ~(0xffull << (8 * k))) | ((unsigned long long)(unsigned char)(signed char)i << (8 * k));
  }
  return bad_mask ? replay_refuse(why, 1, who, "a step's mask index lies outside the mask table") : 0;
}

// (the name the plain kernel's host emulation calls it by)
static inline int replay_job_make(ReplayJob& d, long long src_offset, long long out_offset, int h, int w, int steps,
                                  const int* ops, const char** why) {
  unsigned long long none;
  return replay_job_fill(d, none, "replay_u8", kReplaySharpIndex, src_offset, out_offset, h, w, steps, ops, nullptr, 0, why);
}

struct ReplayArgs {
  const unsigned char* src;
  unsigned char* out;
  const float* params;           // (J, 8, 24)
  ReplayJob jobs[kReplayMaxJobs];
};

struct ReplayLds {
  unsigned raw[kReplayWin * kReplayRawDw];               // source rows, each with its lead-in
  float f[3][kReplayWin][kReplayFStride];                // intermediate image in front of the sharpness
  unsigned ob[kReplayTile * kReplayOutDw];               // output rows, each with its lead-in
};

// the tile at (ty, tx) of a job: origin, and the part of tile + `ring` that lies inside the picture
struct ReplayTile {
  int y0, x0;
  int ry0, ry1, cx0, cx1;
};

T2O_HD int replay_tiles_x(const ReplayJob& j) { return (j.w + kReplayTile - 1) / kReplayTile; }
T2O_HD int replay_tiles(const ReplayJob& j) { return replay_tiles_x(j) * ((j.h + kReplayTile - 1) / kReplayTile); }

T2O_HD ReplayTile replay_tile(const ReplayJob& j, int tile) {
  const int tx = tile % replay_tiles_x(j), ty = tile / replay_tiles_x(j);
  const int ring = j.sharp >= 0 ? 1 : 0;
  ReplayTile t;
  t.y0 = ty * kReplayTile;
  t.x0 = tx * kReplayTile;
  t.ry0 = t.y0 - ring < 0 ? 0 : t.y0 - ring;
  t.cx0 = t.x0 - ring < 0 ? 0 : t.x0 - ring;
  t.ry1 = t.y0 + kReplayTile + ring > j.h ? j.h : t.y0 + kReplayTile + ring;
  t.cx1 = t.x0 + kReplayTile + ring > j.w ? j.w : t.x0 + kReplayTile + ring;
  return t;
}

T2O_HD unsigned replay_misalign(const unsigned char* p) { return (unsigned)((size_t)p & 3); }

// the aligned dword at `a`; [lo, hi) = the picture's bytes.  The host build reads only those (anything else: 0), which
// also shows that no outside byte is ever used.
T2O_HD unsigned replay_load_dword(const unsigned char* a, const unsigned char* lo, const unsigned char* hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)lo; (void)hi;
  return *reinterpret_cast<const unsigned*>(a);
#else
  unsigned v = 0;
  for (int b = 0; b < 4; ++b)
    if (a + b >= lo && a + b < hi) v |= (unsigned)a[b] << (8 * b);
  return v;
#endif
}

T2O_HD void replay_store_dword(unsigned char* a, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<unsigned*>(a) = v;
#else
  memcpy(a, &v, 4);
#endif
}

// ---------------------------------------------------------------- phase: load
T2O_HD void replay_phase_load(const ReplayJob& j, const unsigned char* src, const ReplayTile& t, int tid, ReplayLds& lds) {
  const unsigned char* img = src + j.src_offset;
  const unsigned char* end = img + (size_t)j.h * j.w * 3;
  const int rows = t.ry1 - t.ry0, nb = (t.cx1 - t.cx0) * 3;
  for (int id = tid; id < rows * kReplayRawDw; id += kReplayThreads) {
    const int r = id / kReplayRawDw, d = id - r * kReplayRawDw;
    const unsigned char* a = img + ((size_t)(t.ry0 + r) * j.w + t.cx0) * 3;
    const int m = (int)replay_misalign(a);
    if (4 * d < m + nb) lds.raw[id] = replay_load_dword(a - m + 4 * d, img, end);
  }
}

// pixel (y, x) of the picture (inside the staged region) from the staged bytes, as the loaders convert it
T2O_HD Rgb replay_fetch(const ReplayJob& j, const unsigned char* src, const ReplayTile& t, const ReplayLds& lds, int y, int x) {
  const unsigned char* a = src + j.src_offset + ((size_t)y * j.w + t.cx0) * 3;
  const unsigned char* b = reinterpret_cast<const unsigned char*>(lds.raw) + (y - t.ry0) * (kReplayRawDw * 4) +
                           replay_misalign(a) + (x - t.cx0) * 3;
  Rgb v;
  T2O_UNROLL
  for (int c = 0; c < 3; ++c) v.c[c] = u8_to_unit((int)b[c]);
  return v;
}

// x[i] = clamp01(process(op, x[i], prow)) for a thread's NP pixels: one specialised body per operator (wave-uniform
// switch), the curve loaded once per thread and step
template <int NP>
T2O_HD void replay_apply(int op, const float* prow, Rgb (&x)[NP]) {
  Curve cv;
  if (op == OP_COLOR || op == OP_TONE) curve_load(cv, prow, op == OP_COLOR);
  const float p0[1] = {prow[0]};
  switch (op) {
#define T2O_REPLAY_CASE(K)                                         \
  case K:                                                          \
    T2O_UNROLL                                                     \
    for (int i = 0; i < NP; ++i) {                                 \
      const Rgb r = pointwise_fwd(K, x[i], p0, cv);                \
      T2O_UNROLL                                                   \
      for (int c = 0; c < 3; ++c) x[i].c[c] = clamp01(r.c[c]);     \
    }                                                              \
    break;
    T2O_REPLAY_CASE(OP_BRIGHTNESS) T2O_REPLAY_CASE(OP_CONTRAST) T2O_REPLAY_CASE(OP_SATURATION)
    T2O_REPLAY_CASE(OP_COLOR) T2O_REPLAY_CASE(OP_TONE) T2O_REPLAY_CASE(OP_WHITE)
#undef T2O_REPLAY_CASE
    default: break;              // -1 (END): identity
  }
}

// steps [k0, k1) of the job's list, the sharpness excluded (the caller places it)
template <int NP>
T2O_HD void replay_steps(const ReplayJob& j, const float* params, int k0, int k1, Rgb (&x)[NP]) {
  for (int k = k0; k < k1; ++k) {
    const int op = replay_op(j, k);
    if (op >= 0 && op != OP_SHARPNESS) replay_apply<NP>(op, params + k * kMaxParam, x);
  }
}

// ---------------------------------------------------------------- phase: pre (lists with a sharpness)
// params = this job's (8, 24) rows
T2O_HD void replay_phase_pre(const ReplayJob& j, const unsigned char* src, const float* params, const ReplayTile& t, int tid,
                             ReplayLds& lds) {
  Rgb x[kReplayPrePix];
  bool in[kReplayPrePix];
  T2O_UNROLL
  for (int i = 0; i < kReplayPrePix; ++i) {
    const int idx = tid + i * kReplayThreads, ry = idx / kReplayWin, rx = idx - ry * kReplayWin;
    const int y = t.y0 - 1 + ry, xx = t.x0 - 1 + rx;
    in[i] = idx < kReplayWin * kReplayWin && y >= 0 && y < j.h && xx >= 0 && xx < j.w;
    x[i].c[0] = x[i].c[1] = x[i].c[2] = 0.0f;
    if (in[i]) x[i] = replay_fetch(j, src, t, lds, y, xx);
  }
  replay_steps<kReplayPrePix>(j, params, 0, j.sharp, x);
  T2O_UNROLL
  for (int i = 0; i < kReplayPrePix; ++i) {
    const int idx = tid + i * kReplayThreads, ry = idx / kReplayWin, rx = idx - ry * kReplayWin;
    if (idx >= kReplayWin * kReplayWin) continue;
    T2O_UNROLL
    for (int c = 0; c < 3; ++c) lds.f[c][ry][rx] = in[i] ? x[i].c[c] : 0.0f;      // zero padding of the INTERMEDIATE image
  }
}

// ---------------------------------------------------------------- phase: main
T2O_HD void replay_phase_main(const ReplayJob& j, const unsigned char* src, unsigned char* out, const float* params,
                              const ReplayTile& t, int tid, ReplayLds& lds) {
  Rgb x[kReplayPix];
  bool live[kReplayPix];
  const float p = j.sharp >= 0 ? params[j.sharp * kMaxParam] : 0.0f;
  T2O_UNROLL
  for (int i = 0; i < kReplayPix; ++i) {
    const int idx = tid + i * kReplayThreads, iy = idx / kReplayTile, ix = idx - iy * kReplayTile;
    const int y = t.y0 + iy, xx = t.x0 + ix;
    live[i] = y < j.h && xx < j.w;
    x[i].c[0] = x[i].c[1] = x[i].c[2] = 0.0f;
    if (j.sharp >= 0) {
      T2O_UNROLL
      for (int c = 0; c < 3; ++c) {
        const float ce = lds.f[c][iy + 1][ix + 1];
        x[i].c[c] = clamp01(ce + p * sharp_delta(ce, lds.f[c][iy][ix + 1], lds.f[c][iy + 1][ix], lds.f[c][iy + 1][ix + 2],
                                                 lds.f[c][iy + 2][ix + 1]));
      }
    } else if (live[i]) {
      x[i] = replay_fetch(j, src, t, lds, y, xx);
    }
  }
  replay_steps<kReplayPix>(j, params, j.sharp + 1, j.steps, x);
  unsigned char* ob = reinterpret_cast<unsigned char*>(lds.ob);
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

// ---------------------------------------------------------------- phase: store
T2O_HD void replay_phase_store(const ReplayJob& j, unsigned char* out, const ReplayTile& t, int tid, const ReplayLds& lds) {
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
