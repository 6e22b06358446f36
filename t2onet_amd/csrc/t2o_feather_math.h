// The tile programs of the mask FEATHER kernels (t2o_feather.hip): a uint8 plane m (h, w) blurred by a separable Gaussian
// of standard deviation sigma in INTEGER arithmetic with replicated borders -- the soft edge a local edit wants from a
// hard 0/255 mask.  The arithmetic (include/t2onet_hip.h states it in full):
//   weights  w_0 .. w_R, uint16, w_0 + 2 * sum_{i>=1} w_i = 65536 exactly (feather_weights below, host only)
//   row      a = sum_{i=-R..R} w_|i| * m[y, clamp(x+i, 0, w-1)] <= 255 * 65536;   t = (a + 128) >> 8 <= 65280, uint16
//   column   b = sum_{i=-R..R} w_|i| * t[clamp(y+i, 0, h-1), x] <= 65280 * 65536; out = (b + 2^23) >> 24
// Every sum fits unsigned 32 bits; no float runs on the device.  R = 0 (sigma <= ~0.2) is w_0 = 65536, a plain copy: the
// same program with one tap (65536 does not fit the uint16 table, which holds 0 there; the staged taps are 32-bit).
//
// Like t2o_replay_math.h these are `__host__ __device__` phase functions -- what ONE thread of ONE workgroup does between
// two barriers -- so that tests/host_emul/emul_feather.cpp runs the same programs thread by thread with g++ (a test
// harness, never a fallback).  Two launches, each covering every job of the call:
//   ROW pass     a workgroup owns kFeatherRowW x kFeatherRowH pixels.  `stage`: the 2R+1 taps, zero-padded to a multiple
//                of 4, as dwords; each tile row's bytes from column x0 - R on, CLAMPED to the row, as dwords whose first
//                byte is column x0 - R + 4d whatever the row's byte address -- inside the row two ALIGNED global dwords
//                are funnel-shifted by the address modulo 4, at the row's ends single clamped bytes.  `main`: a thread
//                makes 4 adjacent outputs: per chunk of 4 taps one staged dword joins the previous one, 7 bytes feed
//                16 multiply-adds.  The uint16 intermediate goes to the workspace (row pitch a multiple of 4) as one
//                aligned 8-byte store.
//   COLUMN pass  a workgroup owns kFeatherColW x kFeatherColH pixels, lane = x.  `stage`: the taps, and the tile's rows
//                y0 - R .. clamped to the plane from the workspace as aligned dwords (two uint16).  `main`: a thread
//                makes kFeatherColP vertically adjacent outputs from a register window: per chunk of 4 taps 4 new rows
//                feed 4 * kFeatherColP multiply-adds; bytes go to an LDS row buffer laid out with the DESTINATION rows'
//                address modulo 4.  `store`: whole aligned dwords where all four bytes belong to the tile's row, single
//                bytes at its two ends: no byte outside the plane is written.
// Every source byte is read by the first launch before the second writes any destination byte: a job may run in place,
// and a source may overlap any destination.
#pragma once
#ifndef __HIPCC_RTC__
#include <math.h>
#endif

#include "t2o_replay_math.h"

namespace t2o {

constexpr int kFeatherMaxJobs = 4;                       // = kReplayMaxMasks: the planes of one local edit
constexpr int kFeatherMaxRadius = 192;                   // ceil(3 * 64)
constexpr double kFeatherMaxSigma = 64.0;
constexpr int kFeatherThreads = 256;
constexpr int kFeatherMaxTaps = (2 * kFeatherMaxRadius + 1 + 3) / 4 * 4;      // 388: 385 taps padded to whole chunks
constexpr int kFeatherWStride = kFeatherMaxRadius + 4;   // uint16 per job in the kernel arguments (193, 8-byte multiple)

constexpr int kFeatherRowW = 256, kFeatherRowH = 8;      // row pass tile; 64 threads x 4 outputs span it, 4 rows at a time
constexpr int kFeatherRowPix = 4;
constexpr int kFeatherRowDw = (kFeatherRowW + kFeatherMaxTaps) / 4;           // 161 staged dwords per tile row
constexpr int kFeatherColW = 64, kFeatherColH = 64;      // column pass tile; lane = x, a wave owns 16 rows
constexpr int kFeatherColPix = 8;
constexpr int kFeatherOutDw = (3 + kFeatherColW + 3) / 4;                     // 17 staged dwords per output row (lead-in + 64)

static_assert(kFeatherRowW == 64 * kFeatherRowPix && kFeatherRowH % (kFeatherThreads / 64) == 0, "row pass thread map");
static_assert(kFeatherColW == 64 && kFeatherColH % (kFeatherThreads / 64 * kFeatherColPix) == 0, "column pass thread map");

// Host side: the weights of `sigma` by the tail-sum rule (every |w_i - 65536 g_i / G| <= 1, the sum exact).  w: 193
// uint16; *radius = R after trimming trailing zeros.  R = 0 is the copy: w[0] then holds 65536 modulo 2^16 = 0.
// Returns 0, or 1 for a sigma that is negative, NaN or above 64.
static inline int feather_weights(double sigma, unsigned short* w, int* radius) {
  if (!(sigma >= 0.0) || sigma > kFeatherMaxSigma) return 1;
  for (int i = 0; i <= kFeatherMaxRadius; ++i) w[i] = 0;
  *radius = 0;
  if (sigma == 0.0) return 0;
  int r0 = (int)ceil(3.0 * sigma);
  if (r0 > kFeatherMaxRadius) r0 = kFeatherMaxRadius;
  double g[kFeatherMaxRadius + 1], G = 0.0;
  for (int i = 0; i <= r0; ++i) g[i] = exp(-(double)i * i / (2.0 * sigma * sigma));
  for (int i = r0; i >= 1; --i) G += g[i];
  G = g[0] + 2.0 * G;
  double tail = 0.0, below = 0.0;                        // T_i and rint(T_{i+1})
  int r = 0;
  for (int i = r0; i >= 1; --i) {
    tail += 65536.0 * g[i] / G;
    const double here = rint(tail);
    w[i] = (unsigned short)(int)(here - below);
    if (w[i] && !r) r = i;
    below = here;
  }
  w[0] = (unsigned short)(65536 - 2 * (int)below);       // r = 0: below = 0 and the value wraps to 0
  *radius = r;
  return 0;
}

// one job as the kernels see it
struct FeatherJob {
  long long src_offset, out_offset;
  long long ws_offset;           // first uint16 of the job's intermediate, counted from the workspace
  int h, w;
  int radius;
  int pitch;                     // uint16 per intermediate row: w rounded up to a multiple of 4
};

struct FeatherArgs {
  const unsigned char* src;
  unsigned char* out;
  unsigned short* ws;
  FeatherJob jobs[kFeatherMaxJobs];
  unsigned short w[kFeatherMaxJobs][kFeatherWStride];
};

T2O_HD int feather_pitch(int w) { return (w + 3) / 4 * 4; }
T2O_HD int feather_taps(int radius) { return (2 * radius + 1 + 3) / 4 * 4; }          // taps padded to whole chunks
T2O_HD int feather_row_tiles_x(const FeatherJob& j) { return (j.w + kFeatherRowW - 1) / kFeatherRowW; }
T2O_HD int feather_row_tiles(const FeatherJob& j) { return feather_row_tiles_x(j) * ((j.h + kFeatherRowH - 1) / kFeatherRowH); }
T2O_HD int feather_col_tiles_x(const FeatherJob& j) { return (j.w + kFeatherColW - 1) / kFeatherColW; }
T2O_HD int feather_col_tiles(const FeatherJob& j) { return feather_col_tiles_x(j) * ((j.h + kFeatherColH - 1) / kFeatherColH); }

// LDS of the column pass for a launch whose largest radius is `radius`: taps, (tile + apron) rows of uint16, output rows
T2O_HD int feather_col_rows(int radius) { return kFeatherColH + feather_taps(radius); }
T2O_HD size_t feather_col_lds_bytes(int radius) {
  return (size_t)kFeatherMaxTaps * 4 + (size_t)feather_col_rows(radius) * kFeatherColW * 2 + (size_t)kFeatherColH * kFeatherOutDw * 4;
}

struct FeatherRowLds {
  alignas(16) unsigned taps[kFeatherMaxTaps];            // a chunk's four taps: one 16-byte read, the same address in every lane
  unsigned raw[kFeatherRowH * kFeatherRowDw];
};

// acc + tap * v for tap < 2^17 and v < 2^16: one full-rate 24-bit multiply-add, the low 32 bits of the product
T2O_HD unsigned feather_mad(unsigned acc, unsigned tap, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return acc + __umul24(tap, v);
#else
  return acc + tap * v;
#endif
}

// bytes [s, s+4) of the 8 bytes lo, hi
T2O_HD unsigned feather_funnel(unsigned lo, unsigned hi, int s) {
  return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * s));
}

// taps[j] = w_|j - R| for j <= 2R, 0 up to the next multiple of 4 (R = 0: the single tap 65536)
T2O_HD void feather_stage_taps(const unsigned short* w, int radius, int tid, unsigned* taps) {
  for (int j = tid; j < feather_taps(radius); j += kFeatherThreads) {
    const int i = j < radius ? radius - j : j - radius;
    taps[j] = j > 2 * radius ? 0u : radius == 0 ? 65536u : (unsigned)w[i];
  }
}

// ---------------------------------------------------------------- ROW pass, phase: stage
T2O_HD void feather_row_stage(const FeatherJob& j, const unsigned short* w, const unsigned char* src, int tile, int tid,
                              FeatherRowLds& lds) {
  feather_stage_taps(w, j.radius, tid, lds.taps);
  const int tx = tile % feather_row_tiles_x(j), ty = tile / feather_row_tiles_x(j);
  const int x0 = tx * kFeatherRowW, y0 = ty * kFeatherRowH;
  const int rows = j.h - y0 < kFeatherRowH ? j.h - y0 : kFeatherRowH;
  const int cols = j.w - x0 < kFeatherRowW ? (j.w - x0 + 3) / 4 * 4 : kFeatherRowW;
  const int nd = (cols + feather_taps(j.radius)) / 4;    // dwords of a row that main reads
  const unsigned char* plane = src + j.src_offset;
  const unsigned char* end = plane + (size_t)j.h * j.w;
  for (int id = tid; id < rows * nd; id += kFeatherThreads) {
    const int r = id / nd, d = id - r * nd;
    const unsigned char* row = plane + (size_t)(y0 + r) * j.w;
    const int c = x0 - j.radius + 4 * d;                  // column of this dword's first byte
    unsigned v;
    if (c >= 0 && c + 4 <= j.w) {
      const unsigned char* a = row + c;
      const int m = (int)replay_misalign(a);
      v = replay_load_dword(a - m, plane, end);
      if (m) v = feather_funnel(v, replay_load_dword(a - m + 4, plane, end), m);
    } else {
      v = 0;
      T2O_UNROLL
      for (int b = 0; b < 4; ++b) {
        const int cc = c + b < 0 ? 0 : c + b >= j.w ? j.w - 1 : c + b;
        v |= (unsigned)row[cc] << (8 * b);
      }
    }
    lds.raw[r * kFeatherRowDw + d] = v;
  }
}

// ---------------------------------------------------------------- ROW pass, phase: main
T2O_HD void feather_row_main(const FeatherJob& j, unsigned short* ws, int tile, int tid, const FeatherRowLds& lds) {
  const int tx = tile % feather_row_tiles_x(j), ty = tile / feather_row_tiles_x(j);
  const int cg = tid & 63, x = tx * kFeatherRowW + kFeatherRowPix * cg;
  if (x >= j.w) return;
  const int chunks = feather_taps(j.radius) / 4;
  for (int r = tid >> 6; r < kFeatherRowH; r += kFeatherThreads / 64) {
    const int y = ty * kFeatherRowH + r;
    if (y >= j.h) break;
    const unsigned* raw = lds.raw + r * kFeatherRowDw + cg;
    unsigned acc[kFeatherRowPix] = {0, 0, 0, 0};
    unsigned cur = raw[0];
    for (int c = 0; c < chunks; ++c) {
      const unsigned next = raw[c + 1];
      unsigned tap[4], b[kFeatherRowPix + 3];
      T2O_UNROLL
      for (int k = 0; k < 4; ++k) tap[k] = lds.taps[4 * c + k];
      T2O_UNROLL
      for (int q = 0; q < kFeatherRowPix + 3; ++q) b[q] = ((q < 4 ? cur : next) >> (8 * (q & 3))) & 0xffu;
      T2O_UNROLL
      for (int p = 0; p < kFeatherRowPix; ++p) {
        T2O_UNROLL
        for (int k = 0; k < 4; ++k) acc[p] = feather_mad(acc[p], tap[k], b[p + k]);
      }
      cur = next;
    }
    unsigned t[kFeatherRowPix];
    T2O_UNROLL
    for (int p = 0; p < kFeatherRowPix; ++p) t[p] = (acc[p] + 128u) >> 8;
    // x is a multiple of 4 below the pitch: the four uint16 lie inside the job's intermediate row, 8-byte aligned
    unsigned char* dst = reinterpret_cast<unsigned char*>(ws + j.ws_offset + (size_t)y * j.pitch + x);
    replay_store_dword(dst, t[0] | (t[1] << 16));
    replay_store_dword(dst + 4, t[2] | (t[3] << 16));
  }
}

// ---------------------------------------------------------------- COLUMN pass: the LDS image
struct FeatherColLds {
  unsigned* taps;                // kFeatherMaxTaps
  unsigned* rows;                // feather_col_rows(radius) x (kFeatherColW / 2) dwords: two uint16 per dword
  unsigned* ob;                  // kFeatherColH x kFeatherOutDw
};

T2O_HD FeatherColLds feather_col_lds(unsigned char* smem, int max_radius) {
  FeatherColLds l;
  l.taps = reinterpret_cast<unsigned*>(smem);
  l.rows = l.taps + kFeatherMaxTaps;
  l.ob = l.rows + feather_col_rows(max_radius) * (kFeatherColW / 2);
  return l;
}

// ---------------------------------------------------------------- COLUMN pass, phase: stage
T2O_HD void feather_col_stage(const FeatherJob& j, const unsigned short* w, const unsigned short* ws, int tile, int tid,
                              const FeatherColLds& lds) {
  feather_stage_taps(w, j.radius, tid, lds.taps);
  const int tx = tile % feather_col_tiles_x(j), ty = tile / feather_col_tiles_x(j);
  const int x0 = tx * kFeatherColW, y0 = ty * kFeatherColH;
  const int live = j.h - y0 < kFeatherColH ? j.h - y0 : kFeatherColH;
  const int rows = (live + kFeatherColPix - 1) / kFeatherColPix * kFeatherColPix + feather_taps(j.radius);      // what main reads
  const unsigned short* t = ws + j.ws_offset;
  for (int id = tid; id < rows * (kFeatherColW / 2); id += kFeatherThreads) {
    const int r = id / (kFeatherColW / 2), d = id - r * (kFeatherColW / 2);
    const int y = y0 - j.radius + r, yc = y < 0 ? 0 : y >= j.h ? j.h - 1 : y;
    const int x = x0 + 2 * d;                             // even, and the pitch is even: the pair lies inside the row or outside
    unsigned v = 0;
    if (x < j.pitch) {
      const unsigned short* a = t + (size_t)yc * j.pitch + x;        // 4-byte aligned: the workspace is, x and the pitch are even
#if defined(__HIP_DEVICE_COMPILE__)
      v = *reinterpret_cast<const unsigned*>(a);
#else
      v = (unsigned)a[0] | ((unsigned)a[1] << 16);
#endif
    }
    lds.rows[id] = v;
  }
}

// ---------------------------------------------------------------- COLUMN pass, phase: main
T2O_HD void feather_col_main(const FeatherJob& j, const unsigned char* out, int tile, int tid, const FeatherColLds& lds) {
  const int tx = tile % feather_col_tiles_x(j), ty = tile / feather_col_tiles_x(j);
  const int lane = tid & 63, x = tx * kFeatherColW + lane;
  if (x >= j.w) return;
  const int chunks = feather_taps(j.radius) / 4;
  const unsigned short* col = reinterpret_cast<const unsigned short*>(lds.rows) + lane;
  unsigned char* ob = reinterpret_cast<unsigned char*>(lds.ob);
  for (int r0 = (tid >> 6) * kFeatherColPix; r0 < kFeatherColH; r0 += kFeatherThreads / 64 * kFeatherColPix) {
    if (ty * kFeatherColH + r0 >= j.h) break;
    unsigned acc[kFeatherColPix], win[kFeatherColPix + 3];
    T2O_UNROLL
    for (int p = 0; p < kFeatherColPix; ++p) acc[p] = 0;
    T2O_UNROLL
    for (int q = 0; q < kFeatherColPix - 1; ++q) win[q + 4] = col[(r0 + q) * kFeatherColW];
    for (int c = 0; c < chunks; ++c) {
      unsigned tap[4];
      T2O_UNROLL
      for (int k = 0; k < 4; ++k) tap[k] = lds.taps[4 * c + k];
      T2O_UNROLL
      for (int q = 0; q < kFeatherColPix - 1; ++q) win[q] = win[q + 4];
      T2O_UNROLL
      for (int q = kFeatherColPix - 1; q < kFeatherColPix + 3; ++q) win[q] = col[(r0 + 4 * c + q) * kFeatherColW];
      T2O_UNROLL
      for (int p = 0; p < kFeatherColPix; ++p) {
        T2O_UNROLL
        for (int k = 0; k < 4; ++k) acc[p] = feather_mad(acc[p], tap[k], win[p + k]);
      }
    }
    T2O_UNROLL
    for (int p = 0; p < kFeatherColPix; ++p) {
      const int y = ty * kFeatherColH + r0 + p;
      if (y >= j.h) continue;
      const unsigned char* a = out + j.out_offset + (size_t)y * j.w + tx * kFeatherColW;
      ob[(r0 + p) * (kFeatherOutDw * 4) + replay_misalign(a) + lane] = (unsigned char)((acc[p] + (1u << 23)) >> 24);
    }
  }
}

// ---------------------------------------------------------------- COLUMN pass, phase: store
T2O_HD void feather_col_store(const FeatherJob& j, unsigned char* out, int tile, int tid, const FeatherColLds& lds) {
  const int tx = tile % feather_col_tiles_x(j), ty = tile / feather_col_tiles_x(j);
  const int x0 = tx * kFeatherColW, y0 = ty * kFeatherColH;
  const int rows = j.h - y0 < kFeatherColH ? j.h - y0 : kFeatherColH;
  const int nb = j.w - x0 < kFeatherColW ? j.w - x0 : kFeatherColW;
  for (int id = tid; id < rows * kFeatherOutDw; id += kFeatherThreads) {
    const int r = id / kFeatherOutDw, d = id - r * kFeatherOutDw;
    unsigned char* a = out + j.out_offset + (size_t)(y0 + r) * j.w + x0;
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
