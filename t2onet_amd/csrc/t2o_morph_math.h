// The tile programs of the mask MORPH kernels (t2o_morph.hip): a uint8 plane P (h, w) grown, shrunk or turned into a border
// band by an EXACT Euclidean distance of R <= 64 pixels -- "expand the selection by 4 px".  The definition
// (include/t2onet_hip.h states it in full): S = {p : P[p] >= 128}; Dout(p) / Din(p) = the least squared distance from p to a
// pixel of S / to a pixel of the frame outside S, +infinity where there is none; only pixels INSIDE the frame count.
//   GROW    255 where Dout <= R^2          SHRINK  255 where Din > R^2          BORDER  255 where Dout <= R^2 and Din <= R^2
// (p outside S has Din = 0, so SHRINK needs no test of S, and BORDER = GROW and not SHRINK.)  Integers only, two passes:
//   COLUMN pass  a FIELD g(y, x) = min(|dy| : |dy| <= R, (y + dy, x) in the set) or R + 1; the set is S for GROW, the frame
//                outside S for SHRINK, one field of each for BORDER.  A workgroup owns kMorphColW x kMorphColH pixels, lane =
//                x.  `stage`: the tile's source bytes plus R rows above and below, as far as they lie in the frame, into
//                LDS -- inside a row two ALIGNED global dwords funnel-shifted by the address modulo 4, at a row's end single
//                bytes.  `main`: a thread owns kMorphColSeg rows of one column: a running distance swept DOWN from R rows
//                above its segment and UP from R rows below it, both fields at once, the minimum of the two as a byte into
//                the workspace (row pitch a multiple of 4).
//   ROW pass     Dout(y, x) <= R^2  <=>  some |dx| <= R with x + dx in the frame has g(y, x + dx) <= c[|dx|],
//                c[k] = floor(sqrt(R^2 - k^2)) (morph_thresholds below, host only, integer).  A workgroup owns kMorphRowW x
//                kMorphRowH pixels.  `stage`: thresholds t_j = c[|j - Rp|] + 1 for |j - Rp| <= R, else 0 (Rp = R rounded up
//                to a multiple of 4, j < 2 Rp + 4), and each tile row's field bytes from column x0 - Rp on as ALIGNED
//                workspace dwords, 0xFF at every column outside the frame.  `main`: a thread makes 4 adjacent outputs: per
//                chunk of 4 thresholds one staged dword joins the previous one, 7 bytes feed 16 compares (g < t); the
//                0 / 255 bytes go to an LDS row buffer laid out with the DESTINATION rows' address modulo 4.  `store`:
//                whole aligned dwords where all four bytes belong to the tile's row, single bytes at its two ends.
// Every source byte is read by the first launch before the second writes any destination byte: a job may run in place, and
// a source may overlap any destination.  `__host__ __device__` phase functions, as t2o_feather_math.h's: the same programs
// run thread by thread in tests/host_emul/emul_morph.cpp (a test harness, never a fallback).
#pragma once
#include "t2o_feather_math.h"

namespace t2o {

constexpr int kMorphMaxJobs = 4;
constexpr int kMorphMaxRadius = 64;
constexpr int kMorphThreads = 256;
constexpr int kMorphGrow = 0, kMorphShrink = 1, kMorphBorder = 2;

constexpr int kMorphColW = 64, kMorphColH = 64;          // column pass tile; lane = x
constexpr int kMorphColSeg = 16;                         // rows of one thread: 4 waves x 16 rows span the tile
constexpr int kMorphColRows = kMorphColH + 2 * kMorphMaxRadius;               // 192 staged rows at R = 64
constexpr int kMorphRowW = 256, kMorphRowH = 8;          // row pass tile; 64 threads x 4 outputs span it, 4 rows at a time
constexpr int kMorphRowPix = 4;
constexpr int kMorphMaxTaps = 2 * kMorphMaxRadius + 4;   // 132 thresholds: 2 Rp + 1 padded to whole chunks
constexpr int kMorphRowDw = (kMorphRowW + kMorphMaxTaps) / 4;                 // 97 staged dwords per tile row and field
constexpr int kMorphOutDw = (3 + kMorphRowW + 3) / 4;    // 65 staged dwords per output row (lead-in + 256)
constexpr int kMorphCStride = 68;                        // bytes per job in the kernel arguments: c[0..64], padded

static_assert(kMorphColW == 64 && kMorphColH == kMorphThreads / 64 * kMorphColSeg, "column pass thread map");
static_assert(kMorphRowW == 64 * kMorphRowPix && kMorphRowH % (kMorphThreads / 64) == 0, "row pass thread map");

// Host side: c[k] = floor(sqrt(R^2 - k^2)) for k <= R, 0 behind it, in integer arithmetic.  Returns 0, or 1 when an entry
// fails c^2 + k^2 <= R^2 < (c + 1)^2 + k^2 (it cannot) or R lies outside 0..64.
static inline int morph_thresholds(int radius, unsigned char* c) {
  if (radius < 0 || radius > kMorphMaxRadius) return 1;
  for (int k = 0; k < kMorphCStride; ++k) c[k] = 0;
  int v = radius;
  for (int k = 0; k <= radius; ++k) {
    while (v * v + k * k > radius * radius) --v;
    if (v < 0 || !(v * v + k * k <= radius * radius && radius * radius < (v + 1) * (v + 1) + k * k)) return 1;
    c[k] = (unsigned char)v;
  }
  return 0;
}

// one job as the kernels see it
struct MorphJob {
  long long src_offset, out_offset;
  long long ws_offset;           // first byte of the job's first field, counted from the workspace; a multiple of 4
  int h, w;
  int radius, mode;
  int pitch;                     // bytes per field row: w rounded up to a multiple of 4
  int fields;                    // 1, or 2 for BORDER: the field of S, behind it (h * pitch bytes on) the field of its complement
};

struct MorphArgs {
  const unsigned char* src;
  unsigned char* out;
  unsigned char* ws;
  MorphJob jobs[kMorphMaxJobs];
  unsigned char c[kMorphMaxJobs][kMorphCStride];
};

T2O_HD int morph_pitch(int w) { return (w + 3) / 4 * 4; }
T2O_HD int morph_pad(int radius) { return (radius + 3) / 4 * 4; }                     // Rp
T2O_HD int morph_taps(int radius) { return 2 * morph_pad(radius) + 4; }              // 2 Rp + 1 padded to whole chunks
T2O_HD int morph_col_tiles_x(const MorphJob& j) { return (j.w + kMorphColW - 1) / kMorphColW; }
T2O_HD int morph_col_tiles(const MorphJob& j) { return morph_col_tiles_x(j) * ((j.h + kMorphColH - 1) / kMorphColH); }
T2O_HD int morph_row_tiles_x(const MorphJob& j) { return (j.w + kMorphRowW - 1) / kMorphRowW; }
T2O_HD int morph_row_tiles(const MorphJob& j) { return morph_row_tiles_x(j) * ((j.h + kMorphRowH - 1) / kMorphRowH); }
T2O_HD size_t morph_field_bytes(const MorphJob& j) { return (size_t)j.h * j.pitch; }

struct MorphColLds {
  unsigned src[kMorphColRows * (kMorphColW / 4)];        // row r = frame row y0 - R + r, byte x - x0; rows outside the frame unset
};

struct MorphRowLds {
  alignas(16) unsigned taps[kMorphMaxTaps];              // a chunk's four thresholds: one 16-byte read, the same address in every lane
  unsigned raw[2 * kMorphRowH * kMorphRowDw];            // field f, tile row r at (f * kMorphRowH + r) * kMorphRowDw
  unsigned ob[kMorphRowH * kMorphOutDw];
};

// ---------------------------------------------------------------- COLUMN pass, phase: stage
T2O_HD void morph_col_stage(const MorphJob& j, const unsigned char* src, int tile, int tid, MorphColLds& lds) {
  const int tx = tile % morph_col_tiles_x(j), ty = tile / morph_col_tiles_x(j);
  const int x0 = tx * kMorphColW, y0 = ty * kMorphColH;
  const int live = j.h - y0 < kMorphColH ? j.h - y0 : kMorphColH;
  const int rows = live + 2 * j.radius;                  // what main reads, as far as it lies in the frame
  const unsigned char* plane = src + j.src_offset;
  const unsigned char* end = plane + (size_t)j.h * j.w;
  for (int id = tid; id < rows * (kMorphColW / 4); id += kMorphThreads) {
    const int r = id / (kMorphColW / 4), d = id - r * (kMorphColW / 4);
    const int y = y0 - j.radius + r, c = x0 + 4 * d;     // column of this dword's first byte
    if (y < 0 || y >= j.h || c >= j.w) continue;
    const unsigned char* row = plane + (size_t)y * j.w;
    unsigned v;
    if (c + 4 <= j.w) {
      const unsigned char* a = row + c;
      const int m = (int)replay_misalign(a);
      v = replay_load_dword(a - m, plane, end);
      if (m) v = feather_funnel(v, replay_load_dword(a - m + 4, plane, end), m);
    } else {
      v = 0;
      for (int b = 0; c + b < j.w; ++b) v |= (unsigned)row[c + b] << (8 * b);
    }
    lds.src[id] = v;
  }
}

// ---------------------------------------------------------------- COLUMN pass, phase: main
// one step of the two running distances at frame row y (LDS row r): a row outside the frame belongs to neither set
T2O_HD void morph_col_step(const MorphJob& j, const unsigned char* col, int y, int r, int cap, int& da, int& db) {
  da = da < cap ? da + 1 : cap;
  db = db < cap ? db + 1 : cap;
  if (y >= 0 && y < j.h) {
    if (col[r * kMorphColW] >= 128) da = 0;
    else db = 0;
  }
}

T2O_HD void morph_col_main(const MorphJob& j, unsigned char* ws, int tile, int tid, const MorphColLds& lds) {
  const int tx = tile % morph_col_tiles_x(j), ty = tile / morph_col_tiles_x(j);
  const int lane = tid & 63, x = tx * kMorphColW + lane;
  const int r0 = (tid >> 6) * kMorphColSeg, y0 = ty * kMorphColH + r0;        // the segment's first row, in the tile / the frame
  if (x >= j.w || y0 >= j.h) return;
  const int R = j.radius, cap = R + 1;
  const unsigned char* col = reinterpret_cast<const unsigned char*>(lds.src) + lane;       // LDS row r0 + i = frame row y0 - R + i
  int ga[kMorphColSeg], gb[kMorphColSeg];
  int da = cap, db = cap;
  for (int i = 0; i < R; ++i) morph_col_step(j, col, y0 - R + i, r0 + i, cap, da, db);
  T2O_UNROLL
  for (int i = 0; i < kMorphColSeg; ++i) {
    morph_col_step(j, col, y0 + i, r0 + R + i, cap, da, db);
    ga[i] = da; gb[i] = db;
  }
  da = db = cap;
  for (int i = R - 1; i >= 0; --i) morph_col_step(j, col, y0 + kMorphColSeg + i, r0 + R + kMorphColSeg + i, cap, da, db);
  unsigned char* fa = ws + j.ws_offset;                                       // where the field of S goes, if the mode reads it
  unsigned char* fb = fa + (j.mode == kMorphBorder ? morph_field_bytes(j) : 0);
  T2O_UNROLL
  for (int i = kMorphColSeg - 1; i >= 0; --i) {
    morph_col_step(j, col, y0 + i, r0 + R + i, cap, da, db);
    if (y0 + i >= j.h) continue;
    const size_t at = (size_t)(y0 + i) * j.pitch + x;
    if (j.mode != kMorphShrink) fa[at] = (unsigned char)(da < ga[i] ? da : ga[i]);
    if (j.mode != kMorphGrow) fb[at] = (unsigned char)(db < gb[i] ? db : gb[i]);
  }
}

// ---------------------------------------------------------------- ROW pass, phase: stage
T2O_HD void morph_row_stage(const MorphJob& j, const unsigned char* c, const unsigned char* ws, int tile, int tid, MorphRowLds& lds) {
  const int R = j.radius, Rp = morph_pad(R);
  for (int k = tid; k < morph_taps(R); k += kMorphThreads) {
    const int dx = k < Rp ? Rp - k : k - Rp;
    lds.taps[k] = dx <= R ? (unsigned)c[dx] + 1u : 0u;
  }
  const int tx = tile % morph_row_tiles_x(j), ty = tile / morph_row_tiles_x(j);
  const int x0 = tx * kMorphRowW, y0 = ty * kMorphRowH;
  const int rows = j.h - y0 < kMorphRowH ? j.h - y0 : kMorphRowH;
  const int cols = j.w - x0 < kMorphRowW ? (j.w - x0 + 3) / 4 * 4 : kMorphRowW;
  const int nd = (cols + morph_taps(R)) / 4;             // dwords of a row that main reads
  for (int id = tid; id < j.fields * rows * nd; id += kMorphThreads) {
    const int f = id / (rows * nd), r = (id - f * rows * nd) / nd, d = id - (f * rows + r) * nd;
    const int col = x0 - Rp + 4 * d;                     // a multiple of 4: a dword lies inside the row's pitch or outside it
    unsigned v = 0xffffffffu;
    if (col >= 0 && col < j.w) {
      const unsigned char* a = ws + j.ws_offset + f * morph_field_bytes(j) + (size_t)(y0 + r) * j.pitch + col;     // 4-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
      v = *reinterpret_cast<const unsigned*>(a);
#else
      memcpy(&v, a, 4);
#endif
      if (col + 4 > j.w) v |= 0xffffffffu << (8 * (j.w - col));              // the pitch's padding: never written, never used
    }
    lds.raw[(f * kMorphRowH + r) * kMorphRowDw + d] = v;
  }
}

// ---------------------------------------------------------------- ROW pass, phase: main
T2O_HD void morph_row_main(const MorphJob& j, const unsigned char* out, int tile, int tid, MorphRowLds& lds) {
  const int tx = tile % morph_row_tiles_x(j), ty = tile / morph_row_tiles_x(j);
  const int cg = tid & 63, x = tx * kMorphRowW + kMorphRowPix * cg;
  if (x >= j.w) return;
  const int chunks = morph_taps(j.radius) / 4;
  unsigned char* ob = reinterpret_cast<unsigned char*>(lds.ob);
  for (int r = tid >> 6; r < kMorphRowH; r += kMorphThreads / 64) {
    const int y = ty * kMorphRowH + r;
    if (y >= j.h) break;
    unsigned nr[2][kMorphRowPix];
    T2O_UNROLL
    for (int f = 0; f < 2; ++f) {
      const unsigned* raw = lds.raw + (f * kMorphRowH + r) * kMorphRowDw + cg;
      unsigned hit[kMorphRowPix] = {0, 0, 0, 0};
      const int n = f < j.fields ? chunks : 0;           // (nr[1] is read by BORDER only, which has two fields)
      unsigned cur = raw[0];
      for (int c = 0; c < n; ++c) {
        const unsigned next = raw[c + 1];
        unsigned tap[4], b[kMorphRowPix + 3];
        T2O_UNROLL
        for (int k = 0; k < 4; ++k) tap[k] = lds.taps[4 * c + k];
        T2O_UNROLL
        for (int q = 0; q < kMorphRowPix + 3; ++q) b[q] = ((q < 4 ? cur : next) >> (8 * (q & 3))) & 0xffu;
        T2O_UNROLL
        for (int p = 0; p < kMorphRowPix; ++p) {
          T2O_UNROLL
          for (int k = 0; k < 4; ++k) hit[p] |= (unsigned)(b[p + k] < tap[k]);
        }
        cur = next;
      }
      T2O_UNROLL
      for (int p = 0; p < kMorphRowPix; ++p) nr[f][p] = hit[p];
    }
    const unsigned char* a = out + j.out_offset + (size_t)y * j.w + tx * kMorphRowW;
    unsigned char* dst = ob + r * (kMorphOutDw * 4) + replay_misalign(a) + kMorphRowPix * cg;
    T2O_UNROLL
    for (int p = 0; p < kMorphRowPix; ++p) {
      const unsigned on = j.mode == kMorphGrow ? nr[0][p] : j.mode == kMorphShrink ? nr[0][p] ^ 1u : nr[0][p] & nr[1][p];
      dst[p] = (unsigned char)(on ? 255 : 0);            // (bytes of columns >= w stay in LDS: store leaves them out)
    }
  }
}

// ---------------------------------------------------------------- ROW pass, phase: store
T2O_HD void morph_row_store(const MorphJob& j, unsigned char* out, int tile, int tid, const MorphRowLds& lds) {
  const int tx = tile % morph_row_tiles_x(j), ty = tile / morph_row_tiles_x(j);
  const int x0 = tx * kMorphRowW, y0 = ty * kMorphRowH;
  const int rows = j.h - y0 < kMorphRowH ? j.h - y0 : kMorphRowH;
  const int nb = j.w - x0 < kMorphRowW ? j.w - x0 : kMorphRowW;
  for (int id = tid; id < rows * kMorphOutDw; id += kMorphThreads) {
    const int r = id / kMorphOutDw, d = id - r * kMorphOutDw;
    unsigned char* a = out + j.out_offset + (size_t)(y0 + r) * j.w + x0;
    const int lo = 4 * d - (int)replay_misalign(a);      // this dword's first byte, counted from the row's first
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
