// The tile programs of the mask REFINE kernels (t2o_refine.hip): a uint8 plane p (h, w) snapped to the edges of the photo
// it belongs to by the guided filter of He et al. in INTEGER arithmetic -- the guide is the photo's own luminance, the
// window a (2r+1)^2 box with replicated borders, the regulariser E in byte^2 units.  The arithmetic
// (include/t2onet_hip.h states it in full; // is floor division, n = (2r+1)^2):
//   I = select_lum(R, G, B)                                          t2o_select_math.h's luminance, 0..255
//   S_I, S_p, S_II, S_Ip = box(I), box(p), box(I I), box(I p)        each <= 16641 * 65025 < 2^31
//   cov = n S_Ip - S_I S_p;  den = n S_II - S_I^2 + E n^2 > 0        signed 64-bit
//   A = (2048 cov + den) // (2 den)                                  a in Q10, |A| <= 65281
//   B = (2 (1024 S_p - A S_I) + n) // (2 n)                          |B| < 1.7e7, int32
//   T_A = box(A) (int32), T_B = box(B) (64-bit);  out = clamp((2 (T_A I + T_B) + 1024 n) // (2048 n), 0, 255)
// Integer sums are exact in any order, so every box is a ROW sum followed by a COLUMN sum.
//
// Like t2o_feather_math.h these are `__host__ __device__` phase functions -- what ONE thread of ONE workgroup does between
// two barriers -- so that tests/host_emul/emul_refine.cpp runs the same programs thread by thread with g++ (a test
// harness, never a fallback).  FOUR launches, each covering every job of the call:
//   ROWS 1   a workgroup owns kRefineRowW x kRefineRowH pixels.  `stage`: per tile row the bytes of I and of p from column
//            x0 - r on, CLAMPED to the row, as dwords -- inside the row 12 photo bytes and 4 plane bytes through aligned
//            dwords funnel-shifted by the address modulo 4, at the row's ends single clamped bytes.  `main`: a thread makes
//            4 adjacent outputs: the taps the four windows share once, each window's own on top (additions only).  Three uint32 planes go to the
//            workspace as aligned 16-byte stores: S_I | S_p << 16 (each <= 129 * 255), S_II, S_Ip.
//   COLS 2   a workgroup owns kRefineColW x kRefineColH pixels, lane = x, a wave kRefineColSeg rows: the first window row by
//            row, then a RUNNING sum down the column (one row enters, one leaves; no LDS); A and B per pixel, two int32 planes.
//   ROWS 3   the same tiles on A and B: a tile row's values from column x0 - r on in LDS, de-interleaved by column modulo 4
//            so that the lanes of a wave read consecutive banks; the first window tap by tap, the next three by sliding
//            (plain sums, no products); T_A rows as int32, T_B rows as int64 (129 B's pass 2^31).
//   COLS 4   as COLS 2 on the row sums; I again from the photo's bytes; the byte goes to an LDS row buffer laid out with the
//            DESTINATION rows' address modulo 4.  `store`: whole aligned dwords where all four bytes belong to the tile's
//            row, single bytes at its two ends: no byte outside the plane is written.
// The plane is read by the first launch only and the destination written by the last only: a job may run in place, and a
// source may overlap any destination.  Workspace: 20 bytes per pixel of the padded plane (rows padded to 4 pixels) -- 12
// for the three row-sum planes, which the row sums of A and B then reuse, and 8 for A and B.
#pragma once

#include "t2o_select_math.h"

namespace t2o {

constexpr int kRefineMaxJobs = 4;                        // = kReplayMaxMasks = kFeatherMaxJobs: the planes of one local edit
constexpr int kRefineMaxRadius = 64;
constexpr int kRefineMaxEps2 = 255 * 255;
constexpr int kRefineShift = 10;                         // fractional bits of A and B
constexpr int kRefineThreads = 256;
constexpr int kRefineLaunches = 4;

constexpr int kRefineRowW = 256, kRefineRowH = 8;        // row pass tile; 64 threads x 4 outputs span it, 4 rows at a time
constexpr int kRefineRowPix = 4;
constexpr int kRefineRowCols = kRefineRowW + 2 * kRefineMaxRadius;            // 384 staged columns per tile row
constexpr int kRefineRowDw = kRefineRowCols / 4;         // as bytes: 96 dwords;  as int32: the stride of a column residue
constexpr int kRefineColW = 64, kRefineColH = 256;       // column pass tile; lane = x, a wave owns kRefineColSeg rows
constexpr int kRefineColSeg = kRefineColH / (kRefineThreads / 64);
constexpr int kRefineOutDw = (3 + kRefineColW + 3) / 4;  // 17 staged dwords per output row (lead-in + 64)
constexpr int kRefineWsPerPixel = 20;                    // workspace bytes per pixel of the padded plane

static_assert(kRefineRowW == 64 * kRefineRowPix && kRefineRowH % (kRefineThreads / 64) == 0, "row pass thread map");
static_assert(kRefineColW == 64 && kRefineColSeg * (kRefineThreads / 64) == kRefineColH, "column pass thread map");
static_assert((2 * kRefineMaxRadius + 1) * 255 < 65536, "S_I and S_p of a row share a dword");

// one job as the kernels see it
struct RefineJob {
  long long photo_offset, src_offset, out_offset;
  long long ws_offset;           // first byte of the job's planes, counted from the workspace; a multiple of 16
  long long en2;                 // E n^2
  int h, w;
  int radius, n;                 // n = (2r+1)^2
  int pitch;                     // elements per workspace row: w rounded up to a multiple of 4
  int reserved;
};

struct RefineArgs {
  const unsigned char* photo;
  const unsigned char* src;
  unsigned char* out;
  unsigned char* ws;
  RefineJob jobs[kRefineMaxJobs];
};

T2O_HD int refine_pitch(int w) { return (w + 3) / 4 * 4; }
T2O_HD long long refine_plane(const RefineJob& j) { return (long long)j.h * j.pitch; }          // elements of a workspace plane
T2O_HD int refine_row_tiles_x(const RefineJob& j) { return (j.w + kRefineRowW - 1) / kRefineRowW; }
T2O_HD int refine_row_tiles(const RefineJob& j) { return refine_row_tiles_x(j) * ((j.h + kRefineRowH - 1) / kRefineRowH); }
T2O_HD int refine_col_tiles_x(const RefineJob& j) { return (j.w + kRefineColW - 1) / kRefineColW; }
T2O_HD int refine_col_tiles(const RefineJob& j) { return refine_col_tiles_x(j) * ((j.h + kRefineColH - 1) / kRefineColH); }

// the planes of a job in the workspace
T2O_HD unsigned* refine_ws_sums(const RefineJob& j, unsigned char* ws, int k) {                    // k = 0: S_I | S_p << 16, 1: S_II, 2: S_Ip
  return reinterpret_cast<unsigned*>(ws + j.ws_offset) + k * refine_plane(j);
}
T2O_HD int* refine_ws_ab(const RefineJob& j, unsigned char* ws, int k) {                           // k = 0: A, 1: B
  return reinterpret_cast<int*>(ws + j.ws_offset) + (3 + k) * refine_plane(j);
}
T2O_HD int* refine_ws_ta(const RefineJob& j, unsigned char* ws) { return reinterpret_cast<int*>(ws + j.ws_offset); }
T2O_HD long long* refine_ws_tb(const RefineJob& j, unsigned char* ws) {                            // behind T_A; 4 h pitch is a multiple of 16
  return reinterpret_cast<long long*>(ws + j.ws_offset + 4 * refine_plane(j));
}

T2O_HD int refine_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// floor(num / den) for den > 0
T2O_HD long long refine_floordiv(long long num, long long den) {
  const long long q = num / den;
  return num - q * den < 0 ? q - 1 : q;
}

// A and B of one pixel from its four box sums
T2O_HD void refine_ab(const RefineJob& j, unsigned sI, unsigned sp, unsigned sII, unsigned sIp, int* A, int* B) {
  const long long n = j.n;
  const long long cov = n * (long long)sIp - (long long)sI * (long long)sp;
  const long long den = n * (long long)sII - (long long)sI * (long long)sI + j.en2;
  const long long a = refine_floordiv(2 * (1ll << kRefineShift) * cov + den, 2 * den);
  *A = (int)a;
  *B = (int)refine_floordiv(2 * ((1ll << kRefineShift) * (long long)sp - a * (long long)sI) + n, 2 * n);
}

// the byte of one pixel from its two box sums and its luminance: floor(num / (2048 n)) = floor(floor(num / 2048) / n), and the
// clamp to 0..255 is taken first, which leaves an unsigned 32-bit division (256 n < 2^23)
T2O_HD unsigned refine_byte(const RefineJob& j, int tA, long long tB, int I) {
  const long long num = 2 * ((long long)tA * I + tB) + (long long)j.n * (1ll << kRefineShift);
  const long long t = num >> (kRefineShift + 1);                     // arithmetic: the floor for a negative numerator too
  if (t < 0) return 0u;
  if (t >= 256ll * j.n) return 255u;
  return (unsigned)t / (unsigned)j.n;
}

T2O_HD void refine_store4(void* dst, unsigned a, unsigned b, unsigned c, unsigned d) {            // dst: 16-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<uint4*>(dst) = make_uint4(a, b, c, d);
#else
  const unsigned v[4] = {a, b, c, d};
  memcpy(dst, v, 16);
#endif
}

// the geometry of a row tile
struct RefineRowTile {
  int x0, y0, rows, cols;        // cols: the live columns rounded up to a multiple of 4
};

T2O_HD RefineRowTile refine_row_tile(const RefineJob& j, int tile) {
  RefineRowTile t;
  const int tx = tile % refine_row_tiles_x(j), ty = tile / refine_row_tiles_x(j);
  t.x0 = tx * kRefineRowW; t.y0 = ty * kRefineRowH;
  t.rows = j.h - t.y0 < kRefineRowH ? j.h - t.y0 : kRefineRowH;
  t.cols = j.w - t.x0 < kRefineRowW ? (j.w - t.x0 + 3) / 4 * 4 : kRefineRowW;
  return t;
}

// ---------------------------------------------------------------- ROWS 1
struct RefineRowLds {
  unsigned gi[kRefineRowH * kRefineRowDw];               // luminance bytes, column x0 - r + 4d first in dword d
  unsigned gp[kRefineRowH * kRefineRowDw];               // plane bytes
};

T2O_HD void refine_rows1_stage(const RefineJob& j, const unsigned char* photo_base, const unsigned char* src, int tile, int tid,
                               RefineRowLds& lds) {
  const RefineRowTile t = refine_row_tile(j, tile);
  const int nd = (t.cols + 2 * j.radius + 3) / 4;        // dwords of a row that main reads (<= kRefineRowDw)
  const long long n = (long long)j.h * j.w;
  const unsigned char* photo = photo_base + j.photo_offset;
  const unsigned char* plane = src + j.src_offset;
  for (int id = tid; id < t.rows * nd; id += kRefineThreads) {
    const int r = id / nd, d = id - r * nd;
    const long long row = (long long)(t.y0 + r) * j.w;
    const int c = t.x0 - j.radius + 4 * d;               // column of this dword's first byte
    unsigned vi = 0, vp = 0;
    if (c >= 0 && c + 4 <= j.w) {
      const unsigned char* a = plane + row + c;
      const int m = (int)replay_misalign(a);
      vp = replay_load_dword(a - m, plane, plane + n);
      if (m) vp = select_funnel(vp, replay_load_dword(a - m + 4, plane, plane + n), m);
      unsigned rgb[3];
      select_load<3>(photo + 3 * (row + c), photo, photo + 3 * n, rgb);
      T2O_UNROLL
      for (int b = 0; b < 4; ++b) {
        int ch[3];
        T2O_UNROLL
        for (int k = 0; k < 3; ++k) ch[k] = (int)((rgb[(3 * b + k) >> 2] >> (8 * ((3 * b + k) & 3))) & 0xffu);
        vi |= (unsigned)select_lum(ch[0], ch[1], ch[2]) << (8 * b);
      }
    } else {
      T2O_UNROLL
      for (int b = 0; b < 4; ++b) {
        const long long at = row + refine_clamp(c + b, j.w - 1);
        vp |= (unsigned)plane[at] << (8 * b);
        vi |= (unsigned)select_lum(photo[3 * at], photo[3 * at + 1], photo[3 * at + 2]) << (8 * b);
      }
    }
    lds.gi[r * kRefineRowDw + d] = vi;
    lds.gp[r * kRefineRowDw + d] = vp;
  }
}

T2O_HD void refine_rows1_main(const RefineJob& j, unsigned char* ws, int tile, int tid, const RefineRowLds& lds) {
  const RefineRowTile t = refine_row_tile(j, tile);
  const int cg = tid & 63, x = t.x0 + kRefineRowPix * cg;
  if (x >= j.w) return;
  const int taps = 2 * j.radius + 1;
  for (int r = tid >> 6; r < t.rows; r += kRefineThreads / 64) {
    const unsigned char* bi = reinterpret_cast<const unsigned char*>(lds.gi + r * kRefineRowDw) + kRefineRowPix * cg;
    const unsigned char* bp = reinterpret_cast<const unsigned char*>(lds.gp + r * kRefineRowDw) + kRefineRowPix * cg;
    // window q = columns q .. q + taps - 1 of the staged row.  Additions only (a difference of byte products is what
    // hipcc's dot-product matching gets wrong): the columns 3 .. taps - 1 that all four windows share are summed once,
    // every window adds its own columns below 3 and from max(taps, 3) on
    unsigned cI = 0, cp = 0, cII = 0, cIp = 0;
    for (int k = kRefineRowPix - 1; k < taps; ++k) {
      const unsigned I = bi[k], p = bp[k];
      cI += I; cp += p; cII += I * I; cIp += I * p;
    }
    const int hi = taps > kRefineRowPix - 1 ? taps : kRefineRowPix - 1;
    unsigned o[3][kRefineRowPix];
    T2O_UNROLL
    for (int q = 0; q < kRefineRowPix; ++q) {
      unsigned sI = cI, sp = cp, sII = cII, sIp = cIp;
      T2O_UNROLL
      for (int i = 0; i < 2 * (kRefineRowPix - 1); ++i) {
        const int k = i < kRefineRowPix - 1 ? i : hi + i - (kRefineRowPix - 1);
        if (k >= q && k < q + taps) {
          const unsigned I = bi[k], p = bp[k];
          sI += I; sp += p; sII += I * I; sIp += I * p;
        }
      }
      o[0][q] = sI | (sp << 16); o[1][q] = sII; o[2][q] = sIp;
    }
    // x is a multiple of 4 below the pitch: the four values lie inside the job's workspace row, 16-byte aligned
    const long long at = (long long)(t.y0 + r) * j.pitch + x;
    T2O_UNROLL
    for (int k = 0; k < 3; ++k) refine_store4(refine_ws_sums(j, ws, k) + at, o[k][0], o[k][1], o[k][2], o[k][3]);
  }
}

// ---------------------------------------------------------------- COLS 2
T2O_HD void refine_cols2(const RefineJob& j, unsigned char* ws, int tile, int tid) {
  const int tx = tile % refine_col_tiles_x(j), ty = tile / refine_col_tiles_x(j);
  const int x = tx * kRefineColW + (tid & 63);
  const int ys = ty * kRefineColH + (tid >> 6) * kRefineColSeg;
  if (x >= j.w || ys >= j.h) return;
  const int ye = ys + kRefineColSeg < j.h ? ys + kRefineColSeg : j.h;
  const unsigned* q0 = refine_ws_sums(j, ws, 0) + x;
  const unsigned* q1 = refine_ws_sums(j, ws, 1) + x;
  const unsigned* q2 = refine_ws_sums(j, ws, 2) + x;
  int* A = refine_ws_ab(j, ws, 0) + x;
  int* B = refine_ws_ab(j, ws, 1) + x;
  unsigned sI = 0, sp = 0, sII = 0, sIp = 0;
  for (int dy = -j.radius; dy <= j.radius; ++dy) {
    const long long at = (long long)refine_clamp(ys + dy, j.h - 1) * j.pitch;
    const unsigned v = q0[at];
    sI += v & 0xffffu; sp += v >> 16; sII += q1[at]; sIp += q2[at];
  }
  for (int y = ys; y < ye; ++y) {
    if (y > ys) {                                         // one row enters, one leaves
      const long long in = (long long)refine_clamp(y + j.radius, j.h - 1) * j.pitch;
      const long long out = (long long)refine_clamp(y - j.radius - 1, j.h - 1) * j.pitch;
      const unsigned v = q0[in], v0 = q0[out];
      sI += (v & 0xffffu) - (v0 & 0xffffu); sp += (v >> 16) - (v0 >> 16); sII += q1[in] - q1[out]; sIp += q2[in] - q2[out];
    }
    int a, b;
    refine_ab(j, sI, sp, sII, sIp, &a, &b);
    A[(long long)y * j.pitch] = a;
    B[(long long)y * j.pitch] = b;
  }
}

// ---------------------------------------------------------------- ROWS 3
// column k of a staged row lies at (k & 3) * kRefineRowDw + (k >> 2): lane cg reads k = 4 cg + i, consecutive banks
struct RefineRow3Lds {
  int a[kRefineRowH * kRefineRowCols];
  int b[kRefineRowH * kRefineRowCols];
};

T2O_HD int refine_row3_at(int k) { return (k & 3) * kRefineRowDw + (k >> 2); }

T2O_HD void refine_rows3_stage(const RefineJob& j, unsigned char* ws, int tile, int tid, RefineRow3Lds& lds) {
  const RefineRowTile t = refine_row_tile(j, tile);
  const int nk = t.cols + 2 * j.radius;                  // columns of a row that main reads (<= kRefineRowCols)
  const int* A = refine_ws_ab(j, ws, 0);
  const int* B = refine_ws_ab(j, ws, 1);
  for (int id = tid; id < t.rows * nk; id += kRefineThreads) {
    const int r = id / nk, k = id - r * nk;
    const long long at = (long long)(t.y0 + r) * j.pitch + refine_clamp(t.x0 - j.radius + k, j.w - 1);
    lds.a[r * kRefineRowCols + refine_row3_at(k)] = A[at];
    lds.b[r * kRefineRowCols + refine_row3_at(k)] = B[at];
  }
}

T2O_HD void refine_rows3_main(const RefineJob& j, unsigned char* ws, int tile, int tid, const RefineRow3Lds& lds) {
  const RefineRowTile t = refine_row_tile(j, tile);
  const int cg = tid & 63, x = t.x0 + kRefineRowPix * cg;
  if (x >= j.w) return;
  const int taps = 2 * j.radius + 1;
  for (int r = tid >> 6; r < t.rows; r += kRefineThreads / 64) {
    const int* la = lds.a + r * kRefineRowCols;
    const int* lb = lds.b + r * kRefineRowCols;
    int tA = 0;
    long long tB = 0;
    for (int k = 0; k < taps; ++k) {
      tA += la[refine_row3_at(kRefineRowPix * cg + k)];
      tB += lb[refine_row3_at(kRefineRowPix * cg + k)];
    }
    int oa[kRefineRowPix];
    long long ob[kRefineRowPix];
    T2O_UNROLL
    for (int q = 0; q < kRefineRowPix; ++q) {
      if (q) {
        const int in = refine_row3_at(kRefineRowPix * cg + taps + q - 1), out = refine_row3_at(kRefineRowPix * cg + q - 1);
        tA += la[in] - la[out];
        tB += (long long)lb[in] - lb[out];
      }
      oa[q] = tA; ob[q] = tB;
    }
    const long long at = (long long)(t.y0 + r) * j.pitch + x;
    refine_store4(refine_ws_ta(j, ws) + at, (unsigned)oa[0], (unsigned)oa[1], (unsigned)oa[2], (unsigned)oa[3]);
    long long* tb = refine_ws_tb(j, ws) + at;
    T2O_UNROLL
    for (int q = 0; q < kRefineRowPix; q += 2)
      refine_store4(tb + q, (unsigned)(unsigned long long)ob[q], (unsigned)((unsigned long long)ob[q] >> 32),
                    (unsigned)(unsigned long long)ob[q + 1], (unsigned)((unsigned long long)ob[q + 1] >> 32));
  }
}

// ---------------------------------------------------------------- COLS 4
struct RefineOutLds {
  unsigned ob[kRefineColH * kRefineOutDw];
};

T2O_HD void refine_cols4_main(const RefineJob& j, const unsigned char* photo_base, const unsigned char* out, unsigned char* ws,
                              int tile, int tid, RefineOutLds& lds) {
  const int tx = tile % refine_col_tiles_x(j), ty = tile / refine_col_tiles_x(j);
  const int lane = tid & 63, x = tx * kRefineColW + lane;
  const int r0 = (tid >> 6) * kRefineColSeg, ys = ty * kRefineColH + r0;
  if (x >= j.w || ys >= j.h) return;
  const int ye = ys + kRefineColSeg < j.h ? ys + kRefineColSeg : j.h;
  const int* ta = refine_ws_ta(j, ws) + x;
  const long long* tb = refine_ws_tb(j, ws) + x;
  const unsigned char* photo = photo_base + j.photo_offset;
  unsigned char* ob = reinterpret_cast<unsigned char*>(lds.ob);
  int tA = 0;
  long long tB = 0;
  for (int dy = -j.radius; dy <= j.radius; ++dy) {
    const long long at = (long long)refine_clamp(ys + dy, j.h - 1) * j.pitch;
    tA += ta[at]; tB += tb[at];
  }
  for (int y = ys; y < ye; ++y) {
    if (y > ys) {
      const long long in = (long long)refine_clamp(y + j.radius, j.h - 1) * j.pitch;
      const long long gone = (long long)refine_clamp(y - j.radius - 1, j.h - 1) * j.pitch;
      tA += ta[in] - ta[gone]; tB += tb[in] - tb[gone];
    }
    const long long px = (long long)y * j.w + x;
    const int I = select_lum(photo[3 * px], photo[3 * px + 1], photo[3 * px + 2]);
    const unsigned char* a = out + j.out_offset + (long long)y * j.w + tx * kRefineColW;
    ob[(r0 + y - ys) * (kRefineOutDw * 4) + replay_misalign(a) + lane] = (unsigned char)refine_byte(j, tA, tB, I);
  }
}

T2O_HD void refine_cols4_store(const RefineJob& j, unsigned char* out, int tile, int tid, const RefineOutLds& lds) {
  const int tx = tile % refine_col_tiles_x(j), ty = tile / refine_col_tiles_x(j);
  const int x0 = tx * kRefineColW, y0 = ty * kRefineColH;
  const int rows = j.h - y0 < kRefineColH ? j.h - y0 : kRefineColH;
  const int nb = j.w - x0 < kRefineColW ? j.w - x0 : kRefineColW;
  for (int id = tid; id < rows * kRefineOutDw; id += kRefineThreads) {
    const int r = id / kRefineOutDw, d = id - r * kRefineOutDw;
    unsigned char* a = out + j.out_offset + (long long)(y0 + r) * j.w + x0;
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

// Host side: the checks of the C ABI on one job and the kernels' copy of it.  Returns nullptr or the reason for T2O_EINVAL.
inline const char* refine_prepare(RefineJob& d, long long photo_offset, long long src_offset, long long out_offset, int h, int w,
                                  int radius, int eps2, long long ws_offset) {
  if (h <= 0 || w <= 0) return "refine_u8: h and w must be positive";
  if ((long long)h * w >= (1ll << 31)) return "refine_u8: h * w must stay below 2^31";
  if (photo_offset < 0 || src_offset < 0 || out_offset < 0) return "refine_u8: negative offset";
  if (radius < 0 || radius > kRefineMaxRadius) return "refine_u8: radius must lie in 0..64";
  if (eps2 < 1 || eps2 > kRefineMaxEps2) return "refine_u8: eps2 must lie in 1..65025";
  d.photo_offset = photo_offset; d.src_offset = src_offset; d.out_offset = out_offset;
  d.ws_offset = ws_offset;
  d.h = h; d.w = w;
  d.radius = radius; d.n = (2 * radius + 1) * (2 * radius + 1);
  d.en2 = (long long)eps2 * d.n * d.n;
  d.pitch = refine_pitch(w);
  d.reserved = 0;
  return nullptr;
}

T2O_HD long long refine_ws_bytes(const RefineJob& j) { return (long long)kRefineWsPerPixel * refine_plane(j); }

}  // namespace t2o
