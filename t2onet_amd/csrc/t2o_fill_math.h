// The block programs of the FILL kernels (t2o_fill.hip): a region of a photo removed by a push-pull fill -- the pixels
// under a plane are replaced by a smooth continuation of the pixels around them.  Integers throughout; the definition
// stands in full in include/t2onet_hip.h.  In short, with known(y, x) <=> M = 0 and colours carried in sixteenths:
//   PULL  C_0 = 16 P where known; a cell of level k+1 is the rounded mean of its KNOWN children (2y+a, 2x+b), known when
//         it has one; levels halve (rounding up) down to 1 x 1 = level K.
//   PUSH  F_K = C_K; F_k = C_k where the cell is known, else the 9/3/3/1 tent over F_{k+1}.
//   out = P where M = 0, else (P (255 - M) + ((F_0 + 8) >> 4) M + 127) // 255; out = P everywhere when the top cell is unknown.
//
// THREE launches, each covering every job of the call, whatever the pictures hold:
//   PULL   a workgroup owns kFillTile x kFillTile pixels (tiles start at multiples of 64, so every child pair stays inside a
//          tile up to level 6).  `stage`: a thread takes 4 neighbouring pixels of two rows (12-byte groups through aligned
//          dwords, funnel-shifted; single bytes at a row's end) and makes two cells of level 1; `level`: levels 2..6 in LDS;
//          `store`: levels 1..min(6, K) go to the workspace, 8 bytes per cell (3 x uint16 colour + known).
//   TOP    ONE workgroup per job: levels 7..K pulled and levels K..6 pushed through the workspace, a level per phase; it
//          leaves F_6 (F_K when K < 6).  The "empty" flag is the known field of C_K's one cell.
//   PUSH   a workgroup per tile.  It reads its plane bytes; a tile without a byte > 0, or any tile of an empty job, copies
//          its photo bytes (returns at once when the job is in place).  Otherwise it reads the 3 x 3 neighbourhood of F_6
//          and C_5..C_1 with a ONE-CELL halo from the workspace, pushes down in LDS and writes the blended bytes: aligned
//          dwords, single bytes at the two ends of a misaligned row range.
//
// WHY ONE CELL OF HALO.  A tile's origin at level k < 6 is even.  The halo cell in front of it (odd) has Y = y >> 1 in the
// halo of level k+1 and leans to Yn = Y + 1, inside the tile; the one behind it (even) leans to Yn = Y - 1, inside again;
// a clamp at the frame keeps Yn = Y.  So every cell of a level's haloed region reads only the haloed region above it.
//
// VISIBILITY.  PULL and PUSH read what an earlier launch wrote: the kernel boundary publishes it.  TOP reads what the same
// workgroup wrote a phase earlier: every thread runs __threadfence() (write back, then invalidate this CU's L1) in front
// of the __syncthreads() that ends a phase.  F lies in arrays of its own and every array starts on a 128-byte line of its
// own, so that no line is read by the workgroup before its last write.
//
// PROGRESS.  No workgroup waits for another: no flag, no spin, no grid barrier.  Every loop bound follows from h and w
// alone.  No atomics, no float.  PUSH reads level-0 bytes (photo and plane) of its OWN tile only and writes only those of its
// own tile, every read in front of the barrier that the writes follow: a job may run in place on its photo.
//
// `__host__ __device__` programs like t2o_region_math.h's, so that tests/host_emul/emul_fill.cpp runs what the kernels run
// with g++ (a test harness, never a fallback).
#pragma once

#include "t2o_select_math.h"

namespace t2o {

constexpr int kFillMaxJobs = 4;
constexpr int kFillLaunches = 3;
constexpr int kFillTile = 64;
constexpr int kFillTileLevels = 6;                       // 64 = 2^6: the levels a tile builds alone
constexpr int kFillThreads = 256;                        // PULL and PUSH
constexpr int kFillTopThreads = 512;                     // TOP: rows of kFillTopRow lanes (no division by a size anywhere)
constexpr int kFillTopRow = 32;
constexpr int kFillMaxSide = 65535 * kFillTile;           // a grid dimension of tiles
constexpr int kFillWsAlign = 16;                         // what the caller owes
constexpr int kFillLine = 128;                           // what every array gets (the entry point rounds the base up)
constexpr int kFillRowDw = kFillTile * 3 / 4 + 2;        // PUSH: staged dwords of a tile row, any misalignment

static_assert(kFillTile == 1 << kFillTileLevels && kFillThreads * 16 == kFillTile * kFillTile, "tile thread map");

// a cell of a level: c0 | c1 << 16 | c2 << 32 | known << 48, colours in sixteenths (0..4080)
typedef unsigned long long FillCell;
T2O_HD int fill_ch(FillCell v, int c) { return (int)((v >> (16 * c)) & 0xffffu); }
T2O_HD bool fill_known(FillCell v) { return (v >> 48) != 0; }
T2O_HD FillCell fill_pack(int c0, int c1, int c2, int known) {
  return (FillCell)(unsigned)c0 | (FillCell)(unsigned)c1 << 16 | (FillCell)(unsigned)c2 << 32 | (FillCell)(unsigned)known << 48;
}

// one job as the kernels see it
struct FillJob {
  long long photo_offset, plane_offset, out_offset;
  long long ws_offset;           // first byte of the job's arrays, counted from the workspace rounded up to 128: a multiple of 128
  int h, w;
  int K, reserved;               // the top level: the first one of 1 x 1
};

struct FillArgs {
  const unsigned char* photo;
  const unsigned char* plane;
  unsigned char* out;
  unsigned char* ws;             // rounded up to a multiple of 128
  FillJob jobs[kFillMaxJobs];
};

// ---------------------------------------------------------------- geometry
T2O_HD int fill_dim(int n, int k) { return (int)(((long long)n + ((1ll << k) - 1)) >> k); }        // ceil(n / 2^k), k <= 31
T2O_HD int fill_top_level(int h, int w) {
  int K = 0;
  while (fill_dim(h, K) > 1 || fill_dim(w, K) > 1) ++K;
  return K;
}
T2O_HD int fill_tile_top(const FillJob& j) { return j.K < kFillTileLevels ? j.K : kFillTileLevels; }  // T: the level TOP hands to PUSH
T2O_HD int fill_tiles_x(const FillJob& j) { return (j.w + kFillTile - 1) / kFillTile; }
T2O_HD int fill_tiles_y(const FillJob& j) { return (j.h + kFillTile - 1) / kFillTile; }
T2O_HD long long fill_level_bytes(const FillJob& j, int k) {
  return (8ll * fill_dim(j.h, k) * fill_dim(j.w, k) + kFillLine - 1) / kFillLine * kFillLine;
}
// the workspace of a job: C_1 .. C_K, then F_T .. F_K, every array on a line of its own
T2O_HD long long fill_c_offset(const FillJob& j, int k) {            // 1 <= k <= K + 1 (the end of the C arrays)
  long long at = 0;
  for (int i = 1; i < k; ++i) at += fill_level_bytes(j, i);
  return at;
}
T2O_HD long long fill_f_offset(const FillJob& j, int k) {            // T <= k <= K + 1 (the end of the job's arrays)
  long long at = fill_c_offset(j, j.K + 1);
  for (int i = fill_tile_top(j); i < k; ++i) at += fill_level_bytes(j, i);
  return at;
}
T2O_HD long long fill_ws_bytes(const FillJob& j) { return fill_f_offset(j, j.K + 1); }
T2O_HD FillCell* fill_c(const FillJob& j, unsigned char* ws, int k) { return reinterpret_cast<FillCell*>(ws + j.ws_offset + fill_c_offset(j, k)); }
T2O_HD FillCell* fill_f(const FillJob& j, unsigned char* ws, int k) { return reinterpret_cast<FillCell*>(ws + j.ws_offset + fill_f_offset(j, k)); }

// ---------------------------------------------------------------- the two stencils
// (s + n // 2) // n for 1 <= n <= 4 without a division by a run-time value
T2O_HD int fill_div(int s, int n) { return n == 1 ? s : n == 2 ? (s + 1) >> 1 : n == 3 ? (s + 1) / 3 : (s + 2) >> 2; }

// the rounded mean of the known ones among four children (a child outside the level: 0, which is unknown)
T2O_HD FillCell fill_mean(FillCell a, FillCell b, FillCell c, FillCell d) {
  const FillCell v[4] = {a, b, c, d};
  int n = 0, s[3] = {0, 0, 0};
  T2O_UNROLL
  for (int i = 0; i < 4; ++i)
    if (fill_known(v[i])) {
      ++n;
      T2O_UNROLL
      for (int c3 = 0; c3 < 3; ++c3) s[c3] += fill_ch(v[i], c3);
    }
  return n ? fill_pack(fill_div(s[0], n), fill_div(s[1], n), fill_div(s[2], n), 1) : 0;
}

// U_k(y, x): the 9/3/3/1 tent over F_{k+1}, an (hh, ww) level of which F holds a window: cell (Y, X) at F[(Y - oy) stride + X - ox]
T2O_HD FillCell fill_tent(const FillCell* F, int stride, int oy, int ox, int hh, int ww, int y, int x) {
  const int Y = y >> 1, X = x >> 1;
  int Yn = Y + ((y & 1) ? 1 : -1), Xn = X + ((x & 1) ? 1 : -1);
  Yn = Yn < 0 ? 0 : Yn > hh - 1 ? hh - 1 : Yn;
  Xn = Xn < 0 ? 0 : Xn > ww - 1 ? ww - 1 : Xn;
  const FillCell a = F[(Y - oy) * stride + X - ox], b = F[(Y - oy) * stride + Xn - ox];
  const FillCell c = F[(Yn - oy) * stride + X - ox], d = F[(Yn - oy) * stride + Xn - ox];
  int u[3];
  T2O_UNROLL
  for (int c3 = 0; c3 < 3; ++c3) u[c3] = (9 * fill_ch(a, c3) + 3 * fill_ch(b, c3) + 3 * fill_ch(c, c3) + fill_ch(d, c3) + 8) >> 4;
  return fill_pack(u[0], u[1], u[2], 0);
}

// ---------------------------------------------------------------- PULL
constexpr int fill_pull_off(int k) { return k <= 1 ? 0 : fill_pull_off(k - 1) + (kFillTile >> (k - 1)) * (kFillTile >> (k - 1)); }

struct FillPullLds {
  FillCell lv[fill_pull_off(kFillTileLevels + 1)];       // levels 1..6 of the tile: 1024 + 256 + 64 + 16 + 4 + 1 cells
};

// four neighbouring pixels of row y from x on: the photo's 12 bytes and the plane's 4; `in` = how many lie inside (0..4)
T2O_HD int fill_load4(const FillJob& j, const unsigned char* photo, const unsigned char* plane, int y, int x, unsigned (&rgb)[3], unsigned& m) {
  rgb[0] = rgb[1] = rgb[2] = 0u;
  m = 0u;
  if (y >= j.h || x >= j.w) return 0;
  const long long n = (long long)j.h * j.w, p = (long long)y * j.w + x;
  if (x + 4 <= j.w) {
    select_load<3>(photo + 3 * p, photo, photo + 3 * n, rgb);
    unsigned one[1];
    select_load<1>(plane + p, plane, plane + n, one);
    m = one[0];
    return 4;
  }
  const int in = j.w - x;
  for (int k = 0; k < 3 * in; ++k) rgb[k >> 2] |= (unsigned)photo[3 * p + k] << (8 * (k & 3));
  for (int k = 0; k < in; ++k) m |= (unsigned)plane[p + k] << (8 * k);
  return in;
}
T2O_HD int fill_byte(const unsigned (&rgb)[3], int px, int c) { return (int)((rgb[(3 * px + c) >> 2] >> (8 * ((3 * px + c) & 3))) & 0xffu); }

// level 1 of the tile from the photo and the plane: thread work item = (row cy of level 1, group g of two cells)
T2O_HD void fill_pull_stage(const FillJob& j, const unsigned char* photo_base, const unsigned char* plane_base, int tx, int ty, int tid, FillPullLds& lds) {
  const int x0 = tx * kFillTile, y0 = ty * kFillTile;
  const unsigned char* photo = photo_base + j.photo_offset;
  const unsigned char* plane = plane_base + j.plane_offset;
  constexpr int kGroups = kFillTile / 4, kHalf = kFillTile / 2;
  for (int it = tid; it < kHalf * kGroups; it += kFillThreads) {
    const int cy = it / kGroups, g = it % kGroups;
    int n[2] = {0, 0}, s[2][3] = {{0, 0, 0}, {0, 0, 0}};
    T2O_UNROLL
    for (int r = 0; r < 2; ++r) {
      unsigned rgb[3], m;
      const int in = fill_load4(j, photo, plane, y0 + 2 * cy + r, x0 + 4 * g, rgb, m);
      T2O_UNROLL
      for (int px = 0; px < 4; ++px)
        if (px < in && ((m >> (8 * px)) & 0xffu) == 0u) {
          ++n[px >> 1];
          T2O_UNROLL
          for (int c = 0; c < 3; ++c) s[px >> 1][c] += 16 * fill_byte(rgb, px, c);
        }
    }
    T2O_UNROLL
    for (int b = 0; b < 2; ++b) {
      lds.lv[cy * kHalf + 2 * g + b] = n[b] ? fill_pack(fill_div(s[b][0], n[b]), fill_div(s[b][1], n[b]), fill_div(s[b][2], n[b]), 1) : 0;
    }
  }
}

// level k + 1 of the tile from level k, 1 <= k <= 5 (cells outside the frame are 0 = unknown in LDS)
T2O_HD void fill_pull_level(int k, int tid, FillPullLds& lds) {
  const int sh = kFillTileLevels - (k + 1), s = 1 << sh;
  const FillCell* src = lds.lv + fill_pull_off(k);
  FillCell* dst = lds.lv + fill_pull_off(k + 1);
  for (int i = tid; i < s * s; i += kFillThreads) {
    const int cy = i >> sh, cx = i & (s - 1);
    const FillCell* q = src + 2 * cy * 2 * s + 2 * cx;
    dst[i] = fill_mean(q[0], q[1], q[2 * s], q[2 * s + 1]);
  }
}

T2O_HD void fill_pull_store(const FillJob& j, unsigned char* ws, int tx, int ty, int tid, const FillPullLds& lds) {
  for (int k = 1; k <= fill_tile_top(j); ++k) {
    const int sh = kFillTileLevels - k, s = 1 << sh, hk = fill_dim(j.h, k), wk = fill_dim(j.w, k);
    FillCell* C = fill_c(j, ws, k);
    for (int i = tid; i < s * s; i += kFillThreads) {
      const int y = ty * s + (i >> sh), x = tx * s + (i & (s - 1));
      if (y < hk && x < wk) C[(long long)y * wk + x] = lds.lv[fill_pull_off(k) + i];
    }
  }
}

// ---------------------------------------------------------------- TOP (one workgroup per job; a barrier behind a fence between two calls)
// C_{k+1} from C_k in the workspace, k >= 6
T2O_HD void fill_top_pull(const FillJob& j, unsigned char* ws, int k, int tid) {
  const int hk = fill_dim(j.h, k), wk = fill_dim(j.w, k), hn = fill_dim(j.h, k + 1), wn = fill_dim(j.w, k + 1);
  const FillCell* src = fill_c(j, ws, k);
  FillCell* dst = fill_c(j, ws, k + 1);
  for (int y = tid / kFillTopRow; y < hn; y += kFillTopThreads / kFillTopRow)
    for (int x = tid % kFillTopRow; x < wn; x += kFillTopRow) {
      const bool right = 2 * x + 1 < wk, down = 2 * y + 1 < hk;
      const FillCell* q = src + 2ll * y * wk + 2 * x;
      dst[(long long)y * wn + x] = fill_mean(q[0], right ? q[1] : 0, down ? q[wk] : 0, right && down ? q[wk + 1] : 0);
    }
}

// F_K = C_K (a 1 x 1 picture has no level above 0: its cell of F is written as 0 and never read)
T2O_HD void fill_top_seed(const FillJob& j, unsigned char* ws, int tid) {
  if (tid == 0) fill_f(j, ws, j.K)[0] = j.K > 0 ? fill_c(j, ws, j.K)[0] : 0;
}

// F_k from C_k and F_{k+1} in the workspace, K > k >= 6
T2O_HD void fill_top_push(const FillJob& j, unsigned char* ws, int k, int tid) {
  const int hk = fill_dim(j.h, k), wk = fill_dim(j.w, k), hn = fill_dim(j.h, k + 1), wn = fill_dim(j.w, k + 1);
  const FillCell* C = fill_c(j, ws, k);
  const FillCell* up = fill_f(j, ws, k + 1);
  FillCell* F = fill_f(j, ws, k);
  for (int y = tid / kFillTopRow; y < hk; y += kFillTopThreads / kFillTopRow)
    for (int x = tid % kFillTopRow; x < wk; x += kFillTopRow) {
      const FillCell c = C[(long long)y * wk + x];
      F[(long long)y * wk + x] = fill_known(c) ? c : fill_tent(up, wn, 0, 0, hn, wn, y, x);
    }
}

// ---------------------------------------------------------------- PUSH
constexpr int fill_push_side(int k) { return (kFillTile >> k) + 2; }
constexpr int fill_push_off(int k) { return k <= 1 ? 0 : fill_push_off(k - 1) + fill_push_side(k - 1) * fill_push_side(k - 1); }

struct FillPushLds {
  FillCell f[fill_push_off(kFillTileLevels + 1)];        // F_1..F_6 of the tile with one cell of halo: 34^2 + 18^2 + 10^2 + 6^2 + 4^2 + 3^2
  unsigned ob[kFillTile * kFillRowDw];                   // the tile's output bytes, row by row, each at its global misalignment
  unsigned m[kFillTile * kFillTile / 4];                 // the tile's plane bytes
  int any;                                               // a plane byte > 0 in the tile
};

T2O_HD bool fill_in_place(const FillArgs& a, const FillJob& j) { return a.out + j.out_offset == a.photo + j.photo_offset; }
// the "empty" flag: no pixel of the picture has M = 0 (a 1 x 1 picture comes out as it is, known or not)
T2O_HD bool fill_empty(const FillJob& j, unsigned char* ws) { return j.K == 0 || !fill_known(fill_c(j, ws, j.K)[0]); }

// phase 0: the plane bytes of the tile into LDS; lds.any (cleared before) set where one is > 0
T2O_HD void fill_push_plane(const FillJob& j, const unsigned char* plane_base, int tx, int ty, int tid, FillPushLds& lds) {
  const int x0 = tx * kFillTile, y0 = ty * kFillTile;
  const unsigned char* plane = plane_base + j.plane_offset;
  const long long n = (long long)j.h * j.w;
  for (int it = tid; it < kFillTile * kFillTile / 4; it += kFillThreads) {
    const int y = y0 + it / (kFillTile / 4), x = x0 + it % (kFillTile / 4) * 4;
    unsigned m = 0u;
    if (y < j.h && x + 4 <= j.w) {
      unsigned one[1];
      const long long p = (long long)y * j.w + x;
      select_load<1>(plane + p, plane, plane + n, one);
      m = one[0];
    } else if (y < j.h) {
      for (int k = 0; x + k < j.w && k < 4; ++k) m |= (unsigned)plane[(long long)y * j.w + x + k] << (8 * k);
    }
    lds.m[it] = m;
    if (m) lds.any = 1;
  }
}

// F_k of the tile's haloed window, k from T down to 1, one call per level with a barrier between two
T2O_HD void fill_push_level(const FillJob& j, unsigned char* ws, int k, int tx, int ty, int tid, FillPushLds& lds) {
  const int T = fill_tile_top(j);
  const int side = (kFillTile >> k) + 2, oy = ty * (kFillTile >> k) - 1, ox = tx * (kFillTile >> k) - 1;
  const int hk = fill_dim(j.h, k), wk = fill_dim(j.w, k);
  const int up_side = (kFillTile >> (k + 1)) + 2, up_oy = ty * (kFillTile >> (k + 1)) - 1, up_ox = tx * (kFillTile >> (k + 1)) - 1;
  const FillCell* src = k == T ? fill_f(j, ws, k) : fill_c(j, ws, k);
  FillCell* dst = lds.f + fill_push_off(k);
  for (int ly = tid / kFillTopRow; ly < side; ly += kFillThreads / kFillTopRow)
    for (int lx = tid % kFillTopRow; lx < side; lx += kFillTopRow) {
      const int y = oy + ly, x = ox + lx;
      if (y < 0 || y >= hk || x < 0 || x >= wk) continue;
      const FillCell c = src[(long long)y * wk + x];
      dst[ly * side + lx] = k == T || fill_known(c) ? c
                                                    : fill_tent(lds.f + fill_push_off(k + 1), up_side, up_oy, up_ox, fill_dim(j.h, k + 1), fill_dim(j.w, k + 1), y, x);
    }
}

// the tile's output bytes into lds.ob; plain: a copy of the photo
T2O_HD void fill_push_blend(const FillArgs& a, const FillJob& j, int tx, int ty, int tid, bool plain, FillPushLds& lds) {
  const int x0 = tx * kFillTile, y0 = ty * kFillTile;
  const unsigned char* photo = a.photo + j.photo_offset;
  const unsigned char* dst = a.out + j.out_offset;
  const long long n = (long long)j.h * j.w;
  unsigned char* ob = reinterpret_cast<unsigned char*>(lds.ob);
  const int side = kFillTile / 2 + 2, oy = ty * (kFillTile / 2) - 1, ox = tx * (kFillTile / 2) - 1;
  const int h1 = fill_dim(j.h, 1), w1 = fill_dim(j.w, 1);
  for (int it = tid; it < kFillTile * kFillTile / 4; it += kFillThreads) {
    const int r = it / (kFillTile / 4), y = y0 + r, x = x0 + it % (kFillTile / 4) * 4;
    if (y >= j.h || x >= j.w) continue;
    const long long p = (long long)y * j.w + x;
    const int in = x + 4 <= j.w ? 4 : j.w - x;
    unsigned rgb[3] = {0u, 0u, 0u};
    if (in == 4) {
      select_load<3>(photo + 3 * p, photo, photo + 3 * n, rgb);
    } else {
      for (int k = 0; k < 3 * in; ++k) rgb[k >> 2] |= (unsigned)photo[3 * p + k] << (8 * (k & 3));
    }
    const unsigned m4 = lds.m[it];
    unsigned char* o = ob + r * (kFillRowDw * 4) + replay_misalign(dst + 3 * ((long long)y * j.w + x0)) + 3 * (x - x0);
    for (int px = 0; px < in; ++px) {
      const int m = (int)((m4 >> (8 * px)) & 0xffu);
      if (m == 0 || plain) {
        for (int c = 0; c < 3; ++c) o[3 * px + c] = (unsigned char)fill_byte(rgb, px, c);
      } else {
        const FillCell u = fill_tent(lds.f, side, oy, ox, h1, w1, y, x + px);
        for (int c = 0; c < 3; ++c) {
          const int fill = (fill_ch(u, c) + 8) >> 4;
          o[3 * px + c] = (unsigned char)((fill_byte(rgb, px, c) * (255 - m) + fill * m + 127) / 255);
        }
      }
    }
  }
}

// lds.ob to the destination: aligned dwords, single bytes at the two ends of a misaligned row range
T2O_HD void fill_push_store(const FillArgs& a, const FillJob& j, int tx, int ty, int tid, const FillPushLds& lds) {
  const int x0 = tx * kFillTile, y0 = ty * kFillTile;
  const int nb = 3 * (j.w - x0 < kFillTile ? j.w - x0 : kFillTile);
  for (int i = tid; i < kFillTile * kFillRowDw; i += kFillThreads) {
    const int r = i / kFillRowDw, d = i % kFillRowDw, y = y0 + r;
    if (y >= j.h) continue;
    unsigned char* row = a.out + j.out_offset + 3 * ((long long)y * j.w + x0);
    const int lo = 4 * d - (int)replay_misalign(row);      // this dword's first byte, counted from the row range's first
    if (lo + 4 <= 0 || lo >= nb) continue;
    const unsigned v = lds.ob[i];
    if (lo >= 0 && lo + 4 <= nb) {
      replay_store_dword(row + lo, v);
    } else {
      for (int b = 0; b < 4; ++b)
        if (lo + b >= 0 && lo + b < nb) row[lo + b] = (unsigned char)(v >> (8 * b));
    }
  }
}

// Host side: the checks of the C ABI on one job and the kernels' copy of it.  Returns nullptr or the reason for T2O_EINVAL.
inline const char* fill_prepare(FillJob& d, long long photo_offset, long long plane_offset, long long out_offset, int h, int w, long long ws_offset) {
  if (h <= 0 || w <= 0) return "fill_u8: h and w must be positive";
  if (3ll * h * w >= (1ll << 31)) return "fill_u8: 3 * h * w must stay below 2^31";
  if (h > kFillMaxSide || w > kFillMaxSide) return "fill_u8: h and w may not exceed 4194240 (65535 tiles)";
  if (photo_offset < 0 || plane_offset < 0 || out_offset < 0) return "fill_u8: negative offset";
  d.photo_offset = photo_offset; d.plane_offset = plane_offset; d.out_offset = out_offset; d.ws_offset = ws_offset;
  d.h = h; d.w = w;
  d.K = fill_top_level(h, w); d.reserved = 0;
  return nullptr;
}

}  // namespace t2o
