// The lane and block programs of the REGION kernels (t2o_region.hip): the magic wand of a local edit -- the connected
// region around a seed pixel, labelled on the device by union-find.  Integers throughout (include/t2onet_hip.h states the
// definition in full): with (Rs, Gs, Bs) the photo's bytes at the seed, READ ON THE DEVICE,
//   pass(y, x) <=> max(|R - Rs|, |G - Gs|, |B - Bs|) <= tol          (the seed always passes)
//   out(y, x)  =  255 where (y, x) is joined to the seed by a path of passing pixels (4- or 8-connected steps), else 0.
//
// The parent array L is one int32 per pixel, indexed i = y w + x: L[i] < 0 marks a pixel that does not pass, L[i] == i a
// root, and always L[i] <= i -- a link only ever points DOWN.  THREE launches, each covering every job of the call:
//   TILE     a workgroup owns kRegionTile x kRegionTile pixels.  `stage`: a thread takes 16 neighbouring pixels of a tile
//            row, computes pass from the photo's bytes (12-byte groups through aligned dwords, funnel-shifted; single
//            bytes at a row's end) and labels each with the start of its run (LDS).  `link`: the runs are joined across
//            the 16-pixel seams and with the row above (and its diagonals for 8) by min-index unions on LDS.  `store`:
//            every pixel's parent becomes the GLOBAL index of its tile-local root (row-major in the tile and in the frame,
//            so smaller stays smaller); plain stores -- no other workgroup touches these words in this launch.
//   BORDER   one lane per pixel of a tile's top row and left column: unions with the passing neighbours across the tile
//            edge in the global array.  Lock-free: find both roots, atomicMin the larger root's word to the smaller, and
//            where that word was no root any more continue with the value it held.
//   RESOLVE  one lane per workgroup finds the seed's root and shares it through LDS; then lane q owns the ALIGNED
//            destination dword q as t2o_select_math.h's lane does: finds the roots of its four pixels, compares, stores
//            one dword -- single bytes at the two ends of a misaligned plane.
//
// VISIBILITY.  In BORDER and RESOLVE other workgroups write words of L (unions, path compression), so EVERY access to L
// there is an agent-scope relaxed atomic (region_ld / region_min under RegionGlobal): the loads are served by L2, never by a
// CU's L1.  TILE writes L with plain stores and reads nothing of it; the kernel boundary publishes them.
//
// PROGRESS.  No workgroup ever waits for another one: there is no flag, spin, hand-off or grid barrier, and every loop has a
// measure that falls whatever the other workgroups do and however old a value a load returns:
//   find      follows i -> L[i] only while 0 <= L[i] < i: the index falls strictly, at most i steps.  Every value a word i has
//             ever held is <= i, so a stale value changes the answer (an older ancestor) but never the bound.
//   union     holds a pair (a, b), a > b.  atomicMin(L[a], b) returns the word's true old value; old == a: a was a root and
//             is linked now, the union is done; otherwise the word keeps min(old, b) and the union goes on as (old, b) with
//             old < a strictly.  max(a, b) falls in every round and finds only lower a and b: at most a + b rounds.
//   compress  lowers a word on a walked path to the root found at the end of that path -- an ancestor -- and only by
//             atomicMin, walking down with the same strict test as find.
// So L[i] <= i always holds, a word only falls, and no link ever joins two components that the unions do not join: two
// pixels end under one root exactly when a chain of unions joins them.  A bug here can give wrong bytes, never a hang.
//
// DETERMINISM.  A root is the smallest index of its component (every member's chain falls to it), whatever the order of
// arrival, so the final ROOTS and the output bytes are deterministic; the other words of L are not.
//
// Like t2o_refine_math.h these are `__host__ __device__` programs, so that tests/host_emul/emul_region.cpp runs what the
// kernels run with g++ (a test harness, never a fallback); there RegionGlobal / RegionLocal are plain loads and a plain
// minimum.  Workspace: L alone, 4 bytes per pixel, each job's rounded up to 16 bytes (kRegionWsAlign).  No float.
#pragma once

#include "t2o_select_math.h"

namespace t2o {

constexpr int kRegionMaxJobs = 4;                        // = kSelectMaxJobs: the planes of one local edit
constexpr int kRegionLaunches = 3;
constexpr int kRegionTile = 64;                          // a tile is 64 x 64 pixels: 16 KB of labels in LDS
constexpr int kRegionTilePx = kRegionTile * kRegionTile;
constexpr int kRegionThreads = 256;                      // TILE and RESOLVE
constexpr int kRegionSeg = 16;                           // pixels of a tile row per thread in TILE
constexpr int kRegionBorderThreads = 2 * kRegionTile;    // BORDER: the top row, then the left column
constexpr int kRegionIter = 4;                           // RESOLVE: dwords per lane, kRegionThreads apart
constexpr int kRegionOutDw = kRegionThreads * kRegionIter;
constexpr int kRegionWsAlign = 16;

static_assert(kRegionTilePx == kRegionThreads * kRegionSeg && kRegionTile % kRegionSeg == 0 && kRegionSeg % 4 == 0, "tile pass thread map");

// one job as the kernels see it
struct RegionJob {
  long long photo_offset, out_offset;
  long long ws_offset;           // first byte of the job's parent array, counted from the workspace; a multiple of 16
  int h, w;
  int seed;                      // seed_y * w + seed_x
  int tol, conn, reserved;
};

struct RegionArgs {
  const unsigned char* photo;
  unsigned char* out;
  unsigned char* ws;
  RegionJob jobs[kRegionMaxJobs];
};

struct RegionLds {
  int lab[kRegionTilePx];        // TILE: the tile-local parent of each pixel, -1 where it does not pass or lies outside
};

// ---------------------------------------------------------------- the memory layer
// What another workgroup may write during a launch: agent scope, relaxed.
struct RegionGlobal {};
struct RegionLocal {};                                   // the labels of a tile in LDS: the same operations at workgroup scope

T2O_HD int region_ld(RegionGlobal, const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
T2O_HD int region_min(RegionGlobal, int* p, int v) {     // the old value
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  const int old = *p;
  if (v < old) *p = v;
  return old;
#endif
}
T2O_HD int region_ld(RegionLocal, const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
  return *p;
#endif
}
T2O_HD int region_min(RegionLocal, int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
  const int old = *p;
  if (v < old) *p = v;
  return old;
#endif
}

// ---------------------------------------------------------------- union-find (the progress argument is at the top)
template <class M>
T2O_HD int region_find(const int* L, int i) {
  for (;;) {
    const int p = region_ld(M(), L + i);
    if (p < 0 || p >= i) return i;                       // a root (or a word that is none of ours: stop)
    i = p;                                               // strictly smaller
  }
}

// the root of i; the words on the way are lowered to it
template <class M>
T2O_HD int region_find_compress(int* L, int i) {
  const int r = region_find<M>(L, i);
  while (i > r) {
    const int p = region_ld(M(), L + i);
    if (p < 0 || p >= i) break;
    if (p > r) region_min(M(), L + i, r);
    i = p;                                               // strictly smaller
  }
  return r;
}

template <class M>
T2O_HD void region_union(int* L, int a, int b) {
  for (;;) {
    a = region_find<M>(L, a);
    b = region_find<M>(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = region_min(M(), L + a, b);                    // L[a] = min(L[a], b)
    if (old >= a) return;                                // a was a root: linked
    a = old;                                             // strictly smaller; (old, b) remain to be joined
  }
}

T2O_HD bool region_pass(int r, int g, int b, int rs, int gs, int bs, int tol) {
  const int dr = r > rs ? r - rs : rs - r, dg = g > gs ? g - gs : gs - g, db = b > bs ? b - bs : bs - b;
  return (dr > dg ? (dr > db ? dr : db) : (dg > db ? dg : db)) <= tol;
}

// ---------------------------------------------------------------- geometry
T2O_HD int region_tiles_x(const RegionJob& j) { return (j.w + kRegionTile - 1) / kRegionTile; }
T2O_HD int region_tiles(const RegionJob& j) { return region_tiles_x(j) * ((j.h + kRegionTile - 1) / kRegionTile); }
T2O_HD int* region_parents(const RegionJob& j, unsigned char* ws) { return reinterpret_cast<int*>(ws + j.ws_offset); }
T2O_HD long long region_ws_bytes(const RegionJob& j) {
  return (4ll * j.h * j.w + kRegionWsAlign - 1) / kRegionWsAlign * kRegionWsAlign;
}

// ---------------------------------------------------------------- TILE
T2O_HD void region_tile_stage(const RegionJob& j, const unsigned char* photo_base, int tile, int tid, RegionLds& lds) {
  const int x0 = tile % region_tiles_x(j) * kRegionTile, y0 = tile / region_tiles_x(j) * kRegionTile;
  const int row = tid / (kRegionTile / kRegionSeg), lx0 = tid % (kRegionTile / kRegionSeg) * kRegionSeg;
  const int y = y0 + row;
  const long long n = (long long)j.h * j.w;
  const unsigned char* photo = photo_base + j.photo_offset;
  const int rs = photo[3ll * j.seed], gs = photo[3ll * j.seed + 1], bs = photo[3ll * j.seed + 2];
  int run = -1;                                          // the first pixel of the run that the last pixel was in
  for (int g = 0; g < kRegionSeg; g += 4) {
    const int x = x0 + lx0 + g;
    unsigned rgb[3] = {0u, 0u, 0u};
    const long long p = (long long)y * j.w + x;
    if (y < j.h && x + 4 <= j.w) {
      select_load<3>(photo + 3 * p, photo, photo + 3 * n, rgb);
    } else if (y < j.h) {
      for (int k = 0; k < 12 && x + k / 3 < j.w; ++k) rgb[k >> 2] |= (unsigned)photo[3 * p + k] << (8 * (k & 3));
    }
    T2O_UNROLL
    for (int b = 0; b < 4; ++b) {
      int c[3];
      T2O_UNROLL
      for (int k = 0; k < 3; ++k) c[k] = (int)((rgb[(3 * b + k) >> 2] >> (8 * ((3 * b + k) & 3))) & 0xffu);
      const int li = row * kRegionTile + lx0 + g + b;
      const bool ok = y < j.h && x + b < j.w && region_pass(c[0], c[1], c[2], rs, gs, bs, j.tol);
      run = ok ? (run < 0 ? li : run) : -1;
      lds.lab[li] = run;
    }
  }
}

// What has to be joined by hand: a run with the one in front of the thread's seam, a pixel with the row above.  A union is
// left out where two others of this phase give it: i - left - upleft - up (left and upleft join as the column before).
T2O_HD void region_tile_link(const RegionJob& j, int tid, RegionLds& lds) {
  const int row = tid / (kRegionTile / kRegionSeg), lx0 = tid % (kRegionTile / kRegionSeg) * kRegionSeg;
  int* lab = lds.lab;
  for (int k = 0; k < kRegionSeg; ++k) {
    const int lx = lx0 + k, li = row * kRegionTile + lx;
    if (region_ld(RegionLocal(), lab + li) < 0) continue;
    const bool left = lx > 0 && region_ld(RegionLocal(), lab + li - 1) >= 0;
    if (k == 0 && left) region_union<RegionLocal>(lab, li, li - 1);
    if (row == 0) continue;
    const bool up = region_ld(RegionLocal(), lab + li - kRegionTile) >= 0;
    const bool ul = lx > 0 && region_ld(RegionLocal(), lab + li - kRegionTile - 1) >= 0;
    if (up) {
      if (!(left && ul)) region_union<RegionLocal>(lab, li, li - kRegionTile);
    } else if (j.conn == 8) {
      if (ul && !left) region_union<RegionLocal>(lab, li, li - kRegionTile - 1);
      if (lx + 1 < kRegionTile && region_ld(RegionLocal(), lab + li - kRegionTile + 1) >= 0) region_union<RegionLocal>(lab, li, li - kRegionTile + 1);
    }
  }
}

T2O_HD void region_tile_store(const RegionJob& j, unsigned char* ws, int tile, int tid, RegionLds& lds) {
  const int x0 = tile % region_tiles_x(j) * kRegionTile, y0 = tile / region_tiles_x(j) * kRegionTile;
  int* L = region_parents(j, ws);
  for (int li = tid; li < kRegionTilePx; li += kRegionThreads) {
    const int y = y0 + li / kRegionTile, x = x0 + li % kRegionTile;
    if (y >= j.h || x >= j.w) continue;
    int v = -1;
    if (region_ld(RegionLocal(), lds.lab + li) >= 0) {
      const int r = region_find_compress<RegionLocal>(lds.lab, li);
      v = (y0 + r / kRegionTile) * j.w + x0 + r % kRegionTile;
    }
    L[y * j.w + x] = v;
  }
}

// ---------------------------------------------------------------- BORDER
// Lane tid < kRegionTile: pixel tid of the tile's top row against the row above; the other lanes: the left column against
// the column in front of it.  Every pair of passing neighbours that a tile edge parts is joined here, by hand or -- as in
// region_tile_link -- by two other unions of this launch and links that TILE left inside one tile.
T2O_HD void region_border_lane(const RegionJob& j, unsigned char* ws, int tile, int tid) {
  const int x0 = tile % region_tiles_x(j) * kRegionTile, y0 = tile / region_tiles_x(j) * kRegionTile;
  int* L = region_parents(j, ws);
  const int w = j.w, h = j.h;
  if (tid < kRegionTile) {
    const int x = x0 + tid, y = y0;
    if (y == 0 || x >= w) return;
    const int i = y * w + x;
    if (region_ld(RegionGlobal(), L + i) < 0) return;
    const bool left = x > 0 && region_ld(RegionGlobal(), L + i - 1) >= 0;
    const bool up = region_ld(RegionGlobal(), L + i - w) >= 0;
    const bool ul = x > 0 && region_ld(RegionGlobal(), L + i - w - 1) >= 0;
    if (up) {
      if (!(left && ul && tid > 0)) region_union<RegionGlobal>(L, i, i - w);
    } else if (j.conn == 8) {
      if (ul && !(left && tid > 0)) region_union<RegionGlobal>(L, i, i - w - 1);
      if (x + 1 < w && region_ld(RegionGlobal(), L + i - w + 1) >= 0) region_union<RegionGlobal>(L, i, i - w + 1);
    }
  } else {
    const int ly = tid - kRegionTile, x = x0, y = y0 + ly;
    if (x == 0 || y >= h) return;
    const int i = y * w + x;
    if (region_ld(RegionGlobal(), L + i) < 0) return;
    const bool left = region_ld(RegionGlobal(), L + i - 1) >= 0;
    const bool up = y > 0 && region_ld(RegionGlobal(), L + i - w) >= 0;
    const bool ul = y > 0 && region_ld(RegionGlobal(), L + i - w - 1) >= 0;
    if (left) {
      if (!(up && ul && ly > 0)) region_union<RegionGlobal>(L, i, i - 1);
    } else if (j.conn == 8) {
      if (ul && !(up && ly > 0)) region_union<RegionGlobal>(L, i, i - w - 1);
      if (y + 1 < h && region_ld(RegionGlobal(), L + i + w - 1) >= 0) {
        const bool down = ly + 1 < kRegionTile && region_ld(RegionGlobal(), L + i + w) >= 0;       // (it joins its own left by hand)
        if (!down) region_union<RegionGlobal>(L, i, i + w - 1);
      }
    }
  }
}

// ---------------------------------------------------------------- RESOLVE
T2O_HD int region_seed_root(const RegionJob& j, unsigned char* ws) { return region_find<RegionGlobal>(region_parents(j, ws), j.seed); }

// aligned destination dwords that hold a byte of the job's plane
T2O_HD int region_dwords(const RegionJob& j, const unsigned char* out) {
  return (int)(((long long)replay_misalign(out + j.out_offset) + (long long)j.h * j.w + 3) / 4);
}

T2O_HD int region_out_tiles(const RegionJob& j, const unsigned char* out) { return (region_dwords(j, out) + kRegionOutDw - 1) / kRegionOutDw; }

T2O_HD void region_resolve_lane(const RegionJob& j, unsigned char* ws, unsigned char* out, int q, int root) {
  const int n = j.h * j.w;                                           // < 2^31
  int* L = region_parents(j, ws);
  unsigned char* plane = out + j.out_offset;
  const int p0 = (int)(4ll * q - (long long)replay_misalign(plane)); // the lane's first pixel (< n); its dword is plane + p0, aligned
  const bool whole = p0 >= 0 && p0 <= n - 4;
  unsigned word = 0;
  for (int b = 0; b < 4; ++b) {
    const long long p = (long long)p0 + b;
    if (p < 0 || p >= n) continue;
    const int l = region_ld(RegionGlobal(), L + p);
    if (l < 0) continue;
    // the pixel's own word is read by this lane alone: the walk starts, and compresses, at its parent
    if (l == root || region_find_compress<RegionGlobal>(L, l) == root) word |= 255u << (8 * b);
  }
  if (whole) {
    replay_store_dword(plane + p0, word);
  } else {
    for (int b = 0; b < 4; ++b)
      if ((long long)p0 + b >= 0 && (long long)p0 + b < n) plane[(long long)p0 + b] = (unsigned char)(word >> (8 * b));
  }
}

// what thread `tid` of workgroup (block_x, block_y) of the grid (max tiles over the jobs, J) does behind the barrier
T2O_HD void region_resolve_thread(const RegionArgs& a, int block_x, int block_y, int tid, int root) {
  const RegionJob& j = a.jobs[block_y];
  const int dwords = region_dwords(j, a.out);
  int q = block_x * kRegionOutDw + tid;                              // < 2^29 + 1024
  for (int i = 0; i < kRegionIter; ++i, q += kRegionThreads)
    if (q < dwords) region_resolve_lane(j, a.ws, a.out, q, root);
}

// Host side: the checks of the C ABI on one job and the kernels' copy of it.  Returns nullptr or the reason for T2O_EINVAL.
inline const char* region_prepare(RegionJob& d, long long photo_offset, long long out_offset, int h, int w, int seed_x, int seed_y,
                                  int tol, int conn, long long ws_offset) {
  if (h <= 0 || w <= 0) return "region_u8: h and w must be positive";
  if ((long long)h * w >= (1ll << 31)) return "region_u8: h * w must stay below 2^31";
  if (photo_offset < 0 || out_offset < 0) return "region_u8: negative offset";
  if (seed_x < 0 || seed_x >= w || seed_y < 0 || seed_y >= h) return "region_u8: the seed must lie inside the frame";
  if (tol < 0 || tol > 255) return "region_u8: tol must lie in 0..255";
  if (conn != 4 && conn != 8) return "region_u8: conn must be 4 or 8";
  d.photo_offset = photo_offset; d.out_offset = out_offset; d.ws_offset = ws_offset;
  d.h = h; d.w = w;
  d.seed = seed_y * w + seed_x;
  d.tol = tol; d.conn = conn; d.reserved = 0;
  return nullptr;
}

}  // namespace t2o
