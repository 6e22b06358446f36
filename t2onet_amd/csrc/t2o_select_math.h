// The programs of the SELECTION kernel (t2o_select.hip): the uint8 mask plane of a local edit computed from a RULE -- a
// range of luminance, saturation or hue of the photo's own bytes, a linear or radial gradient over the frame, an
// existing plane -- instead of being painted and uploaded.  Integer arithmetic throughout, floor divisions of
// non-negative integers, so that numpy, g++ and gfx950 agree byte for byte (include/t2onet_hip.h states the definition
// in full).  A selection is 1..4 terms; term k gives t_k in 0..255 (255 - t_k when inverted); m = t_1, then
// m = (m * t_k + 127) / 255.
//
// Like t2o_feather_math.h these are `__host__ __device__` programs, so that tests/host_emul/emul_select.cpp runs what
// the kernel runs with g++ (a test harness, never a fallback):
//   select_pixel   the PER-PIXEL program: one pixel's bytes, its position and the bytes of the job's plane terms -> m
//   select_lane    the LANE program: a plane is a stream of h * w pixels; lane q owns the ALIGNED destination dword q
//                  of the plane, i.e. pixels 4q - a .. 4q - a + 3 with a = the destination's address modulo 4.  It
//                  reads their 12 source bytes (any alignment: aligned dwords funnel-shifted by the source's address
//                  modulo 4, which is the same for every lane of a job) and one dword per plane term the same way,
//                  runs select_pixel four times and stores one dword.  The first and the last lane of a misaligned
//                  plane hold pixels outside it: those lanes read and write single bytes, so no byte outside a photo,
//                  a plane term or a destination plane is touched.  y and x are made (one division per lane) only when
//                  the job has a position term.
// 3 + 1 bytes of traffic per pixel plus 1 per plane term -- 1 + plane terms where the job has no colour term, the photo
// then is not read; no LDS, no barrier, no float, no atomics.
#pragma once

#include "t2o_replay_math.h"

namespace t2o {

constexpr int kSelectMaxJobs = 4;                        // = kReplayMaxMasks = kFeatherMaxJobs: the planes of one local edit
constexpr int kSelectMaxTerms = 4;
constexpr int kSelectThreads = 256;
constexpr int kSelectIter = 4;                           // dwords per lane, kSelectThreads apart
constexpr int kSelectTileDw = kSelectThreads * kSelectIter;
constexpr int kSelectTilePx = 4 * kSelectTileDw;         // 4096 pixels of the stream per workgroup
constexpr int kSelectMaxSide = 65535;                    // h, w of a job with a position term
constexpr int kSelectMaxCoord = 2 * kSelectMaxSide;      // |coordinate| and radius of a position term
constexpr int kSelectHueSteps = 1536;                    // six sectors of 256

enum { SELECT_LUM = 0, SELECT_SAT = 1, SELECT_HUE = 2, SELECT_LINEAR = 3, SELECT_RADIAL = 4, SELECT_PLANE = 5, SELECT_KINDS = 6 };

// t2o_select_term_t / t2o_select_job_t of include/t2onet_hip.h, field for field
struct SelectTerm {
  int kind, invert;
  int p[4];                      // lum, sat, hue: lo, hi, soft (+ select_prepare's magic);  linear: X0, Y0, X1, Y1;  radial: CX, CY, RI, RO
  long long plane_offset;        // plane: first byte of the (h, w) plane, counted from src
};

struct SelectJob {
  long long src_offset, out_offset;
  int h, w, n_terms, reserved;
  SelectTerm terms[kSelectMaxTerms];
};

struct SelectArgs {
  const unsigned char* src;
  unsigned char* out;
  SelectJob jobs[kSelectMaxJobs];
};

// ---------------------------------------------------------------- the colour measures
T2O_HD int select_lum(int r, int g, int b) { return (69 * r + 172 * g + 15 * b + 128) >> 8; }

T2O_HD int select_sat(int r, int g, int b) {
  const int mx = r > g ? (r > b ? r : b) : (g > b ? g : b), mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
  return mx == 0 ? 0 : (int)((unsigned)(255 * (mx - mn) + mx / 2) / (unsigned)mx);
}

// 0..1535, or -1 where it is undefined (r = g = b)
T2O_HD int select_hue(int r, int g, int b) {
  const int mx = r > g ? (r > b ? r : b) : (g > b ? g : b), mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
  const int d = mx - mn;
  if (d == 0) return -1;
  const int n = mx == r ? g - b : mx == g ? b - r : r - g;
  const int base = mx == r ? 0 : mx == g ? 512 : 1024;
  const int q = (int)((unsigned)(512 * (n + d) + d) / (unsigned)(2 * d)) - 256;      // -256 .. 256
  const int hue = base + q;
  return hue < 0 ? hue + kSelectHueSteps : hue >= kSelectHueSteps ? hue - kSelectHueSteps : hue;
}

// ---------------------------------------------------------------- the weights
// The division of a ramp without a divider: floor(a / soft) = (a * magic) >> 32 with magic = floor(2^32 / soft) + 1,
// exact while a * soft < 2^32 -- here a <= 255 * 768 + 384 < 2^18 and soft <= 768.  soft <= 1 never divides (0 stands in).
inline unsigned select_magic(int soft) { return soft >= 2 ? (unsigned)((1ull << 32) / (unsigned)soft) + 1u : 0u; }

T2O_HD unsigned select_mulhi(unsigned a, unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (unsigned)(((unsigned long long)a * b) >> 32);
#endif
}

// branch-free: the middle value is computed for every distance and kept only strictly inside the ramp
T2O_HD int select_ramp(int dist, int soft, unsigned magic) {
  const unsigned mid = select_mulhi((unsigned)(255 * (soft - dist) + (soft >> 1)), magic);
  return dist <= 0 ? 255 : dist >= soft ? 0 : (int)mid;
}

T2O_HD int select_range(int v, int lo, int hi, int soft, unsigned magic) { return select_ramp(v < lo ? lo - v : v > hi ? v - hi : 0, soft, magic); }

// the arc runs upward from lo to hi modulo 1536; an undefined hue (-1) weighs 0
T2O_HD int select_hue_range(int hue, int lo, int hi, int soft, unsigned magic) {
  if (hue < 0) return 0;
  const int span = hi >= lo ? hi - lo : hi - lo + kSelectHueSteps;
  const int rel = hue >= lo ? hue - lo : hue - lo + kSelectHueSteps;
  if (rel <= span) return 255;
  const int up = rel - span, down = kSelectHueSteps - rel;          // beyond hi going up, in front of lo going down
  return select_ramp(up < down ? up : down, soft, magic);
}

// a / den for a < 256 den: 32-bit where den < 2^24 (wave-uniform: den comes from the job table)
T2O_HD int select_div(long long a, long long den) {
  if (den < (1ll << 24)) return (int)((unsigned)a / (unsigned)den);
  return (int)((unsigned long long)a / (unsigned long long)den);
}

T2O_HD int select_linear(const int* p, int x, int y) {
  const long long dx = (long long)p[2] - p[0], dy = (long long)p[3] - p[1];
  const long long num = (x - p[0]) * dx + (y - p[1]) * dy, den = dx * dx + dy * dy;
  if (num <= 0) return 255;
  if (num >= den) return 0;
  return select_div(255 * (den - num) + den / 2, den);
}

T2O_HD int select_radial(const int* p, int x, int y) {
  const long long ex = x - p[0], ey = y - p[1];
  const long long d2 = ex * ex + ey * ey, ri2 = (long long)p[2] * p[2], ro2 = (long long)p[3] * p[3];
  if (d2 <= ri2) return 255;
  if (d2 >= ro2) return 0;
  return select_div(255 * (ro2 - d2) + (ro2 - ri2) / 2, ro2 - ri2);
}

T2O_HD bool select_is_position(int kind) { return kind == SELECT_LINEAR || kind == SELECT_RADIAL; }

T2O_HD bool select_is_colour(int kind) { return kind == SELECT_LUM || kind == SELECT_SAT || kind == SELECT_HUE; }

T2O_HD bool select_has_colour(const SelectJob& j) {
  bool any = false;
  for (int t = 0; t < j.n_terms; ++t) any = any || select_is_colour(j.terms[t].kind);
  return any;
}

// Host side, on the kernel's copy of a job: p[3] of a lum / sat / hue term (unused by the C ABI) receives select_magic(soft)
inline void select_prepare(SelectJob& j) {
  for (int t = 0; t < j.n_terms && t < kSelectMaxTerms; ++t)
    if (select_is_colour(j.terms[t].kind)) j.terms[t].p[3] = (int)select_magic(j.terms[t].p[2]);
}

T2O_HD bool select_has_position(const SelectJob& j) {
  bool any = false;
  for (int t = 0; t < j.n_terms; ++t) any = any || select_is_position(j.terms[t].kind);
  return any;
}

// ---------------------------------------------------------------- the per-pixel program
// pb[t]: the pixel's byte of term t's plane (read only where term t is a plane term)
T2O_HD int select_pixel(const SelectJob& j, int r, int g, int b, int x, int y, const int* pb) {
  int m = 255;
  for (int t = 0; t < j.n_terms; ++t) {
    const SelectTerm& s = j.terms[t];
    int v;
    switch (s.kind) {
      case SELECT_LUM:    v = select_range(select_lum(r, g, b), s.p[0], s.p[1], s.p[2], (unsigned)s.p[3]); break;
      case SELECT_SAT:    v = select_range(select_sat(r, g, b), s.p[0], s.p[1], s.p[2], (unsigned)s.p[3]); break;
      case SELECT_HUE:    v = select_hue_range(select_hue(r, g, b), s.p[0], s.p[1], s.p[2], (unsigned)s.p[3]); break;
      case SELECT_LINEAR: v = select_linear(s.p, x, y); break;
      case SELECT_RADIAL: v = select_radial(s.p, x, y); break;
      default:            v = pb[t]; break;
    }
    if (s.invert) v = 255 - v;
    m = t == 0 ? v : (int)((unsigned)(m * v + 127) / 255u);
  }
  return m;
}

// ---------------------------------------------------------------- the lane program
// aligned destination dwords that hold a byte of the job's plane
T2O_HD int select_dwords(const SelectJob& j, const unsigned char* out) {
  return (int)(((long long)replay_misalign(out + j.out_offset) + (long long)j.h * j.w + 3) / 4);
}

T2O_HD int select_tiles(const SelectJob& j, const unsigned char* out) { return (select_dwords(j, out) + kSelectTileDw - 1) / kSelectTileDw; }

// bytes [s, s+4) of the 8 bytes lo, hi
T2O_HD unsigned select_funnel(unsigned lo, unsigned hi, int s) {
  return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * s));
}

// n <= 3 dwords whose first byte is `a` (any alignment), every byte of them inside [lo, hi)
template <int N>
T2O_HD void select_load(const unsigned char* a, const unsigned char* lo, const unsigned char* hi, unsigned (&v)[N]) {
  const int s = (int)replay_misalign(a);
  unsigned d[N + 1];
  T2O_UNROLL
  for (int k = 0; k < N; ++k) d[k] = replay_load_dword(a - s + 4 * k, lo, hi);
  d[N] = s ? replay_load_dword(a - s + 4 * N, lo, hi) : 0u;         // (s = 0: that dword holds no byte of ours)
  T2O_UNROLL
  for (int k = 0; k < N; ++k) v[k] = s ? select_funnel(d[k], d[k + 1], s) : d[k];
}

T2O_HD void select_lane(const SelectJob& j, const unsigned char* src, unsigned char* out, int q) {
  const int n = j.h * j.w;                                           // < 2^31
  unsigned char* plane = out + j.out_offset;
  const int p0 = (int)(4ll * q - (long long)replay_misalign(plane)); // the lane's first pixel (< n); its dword is plane + p0, aligned
  const bool whole = p0 >= 0 && p0 <= n - 4;
  const unsigned char* photo = src + j.src_offset;
  unsigned rgb[3] = {0u, 0u, 0u}, pl[kSelectMaxTerms] = {0u, 0u, 0u, 0u};
  const bool colour = select_has_colour(j);                          // (no colour term: the photo is not read at all)
  if (whole) {
    if (colour) select_load<3>(photo + 3ll * p0, photo, photo + 3ll * n, rgb);
    for (int t = 0; t < j.n_terms; ++t)
      if (j.terms[t].kind == SELECT_PLANE) {
        const unsigned char* m = src + j.terms[t].plane_offset;
        unsigned one[1];
        select_load<1>(m + p0, m, m + n, one);
        pl[t] = one[0];
      }
  } else {
    for (int b = 0; b < 4; ++b) {
      const long long p = (long long)p0 + b;
      if (p < 0 || p >= n) continue;
      for (int c = 0; colour && c < 3; ++c) rgb[(3 * b + c) >> 2] |= (unsigned)photo[3 * p + c] << (8 * ((3 * b + c) & 3));
      for (int t = 0; t < j.n_terms; ++t)
        if (j.terms[t].kind == SELECT_PLANE) pl[t] |= (unsigned)src[j.terms[t].plane_offset + p] << (8 * b);
    }
  }
  int x = 0, y = 0;
  if (select_has_position(j)) {
    const int pc = p0 < 0 ? 0 : p0;
    y = (int)((unsigned)pc / (unsigned)j.w);
    x = pc - y * j.w - (pc - p0);                                    // the position of pixel p0, were it in row y
  }
  unsigned word = 0;
  T2O_UNROLL
  for (int b = 0; b < 4; ++b) {
    int c[3], pb[kSelectMaxTerms];
    T2O_UNROLL
    for (int k = 0; k < 3; ++k) c[k] = (int)((rgb[(3 * b + k) >> 2] >> (8 * ((3 * b + k) & 3))) & 0xffu);
    T2O_UNROLL
    for (int t = 0; t < kSelectMaxTerms; ++t) pb[t] = (int)((pl[t] >> (8 * b)) & 0xffu);
    int xb = x + b, yb = y;
    while (xb >= j.w) { xb -= j.w; ++yb; }                           // (pixels outside the plane get some position: they are not stored)
    word |= (unsigned)select_pixel(j, c[0], c[1], c[2], xb, yb, pb) << (8 * b);
  }
  if (whole) {
    replay_store_dword(plane + p0, word);
  } else {
    for (int b = 0; b < 4; ++b)
      if ((long long)p0 + b >= 0 && (long long)p0 + b < n) plane[(long long)p0 + b] = (unsigned char)(word >> (8 * b));
  }
}

// what thread `tid` of workgroup (block_x, block_y) of the grid (max tiles over the jobs, J) does
T2O_HD void select_thread(const SelectArgs& a, int block_x, int block_y, int tid) {
  const SelectJob& j = a.jobs[block_y];
  const int dwords = select_dwords(j, a.out);
  int q = block_x * kSelectTileDw + tid;                             // < 2^29 + 2048
  for (int i = 0; i < kSelectIter; ++i, q += kSelectThreads)
    if (q < dwords) select_lane(j, a.src, a.out, q);
}

}  // namespace t2o
