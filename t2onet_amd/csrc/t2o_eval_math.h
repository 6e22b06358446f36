// The per-workgroup programs of the evaluation kernels (t2o_eval.hip): what the test loop of
// experiments/t2onet/test_seq2seqL1.py measures per image, without a host value between two images.
//
//   metrics   utils/eval.py:50-60 + test_seq2seqL1.py:60-74: mean |input - target|, mean |out - target|, SSIM(input, target),
//             SSIM(out, target), where out[b] = imgs[first[b]][b] is read where it lies (no (B,T,3,H,W) stack, no gather).
//             A workgroup owns a 32 x 32 tile of one (b, c) plane.  Phases:
//               load   the three 42 x 42 windows (input, selected output, target) into LDS, ZERO outside the plane
//               rows   the horizontal Gaussian pass: EIGHT maps of 42 rows x 32 columns -- mu of the three images, E[.^2] of
//                      the three, E[in tgt], E[out tgt]; the target's two moments serve both pairs
//               cols   the vertical pass and the two SSIM values per pixel; the two |.| terms from the centre pixels that
//                      already lie in LDS; returns the thread's four sums
//             Per-element arithmetic is ssim_phase_rows / ssim_phase_cols of t2o_block_programs.h: same window, same order
//             over k, same C1 / C2 formula.  Without SSIM only the 32 x 32 centre is loaded and no Gaussian pass runs.
//   variance  test_seq2seqL1.py:130-133, torch.var(torch.cat(ends), dim=0).mean(): for element p of a row the N = R B values
//             imgs[r T + first[r][b]][b row + p]; unbiased variance in TWO passes (the mean, then the squared deviations over
//             N - 1; the second read comes from cache), summed per thread.
//
// Like t2o_block_programs.h these are `__host__ __device__` phase functions -- what ONE thread of ONE workgroup does between
// two barriers -- so that tests/host_emul/emul_eval.cpp runs the same programs thread by thread with g++ (a test harness,
// never a fallback).
#pragma once
#include "t2o_block_programs.h"

namespace t2o {

constexpr int kEvalMaxT = 8;                             // step images per episode (the pointer table of the kernel arguments)
constexpr int kEvalMaxR = 16;                            // requests of a variance call
constexpr int kEvalMaps = 8;
constexpr int kEvalWin = kSsimIn * kSsimInStride;        // floats of one 42 x 42 window (row stride 43)
constexpr int kEvalMap = kSsimIn * kSsimHStride;         // floats of one row-filtered map (42 rows x 32, row stride 33)
constexpr int kEvalLdsFloats = 3 * kEvalWin + kEvalMaps * kEvalMap;      // 16506 floats = 66024 bytes of the CU's 160 KiB

struct EvalArgs {
  const float* input;              // (B,C,H,W)
  const float* img[kEvalMaxT];     // T step images (B,C,H,W)
  const float* target;             // (B,C,H,W)
  const long long* first;          // (B) int64: the step whose image is sample b's output
  float* partials;                 // (4, B*C*tiles): slot-major sums of the workgroups
  float g[kSsimWin];               // normalised 1-D Gaussian (ssim_window)
  int T, B, C, H, W, tiles_x, tiles, with_ssim;
};

// the selected step of sample b: a value outside [0, T) counts as T - 1, so the table is never indexed past its end
T2O_HD int eval_step(long long f, int T) { return (f < 0 || f >= (long long)T) ? T - 1 : (int)f; }

// s.img[f] without an indexed read of the kernel arguments (as end_sel_src of t2o_kernels.hip)
T2O_HD const float* eval_out_image(const EvalArgs& s, int f) {
  const float* p = s.img[0];
  T2O_UNROLL
  for (int t = 1; t < kEvalMaxT; ++t) p = (f == t) ? s.img[t] : p;
  return p;
}

// phase 1: the three windows, zero outside the plane (without SSIM: the 32 x 32 centre only, nothing else is read)
T2O_HD void eval_phase_load(const EvalArgs& s, int plane, int tile, int tid, float* lds) {
  const int y0 = (tile / s.tiles_x) * kSsimTile - kSsimPad, x0 = (tile % s.tiles_x) * kSsimTile - kSsimPad;
  const size_t base = (size_t)plane * s.H * s.W;
  const float* out = eval_out_image(s, eval_step(s.first[plane / s.C], s.T));
  for (int i = tid; i < kSsimIn * kSsimIn; i += kThreads) {
    const int r = i / kSsimIn, c = i % kSsimIn, gy = y0 + r, gx = x0 + c;
    if (!s.with_ssim && (r < kSsimPad || r >= kSsimPad + kSsimTile || c < kSsimPad || c >= kSsimPad + kSsimTile)) continue;
    const bool in = gy >= 0 && gy < s.H && gx >= 0 && gx < s.W;
    const size_t at = base + (size_t)(in ? gy : 0) * s.W + (in ? gx : 0);
    float* o = lds + r * kSsimInStride + c;
    o[0] = in ? s.input[at] : 0.0f;
    o[kEvalWin] = in ? out[at] : 0.0f;
    o[2 * kEvalWin] = in ? s.target[at] : 0.0f;
  }
}

// phase 2: horizontal pass -> 8 maps of 42 rows x 32 columns: mu_in, mu_out, mu_tgt, E[in^2], E[out^2], E[tgt^2], E[in tgt], E[out tgt]
T2O_HD void eval_phase_rows(const EvalArgs& s, int tid, float* lds) {
  const float* A = lds;
  const float* O = lds + kEvalWin;
  const float* Tg = lds + 2 * kEvalWin;
  float* Hm = lds + 3 * kEvalWin;
  for (int i = tid; i < kSsimIn * kSsimTile; i += kThreads) {
    const int r = i / kSsimTile, c = i % kSsimTile;
    float ma = 0.0f, mo = 0.0f, mt = 0.0f, eaa = 0.0f, eoo = 0.0f, ett = 0.0f, eat = 0.0f, eot = 0.0f;
    for (int k = 0; k < kSsimWin; ++k) {
      const float a = A[r * kSsimInStride + c + k], o = O[r * kSsimInStride + c + k], t = Tg[r * kSsimInStride + c + k], w = s.g[k];
      ma += w * a; mo += w * o; mt += w * t;
      eaa += w * (a * a); eoo += w * (o * o); ett += w * (t * t);
      eat += w * (a * t); eot += w * (o * t);
    }
    float* h = Hm + r * kSsimHStride + c;
    h[0] = ma; h[kEvalMap] = mo; h[2 * kEvalMap] = mt; h[3 * kEvalMap] = eaa;
    h[4 * kEvalMap] = eoo; h[5 * kEvalMap] = ett; h[6 * kEvalMap] = eat; h[7 * kEvalMap] = eot;
  }
}

// the SSIM value of one pixel from the window moments of a pair (ssim_phase_cols)
T2O_HD float eval_ssim_value(float mu1, float mu2, float e11, float e22, float e12) {
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
  const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
  return ((2.0f * mu12 + C1) * (2.0f * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
}

// phase 3: vertical pass, the two SSIM values and the two |.| terms of this thread's in-plane pixels, added to
// sum = {|in - tgt|, |out - tgt|, SSIM(in, tgt), SSIM(out, tgt)}
T2O_HD void eval_phase_cols(const EvalArgs& s, int tile, int tid, const float* lds, float (&sum)[4]) {
  const float* Hm = lds + 3 * kEvalWin;
  const int y0 = (tile / s.tiles_x) * kSsimTile, x0 = (tile % s.tiles_x) * kSsimTile;
  for (int i = tid; i < kSsimTile * kSsimTile; i += kThreads) {
    const int r = i / kSsimTile, c = i % kSsimTile;
    if (y0 + r >= s.H || x0 + c >= s.W) continue;
    const float* ce = lds + (r + kSsimPad) * kSsimInStride + c + kSsimPad;
    const float a = ce[0], o = ce[kEvalWin], t = ce[2 * kEvalWin];
    sum[0] += fabsf(a - t);
    sum[1] += fabsf(o - t);
    if (!s.with_ssim) continue;
    float v[kEvalMaps];
    for (int m = 0; m < kEvalMaps; ++m) {
      float acc = 0.0f;
      for (int k = 0; k < kSsimWin; ++k) acc += s.g[k] * Hm[m * kEvalMap + (r + k) * kSsimHStride + c];
      v[m] = acc;
    }
    sum[2] += eval_ssim_value(v[0], v[2], v[3], v[5], v[6]);
    sum[3] += eval_ssim_value(v[1], v[2], v[4], v[5], v[7]);
  }
}

// ===================================================================== variance over requests
constexpr int kVarIters = 4;       // element groups per thread

struct VarArgs {
  const float* img[kEvalMaxR * kEvalMaxT];      // request r, step t: img[r * T + t], (B, row)
  const long long* first[kEvalMaxR];            // request r: (B) int64
  float* partials;                              // (nblk)
  size_t row;
  int R, T, B;
};

// element p of sample n = r B + b of the concatenated END images: V consecutive floats
template <int V>
T2O_HD void var_load(const VarArgs& a, int n, size_t p, float (&v)[V]) {
  const int r = n / a.B, b = n - r * a.B;
  const int f = eval_step(a.first[r][b], a.T);
  const float* src = a.img[r * a.T + f] + (size_t)b * a.row + p;
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (V == 2) {
    const float2 t = *reinterpret_cast<const float2*>(src);
    v[0] = t.x; v[1] = t.y;
    return;
  }
#endif
  load_vec<V>(src, v);
}

// this thread's sum of the unbiased variances of its elements (two passes over the N samples)
template <int V>
T2O_HD float var_thread(const VarArgs& a, size_t blk, int tid) {
  const int N = a.R * a.B;
  const float fn = (float)N, fn1 = (float)(N - 1);
  float acc = 0.0f;
  for (int it = 0; it < kVarIters; ++it) {
    const size_t p = ((blk * kVarIters + it) * kThreads + (size_t)tid) * V;
    if (p >= a.row) break;
    float v[V], mean[V], ss[V];
    T2O_UNROLL
    for (int i = 0; i < V; ++i) mean[i] = ss[i] = 0.0f;
    for (int n = 0; n < N; ++n) {
      var_load<V>(a, n, p, v);
      T2O_UNROLL
      for (int i = 0; i < V; ++i) mean[i] += v[i];
    }
    T2O_UNROLL
    for (int i = 0; i < V; ++i) mean[i] = mean[i] / fn;
    for (int n = 0; n < N; ++n) {
      var_load<V>(a, n, p, v);
      T2O_UNROLL
      for (int i = 0; i < V; ++i) { const float d = v[i] - mean[i]; ss[i] += d * d; }
    }
    T2O_UNROLL
    for (int i = 0; i < V; ++i) acc += ss[i] / fn1;
  }
  return acc;
}

T2O_HD size_t var_blocks(size_t row, int V) {
  const size_t per = (size_t)kThreads * kVarIters * V;
  return (row + per - 1) / per;
}

}  // namespace t2o
