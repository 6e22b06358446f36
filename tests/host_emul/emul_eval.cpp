// Host emulation of the evaluation kernels (t2onet_amd/csrc/t2o_eval.hip), compiled with g++ by tests/test_eval_cpu.py.
// TEST HARNESS ONLY: the phase functions of t2o_eval_math.h -- the ones the kernels run -- for every tile of every plane
// (metrics) and every workgroup of a row (variance), thread by thread, a loop over the threads standing in for each barrier;
// the partials are added as the finalize kernels add them (per sample, then over the samples).
#include <math.h>
#include <string.h>

#include <vector>

#include "../../t2onet_amd/csrc/t2o_eval_math.h"

using namespace t2o;

template <int V>
static float var_all(const VarArgs& a) {
  float acc = 0.0f;
  for (size_t blk = 0; blk < var_blocks(a.row, V); ++blk) {
    float total = 0.0f;
    for (int tid = 0; tid < kThreads; ++tid) total += var_thread<V>(a, blk, tid);
    acc += total;
  }
  return acc / (float)a.row;
}

extern "C" {

int emul_eval_lds_floats(void) { return kEvalLdsFloats; }

// t2o_eval_metrics: imgs = T pointers to (B,C,H,W), first (B) -> out4
int emul_eval_metrics(const float* input, const float* const* imgs, int T, const long long* first, const float* target, float* out4,
                      int with_ssim, int B, int C, int H, int W) {
  if (T < 1 || T > kEvalMaxT || B <= 0 || C <= 0 || H <= 0 || W <= 0) return 1;
  EvalArgs s;
  memset(&s, 0, sizeof(s));
  for (int t = 0; t < T; ++t) s.img[t] = imgs[t];
  s.input = input; s.target = target; s.first = first;
  ssim_window(s.g);
  s.T = T; s.B = B; s.C = C; s.H = H; s.W = W;
  s.tiles_x = (W + kSsimTile - 1) / kSsimTile;
  s.tiles = s.tiles_x * ((H + kSsimTile - 1) / kSsimTile);
  s.with_ssim = with_ssim ? 1 : 0;
  const size_t per_slot = (size_t)B * C * s.tiles;
  std::vector<float> partials(4 * per_slot, NAN);
  std::vector<float> lds(kEvalLdsFloats);
  for (int plane = 0; plane < B * C; ++plane)
    for (int tile = 0; tile < s.tiles; ++tile) {
      for (float& v : lds) v = NAN;                       // nothing may rest on what a previous tile left
      for (int tid = 0; tid < kThreads; ++tid) eval_phase_load(s, plane, tile, tid, lds.data());
      if (s.with_ssim)
        for (int tid = 0; tid < kThreads; ++tid) eval_phase_rows(s, tid, lds.data());
      float total[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int tid = 0; tid < kThreads; ++tid) {
        float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        eval_phase_cols(s, tile, tid, lds.data(), sum);
        for (int k = 0; k < 4; ++k) total[k] += sum[k];
      }
      for (int k = 0; k < 4; ++k) partials[k * per_slot + (size_t)plane * s.tiles + tile] = total[k];
    }
  const int per_sample = C * s.tiles;
  const float inv = 1.0f / ((float)C * (float)H * (float)W);
  for (int k = 0; k < 4; ++k) {
    if (k >= 2 && !s.with_ssim) { out4[k] = 0.0f; continue; }
    float total = 0.0f;
    for (int b = 0; b < B; ++b) {
      float acc = 0.0f;
      for (int i = 0; i < per_sample; ++i) acc += partials[k * per_slot + (size_t)b * per_sample + i];
      total += acc * inv;
    }
    out4[k] = total / (float)B;
  }
  return 0;
}

// t2o_end_select_var_mean with loads of V floats (V = 0: the widest the row length allows, as the entry point chooses)
int emul_end_select_var_mean(const float* const* imgs, const long long* const* first, int R, int T, int B, size_t row, int V, float* out) {
  if (R < 1 || R > kEvalMaxR || T < 1 || T > kEvalMaxT || B <= 0 || row == 0 || (long long)R * B < 2) return 1;
  VarArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < R * T; ++i) a.img[i] = imgs[i];
  for (int r = 0; r < R; ++r) a.first[r] = first[r];
  a.row = row; a.R = R; a.T = T; a.B = B;
  if (V == 0) V = row % 4 == 0 ? 4 : row % 2 == 0 ? 2 : 1;
  if (row % V != 0) return 1;
  out[0] = V == 4 ? var_all<4>(a) : V == 2 ? var_all<2>(a) : var_all<1>(a);
  return 0;
}

}  // extern "C"
