// Host emulation of the masked planner kernels' per-pixel work -- TEST HARNESS ONLY (see emul.cpp).
//
// g++ compiles t2o_pixel_math.h / t2o_block_programs.h and this file walks the pixels the way k_fit_eval<GRAD, true> and
// k_candidates_multi_l1<true> do: the operator's unclamped output, masked_l1_term (blend, clamp, clamp backward, the
// factor m), the unmasked closed-form parameter terms times that g_z, curve_param_grad on the raw sums.  Sums are kept
// in double (the kernels keep fp64 partials from the wave reduction on).  Never shipped, never a fallback.
#include <math.h>
#include <string.h>

#include "../../t2onet_amd/csrc/t2o_block_programs.h"

using namespace t2o;

namespace {

float at(const float* plane, int y, int x, int H, int W) {
  return (y >= 0 && y < H && x >= 0 && x < W) ? plane[(size_t)y * W + x] : 0.0f;
}

}  // namespace

extern "C" {

// mean |clamp(blend(op(img; params), img, mask)) - target| -> *loss, and its parameter gradient -> grad[24].
// mask: (H,W) bytes at any address, or null (m = 1).  Returns 0, or 1 for an operator the fit does not take.
int emul_fit_eval_masked(int op, const float* img, const float* tgt, const float* params, const unsigned char* mask, int H, int W,
                         double* loss, float* grad) {
  if (!(op == OP_BRIGHTNESS || op == OP_CONTRAST || op == OP_SATURATION || op == OP_COLOR || op == OP_TONE || op == OP_SHARPNESS)) return 1;
  const unsigned hw = (unsigned)H * (unsigned)W;
  const float inv_n = 1.0f / (3.0f * (float)H * (float)W);
  const bool curve = op == OP_COLOR || op == OP_TONE;
  Curve cv = {};
  if (curve) curve_load(cv, params, op == OP_COLOR);
  const float p0[1] = {params[0]};
  double raw[kMaxParam];
  for (int k = 0; k < kMaxParam; ++k) raw[k] = 0.0;
  double sum = 0.0;
  for (unsigned px = 0; px < hw; ++px) {
    Rgb x, z;
    float t[3], d[3] = {0.0f, 0.0f, 0.0f}, red[kMaxParam];
    for (int k = 0; k < kMaxParam; ++k) red[k] = 0.0f;
    for (int c = 0; c < 3; ++c) { x.c[c] = img[c * (size_t)hw + px]; t[c] = tgt[c * (size_t)hw + px]; }
    if (op == OP_SHARPNESS) {
      const int y = (int)(px / (unsigned)W), xx = (int)(px % (unsigned)W);
      for (int c = 0; c < 3; ++c) {
        const float* plane = img + c * (size_t)hw;
        d[c] = sharp_delta(x.c[c], at(plane, y - 1, xx, H, W), at(plane, y, xx - 1, H, W), at(plane, y, xx + 1, H, W), at(plane, y + 1, xx, H, W));
        z.c[c] = x.c[c] + p0[0] * d[c];
      }
    } else {
      z = pointwise_fwd(op, x, p0, cv);
    }
    const float m = mask ? (float)mask[px] : 1.0f;
    Rgb go;
    float l = 0.0f;
    for (int c = 0; c < 3; ++c) l += masked_l1_term(z.c[c], x.c[c], m, t[c], inv_n, go.c[c]);
    sum += (double)l;
    if (op == OP_SHARPNESS) {
      for (int c = 0; c < 3; ++c) red[0] += go.c[c] * d[c];
    } else if (curve) {
      for (int c = 0; c < 3; ++c)
        for (int j = 0; j < kCurveSteps; ++j) {
          const float tj = fminf(fmaxf(x.c[c] - (float)j / kCurveSteps, 0.0f), 1.0f / kCurveSteps);
          if (op == OP_COLOR) red[c * kCurveSteps + j] += go.c[c] * tj;
          else red[j] += go.c[c] * tj;
        }
    } else {
      pointwise_bwd(op, x, p0, cv, go, red);
    }
    for (int k = 0; k < kMaxParam; ++k) raw[k] += (double)red[k];
  }
  *loss = sum / (3.0 * (double)H * (double)W);
  float A[kMaxParam];
  for (int k = 0; k < kMaxParam; ++k) { A[k] = (float)raw[k]; grad[k] = 0.0f; }
  if (curve) {
    const int rows = op == OP_COLOR ? 3 : 1;
    for (int r = 0; r < rows; ++r) curve_param_grad(params + r * kCurveSteps, A + r * kCurveSteps, grad + r * kCurveSteps);
  } else {
    grad[0] = A[0];
  }
  return 0;
}

// The sweep's value for ONE candidate row through the kernel's own thread functions (cand_build_table, cand_load,
// cand_load_mask, cand_eval_masked), every workgroup and thread in turn -> *loss.
int emul_cand_masked(int op, const float* img, const float* tgt, const float* params, int param_stride, const unsigned char* mask,
                     int H, int W, double* loss) {
  if (op == OP_SHARPNESS || op == OP_IDENTITY || op < 0 || op > 7 || op == OP_INPAINT) return 1;
  CandArgs a;
  memset(&a, 0, sizeof(a));
  a.img = img; a.target = tgt; a.params = params; a.op = op; a.C = 1; a.param_stride = param_stride; a.H = H; a.W = W;
  a.nblk = (int)(((size_t)H * W + (size_t)kThreads * kCandPix - 1) / ((size_t)kThreads * kCandPix));
  float tab[kTabStride];
  memset(tab, 0, sizeof(tab));
  cand_build_table(a, 0, tab);
  double sum = 0.0;
  for (int blk = 0; blk < a.nblk; ++blk)
    for (int tid = 0; tid < kThreads; ++tid) {
      float x[3][kCandPix], tg[3][kCandPix];
      unsigned mk[kCandMaskWords];
      const int npx = cand_load(a, blk, tid, x, tg);
      cand_load_mask(a, mask, blk, tid, mk);
      sum += (double)cand_eval_masked(a, tab, x, tg, mk, npx);
    }
  *loss = sum / (3.0 * (double)H * (double)W);
  return 0;
}

}  // extern "C"
