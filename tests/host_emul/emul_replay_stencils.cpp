// Host emulation of the stencils replay kernel (t2onet_amd/csrc/t2o_replay_stencils.hip), compiled with g++ by
// tests/test_replay_stencils_cpu.py (and included by sanitize_replay_stencils.cpp).  TEST HARNESS ONLY.  Two programs:
//   emul_replay_u8_stencils   the phase functions of t2o_replay_stencils_math.h -- the ones the kernel runs, in the
//                             kernel's order -- for every tile of a picture, thread by thread, a loop over the threads
//                             standing in for each barrier; the held registers of a thread are a row of an array
//   chain_replay_u8_stencils  a plain WHOLE-IMAGE chain from the same device functions: bytes -> floats, per step one
//                             pass over the full image (a sharpness reads a zero-padded copy of the image in front of
//                             it), floats -> bytes.  No tiles, no window, no LDS struct.
#include <vector>

#include "../../t2onet_amd/csrc/t2o_replay_stencils_math.h"

using namespace t2o;

namespace {

template <int NP, class L>
void run_first_chunk(const ReplayMaskJob& mj, const unsigned char* src, unsigned char* out, const float* params,
                     const unsigned char* masks, const long long* offs, const ReplayTile& t, int E, int base, L& lds) {
  for (int tid = 0; tid < kReplayThreads; ++tid) {
    const int tid0 = tid + base;
    if (tid0 >= E * E) continue;
    Rgb hold[NP];
    replay_st_phase_first<NP>(mj, src, params, masks, offs, t, E, tid0, lds, hold);
    if (mj.j.sharp > 0) replay_st_phase_put<NP>(mj.j, t, E, tid0, lds, hold);
    else if constexpr (NP == kReplayPix) replay_st_phase_out(mj.j, out, t, tid0, lds, hold);
  }
}

template <int NP, class L>
void run_segment(const ReplayMaskJob& mj, unsigned char* out, const float* params, const unsigned char* masks,
                 const long long* offs, const ReplayTile& t, int E, int n, int s, L& lds) {
  static Rgb hold[kReplayThreads][NP];                               // a thread's registers across the barrier
  for (int tid = 0; tid < kReplayThreads; ++tid) replay_st_phase_stencil<NP>(mj, params, masks, offs, t, E, s, tid, lds, hold[tid]);
  if (n + 1 < mj.j.sharp) {
    for (int tid = 0; tid < kReplayThreads; ++tid) replay_st_phase_put<NP>(mj.j, t, E, tid, lds, hold[tid]);
  } else if constexpr (NP == kReplayPix) {
    for (int tid = 0; tid < kReplayThreads; ++tid) replay_st_phase_out(mj.j, out, t, tid, lds, hold[tid]);
  }
}

template <class L>
void run_tile(const ReplayMaskJob& mj, const unsigned char* src, unsigned char* out, const float* params,
              const unsigned char* masks, const long long* offs, int tile, L& lds) {
  const ReplayTile t = replay_st_tile(mj.j, tile);
  memset(&lds, 0xFF, sizeof(lds));                                   // nothing may rest on what a previous tile left
  for (int tid = 0; tid < kReplayThreads; ++tid) replay_st_phase_load(mj.j, src, t, tid, lds);
  if (replay_masks_used(mj))
    for (int tid = 0; tid < kReplayThreads; ++tid) replay_st_phase_mask_load(mj, masks, offs, t, tid, lds);
  const int R = mj.j.sharp, W = kReplayTile + 2 * R;
  for (int base = 0; base < W * W;) {
    const int np = replay_st_first_np(W * W - base);
    if (np == 4) run_first_chunk<4>(mj, src, out, params, masks, offs, t, W, base, lds);
    else if (np == 2) run_first_chunk<2>(mj, src, out, params, masks, offs, t, W, base, lds);
    else run_first_chunk<1>(mj, src, out, params, masks, offs, t, W, base, lds);
    base += np * kReplayThreads;
  }
  int s = -1;
  for (int n = 0; n < R; ++n) {
    const int E = kReplayTile + 2 * (R - n - 1);
    s = replay_st_next_sharp(mj.j, s + 1);
    switch (replay_st_np(E)) {
      case 4: run_segment<4>(mj, out, params, masks, offs, t, E, n, s, lds); break;
      case 5: run_segment<5>(mj, out, params, masks, offs, t, E, n, s, lds); break;
      case 6: run_segment<6>(mj, out, params, masks, offs, t, E, n, s, lds); break;
      default: run_segment<9>(mj, out, params, masks, offs, t, E, n, s, lds); break;
    }
  }
  for (int tid = 0; tid < kReplayThreads; ++tid) replay_st_phase_store(mj.j, out, t, tid, lds);
}

}  // namespace

// the tile program over one picture with the LDS struct at `lds` (the sanitizer program passes real heap objects); L is
// the small or the large struct: the large one serves every list, the small one those with R <= 2 (else status 1)
template <class L>
int replay_stencils_run(L& lds, const unsigned char* src, long long src_offset, unsigned char* out, long long out_offset,
                        int h, int w, int steps, const int* ops, const int* mask_of, const float* params,
                        const unsigned char* masks, const long long* mask_offsets, int n_masks) {
  if (n_masks < 0 || n_masks > kReplayMaxMasks) return 1;
  ReplayMaskJob mj;
  const char* why = "";
  if (const int rc = replay_st_job_make(mj, src_offset, out_offset, h, w, steps, ops, mask_of, n_masks, &why)) return rc;
  if (mj.j.sharp > L::kRing) return 1;
  long long offs[kReplayMaxMasks] = {0, 0, 0, 0};
  for (int i = 0; i < n_masks; ++i) offs[i] = mask_offsets[i];
  for (int tile = 0; tile < replay_tiles(mj.j); ++tile) run_tile(mj, src, out, params, masks, offs, tile, lds);
  return 0;
}

extern "C" {

int emul_replay_stencils_tile(void) { return kReplayTile; }
int emul_replay_stencils_lds_bytes(void) { return (int)sizeof(ReplayStLds); }
int emul_replay_stencils_small_lds_bytes(void) { return (int)sizeof(ReplayStLdsSmall); }
int emul_replay_stencils_small_ring(void) { return kStSmallRing; }
int emul_replay_stencils_args_bytes(void) { return (int)sizeof(ReplayMaskArgs); }

// one job of t2o_replay_u8_stencils: (h, w, 3) uint8 at src + src_offset -> out + out_offset; params (8, 24); mask_of: 8
// indices into mask_offsets (n_masks entries, counted from masks), -1 = none; NULL when n_masks = 0.  Returns the status
// of the job check.  The instance is the one a launch of this job alone takes: the small one when R <= 2.
int emul_replay_u8_stencils(const unsigned char* src, long long src_offset, unsigned char* out, long long out_offset, int h, int w,
                            int steps, const int* ops, const int* mask_of, const float* params, const unsigned char* masks,
                            const long long* mask_offsets, int n_masks) {
  static ReplayStLds lds;
  static ReplayStLdsSmall small;
  int R = 0;
  for (int k = 0; k < steps && k < kReplayMaxSteps; ++k) R += ops[k] == OP_SHARPNESS;
  if (R <= kStSmallRing)
    return replay_stencils_run(small, src, src_offset, out, out_offset, h, w, steps, ops, mask_of, params, masks, mask_offsets, n_masks);
  return replay_stencils_run(lds, src, src_offset, out, out_offset, h, w, steps, ops, mask_of, params, masks, mask_offsets, n_masks);
}

// the same job on the LARGE instance whatever R: what a job meets in a launch beside a job with R > 2
int emul_replay_u8_stencils_large(const unsigned char* src, long long src_offset, unsigned char* out, long long out_offset, int h, int w,
                                  int steps, const int* ops, const int* mask_of, const float* params, const unsigned char* masks,
                                  const long long* mask_offsets, int n_masks) {
  static ReplayStLds lds;
  return replay_stencils_run(lds, src, src_offset, out, out_offset, h, w, steps, ops, mask_of, params, masks, mask_offsets, n_masks);
}

// the same job as a whole-image chain: one full-image pass per step
int chain_replay_u8_stencils(const unsigned char* src, long long src_offset, unsigned char* out, long long out_offset, int h, int w,
                             int steps, const int* ops, const int* mask_of, const float* params, const unsigned char* masks,
                             const long long* mask_offsets, int n_masks) {
  if (h <= 0 || w <= 0 || steps < 0 || steps > 8) return 1;
  const size_t n = (size_t)h * w;
  std::vector<Rgb> x(n), y(n);
  const unsigned char* img = src + src_offset;
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) x[i].c[c] = u8_to_unit((int)img[3 * i + c]);
  for (int k = 0; k < steps; ++k) {
    const int op = ops[k], mi = mask_of ? mask_of[k] : -1;
    if (op == OP_INPAINT) return 2;
    if (op < OP_IDENTITY || op > OP_WHITE || mi < -1 || mi >= n_masks) return 1;
    if (op < 0) continue;
    const float* prow = params + k * kMaxParam;
    const unsigned char* plane = mi >= 0 ? masks + mask_offsets[mi] : nullptr;
    Curve cv;
    if (op == OP_COLOR || op == OP_TONE) curve_load(cv, prow, op == OP_COLOR);
    const float p0[1] = {prow[0]};
    for (int yy = 0; yy < h; ++yy)
      for (int xx = 0; xx < w; ++xx) {
        const size_t i = (size_t)yy * w + xx;
        const float m = plane ? u8_to_unit((int)plane[i]) : 0.0f;
        Rgb o;
        if (op == OP_SHARPNESS) {
          for (int c = 0; c < 3; ++c) {
            const float ce = x[i].c[c];
            const float up = yy > 0 ? x[i - w].c[c] : 0.0f, dn = yy + 1 < h ? x[i + w].c[c] : 0.0f;
            const float le = xx > 0 ? x[i - 1].c[c] : 0.0f, ri = xx + 1 < w ? x[i + 1].c[c] : 0.0f;
            o.c[c] = ce + prow[0] * sharp_delta(ce, up, le, ri, dn);
          }
        } else {
          o = pointwise_fwd(op, x[i], p0, cv);
        }
        for (int c = 0; c < 3; ++c) y[i].c[c] = clamp01(plane ? blend(o.c[c], x[i].c[c], m) : o.c[c]);
      }
    x.swap(y);
  }
  unsigned char* dst = out + out_offset;
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) dst[3 * i + c] = unit_to_u8(x[i].c[c]);
  return 0;
}

}  // extern "C"
