/* t2onet_hip.h -- C ABI of libt2onet_hip.so, the MI355X (gfx950) implementation of
 * the T2ONet executor/operator hot path.
 *
 * Drop-in boundary.  The reference has no FFI; the interface these entry points
 * replace is the Python one, cited per function (paths relative to the reference):
 *     Executor.execute            executors/executor.py:33-55
 *     Operator.execute / process  models/operators.py:112-131 and the process()
 *                                 bodies :240-245 :277-283 :351-358 :473-479 :509-511
 *                                 :571-585 :607-616
 *     L1 step                     experiments/t2onet/train_seq2seqL1.py:78-85
 *     Attention.forward           models/attention.py:37-40 (score / softmax / mix)
 *     BatchNorm2d + add + ReLU    models/actor_resnet.py:38-44, :99-100 (training mode)
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - all tensors are fp32, contiguous, DEVICE pointers: images (B,3,H,W) NCHW RGB in
 *     [0,1]; params (B,param_stride) rows; masks (B,mask_ch,H,W), mask_ch in {1,3};
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it:
 *     no allocation, no host synchronisation, safe to capture in a hipGraph;
 *   - caller-owned scratch: `workspace` of at least t2o_workspace_bytes(B,H,W) bytes;
 *   - return value: 0 = ok, otherwise a T2O_E* code; t2o_last_error() gives the text
 *     (thread-local).  Nothing throws.
 *
 * Operator indices (executors/executor.py:30):
 *   0 brightness 1 contrast 2 saturation 3 color-curve 4 inpaint(unsupported)
 *   5 tone-curve 6 sharpness 7 white;  -1 = identity (executor.py:44-46).
 */
#ifndef T2ONET_HIP_H
#define T2ONET_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2O_OK 0
#define T2O_EINVAL 1        /* bad pointer / shape / stride */
#define T2O_EUNSUPPORTED 2  /* operator 4 (inpaint) or unknown operator index */
#define T2O_EWORKSPACE 3    /* workspace too small */
#define T2O_ELAUNCH 4       /* HIP reported a launch error */

#define T2O_OP_IDENTITY (-1)
#define T2O_MAX_PARAM 24

int t2o_abi_version(void);
const char* t2o_last_error(void);
/* sha256 (hex) of the sources + compiler flags this binary was built from (compiled in by
 * t2onet_amd/build.py); the loader refuses a library whose digest differs from the tree's. */
const char* t2o_source_digest(void);

/* number of parameters of operator `op` (Executor.get_param_num, executor.py:61-63); -1 if unknown */
int t2o_op_num_params(int op);

/* bytes of scratch needed by the *_bwd / *_l1 / sequence calls for images of this shape */
size_t t2o_workspace_bytes(int B, int H, int W);

/* ---- one operator over a whole (sub)batch: Operator.execute once `param` is known ----
 * out = clamp(process(img, param) * mask + img * (1 - mask), 0, 1)   (operators.py:128-130)
 * mask may be NULL (mask_ch = 0).  op = -1 copies img to out (no clamp). */
int t2o_op_fwd(int op, const float* img, const float* param, int param_stride,
               const float* mask, int mask_ch, float* out, int B, int H, int W, void* stream);

/* gradient of the above: gimg (nullable) and gparam (B,gparam_stride; first n columns written) */
int t2o_op_bwd(int op, const float* img, const float* param, int param_stride,
               const float* mask, int mask_ch, const float* gout,
               float* gimg, float* gparam, int gparam_stride,
               void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);

/* ---- per-sample operators in ONE launch: replaces Actor.divide_op_group + the per-group
 * execute + index_select regrouping (models/actor.py:100-114, :244-259).
 * op_id: (B) int32 DEVICE array; param rows padded to param_stride (24 in the actor). */
int t2o_apply_fwd(const int* op_id, const float* img, const float* param, int param_stride,
                  const float* mask, int mask_ch, float* out, int B, int H, int W, void* stream);
int t2o_apply_bwd(const int* op_id, const float* img, const float* param, int param_stride,
                  const float* mask, int mask_ch, const float* gout,
                  float* gimg, float* gparam, int gparam_stride,
                  void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);

/* ---- L1 loss, train_seq2seqL1.py:85: loss[0] = mean |pred - target| over n floats ---- */
int t2o_l1_fwd(const float* pred, const float* target, float* loss, size_t n,
               void* workspace, size_t workspace_bytes, void* stream);
/* gpred = sign(pred - target) * gloss[0] / n      (gloss: device scalar) */
int t2o_l1_bwd(const float* pred, const float* target, const float* gloss, float* gpred,
               size_t n, void* stream);

/* ---- END select fused with the L1 loss (train_seq2seqL1.py:78-85): pred[b] = imgs[first[b]][b], first[b] = the step of
 * sample b's first END token (else the last step), loss[0] = mean |pred - target| over B * row floats.  imgs / gimgs: HOST
 * arrays of T <= 8 device pointers to (B, row) step images / their gradients; first: device int64 (B).  The backward
 * writes all T gradients in one launch: sign(pred - target) * gloss[0] / (B row) where selected, zero elsewhere.
 * Replaces torch.stack + advanced indexing + t2o_l1_* (and their zero-filled scatter in the backward); the loss equals
 * t2o_l1_fwd on the gathered images bit for bit.  workspace: as t2o_l1_fwd for n = B * row. */
int t2o_end_select_l1_fwd(const float* const* imgs, int T, const long long* first, const float* target, float* loss, int B,
                          size_t row, void* workspace, size_t workspace_bytes, void* stream);
int t2o_end_select_l1_bwd(const float* const* imgs, float* const* gimgs, int T, const long long* first, const float* target,
                          const float* gloss, int B, size_t row, void* stream);

/* ---- operator fused with the L1 loss on its output (last operator of a sequence) ----
 * forward also reads `target` and writes loss[0] = mean |out - target|;
 * backward takes the target instead of gout: gout = sign(out - target) * gloss[0] / (B*3*H*W). */
int t2o_op_fwd_l1(int op, const float* img, const float* param, int param_stride,
                  const float* mask, int mask_ch, const float* target, float* out, float* loss,
                  void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);
int t2o_op_bwd_l1(int op, const float* img, const float* param, int param_stride,
                  const float* mask, int mask_ch, const float* target, const float* gloss,
                  float* gimg, float* gparam, int gparam_stride,
                  void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);

/* ---- a known operator sequence (executor benchmark / planner: utils/beam_search.py:79) ----
 * ops: K HOST ints; params: (K,B,24) device; acts: (K,B,3,H,W) device, acts[k] = output of
 * operator k (every intermediate image is materialised, as Executor.execute returns it);
 * loss[0] = mean |acts[K-1] - target|.  One host call, 2K+2 kernel launches, no sync. */
int t2o_sequence_fwd(const int* ops, int K, const float* img, const float* params,
                     const float* target, float* acts, float* loss,
                     void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);
/* gimg (nullable), gparams (K,B,24); gbuf: scratch of 2 images (2,B,3,H,W) */
int t2o_sequence_bwd(const int* ops, int K, const float* img, const float* params,
                     const float* target, const float* acts, const float* gloss,
                     float* gimg, float* gparams, float* gbuf,
                     void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);

/* ---- the same, FUSED: runs of pointwise operators execute in registers in one kernel pair;
 * only the image at segment boundaries (before/after each sharpness, every 8 operators) goes
 * through HBM.  out (B,3,H,W) = final image.  seg_bufs: t2o_fused_sequence_buffers(ops,K) images
 * of scratch (B,3,H,W each), written by fwd and read by bwd.  Same results as t2o_sequence_*
 * (bit-identical images; parameter gradients equal up to summation order). */
int t2o_fused_sequence_buffers(const int* ops, int K);
int t2o_fused_sequence_fwd(const int* ops, int K, const float* img, const float* params,
                           const float* target, float* out, float* loss, float* seg_bufs,
                           void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);
/* backward: either (target, gloss) -- fused L1, gout = NULL -- or target = NULL and gout =
 * gradient w.r.t. the final image.  gbuf: scratch of 2 images. */
int t2o_fused_sequence_bwd(const int* ops, int K, const float* img, const float* params,
                           const float* target, const float* gloss, const float* gout,
                           float* gimg, float* gparams, const float* seg_bufs, float* gbuf,
                           void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);

/* value AND gradient of loss = mean|sequence(img) - target| in one call (what one train iteration of the planner's and
 * the L1 trainer's inner loop needs: Executor.execute K times, executors/executor.py:33-55, then L1Loss + backward,
 * experiments/t2onet/train_seq2seqL1.py:82-86, utils/beam_search.py:65-91).  The forward of the LAST segment is not
 * launched: its backward kernels recompute the final pixel anyway (for sign(out - target)) and also emit |out - target|
 * partials and, when out != NULL, the final image.  BASELINE configs[1] (5 per-pixel operators + sharpness): 3 launches
 * instead of 4; a list without sharpness: ONE launch.  gimg, gparams and out are bit-identical to
 * t2o_fused_sequence_fwd(target) + t2o_fused_sequence_bwd(target, gloss) (the same kernels in the same geometry); loss
 * is the same sum in another order (partials per backward workgroup), equal to ~1e-7 relative.  out may be NULL;
 * seg_bufs / gbuf as for the two-call form.  Image sizes whose sharpness runs on the LDS-tile kernels (W % 4 != 0 ...)
 * fall back to the two calls internally (then out is required when the list is a single sharpness segment). */
int t2o_fused_sequence_l1_value_grad(const int* ops, int K, const float* img, const float* params,
                                     const float* target, const float* gloss, float* out, float* loss,
                                     float* gimg, float* gparams, float* seg_bufs, float* gbuf,
                                     void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);

/* ---- run-time specialisation of the fused chain kernels for an arbitrary operator list (t2o_jit.hip).
 * The fastest kernels behind t2o_fused_sequence_fwd/bwd take the operator list as a compile-time constant; ahead of time
 * only BASELINE.json's two lists are instantiated.  t2o_fused_sequence_prepare(ops, K) compiles (hipRTC, from the headers
 * embedded in this library, same flags as the ahead-of-time build) and loads the kernels for every per-pixel segment of
 * this list that has none; later t2o_fused_sequence_* calls with the same list pick them up.  Results are bit-identical
 * to the run-time-loop kernels (same arithmetic per pixel; parameter gradients up to summation order).  Blocking (seconds
 * per new list), HOST side: call it outside any stream capture.  T2O_EUNSUPPORTED when libhiprtc is not on the machine
 * (the sequence calls then keep using the run-time-loop kernels).  t2o_jit_set_cache_dir: directory where compiled code
 * objects are kept (keyed by source digest + operator list), NULL/"" = no disk cache.  Executor.execute permits any order
 * (executors/executor.py:33-55); the planner enumerates them (utils/beam_search.py:218-231). */
int t2o_fused_sequence_prepare(const int* ops, int K);
int t2o_jit_set_cache_dir(const char* dir);
int t2o_jit_specialisations(void);      /* operator lists specialised so far in this process */

/* ---- planner candidate sweep (utils/beam_search.py:65-91: one executor call + .item() per
 * evaluated parameter): loss[c] = mean |clamp(process(img, params[c])) - target| for C candidate
 * parameter rows of ONE per-pixel operator (0,1,2,3,5,7) against ONE image pair (3,H,W), in a
 * single launch; the image is read once per 8 candidates. */
size_t t2o_candidates_workspace_bytes(int C, int H, int W);
int t2o_op_candidates_l1(int op, const float* img, const float* target, const float* params, int C,
                         int param_stride, float* loss, void* workspace, size_t workspace_bytes,
                         int H, int W, void* stream);

/* The same for up to 64 (image, operator) jobs in ONE launch -- a whole beam-search step of the planner
 * (utils/beam_search.py:218-231: every beam image x every operation): job j evaluates its C candidate rows
 * params[j] of operator ops[j] on image imgs[img_index[j]] against the common target.  ops / img_index are HOST
 * arrays (copied into the kernel arguments); loss is (J, C). */
size_t t2o_candidates_multi_workspace_bytes(int J, int C, int H, int W);
int t2o_op_candidates_multi_l1(const int* ops, const int* img_index, int J, const float* imgs, int n_img,
                               const float* target, const float* params, int C, int param_stride, float* loss,
                               void* workspace, size_t workspace_bytes, int H, int W, void* stream);

/* ---- planner parameter fits, batched and device resident (utils/beam_search.py:65-91,148-167: one minimisation per
 * candidate step, one executor call and one host sync per objective evaluation).  Adam on the parameters of up to 64
 * jobs at once; job j fits operator ops[j] (0, 1, 2, 3, 5 or 6) so that
 *     mean |clamp(process(imgs[img_index[j]], params[j])) - targets[target_index[j]]|
 * becomes small.  ops / img_index / target_index are HOST arrays (copied into the kernel arguments); imgs (n_img,3,H,W),
 * targets (n_target,3,H,W) and params (J,24: start values in, fitted values out, in place) are device memory; dist (J)
 * receives the loss at the returned parameters.  Two launches per iteration, none of them waits on the host; nothing
 * is allocated: Adam's moments, the per-job stop state and the per-workgroup partial sums live in `workspace`
 * (t2o_fit_multi_workspace_bytes, 8-byte aligned).  The update is torch.optim.Adam's (bias corrected, no weight decay,
 * no projection onto the operator's range).  Stop rule, per job on the device: at iterations check_every,
 * 2 check_every, ... a job whose loss fell by less than tol since its previous check stops moving (the first check only
 * records the loss); check_every <= 0 disables it.  Deterministic: fixed summation order, no atomics; a job's result
 * does not depend on the other jobs of the call.  Any H, W. */
size_t t2o_fit_multi_workspace_bytes(int J, int H, int W);
int t2o_fit_multi_l1_adam(const int* ops, const int* img_index, const int* target_index, int J, const float* imgs,
                          int n_img, const float* targets, int n_target, float* params, float* dist, void* workspace,
                          size_t workspace_bytes, int H, int W, int steps, double lr, double beta1, double beta2,
                          double eps, int check_every, double tol, void* stream);

/* ---- the two planner entry points under local-edit masks (the GIER planner: a candidate of an operator that the pair
 * annotates a region for is fitted and scored under that region's plane).  Everything is as in the unmasked forms above
 * -- operators, status codes, workspace, determinism, job independence, two launches per Adam iteration -- plus:
 *   masks       (n_mask, H, W) uint8 device memory, packed with no padding: plane k starts at byte k H W (odd for odd
 *               H W; the kernels read bytes, no alignment is assumed).  As t2o_rle_union_u8 writes them.
 *   mask_index  HOST array like ops: -1 = no mask for job j, 0 .. n_mask - 1 = a plane; anything else is T2O_EINVAL.
 *               masks may be NULL only when every index is -1.
 * Forward, per pixel and channel: out = clamp01(z m + x (1 - m)), z = the operator's unclamped output, x = the input
 * value, m = (float) of the mask byte -- a COUNT (overlapping annotated masks give 2), NOT divided by 255: what
 * t2o_mask_select hands the episode, so a planned step replayed under the same plane gives the same picture.  The
 * sharpness stencil reads the unmasked neighbours of the image.  Backward (the fit): g_z = sign(out - t) inv_n m, zero where
 * the BLENDED value lies outside [0, 1]; the parameter terms are the unmasked closed forms times that g_z.
 * A job with index -1, and a job under an all-ones plane, return the unmasked forms' numbers bit for bit (z 1 + x 0 = z
 * for finite fp32); a call whose indices are all -1 runs the unmasked kernels themselves.  Under an all-zero plane the
 * gradient is exactly zero and the fit returns its start values.  The workspace sizes equal the unmasked ones. */
size_t t2o_candidates_multi_masked_workspace_bytes(int J, int C, int H, int W);
int t2o_op_candidates_multi_l1_masked(const int* ops, const int* img_index, const int* mask_index, int J,
                                      const float* imgs, int n_img, const unsigned char* masks, int n_mask,
                                      const float* target, const float* params, int C, int param_stride, float* loss,
                                      void* workspace, size_t workspace_bytes, int H, int W, void* stream);
size_t t2o_fit_multi_masked_workspace_bytes(int J, int H, int W);
int t2o_fit_multi_l1_adam_masked(const int* ops, const int* img_index, const int* target_index, const int* mask_index,
                                 int J, const float* imgs, int n_img, const float* targets, int n_target,
                                 const unsigned char* masks, int n_mask, float* params, float* dist, void* workspace,
                                 size_t workspace_bytes, int H, int W, int steps, double lr, double beta1, double beta2,
                                 double eps, int check_every, double tol, void* stream);

/* ---- SSIM: utils/ssim/__init__.py:20-40 (forward: the evaluation metric; backward: its closed-form gradient) ----
 * 11x11 Gaussian window (sigma 1.5), zero padding, C1 = 1e-4, C2 = 9e-4.
 * out[b] = mean over (C,H,W) of the SSIM map of sample b (size_average=False of the reference;
 * its size_average=True is the mean of out).  workspace: t2o_ssim_workspace_bytes(B,C,H,W). */
size_t t2o_ssim_workspace_bytes(int B, int C, int H, int W);
int t2o_ssim_fwd(const float* img1, const float* img2, float* out,
                 void* workspace, size_t workspace_bytes, int B, int C, int H, int W, void* stream);
/* Backward of t2o_ssim_fwd (the reference differentiates utils/ssim/__init__.py:20-40 by autograd; there is no reference
 * kernel): gout (B) = gradient w.r.t. out[b]; g1 / g2 (B,C,H,W) = gradients w.r.t. img1 / img2, either may be NULL.
 * One launch, one workgroup per 32 x 32 tile of a plane; the four derivative maps live in LDS only.  Writes (does not
 * accumulate); no workspace; deterministic. */
int t2o_ssim_bwd(const float* img1, const float* img2, const float* gout, float* g1, float* g2,
                 int B, int C, int H, int W, void* stream);

/* ---- dot-product attention core, models/attention.py:37-40 ----
 * q (B,D), ctx (B,L,D) -> attn (B,L) = softmax_l(q . ctx_l) over ALL L rows (no padding
 * mask, as the reference), mix (B,D) = sum_l attn_l ctx_l.   D % 64 == 0, D <= 1024, L <= 64 */
int t2o_attn_fwd(const float* q, const float* ctx, float* attn, float* mix,
                 int B, int L, int D, void* stream);
/* gmix (B,D), gattn (B,L) nullable -> gq (B,D), gctx (B,L,D) */
int t2o_attn_bwd(const float* q, const float* ctx, const float* attn, const float* gmix,
                 const float* gattn, float* gq, float* gctx, int B, int L, int D, void* stream);

/* ---- choice of the next operator in the free-running decode, models/actor.py:222-236 (one launch for: exp, explore
 * mix, op-mask, renormalisation, Categorical draw or arg-max, op-mask update).  logp (B,n) log-probabilities, op_mask
 * (B,n) in/out (the chosen entry is cleared), u (B) uniform [0,1) numbers or NULL for arg-max, pred_op (B) int64
 * operator-vocabulary ids, exec_op (B) int32 = pred_op - 3 (the executor index t2o_apply_* takes; negative = identity). */
int t2o_choose_op(const float* logp, float* op_mask, const float* u, float explore_prob, long long* pred_op, int* exec_op,
                  int B, int n_cls, void* stream);

/* ---- training-mode BatchNorm2d fused with the residual add and ReLU that follow it in the image
 * encoder: models/actor_resnet.py:38-44 (BasicBlock.forward: relu(bn1(conv1(x))), relu(bn2(conv2(.)) +
 * shortcut(x))) and :99-100 (stem).  x, res, out: (N,C,H*W) contiguous NCHW; HW = H*W.
 *   out = max((x - mean_c) * invstd_c * weight_c + bias_c (+ res), 0), batch statistics per channel
 *   (biased variance), running_mean / running_var (nullable, both or neither) updated in place with
 *   `momentum` and the unbiased variance, as torch.nn.BatchNorm2d in training mode.
 * save_mean / save_invstd (C) are written for the backward.  workspace: t2o_bn_workspace_bytes(N, C). */
size_t t2o_bn_workspace_bytes(int N, int C);
int t2o_bn_relu_fwd(const float* x, const float* res, const float* weight, const float* bias,
                    float* running_mean, float* running_var, float* save_mean, float* save_invstd, float* out,
                    float momentum, float eps, void* workspace, size_t workspace_bytes,
                    int N, int C, int HW, void* stream);
/* dy = gradient w.r.t. out.  has_res = 1: a residual was added (y = the forward's out is needed for the ReLU
 * mask; dres (nullable) receives the residual's gradient); has_res = 0: the mask is recomputed from x, y may
 * be NULL.  dx (N,C,HW), dweight / dbias (C, nullable). */
int t2o_bn_relu_bwd(const float* x, const float* y, const float* dy, const float* weight, const float* bias,
                    const float* save_mean, const float* save_invstd, float* dx, float* dres,
                    float* dweight, float* dbias, int has_res, void* workspace, size_t workspace_bytes,
                    int N, int C, int HW, void* stream);

/* The same pair on channels-last activations: x, res, out, y, dy, dx, dres are (M, C) with M = N*H*W rows of C
 * contiguous channels (torch.channels_last storage of an (N,C,H,W) tensor), the layout the convolutions run in
 * natively on MI355X.  C must be a power of two in [4, 1024].  Same arithmetic, same running-statistics update.
 * relu = 0: plain batch norm without the activation (the shortcut branch, models/actor_resnet.py:33-36).
 * workspace: t2o_bn_nhwc_workspace_bytes(M, C). */
size_t t2o_bn_nhwc_workspace_bytes(int M, int C);
int t2o_bn_relu_nhwc_fwd(const float* x, const float* res, const float* weight, const float* bias,
                         float* running_mean, float* running_var, float* save_mean, float* save_invstd, float* out,
                         float momentum, float eps, int relu, void* workspace, size_t workspace_bytes,
                         int M, int C, void* stream);
/* t2o_bn_relu_nhwc_fwd with the batch statistics taken from per-tile partial sums a producer already holds
 * (t2o_conv3x3_fwd_stats_nhwc: the convolution's accumulators) instead of a pass over x: partial is
 * (partial_rows, 2, C) fp32 -- per row the channels' sums, then their sums of squares -- combined in fp64 in row order.
 * Everything else as t2o_bn_relu_nhwc_fwd. */
int t2o_bn_relu_nhwc_fwd_partials(const float* x, const float* res, const float* weight, const float* bias, float* running_mean,
                                  float* running_var, float* save_mean, float* save_invstd, float* out, float momentum,
                                  float eps, int relu, const float* partial, int partial_rows, void* workspace,
                                  size_t workspace_bytes, int M, int C, void* stream);
int t2o_bn_relu_nhwc_bwd(const float* x, const float* y, const float* dy, const float* weight, const float* bias,
                         const float* save_mean, const float* save_invstd, float* dx, float* dres,
                         float* dweight, float* dbias, int has_res, int relu, void* workspace,
                         size_t workspace_bytes, int M, int C, void* stream);

/* ---- 3x3 stride-1 padding-1 convolution of the image encoder, weight gradient (models/actor_resnet.py:27-44,
 * the BasicBlock convolutions) on the fp32 matrix cores (t2o_conv.hip).  Replaces the library's weight-gradient call
 * (torch.ops.aten.convolution_backward, output_mask [0,1,0]) for these layers.
 *   x  (N,H,W,Ci) and dy (N,H,W,Co): NHWC = torch.channels_last storage of (N,C,H,W) tensors
 *   dw (Co,3,3,Ci)                 = channels_last storage of a (Co,Ci,3,3) weight gradient
 *   dw[co][kh][kw][ci] = sum_{n,h,w} dy[n][h][w][co] * x[n][h+kh-1][w+kw-1][ci]   (zero padding)
 * Ci and Co must be multiples of 64, W a multiple of 4.  Deterministic: split-K partial sums in `workspace`
 * (t2o_conv3x3_wgrad_workspace_bytes) are added in a fixed order. */
size_t t2o_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Ci, int Co);
int t2o_conv3x3_wgrad_nhwc(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                           int N, int H, int W, int Ci, int Co, void* stream);

/* ---- the same convolutions, forward and data gradient (t2o_conv.hip: one implicit-GEMM kernel on the fp32 matrix
 * cores; the data gradient runs it on dy with the transposed, tap-mirrored weight).  Replace F.conv2d(x, w, None, 1, 1)
 * (models/actor_resnet.py:27-30 conv3x3) and torch.ops.aten.convolution_backward(..., output_mask [1,0,0]).
 *   y[n][h][w][co]  = sum_{kh,kw,ci} x[n][h+kh-1][w+kw-1][ci] * w[co][kh][kw][ci]        (zero padding)
 *   dx[n][h][w][ci] = sum_{kh,kw,co} dy[n][h-kh+1][w-kw+1][co] * w[co][kh][kw][ci]
 * Tensors as above (NHWC activations, (Co,3,3,Ci) weight).  Forward: Ci % 32 == 0, Co % 64 == 0; data gradient:
 * Co % 32 == 0, Ci % 64 == 0; both: W % 8 == 0.  `workspace` holds a zero region (padding source of the LDS-DMA)
 * and, for the data gradient, the transformed weight; it is (re)written by every call. */
size_t t2o_conv3x3_fwd_workspace_bytes(int N, int H, int W, int Ci, int Co);
int t2o_conv3x3_fwd_nhwc(const float* x, const float* w, float* y, void* workspace, size_t workspace_bytes,
                         int N, int H, int W, int Ci, int Co, void* stream);
size_t t2o_conv3x3_dgrad_workspace_bytes(int N, int H, int W, int Ci, int Co);
int t2o_conv3x3_dgrad_nhwc(const float* dy, const float* w, float* dx, void* workspace, size_t workspace_bytes,
                           int N, int H, int W, int Ci, int Co, void* stream);

/* ---- forward of the stride-2 3x3 convolutions (F.conv2d(x, w, None, 2, 1), models/actor_resnet.py:32-36 with stride 2):
 *   y[n][a][b][co] = sum_{kh,kw,ci} x[n][2a+kh-1][2b+kw-1][ci] * w[co][kh][kw][ci]      (zero padding)
 *   x (N,2Ho,2Wo,Ci), w (Co,3,3,Ci), y (N,Ho,Wo,Co).  Ci % 32 == 0, Co % 64 == 0, Wo % 8 == 0. */
size_t t2o_conv3x3s2_fwd_workspace_bytes(int N, int Ho, int Wo, int Ci, int Co);
int t2o_conv3x3s2_fwd_nhwc(const float* x, const float* w, float* y, void* workspace, size_t workspace_bytes,
                           int N, int Ho, int Wo, int Ci, int Co, void* stream);

/* The forward convolution (stride 1 or 2, shapes as t2o_conv3x3_fwd_nhwc / t2o_conv3x3s2_fwd_nhwc; Ho, Wo = output
 * grid) that also leaves the batch-norm statistics of its output: stats is (rows, 2, Co) fp32 with rows =
 * t2o_conv3x3_fwd_stats_rows(...) -- per pixel tile the per-channel sum and sum of squares of y, summed in a fixed
 * order from the accumulators -- the input of t2o_bn_relu_nhwc_fwd_partials.  Replaces conv2d + the statistics half
 * of BatchNorm2d (models/actor_resnet.py:38-44: bn(conv(x))): the activation is not read back for its mean. */
int t2o_conv3x3_fwd_stats_rows(int N, int Ho, int Wo, int Co, int stride);
int t2o_conv3x3_fwd_stats_nhwc(const float* x, const float* w, float* y, float* stats, void* workspace, size_t workspace_bytes,
                               int N, int Ho, int Wo, int Ci, int Co, int stride, void* stream);

/* Forward of the image encoder's stem, conv2d(x, w, None, stride 2, padding 1) with 3 input and 32 / 64 output channels
 * (models/actor_resnet.py:99): x (N, 2Ho, 2Wo, 3), w (Co,3,3,3) channels-last, y (N, Ho, Wo, Co).  stats: null, or
 * (t2o_stem_fwd_stats_rows(N, Ho, Wo), 2, Co) per-workgroup channel sums / sums of squares of y for
 * t2o_bn_relu_nhwc_fwd_partials (the stem's batch norm then makes no statistics pass over its 268 MB at bs=64). */
int t2o_stem_fwd_stats_rows(int N, int Ho, int Wo);
int t2o_stem_fwd_nhwc(const float* x, const float* w, float* y, float* stats, int N, int Ho, int Wo, int Co, void* stream);

/* Weight gradient of the same stem convolution: x (N, 2Ho, 2Wo, 3), dy (N, Ho, Wo, Co) -> dw (Co,3,3,3) channels-last.
 * Deterministic (per-workgroup partial blocks in the workspace, added in order), unlike the atomic kernel the library
 * picks for this layer.  Workspace: t2o_stem_wgrad_workspace_bytes. */
size_t t2o_stem_wgrad_workspace_bytes(int N, int Ho, int Wo, int Co);
int t2o_stem_wgrad_nhwc(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes, int N, int Ho, int Wo,
                        int Co, void* stream);

/* ---- weight gradient of the same stride-2 convolutions (t2o_conv.hip, the stride-1 kernel with a two-plane x tile):
 *   dw[co][kh][kw][ci] = sum_{n,a,b} dy[n][a][b][co] * x[n][2a+kh-1][2b+kw-1][ci]   (zero padding)
 *   x (N,2Ho,2Wo,Ci), dy (N,Ho,Wo,Co), dw (Co,3,3,Ci).  Ci, Co multiples of 64, Wo a multiple of 4.  Deterministic
 *   (fixed-order split-K), replaces convolution_backward(..., stride 2, output_mask [0,1,0]). */
size_t t2o_conv3x3s2_wgrad_workspace_bytes(int N, int Ho, int Wo, int Ci, int Co);
int t2o_conv3x3s2_wgrad_nhwc(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                             int N, int Ho, int Wo, int Ci, int Co, void* stream);

/* Optional: register `bytes` of device memory on `device` that hold zeros and that nobody writes while convolutions
 * run (NULL unregisters).  The t2o_conv3x3* calls then read their padding from it instead of clearing the zero
 * region at the start of their workspace on every call (it must be at least that large, 20 KiB covers the
 * encoder; smaller: ignored).  Process-wide state, set before the calls it should affect. */
int t2o_conv_set_zero_region(int device, const void* zeros, size_t bytes);

/* ---- data gradient of the encoder's STRIDE-2 3x3 convolutions (the first convolution of each stage,
 * models/actor_resnet.py:32-36 with stride 2; replaces torch.ops.aten.convolution_backward(..., output_mask [1,0,0])):
 *   dx[n][i][j][ci] = sum_{kh,kw,co} dy[n][(i+1-kh)/2][(j+1-kw)/2][co] * w[co][kh][kw][ci]   over the taps for which
 *   both quotients are integers inside the (Ho, Wo) grid.   dy (N,Ho,Wo,Co), w (Co,3,3,Ci), dx (N,2Ho,2Wo,Ci), NHWC.
 * Co % 32 == 0, Ci % 64 == 0, Wo % 8 == 0.  `workspace`: zero region + the transposed weight, rewritten per call. */
size_t t2o_conv3x3s2_dgrad_workspace_bytes(int N, int Ho, int Wo, int Ci, int Co);
int t2o_conv3x3s2_dgrad_nhwc(const float* dy, const float* w, float* dx, void* workspace, size_t workspace_bytes,
                             int N, int Ho, int Wo, int Ci, int Co, void* stream);

/* ---- operator parameter heads for a batch whose samples use different operators: models/operators.py:73-88
 * (param = op_param_regressor(fc2(LeakyReLU_0.01(fc1(features))))) as called per operator group by
 * models/actor.py:244-255.  op_id (B) device int32: executor index of each sample, < 0 or 4 -> no head, zeros.
 * w1/b1/w2/b2: HOST arrays of 8 device pointers indexed by executor index (entry 4 may be NULL): fc1 (512,512) /
 * (512), fc2 (n,512) / (n), n = 1, 8 (tone) or 24 (color).  ctx (B,512) -> param (B,24) zero padded; hidden (B,512)
 * and raw (B,24) are written for the backward.  Regressor constants: brightness_range, saturation_range (lo, hi),
 * sharpness_range of the options.  D must be 512. */
int t2o_param_heads_fwd(const int* op_id, const float* ctx, const float* const* w1, const float* const* b1,
                        const float* const* w2, const float* const* b2, float* hidden, float* raw, float* param,
                        float brightness_range, float sat_lo, float sat_hi, float sharpness_range, int B, int D,
                        void* stream);
/* gparam (B,24) -> gctx (B,512) and DENSE gradients of every head (gw1 .. gb2: HOST arrays of 8 device pointers;
 * heads no sample selected receive zeros).  dpre (B,512): scratch.  Deterministic (batch-order sums). */
int t2o_param_heads_bwd(const int* op_id, const float* ctx, const float* const* w1, const float* const* b1,
                        const float* const* w2, const float* const* b2, const float* hidden, const float* raw,
                        const float* gparam, float* gctx, float* dpre, float* const* gw1, float* const* gb1,
                        float* const* gw2, float* const* gb2, float brightness_range, float sat_lo, float sat_hi,
                        float sharpness_range, int B, int D, void* stream);
/* The same with accumulate != 0: the heads' weight gradients are ADDED to gw1 / gb1 / gw2 / gb2 (every element has
 * exactly one writer: still deterministic).  For a trainer whose gradient buffers are persistent and zeroed before
 * the backward: the 28 gradient tensors of a decoder step then need no accumulation launches of their own
 * (140 per episode step under autograd). */
int t2o_param_heads_bwd_acc(const int* op_id, const float* ctx, const float* const* w1, const float* const* b1,
                        const float* const* w2, const float* const* b2, const float* hidden, const float* raw,
                        const float* gparam, float* gctx, float* dpre, float* const* gw1, float* const* gb1,
                        float* const* gw2, float* const* gb2, float brightness_range, float sat_lo, float sat_hi,
                        float sharpness_range, int B, int D, int accumulate, void* stream);

/* ---- round 3: the forms the encoder's explicit forward/backward schedule (t2onet_amd/encoder.py) calls ----
 * Gradient buffers of a trainer are persistent and zeroed once per step, so the weight-gradient kernels can ADD their
 * result (accumulate != 0; every element has one writer: still deterministic) instead of handing a fresh tensor to an
 * accumulation launch; transformed weights are made once per optimiser step, not once per data-gradient call. */

/* t2o_bn_relu_nhwc_bwd with accumulate: dweight / dbias += instead of = (models/actor_resnet.py:38-44 backward). */
int t2o_bn_relu_nhwc_bwd_acc(const float* x, const float* y, const float* dy, const float* weight, const float* bias,
                             const float* save_mean, const float* save_invstd, float* dx, float* dres, float* dweight,
                             float* dbias, int has_res, int relu, int accumulate, void* workspace, size_t workspace_bytes,
                             int M, int C, void* stream);
/* ... with the sums supplied by the producer of dy (see t2o_conv3x3_dgrad_pre_bnsums_nhwc): finalize + apply only; no residual. */
int t2o_bn_relu_nhwc_bwd_partials_acc(const float* x, const float* dy, const float* weight, const float* bias,
                                      const float* save_mean, const float* save_invstd, float* dx, float* dweight,
                                      float* dbias, int relu, int accumulate, const float* partial, int partial_rows,
                                      void* workspace, size_t workspace_bytes, int M, int C, void* stream);

/* Weight gradient of a 3x3 convolution, stride 1 or 2 ((N,Ho,Wo) = the dy grid; shapes / workspace as
 * t2o_conv3x3_wgrad_nhwc / t2o_conv3x3s2_wgrad_nhwc); accumulate != 0: dw += . */
int t2o_conv3x3_wgrad_acc_nhwc(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                               int N, int Ho, int Wo, int Ci, int Co, int stride, int accumulate, void* stream);

/* wt[ci][t'][co] = w[co][t][ci] for a (Co, taps, Ci) weight, t' = taps-1-t when flip != 0 else t.  taps = 9, flip = 1: the
 * weight the stride-1 data gradient runs the forward kernel with; taps = 9, flip = 0: the stride-2 data gradient's;
 * taps = 1: the transposed 1x1 shortcut weight.  Co, Ci multiples of 32. */
int t2o_conv_weight_transform(const float* w, float* wt, int Co, int Ci, int taps, int flip, void* stream);
/* n <= 32 of them in one launch (HOST arrays of length n): an encoder's 20 weights once per optimiser step */
int t2o_conv_weight_transform_batch(const float* const* w, float* const* wt, const int* Co, const int* Ci, const int* taps,
                                    const int* flip, int n, void* stream);

/* t2o_conv3x3_dgrad_nhwc with the transformed weight supplied (wt from t2o_conv_weight_transform(w, wt, Co, Ci, 9, 1))
 * and an optional addend (N,H,W,Ci) added to dx in the kernel's epilogue: the gradient a BasicBlock's input receives
 * through the identity shortcut (models/actor_resnet.py:43 `out += self.shortcut(x)`), so no separate add pass.
 * workspace: t2o_conv3x3_fwd_workspace_bytes(N, H, W, Co, Ci) (the zero region only). */
int t2o_conv3x3_dgrad_pre_nhwc(const float* dy, const float* wt, const float* addend, float* dx, void* workspace,
                               size_t workspace_bytes, int N, int H, int W, int Ci, int Co, void* stream);
/* The same data gradient (no addend) in front of y = relu(bn(bn_x)) -- a BasicBlock's second convolution, models/actor_resnet.py:
 * 38-44: the epilogue ALSO leaves the batch norm's backward sums, rows (t2o_conv3x3_dgrad_bnsums_rows(...), 2, Ci): per pixel
 * tile the channels' sums of g = dx * [bn_x * gamma * invstd + (beta - mean * gamma * invstd) > 0] and of g * xhat, the gate
 * evaluated exactly as t2o_bn_relu_nhwc_bwd does.  Feed them to t2o_bn_relu_nhwc_bwd_partials_acc: that batch norm's own
 * sums pass (one read of dx and one of bn_x) is not launched; bn_x is fetched under the last loop iteration's MFMAs. */
int t2o_conv3x3_dgrad_bnsums_rows(int N, int H, int W, int Ci, int Co);
int t2o_conv3x3_dgrad_pre_bnsums_nhwc(const float* dy, const float* wt, float* dx, const float* bn_x,
                                      const float* save_mean, const float* save_invstd, const float* weight,
                                      const float* bias, float* rows, void* workspace, size_t workspace_bytes,
                                      int N, int H, int W, int Ci, int Co, void* stream);
/* t2o_conv3x3s2_dgrad_nhwc with wt = t2o_conv_weight_transform(w, wt, Co, Ci, 9, 0) supplied. */
int t2o_conv3x3s2_dgrad_pre_nhwc(const float* dy, const float* wt, float* dx, void* workspace, size_t workspace_bytes,
                                 int N, int Ho, int Wo, int Ci, int Co, void* stream);

/* The stem (models/actor_resnet.py:99, conv 3 -> 32 / 64, stride 2) reading / writing the image in its own layout:
 * planar != 0: x / dx are (N,3,2Ho,2Wo) NCHW (what the operators produce: no channels-last copy of the image per encoder
 * call); planar == 0: (N,2Ho,2Wo,3).  y / dy are (N,Ho,Wo,Co) NHWC, w (Co,3,3,3) channels-last.  accumulate != 0: the
 * weight gradient is added to dw, the data gradient to dx (the image gradient already holds the operator's part). */
int t2o_stem_fwd(const float* x, const float* w, float* y, float* stats, int N, int Ho, int Wo, int Co, int planar, void* stream);
/* forward for an input of ANY size (Hi, Wi; Ho = (Hi+1)/2): full-resolution inference images have odd sizes */
int t2o_stem_fwd_any(const float* x, const float* w, float* y, float* stats, int N, int Hi, int Wi, int Co, int planar, void* stream);
int t2o_stem_wgrad(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes, int N, int Ho, int Wo,
                   int Co, int planar, int accumulate, void* stream);
int t2o_stem_dgrad(const float* dy, const float* w, float* dx, int N, int Ho, int Wo, int Co, int planar, int accumulate, void* stream);

/* ---- the 1x1 stride-2 shortcut convolutions of the encoder's stages (models/actor_resnet.py:33-36: nn.Conv2d(in, out,
 * kernel_size=1, stride=stride, bias=False)), fp32 matrix cores (t2o_conv1x1.hip).  Ho = (H+1)/2, Wo = (W+1)/2.
 *   forward        y[n][a][b][co]    = sum_ci x[n][2a][2b][ci] * w[co][ci]                x (N,H,W,Ci), w (Co,Ci), y (N,Ho,Wo,Co)
 *   data gradient  dx[n][2a][2b][ci] += sum_co dy[n][a][b][co] * w[co][ci]                ADDS into an existing dx (the 3x3
 *                  branch's data gradient, which covers every pixel); wt (Ci,Co) = t2o_conv_weight_transform(w, wt, Co, Ci, 1, 0)
 *   weight gradient dw[co][ci]       (+)= sum_{n,a,b} dy[n][a][b][co] * x[n][2a][2b][ci]   deterministic split-K
 * Ci, Co multiples of 64.  Replace F.conv2d(x, w, None, 2) and both halves of convolution_backward for these layers
 * (the library's kernels add atomically and need their output cleared first). */
int t2o_conv1x1s2_fwd_nhwc(const float* x, const float* w, float* y, int N, int H, int W, int Ci, int Co, void* stream);
int t2o_conv1x1s2_dgrad_acc_nhwc(const float* dy, const float* wt, float* dx, int N, int H, int W, int Ci, int Co, void* stream);
size_t t2o_conv1x1s2_wgrad_workspace_bytes(int N, int H, int W, int Ci, int Co);
int t2o_conv1x1s2_wgrad_nhwc(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                             int N, int H, int W, int Ci, int Co, int accumulate, void* stream);

/* ---- the same 3x3 convolutions (padding 1, stride 1 or 2) for ANY image size (t2o_conv_generic.hip): gathered-row
 * implicit GEMMs on the fp32 matrix cores, about half the rate of the LDS-DMA kernels above, for the layers those
 * cannot take (image width not a multiple of 8 / 4, odd sizes under stride 2: the 4 x 4 stage of a 128 x 128 training
 * image, every stage of a full-resolution inference image) -- replaces the library fall-back there, deterministic.
 *   forward        x (N,H,W,Ci), w (Co,3,3,Ci) -> y (N,Ho,Wo,Co), Ho = (H-1)/stride + 1
 *   data gradient  dy (N,Ho,Wo,Co), wt = t2o_conv_weight_transform(w, wt, Co, Ci, 9, stride == 1) -> dx (N,H,W,Ci)
 *                  (+ addend (N,H,W,Ci), nullable)
 *   weight gradient x, dy -> dw (Co,3,3,Ci), split-K partials in `workspace`, accumulate != 0: dw +=
 * Ci % 32 == 0 (weight gradient: % 64), Co % 64 == 0 (data gradient: Co % 32, Ci % 64). */
int t2o_conv3x3_any_fwd_nhwc(const float* x, const float* w, float* y, int N, int H, int W, int Ci, int Co, int stride, void* stream);
int t2o_conv3x3_any_dgrad_nhwc(const float* dy, const float* wt, const float* addend, float* dx, int N, int H, int W, int Ci, int Co,
                               int stride, void* stream);
size_t t2o_conv3x3_any_wgrad_workspace_bytes(int N, int H, int W, int Ci, int Co, int stride);
int t2o_conv3x3_any_wgrad_nhwc(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                               int N, int H, int W, int Ci, int Co, int stride, int accumulate, void* stream);

/* ---- Winograd F(2x2, 3x3) for the stride-1 3x3 convolutions of the deep encoder stages (t2o_winograd.hip transforms,
 * t2o_conv.hip GEMMs; models/actor_resnet.py:24-44, the 256- and 512-channel BasicBlocks).  y = conv2d(x, w, None, 1, 1),
 * NHWC, H and W even, T = N * H/2 * W/2 output tiles, Tpad = t2o_wino_padded_tiles(N,H,W) (T rounded up to 256):
 *   U (16, Co, Ci)   = t2o_wino_weight_transform(w (Co,3,3,Ci), Cn = Co, Ck = Ci)                once per weight update
 *   V (16, Tpad, Ci) = t2o_wino_input_transform(x (N,H,W,Ci))                                     rows T.. are zero
 *   M (16, T, Co)    = t2o_gemm_nt_batched(V, U, M, 16, T, Co, Ci, Tpad)                          M[xi] = V[xi] U[xi]^T
 *   y (N,H,W,Co)     = t2o_wino_output_transform(M, addend, y, stats)
 * addend: null or (N,H,W,Co), added to y (the gradient through a block's identity shortcut, as in
 * t2o_conv3x3_dgrad_pre_nhwc); stats: null or (t2o_wino_stats_rows(N,H,W,Co), 2, Co) per-workgroup channel sums / sums
 * of squares of y for t2o_bn_relu_nhwc_fwd_partials (as t2o_conv3x3_fwd_stats_nhwc).  The data gradient is the same
 * pipeline on dy with U = t2o_wino_weight_transform(wt, Cn = Ci, Ck = Co), wt = t2o_conv_weight_transform(w, ., Co, Ci, 9, 1).
 * Weight gradient (in the transformed domain, deterministic):
 *   Ad (16, Tpad, Co)      = t2o_wino_dy_transform(dy (N,H,W,Co))                                 A dY A^T, rows T.. zero
 *   dU (splits, 16, Co, Ci) = t2o_gemm_tn_batched(Ad, V, dU, 16, Tpad, Co, Ci, splits)            dU[xi] = Ad[xi]^T V[xi]
 *                            splits = t2o_gemm_tn_splits(16, Tpad, Co, Ci): pieces of the tile range (fixed partition)
 *   dw (Co,3,3,Ci)  (+)=   t2o_wino_dw_transform(dU, dw, Co, Ci, splits, accumulate)              G^T (sum of the pieces) G
 * C: a power of two in [4, 1024] for the transforms; the GEMMs: t2o_gemm_nt_batched N % 64 == 0, K % 32 == 0;
 * t2o_gemm_tn_batched M, N % 128 == 0, rows % (64 * splits) == 0; all tensors 16-byte aligned. */
int t2o_wino_padded_tiles(int N, int H, int W);
int t2o_wino_weight_transform(const float* w, float* U, int Cn, int Ck, void* stream);
int t2o_wino_weight_transform_batch(const float* const* w, float* const* U, const int* Cn, const int* Ck, int n, void* stream);   /* n <= 32 banks, one launch */
/* ... straight into the chunk-major layout (Ck/8, 16, Cn, 8) of t2o_wino_fused_conv_nhwc (= t2o_wino_u_chunked of the above) */
int t2o_wino_weight_transform_chunked_batch(const float* const* w, float* const* Uc, const int* Cn, const int* Ck, int n, void* stream);
int t2o_wino_input_transform(const float* x, float* V, int N, int H, int W, int C, void* stream);
/* the same into rows [0, Tpad) of every plane of a LARGER (16, plane_rows, C) tensor whose first plane starts at V (a train
 * step's passes side by side: the weight gradient then runs once over all of them); plane_rows = 0: Tpad */
int t2o_wino_input_transform_ld(const float* x, float* V, int N, int H, int W, int C, int plane_rows, void* stream);
int t2o_wino_stats_rows(int N, int H, int W, int C);
int t2o_wino_output_transform(const float* M, const float* addend, float* y, float* stats, int N, int H, int W, int C, void* stream);
int t2o_wino_dy_transform(const float* dy, float* Ad, int N, int H, int W, int C, void* stream);
/* t2o_wino_input_transform(dy) and t2o_wino_dy_transform(dy) in one pass over dy (a layer's backward needs both) */
int t2o_wino_dy_transforms(const float* dy, float* V, float* Ad, int N, int H, int W, int C, void* stream);
int t2o_wino_dy_transforms_ld(const float* dy, float* V, float* Ad, int N, int H, int W, int C, int ad_plane_rows, void* stream);
/* A dY A^T alone into a row range of a larger (16, plane_rows, C) tensor (the data gradient then runs on t2o_wino_fused_conv_nhwc) */
int t2o_wino_dy_transform_ld(const float* dy, float* Ad, int N, int H, int W, int C, int plane_rows, void* stream);   /* Ad as a row range of a (16, ad_plane_rows, C) tensor */
int t2o_wino_dw_transform(const float* dU, float* dw, int Co, int Ci, int splits, int accumulate, void* stream);
/* the batched fp32 matrix-core GEMMs behind them (t2o_conv.hip k_gemm_nt / k_gemm_tn: the forward convolution's LDS-DMA
 * machinery without taps), dense row-major operands:
 *   nt: C[b] (M,N) = A[b] (a_rows >= M rows of K) * B[b] (N,K)^T          for b < batches
 *   tn: C[s][b] (M,N) = sum over the rows t of piece s of A[b] (rows,M)[t]^T B[b] (rows,N)[t]   for s < splits, b < batches */
int t2o_gemm_nt_batched(const float* A, const float* B, float* C, int batches, int M, int N, int K, int a_rows, void* stream);
int t2o_gemm_tn_splits(int batches, int rows, int M, int N);
int t2o_gemm_tn_batched(const float* A, const float* B, float* C, int batches, int rows, int M, int N, int splits, void* stream);
/* ... with A / B row ranges [0, rows) of every plane of LARGER (batches, a_plane_rows | b_plane_rows, .) tensors: the weight
 * gradient over the first passes of a train step's V / A dY A^T arenas when a step used fewer passes than the arena holds */
int t2o_gemm_tn_batched_ld(const float* A, const float* B, float* C, int batches, int rows, int a_plane_rows, int b_plane_rows, int M, int N,
                           int splits, void* stream);

/* ---- LSTM layers of the request encoder (models/lang_encoder.py:70-113: 2-layer bidirectional LSTM over packed, i.e.
 * per-sample-length, sequences; nn.LSTM gate order i, f, g, o), one launch per time step for both directions (t2o_rnn.hip).
 *   gi    (B, L, D*4H)  x W_ih^T for every step and direction (a library GEMM), no bias
 *   whh_t (D, H, H, 4)  whh_t[d][k][j][g] = W_hh[d][g*H + j][k]  (forward);   whh (D, H, H, 4): whh[d][c][k][q] =
 *                       W_hh[d][4*c + q][k]  (backward) -- both 16-byte-load repackings of nn.LSTM's (4H, H) weight;
 *                       b_ih / b_hh (D, 4H) nullable
 *   len   (B) int64     valid lengths on the DEVICE: a sample's state stops changing at its last token (direction 0) /
 *                       starts from zero there (direction 1), outputs are zero at pads -- what pack_padded_sequence ->
 *                       LSTM -> pad_packed_sequence computes, without the length sort and without host-side lengths
 *   out   (B, L, D*H);  hnew, cnew (L, D, B, H): state after processing time t (final state: t = L-1 for direction 0,
 *                       t = 0 for direction 1);  gates (L, D, B, 4H): post-activation gates, kept for the backward.
 * Backward: dout (B, L, D*H), dhn / dcn (D, B, H) nullable -> dgates (L, D, B, 4H) = gradients of the gate pre-activations
 * (weight, bias and input gradients are GEMMs / sums over them: host side); carry_h, dc (D, B, H): scratch.
 * H % 64 == 0, H <= 256, D in {1, 2}. */
int t2o_lstm_layer_fwd(const float* gi, const float* whh_t, const float* b_ih, const float* b_hh, const long long* len,
                       float* out, float* hnew, float* cnew, float* gates, int B, int L, int H, int D, void* stream);
int t2o_lstm_layer_bwd(const float* whh, const long long* len, const float* cnew, const float* gates, const float* dout,
                       const float* dhn, const float* dcn, float* dgates, float* carry_h, float* dc,
                       int B, int L, int H, int D, void* stream);

/* ---- image feature head: models/actor.py:50,142-143,215-216  feat = relu(bn1(vis_encoder.fc(pooled))) -- Linear(K -> D),
 * BatchNorm1d(D) in training (batch statistics over the B rows, running statistics updated as torch does: momentum,
 * unbiased variance, num_batches_tracked += 1) or evaluation mode, ReLU -- one launch (a workgroup owns 16 feature
 * columns of the whole batch, so the statistics never leave it).  B <= 64, K % 4 == 0, D % 4 == 0 (forward and backward
 * alike: the backward's products read d_fc in 16-byte pieces); rows 16-byte aligned.
 * Backward: g_feat -> d_fc (gradient of the Linear's output, kept for the caller's weight-gradient product
 * d_fc^T . pooled), d_bn (2, D) = [d weight; d bias] of the batch norm, d_pooled = d_fc . fc_w (skipped when NULL). */
typedef struct t2o_image_feature {
  const float *fc_w, *fc_b;                    /* (D, K), (D) nullable */
  const float *bn_w, *bn_b;                    /* (D) nullable (affine=False) */
  float *running_mean, *running_var;           /* (D); nullable in training mode (no update) */
  long long* num_batches_tracked;              /* nullable */
  const float* pooled;                         /* (B, K) */
  float* pooled_copy;                          /* nullable: (B, K) copy for the caller's weight-gradient product */
  float *fc_out, *stats, *feat;                /* (B, D) pre-norm, (2, D) = mean, 1/std, (B, D) */
  const float* g_feat;                         /* backward: (B, D) */
  float *d_fc, *d_bn, *d_pooled;               /* (B, D), (2, D), (B, K) nullable */
  float momentum, eps;
  int training, B, K, D;
} t2o_image_feature_t;
int t2o_image_feature_fwd(const t2o_image_feature_t* args, void* stream);
int t2o_image_feature_bwd(const t2o_image_feature_t* args, void* stream);

/* ---- one decoding step: models/action_decoder.py:38-64 Decoder.forward_step with models/attention.py:17-44 inside --
 *   step_in = [embedding[prev_op] (E) | relu(vis_linear(feat)) (D)]
 *   2-layer LSTM(E + D -> D) one step (gate order i, f, g, o; biases nullable)  ->  q = h1n
 *   attn = softmax_l(q . enc_l) over ALL L rows, mix = sum_l attn_l enc_l          (t2o_attn_fwd)
 *   ctx = tanh(linear_out([mix | q]));  logp = log_softmax(out_linear(ctx))
 * as 6 launches.  Everything a backward needs is left in caller storage (`saved`): the activated gates, both new
 * states, copies hp0 / hp1 of the previous hidden states (nullable), mix, ctx, logp.
 * Backward (9 launches): gradients of logp / ctx / the new states (each nullable; at least one of g_ctx, g_logp) ->
 * d_feat, d_h0, d_c0, d_h1, d_c1, d_enc.  Only DATA gradients: the pre-activation gradients d_logits (B, V; written
 * only when g_logp is given), d_lin (B, D), d_gates1, d_gates0 (B, 4D), d_step_in (B, E + D), d_vis (B, D) stay in
 * caller storage and the caller forms each weight gradient as ONE product over all the steps of a train step
 * (out_linear: d_logits^T ctx; linear_out: d_lin^T [mix | h1n]; LSTM layer 1: d_gates1^T h0n, d_gates1^T hp1; layer 0:
 * d_gates0^T step_in, d_gates0^T hp0; vis_linear: d_vis^T feat_copy; embedding: rows prev_op += d_step_in[:, :E]).
 * D % 64 == 0, D <= 1024, E % 4 == 0, V <= 16, L <= 64; every buffer 16-byte aligned, rows dense. */
typedef struct t2o_decoder_step {
  /* parameters */
  const float *emb;                            /* (V, E) */
  const float *vis_w, *vis_b;                  /* (D, D), (D) nullable */
  const float *w_ih0, *w_hh0, *b_ih0, *b_hh0;  /* (4D, E + D), (4D, D), (4D), (4D) */
  const float *w_ih1, *w_hh1, *b_ih1, *b_hh1;  /* (4D, D), (4D, D), (4D), (4D) */
  const float *lo_w, *lo_b;                    /* attention.linear_out (D, 2D), (D) nullable */
  const float *out_w, *out_b;                  /* out_linear (V, D), (V) nullable */
  /* forward inputs */
  const long long* prev_op;                    /* (B) token of the previous operator */
  const float *feat, *h0, *c0, *h1, *c1;       /* (B, D) each */
  const float* enc;                            /* (B, L, D) request encoding */
  /* forward outputs and saved values */
  float *step_in;                              /* (B, E + D) */
  float *feat_copy, *hp0, *hp1;                /* (B, D) each, nullable: copies of feat / h0 / h1 (the X of their products) */
  long long* prev_op_copy;                     /* (B) nullable */
  float *gates0, *gates1;                      /* (B, 4D) activated i, f, g, o */
  float *h0n, *c0n, *h1n, *c1n;                /* (B, D) new states */
  float *attn, *mix, *ctx, *logp;              /* (B, L), (B, D), (B, D), (B, V) */
  /* backward inputs (nullable) */
  const float *g_logp, *g_ctx, *g_h0n, *g_c0n, *g_h1n, *g_c1n;
  /* backward: kept for the weight gradients */
  float *d_logits, *d_lin, *d_gates1, *d_gates0, *d_step_in, *d_vis;
  /* backward scratch */
  float *d_ctx, *d_mix, *d_qa, *d_q, *d_x1;    /* (B, D) each */
  /* backward outputs */
  float *d_feat, *d_h0, *d_c0, *d_h1, *d_c1;   /* (B, D) each */
  float* d_enc;                                /* (B, L, D) */
  int B, L, D, E, V;
} t2o_decoder_step_t;
int t2o_decoder_step_fwd(const t2o_decoder_step_t* args, void* stream);
int t2o_decoder_step_bwd(const t2o_decoder_step_t* args, void* stream);

/* ---- the two batch norms of a shortcut block in one pass each way: models/actor_resnet.py:33-36, 42-44
 *   out = relu(bn2(x) + bn_s(xs))        x = conv2's output, xs = the 1x1 stride-2 shortcut convolution's output, both (M, C)
 * Forward (3 launches instead of 5: the normalised shortcut is never stored): `partial` = the main branch's statistics rows
 * left by its producing convolution (t2o_conv3x3_fwd_stats_nhwc / t2o_wino_output_transform; NULL: a statistics pass is
 * made here), the shortcut branch's statistics are always made here.  Both batch norms get their batch statistics
 * (save_*), running statistics and — backward, 3 launches instead of 6: the gated gradient shared by both branches is
 * never stored — their input gradients dx / dxs and parameter gradients (accumulate != 0: added).  Same arithmetic in the
 * same order as t2o_bn_relu_nhwc_fwd(relu = 0) followed by t2o_bn_relu_nhwc_fwd_partials(res): bit-identical results. */
size_t t2o_bn_dual_nhwc_workspace_bytes(int M, int C);
int t2o_bn_dual_relu_nhwc_fwd(const float* x, const float* partial, int partial_rows, const float* xs,
                              const float* weight, const float* bias, float* running_mean, float* running_var, float* save_mean,
                              float* save_invstd, const float* weight_s, const float* bias_s, float* running_mean_s,
                              float* running_var_s, float* save_mean_s, float* save_invstd_s, float* out, float momentum, float eps,
                              float momentum_s, float eps_s, void* workspace, size_t workspace_bytes, int M, int C, void* stream);
int t2o_bn_dual_relu_nhwc_bwd_acc(const float* x, const float* xs, const float* y, const float* dy, const float* weight,
                                  const float* bias, const float* save_mean, const float* save_invstd, const float* weight_s,
                                  const float* bias_s, const float* save_mean_s, const float* save_invstd_s, float* dx, float* dxs,
                                  float* dweight, float* dbias, float* dweight_s, float* dbias_s, int accumulate, void* workspace,
                                  size_t workspace_bytes, int M, int C, void* stream);

/* Rewrites a captured, not yet instantiated hipGraph (hipGraph_t) in place: every memset node becomes a kernel node
 * doing the same fill, with the same dependencies and dependents; *replaced = how many.  Memset nodes were seen to
 * run out of order with neighbouring kernel nodes on replay (ROCm 7.2 / gfx950): t2onet_amd/graphs.py calls this on
 * the encoder's graphs before instantiating them (library calls inside them may enqueue hipMemsetAsync). */
int t2o_graph_memsets_to_kernels(void* graph, int* replaced);

/* ---- Adam over one flat fp32 buffer: experiments/t2onet/train_seq2seqL1.py:169 (torch.optim.Adam, default betas and
 * eps, no weight decay) -- param, grad, exp_avg, exp_avg_sq: n floats each, 16-byte aligned; `step` = 1 for the first
 * update (bias corrections are computed on the host in double).  In place; one streaming pass. */
int t2o_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                  float beta2, float eps, int step, void* stream);

/* ---- WEIGHT GRADIENT of the same layers in the Winograd domain with both transforms on chip (t2o_wino_wgrad.hip;
 * models/actor_resnet.py:24-44 under autograd in the reference): dw (Co,3,3,Ci) (+)= d loss / d w of y = conv2d(x, w, None, 1, 1)
 * for x (n_img,H,W,Ci), dy (n_img,H,W,Co) NHWC, H and W multiples of 16, Ci and Co multiples of 64 (<= 512), fewer than 2^31
 * pixels.  n_img may span several encoder passes laid side by side (encoder.WgradArena).  16 of the direct kernel's 36
 * multiplies; V = B^T d B and A dY A^T live in LDS only.  Deterministic: per-workgroup partial sums in the workspace
 * (t2o_wino_fused_wgrad_workspace_bytes), added in a fixed order, then G^T dU G (t2o_wino_dw_transform).  zeros: >= 17 * Ci * 4 +
 * 256 bytes of zeros, 16-byte aligned (t2o_conv_set_zero_region's block serves). */
int t2o_wino_fused_wgrad_supported(int n_img, int H, int W, int Ci, int Co);
size_t t2o_wino_fused_wgrad_workspace_bytes(int n_img, int H, int W, int Ci, int Co);
int t2o_wino_fused_wgrad_nhwc(const float* x, const float* dy, float* dw, const float* zeros, void* workspace, size_t workspace_bytes,
                              int n_img, int H, int W, int Ci, int Co, int accumulate, void* stream);

/* ---- the train step's one collective (the reference runs one process: train_seq2seqL1.py:74-88 has no
 * counterpart).  t2o_allreduce: in-place SUM all-reduce of n fp32 values over the caller's communicator (an ncclComm_t, passed
 * as void*), stream-ordered on `stream`, no host synchronisation; t2o_allreduce_mean: the same followed by x 1/nranks (the
 * data-parallel gradient average; flat 16-byte aligned).  RCCL is resolved at first use (dlopen: the copy the process already
 * holds, else librccl.so) -- not a link-time dependency; without it every entry point here returns T2O_EUNSUPPORTED and
 * t2o_comm_available() is 0.  For a host that has no communicator of its own: rank 0 calls t2o_comm_unique_id (128 bytes),
 * hands them to every rank by any means, all ranks call t2o_comm_init_rank (collective; the calling thread's current HIP
 * device is the rank's GPU) and, at the end, t2o_comm_destroy. */
int t2o_comm_available(void);
int t2o_comm_unique_id(void* id128);
int t2o_comm_init_rank(void** comm, int nranks, const void* id128, int rank);
int t2o_comm_destroy(void* comm);
int t2o_allreduce(float* flat, size_t n, void* comm, void* stream);
int t2o_allreduce_mean(float* flat, size_t n, void* comm, void* stream);

/* ---- the general fp32 matrix-core GEMM (t2o_gemm.hip) behind the dense products no specialised kernel takes: the request
 * encoder's input projection over all time steps and its weight / input gradients (models/lang_encoder.py:91-102, nn.LSTM's
 * x W_ih^T and the gradients of W_ih, W_hh), the decoder tape's weight gradients over all decoder steps of a train step
 * (models/action_decoder.py:52-63: vis_linear, both LSTM cells, attention.linear_out, out_linear) and fc (models/
 * actor_resnet.py:107).   C (M,N) = [C +] op(A) op(B), row-major, leading dimensions in floats:
 *   a_kmajor = 1: A is stored (K, M) (a "dy^T x" product sums over the rows of both operands), 0: (M, K);
 *   b_kmajor = 1: B is stored (K, N), 0: (N, K) (nn.Linear's weight).
 * Any M, N, K >= 1; operands / C may be column slices of larger matrices.  One workgroup per 64 x 64 tile of C; its 1, 2 or 4
 * contraction groups (chosen by K alone) walk their 32-deep chunks of K front to back and are added in group order: the rounding
 * depends on the shape only (no split-K across workgroups, no atomics) -- bitwise the same on every run and machine.
 * t2o_colsum: out[n] = [out[n] +] sum over the rows of X (R, N) (bias gradients), fixed order. */
int t2o_gemm(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int a_kmajor, int b_kmajor,
             int accumulate, void* stream);
int t2o_colsum(const float* X, float* out, int R, int N, int ldx, int accumulate, void* stream);

/* ---- Winograd F(2x2,3x3) with V and M kept on chip (t2o_wino_fused.hip): conv2d(x, w, None, 1, 1) on NHWC activations for the
 * stride-1 3x3 layers of the 64- / 128-channel stages (models/actor_resnet.py:24-44), H and W multiples of 16, Ci of 8, Co of
 * 64 -- ONE launch per layer where t2o_wino_input_transform + t2o_gemm_nt_batched + t2o_wino_output_transform move 8x the
 * activation through HBM.  uc = t2o_wino_u_chunked(U) with U = t2o_wino_weight_transform(w) (or of the mirrored transpose
 * for the data gradient): (Ci/8, 16, Co, 8).  addend (N,H,W,Co) or NULL is added in the epilogue; stats or NULL receives
 * (t2o_wino_fused_stats_rows, 2, Co) partial sums / sums of squares of y for t2o_bn_relu_nhwc_fwd_partials.  zeros: >= Ci*4 +
 * 32 bytes of zeros, 16-byte aligned (t2o_conv_set_zero_region's block serves); Ci, Co <= 1024 (so 4,128 bytes always suffice). */
int t2o_wino_fused_supported(int N, int H, int W, int Ci, int Co);
int t2o_wino_fused_stats_rows(int N, int H, int W);
int t2o_wino_u_chunked(const float* U, float* Uc, int Cn, int Ck, void* stream);
int t2o_wino_fused_conv_nhwc(const float* x, const float* uc, const float* addend, float* y, float* stats,
                             const float* zeros, int N, int H, int W, int Ci, int Co, void* stream);
/* ... as a data gradient in front of y = relu(bn(bn_x)) (see t2o_conv3x3_dgrad_pre_bnsums_nhwc): rows (t2o_wino_fused_stats_rows,
 * 2, Co) receive that batch norm's backward sums for t2o_bn_relu_nhwc_bwd_partials_acc; bn_x is fetched under the last chunk. */
int t2o_wino_fused_conv_bnsums_nhwc(const float* x, const float* uc, float* y, const float* bn_x, const float* save_mean,
                                    const float* save_invstd, const float* weight, const float* bias, float* rows,
                                    const float* zeros, int N, int H, int W, int Ci, int Co, void* stream);

/* ---- the data step's pixel work (t2o_image_io.hip): utils/visual_utils.py:6-58.
 * t2o_resize_u8_to_f32: what the reference's loaders do after decoding (visual_utils.py:6-47: cv2.resize, the channel
 * transpose, / 255) for a whole batch in ONE launch.  src: DEVICE bytes holding n uint8 (h,w,3) RGB images of differing
 * sizes at arbitrary byte offsets (no alignment needed); descs: DEVICE table of n descriptors, 8-byte aligned; out:
 * (n,3,out_h,out_w) fp32.  out[i] = resize(image i).astype(float32).transpose(2,0,1) / 255 with OpenCV's 8-bit INTER_LINEAR
 * as t2onet_amd/data.py:resize_linear_u8 states it (fp64 half-pixel taps, 11-bit coefficients rounded half to even, int32
 * passes; a source of the output's size is converted as is, an exact 2x shrink is the rounded 2x2 block mean) -- bit for
 * bit.  A descriptor with h = w = 0 stands for an absent image: out[i] = 0 (the unused steps of a planned sequence,
 * datasets/FiveKdataset.py:118-130).  The caller guarantees offset + 3 h w <= the size of src: descriptors live on the
 * device and are not read back.
 * t2o_f32_to_u8_hwc: tensor2img (visual_utils.py:50-58) for a batch: img (n,3,h,w) fp32 in [0,1] -> out (n,h,w,3) uint8 =
 * img * 255 truncated; any h, w and any alignment of out. */
typedef struct {
  long long offset;   /* first byte of the image, counted from src */
  int h, w;           /* rows and columns of the source; 0, 0 = absent */
} t2o_image_desc_t;
int t2o_resize_u8_to_f32(const unsigned char* src, const t2o_image_desc_t* descs, int n, int out_h, int out_w, float* out,
                         void* stream);
int t2o_f32_to_u8_hwc(const float* img, int n, int h, int w, unsigned char* out, void* stream);

/* ---- a training batch out of a device-resident set of 8-bit pictures (t2o_resident.hip).  store: DEVICE bytes, 16-byte
 * aligned, holding the set after its resize: item i of N has up to K <= 8 pictures, picture (i, k) being (h,w,3) uint8
 * RGB in HWC order at store + slot_offsets[i * K + k]; slot_offsets: DEVICE (N, K) int64, every offset a multiple of 16
 * (the kernel reads a slot as aligned dwords), -1 = item i has no picture k.  index: DEVICE (B) int64, the batch's
 * items; it is read ON THE DEVICE, so a captured launch serves another batch once the caller has overwritten it;
 * indices may repeat.  For b < B and i = index[b]: out_x[b] = picture (i, 0) and out_ys[b, k - 1] = picture (i, k),
 * k = 1 .. K - 1, each .astype(float32).transpose(2,0,1) / 255 -- the values the resize entry above writes for a source
 * of the output's size, bit for bit; an absent picture gives zeros (the unused steps of a planned sequence, like the
 * h = w = 0 descriptor).  out_x: (B,3,h,w) fp32; out_ys: (B,K-1,3,h,w) fp32, may be NULL when K = 1; any h, w.
 * One launch; every output element is written exactly once; no atomics, no allocation, no host synchronisation,
 * deterministic, capturable.
 * The caller guarantees 0 <= index[b] < N and that every slot lies inside store: both tables live on the device and are
 * not read back (an index outside [0, N) is treated as an item without pictures: nothing is read through it).
 * T2O_EINVAL, before any launch: null pointers; N, K, B, h or w not positive; K > 8; a store that is not 16-byte, tables
 * that are not 8-byte or outputs that are not 4-byte aligned; more than 2^31 - 1 workgroups (B K ceil(h w / 1024)). */
int t2o_gather_u8_to_f32(const unsigned char* store, const long long* slot_offsets, const long long* index, int N, int K,
                         int B, int h, int w, float* out_x, float* out_ys, void* stream);

/* ---- the same batch for ITEMS of up to 16 pictures that may share slots, with one row of a device table per sample
 * (t2o_resident_items.hip; a GIER item: input, 8 planned steps, target, and the plane numbers of its local-edit masks).
 * Pictures: the contract of t2o_gather_u8_to_f32 with K <= 16 -- the same thread program; for K <= 8 the outputs are
 * bit-identical to that entry's.  A slot may appear in several items and several columns: a shared picture is stored once.
 * rows: DEVICE (N, V) int32; out_rows: (B, V) int32 with out_rows[b][v] = rows[index[b]][v], all -1 for an index outside
 * [0, N).  rows == NULL only together with V == 0 and out_rows == NULL (pictures only).  The rows are written by the SAME
 * launch: ceil(B V / 256) workgroups appended to the flat grid of the pictures' B K ceil(h w / 1024).  Index and both
 * tables are read on the device; every output element is written exactly once; no atomics, no allocation, no host
 * synchronisation, deterministic, capturable.
 * T2O_EINVAL, before any launch: the cases of t2o_gather_u8_to_f32 with K > 16 in place of K > 8; V < 0; rows, out_rows
 * and V that do not agree; rows or out_rows not 4-byte aligned; more than 2^31 - 1 workgroups, the row workgroups included. */
int t2o_gather_items_u8_to_f32(const unsigned char* store, const long long* slot_offsets, const long long* index, int N, int K,
                               int B, int h, int w, float* out_x, float* out_ys, const int* rows, int V, int* out_rows,
                               void* stream);

/* ---- a known operator list replayed on 8-bit pictures at their native size, 8-bit in and 8-bit out (t2o_replay.hip):
 * what an edit's decision, taken on a bounded proxy, costs on the original photo.  Job j reads the (h,w,3) uint8 RGB
 * picture at src + src_offset (any byte alignment; several jobs may name the same source) and writes (h,w,3) uint8 at
 * out + out_offset.  Per pixel x = byte / 255 (the conversion of t2o_resize_u8_to_f32 for a source of the output's size);
 * for k < steps: x = clamp(process(ops[k], x, params[j][k]), 0, 1), Operator.execute with specified_param and no mask
 * (models/operators.py:112-131), ops[k] = -1 being the identity; byte = x * 255 truncated, as t2o_f32_to_u8_hwc.  The
 * bytes are those of that materialised path (resize at the picture's size, t2o_op_fwd per step, f32_to_u8_hwc): the same
 * device functions run, at 6 bytes of global traffic per pixel.  steps = 0 is the two conversions back to back.
 * Operators 0, 1, 2, 3, 5, 6, 7 and -1; the sharpness zero-pads the INTERMEDIATE image at the picture's border.
 * jobs: HOST array of J <= 64 (copied into the kernel arguments); params: DEVICE (J, 8, 24) fp32, may be NULL when no
 * job applies an operator.  One launch for all jobs; no allocation, no host synchronisation, capturable, deterministic.
 * The caller guarantees that the offsets and sizes lie inside src / out.
 * T2O_EUNSUPPORTED: operator 4, or more than one sharpness among a job's steps (the actor's op mask forbids repeats,
 * models/actor.py:235-236; one sharpness keeps the halo at one pixel).  T2O_EINVAL: J outside 1..64, steps outside
 * 0..8, any other operator index, null pointers, non-positive sizes, negative offsets. */
typedef struct {
  long long src_offset, out_offset;   /* first byte of the source / destination picture, counted from src / out */
  int h, w;
  int steps;                          /* operators applied: ops[0 .. steps) */
  int ops[8];
} t2o_replay_job_t;
int t2o_replay_u8(const unsigned char* src, unsigned char* out, const t2o_replay_job_t* jobs, int J, const float* params,
                  void* stream);

/* ---- the same replay with Operator.execute's MASK operand (t2o_replay_mask.hip): a local edit at native size.  Step k
 * of job j may name one of n_masks <= 4 uint8 (h,w) planes of the job's own size, plane i starting at masks +
 * mask_offsets[i] (any byte alignment; the jobs of a call share the planes): mask_of[8 j + k] is its index, or -1.  Per
 * pixel x = byte / 255; for k < steps, with o = process(ops[k], x, params[j][k]):
 *   x = clamp(o * m + x * (1 - m), 0, 1), m = maskbyte / 255      where the step names a mask
 *   x = clamp(o, 0, 1)                                            where it names none
 * (models/operators.py:112-131; 0 leaves the pixel, 255 applies the operator, values between feather the edge); byte =
 * x * 255 truncated.  A masked sharpness blends the stencil's result with the stencil's input at the centre pixel, and a
 * masked step in front of a sharpness is blended on the ring as well; the zero padding of the intermediate image at the
 * picture's border is t2o_replay_u8's.  The bytes are those of the materialised path (resize at the picture's size,
 * t2o_op_fwd per step with the mask as (1,1,h,w) fp32 = byte / 255, f32_to_u8_hwc): the same device functions run, at
 * 6 bytes of global traffic per pixel plus 1 per distinct mask the job's list names.  A workgroup skips a step whose
 * mask is 0 on its whole 32 x 32 window (the bytes are the same: o * 0 + x * 1 = x), so a small region costs little on
 * a large photo.  An index on an identity step (-1) or beyond `steps` is ignored.
 * jobs, mask_of ((J, 8) ints), mask_offsets: HOST arrays, copied into the kernel arguments; params, masks: DEVICE.
 * masks / mask_offsets may be NULL when n_masks = 0.  One launch; no allocation, no host synchronisation, capturable,
 * deterministic.  The caller guarantees that offsets and sizes lie inside src / out / masks.
 * Status codes as t2o_replay_u8 (operator 4 and a second sharpness: T2O_EUNSUPPORTED); T2O_EINVAL also for n_masks
 * outside 0..4, a mask index outside -1..n_masks-1 among a job's steps, a negative mask offset.
 * Measured on one synthetic 4000 x 6000 picture only (profiles/replay_u8_masked.txt); not measured: real photos through
 * the decoder, masks larger than the L2 working set as a case of their own, the kernel's share of peak. */
int t2o_replay_u8_masked(const unsigned char* src, unsigned char* out, const t2o_replay_job_t* jobs, const int* mask_of, int J,
                         const float* params, const unsigned char* masks, const long long* mask_offsets, int n_masks,
                         void* stream);

/* ---- the same replay for lists with ANY number of sharpness steps (t2o_replay_stencils.hip), masks optional: the
 * arguments, limits (J <= 64 jobs, n_masks <= 4, steps <= 8) and per-step semantics of t2o_replay_u8_masked, and no limit
 * on the sharpness steps among a list's 8.  Per job, with x = byte / 255, for k < steps:
 *   x = clamp01(blend(process(ops[k], x, params[j][k]), x, m_k / 255))   where step k names a mask,
 *   x = clamp01(process(ops[k], x, params[j][k]))                        where it names none;
 * EVERY sharpness reads the four neighbours of the image in front of it, and that intermediate image counts as ZERO
 * outside the picture (the intermediate image is padded, not the source; the zeros are not process(0)).  A masked
 * sharpness blends with the stencil's input at the centre pixel.  byte = x * 255 truncated.  The bytes are those of the
 * materialised path (resize at the picture's size, t2o_op_fwd per step, f32_to_u8_hwc): the same device functions in the
 * same order.  A workgroup stages its 32 x 32 tile plus a ring of R pixels (R = the job's number of sharpness steps) and
 * recomputes the per-pixel steps on the ring, up to (32 + 2R)^2 / 32^2 of the work; global traffic stays 6 bytes per
 * pixel plus 1 per distinct mask named, plus the ring.  Lists with no or one sharpness are served too (same bytes as
 * t2o_replay_u8 / t2o_replay_u8_masked, which are the cheaper kernels for them).  A step whose mask is 0 on a
 * workgroup's whole window is skipped (same bytes).
 * mask_of, masks and mask_offsets may be NULL when n_masks = 0.  jobs, mask_of, mask_offsets: HOST; params, masks:
 * DEVICE.  One launch; no allocation, no host synchronisation, capturable, deterministic.  The caller guarantees that
 * offsets and sizes lie inside src / out / masks.
 * Status codes: operator 4 (inpaint) T2O_EUNSUPPORTED; everything else as t2o_replay_u8_masked; there is no status for
 * "too many sharpness steps".  Adding this entry point does not change t2o_abi_version() (4): no existing form changed.
 * Measured on one synthetic 4000 x 6000 picture only (profiles/replay_u8_stencils.txt); not measured: real photos
 * through the decoder, more than two sharpness steps, the kernel's share of peak. */
int t2o_replay_u8_stencils(const unsigned char* src, unsigned char* out, const t2o_replay_job_t* jobs, const int* mask_of, int J,
                           const float* params, const unsigned char* masks, const long long* mask_offsets, int n_masks,
                           void* stream);

/* ---- feathering the mask planes of a local edit on the device (t2o_feather.hip): a hard 0/255 selection gets the soft
 * edge a photo wants.  Job j blurs the (h,w) uint8 plane at src + src_offset (any byte alignment) with a separable
 * Gaussian of standard deviation sigma (pixels of the plane, 0 <= sigma <= 64) in INTEGER arithmetic with replicated
 * borders and writes (h,w) uint8 at out + out_offset (any byte alignment; no byte outside the plane is written).
 * Weights (t2o_feather_weights, host only, fp64): R0 = min(ceil(3 sigma), 192); g_i = exp(-i^2 / (2 sigma^2)) for
 * i = 0..R0; G = g_0 + 2 sum_{i>=1} g_i; e_i = 65536 g_i / G; tail sums T_i = sum_{k=i..R0} e_k, T_{R0+1} = 0;
 *   w_i = rint(T_i) - rint(T_{i+1}) for i >= 1,   w_0 = 65536 - 2 rint(T_1);
 * trailing zero weights are trimmed, which gives the radius R.  So w_0 + 2 sum_{i>=1} w_i = 65536 exactly, every
 * w_i >= 0 and |w_i - e_i| <= 1.  R = 0 (sigma = 0, or at or below about 0.2) is w_0 = 65536, a plain copy; otherwise
 * w_0 <= 65534 and the weights are uint16 (w[0] holds 0, 65536 modulo 2^16, when R = 0).
 *   row pass     a = sum_{i=-R..R} w_|i| m[y, clamp(x+i, 0, w-1)] <= 255 * 65536;     t = (a + 128) >> 8 <= 65280, uint16
 *   column pass  b = sum_{i=-R..R} w_|i| t[clamp(y+i, 0, h-1), x] <= 65280 * 65536;   out = (b + 2^23) >> 24
 * in unsigned 32-bit arithmetic, exact.  A constant plane comes out unchanged, the output lies within [min m, max m],
 * and flipping the input in both axes flips the output; the intermediate is rounded after the row pass, so the
 * transposed input does not give the transposed output in general.
 * Two launches cover all jobs; every source byte is read by the first before the second writes any destination byte, so
 * a job may run in place (out + out_offset == src + src_offset) and a source may overlap any destination; the
 * destinations of different jobs may not overlap each other.  jobs: HOST array of 1 <= J <= 4, copied with the weights
 * into the kernel arguments.  workspace: DEVICE, 8-byte aligned, t2o_feather_workspace_bytes (2 bytes per pixel, rows
 * padded to 4 pixels; 0 for a job table that t2o_feather_u8 would refuse).  No allocation, no host synchronisation, no
 * float, no atomics; deterministic, capturable.  The caller guarantees that offsets and sizes lie inside src / out.
 * T2O_EINVAL, before any launch: null pointers, J outside 1..4, sigma negative, NaN or above 64, non-positive sizes,
 * h * w >= 2^31, negative offsets, overlapping destinations.  T2O_EWORKSPACE: workspace null or too small. */
#define T2O_FEATHER_MAX_SIGMA 64.0
#define T2O_FEATHER_MAX_RADIUS 192
#define T2O_FEATHER_MAX_JOBS 4
typedef struct {
  long long src_offset, out_offset;   /* first byte of the source / destination plane, counted from src / out */
  int h, w;
  double sigma;
} t2o_feather_job_t;
int t2o_feather_weights(double sigma, unsigned short* w /* 193 */, int* radius);
size_t t2o_feather_workspace_bytes(const t2o_feather_job_t* jobs, int J);
int t2o_feather_u8(const unsigned char* src, unsigned char* out, const t2o_feather_job_t* jobs, int J, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- growing, shrinking and bordering the mask planes of a local edit on the device (t2o_morph.hip): the plane's boundary
 * moved by R pixels of EXACT Euclidean distance -- "expand the selection by 4 px, then remove".  Job j reads the (h,w)
 * uint8 plane P at src + src_offset (any byte alignment) and writes a hard 0 / 255 (h,w) plane at out + out_offset (any byte
 * alignment; no byte outside the plane is written).  S = {p : P[p] >= 128}; over pixels INSIDE THE FRAME ONLY
 *   Dout(p) = min over q in S of |p - q|^2,   Din(p) = min over q not in S of |p - q|^2,   +infinity where there is no such q;
 * the frame edge is not an edge of the selection: a sky that touches the top of the photo still touches it after a shrink.
 * For the integer radius 0 <= R <= 64:
 *   T2O_MORPH_GROW    255 where Dout(p) <= R^2, else 0
 *   T2O_MORPH_SHRINK  255 where p is in S and Din(p) > R^2, else 0
 *   T2O_MORPH_BORDER  255 where GROW is 255 and SHRINK is 0, else 0
 * So SHRINK(P) = 255 - GROW(255 - P); GROW at R = 0 is the binarised plane and BORDER at R = 0 is all 0; an empty S gives
 * all 0 in every mode, a full S all 255 for GROW and SHRINK and all 0 for BORDER; one set pixel grown by R = 25 is the 1961
 * lattice points of the disc.  No approximation (no chamfer, no iterated 3 x 3 steps): integers, two passes.  The column
 * pass writes g(y,x) = min(|dy| : |dy| <= R, (y+dy,x) in the set), or R + 1, as bytes to the workspace (the set is S for
 * GROW, the frame outside S for SHRINK, one field of each for BORDER); the row pass uses Dout(y,x) <= R^2 <=> some |dx| <= R
 * with x + dx in the frame has g(y,x+dx) <= c[|dx|], c[k] = floor(sqrt(R^2 - k^2)) built on the host in integer arithmetic
 * (c^2 + k^2 <= R^2 < (c+1)^2 + k^2 is checked for each entry).
 * Two launches cover all jobs; every source byte is read by the first before the second writes any destination byte, so
 * a job may run in place (out + out_offset == src + src_offset) and a source may overlap any destination; the
 * destinations of different jobs may not overlap each other.  jobs: HOST array of 1 <= J <= 4, copied with the threshold
 * tables into the kernel arguments.  workspace: DEVICE, 8-byte aligned, t2o_morph_workspace_bytes (1 byte per pixel, 2 for
 * BORDER, rows padded to 4 pixels; 0 for a job table that t2o_morph_u8 would refuse).  No allocation, no host
 * synchronisation, no float, no atomics; deterministic, capturable.  The caller guarantees that offsets and sizes lie
 * inside src / out.
 * T2O_EINVAL, before any launch: null pointers, J outside 1..4, non-positive sizes, h * w >= 2^31, negative offsets, a radius
 * outside 0..64, an unknown mode, overlapping destinations, a misaligned workspace.  T2O_EWORKSPACE: workspace null or too
 * small. */
#define T2O_MORPH_MAX_JOBS 4
#define T2O_MORPH_MAX_RADIUS 64
enum { T2O_MORPH_GROW = 0, T2O_MORPH_SHRINK = 1, T2O_MORPH_BORDER = 2 };
typedef struct {
  long long src_offset, out_offset;   /* first byte of the source / destination plane, counted from src / out */
  int h, w;
  int radius, mode;
} t2o_morph_job_t;
size_t t2o_morph_workspace_bytes(const t2o_morph_job_t* jobs, int J);
int t2o_morph_u8(const unsigned char* src, unsigned char* out, const t2o_morph_job_t* jobs, int J, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- the mask planes of a local edit made from a RULE on the device (t2o_select.hip): no painted file, no host-built
 * plane, no upload of h * w bytes per plane.  Job j writes the (h,w) uint8 plane at out + out_offset (any byte
 * alignment; no byte outside the plane is written) from the uint8 HWC RGB photo of the same size at src + src_offset
 * (any byte alignment).  A SELECTION is n_terms = 1..4 terms; term k gives a weight t_k in 0..255 per pixel,
 * t_k := 255 - t_k when `invert` is 1; m = t_1, then m = (m * t_k + 127) / 255 left to right.  INTEGER arithmetic, every
 * division a floor division of non-negative integers.  With R, G, B the pixel's bytes, mx / mn their max / min:
 *   L = (69 R + 172 G + 15 B + 128) >> 8                       luminance 0.27 / 0.67 / 0.06 in 8 fractional bits, 0..255
 *   S = 0 if mx = 0, else (255 (mx - mn) + mx / 2) / mx        saturation, 0..255
 *   H: d = mx - mn; undefined for d = 0; if mx = R: n = G - B, base 0; else if mx = G: n = B - R, base 512; else
 *      n = R - G, base 1024;  q = (512 (n + d) + d) / (2 d) - 256;  H = (base + q) mod 1536        six sectors of 256:
 *      red 0, yellow 256, green 512, cyan 768, blue 1024, magenta 1280
 *   ramp(dist, soft) = 255 at dist = 0, 0 at dist >= soft, else (255 (soft - dist) + soft / 2) / soft  (soft = 0: a step)
 * Kinds and their parameters p[0..3]:
 *   T2O_SELECT_LUM, T2O_SELECT_SAT  lo, hi, soft: ramp(how far L / S lies outside [lo, hi], soft); 0 <= lo <= hi <= 255,
 *                      0 <= soft <= 255
 *   T2O_SELECT_HUE     lo, hi, soft: the arc runs upward from lo to hi modulo 1536 (wrapping when hi < lo); ramp(circular
 *                      distance of H to the arc, soft); an undefined hue weighs 0 (before inversion); lo, hi in 0..1535,
 *                      0 <= soft <= 768
 *   T2O_SELECT_LINEAR  X0, Y0, X1, Y1 (pixels, not equal): num = (x - X0) DX + (y - Y0) DY, den = DX^2 + DY^2; 255 for
 *                      num <= 0, 0 for num >= den, else (255 (den - num) + den / 2) / den
 *   T2O_SELECT_RADIAL  CX, CY, RI, RO (0 <= RI < RO): d2 = (x - CX)^2 + (y - CY)^2, den = RO^2 - RI^2; 255 for d2 <= RI^2,
 *                      0 for d2 >= RO^2, else (255 (RO^2 - d2) + den / 2) / den -- linear in the squared distance
 *   T2O_SELECT_PLANE   the byte of the (h,w) uint8 plane at src + plane_offset (any byte alignment) is the weight: a
 *                      painted mask intersected with a rule
 * Position terms compute in 64 bits; they need h, w <= 65535 and parameters within +-131070.
 * jobs: HOST array of 1 <= J <= 4, copied into the kernel arguments; jobs may differ in size and may share a photo.  ONE
 * launch: a lane owns four neighbouring pixels of a plane taken as a stream of h * w pixels, 12 source bytes in, one
 * aligned plane dword out, single bytes at the two ends of a misaligned plane; 3 + 1 bytes of traffic per pixel plus 1
 * per plane term, the 3 only for a job with a lum, sat or hue term (the photo is not read otherwise).  No workspace, no allocation, no host synchronisation, no float, no atomics; deterministic, capturable.
 * The caller guarantees that offsets and sizes lie inside src / out.
 * T2O_EINVAL, before any launch: null pointers, J or n_terms outside 1..4, non-positive sizes, h * w >= 2^31, a position
 * term with h or w above 65535, negative offsets, an unknown kind, invert other than 0 / 1, parameters outside the
 * ranges above, a destination that overlaps another destination or (by address: src and out may be one buffer) any
 * photo or plane term of the call. */
#define T2O_SELECT_MAX_JOBS 4
#define T2O_SELECT_MAX_TERMS 4
enum { T2O_SELECT_LUM = 0, T2O_SELECT_SAT = 1, T2O_SELECT_HUE = 2, T2O_SELECT_LINEAR = 3, T2O_SELECT_RADIAL = 4, T2O_SELECT_PLANE = 5 };
typedef struct {
  int kind, invert;
  int p[4];                           /* see the kinds above; unused entries are ignored */
  long long plane_offset;             /* T2O_SELECT_PLANE: first byte of the plane, counted from src */
} t2o_select_term_t;
typedef struct {
  long long src_offset, out_offset;   /* first byte of the photo / the destination plane, counted from src / out */
  int h, w;
  int n_terms, reserved;
  t2o_select_term_t terms[T2O_SELECT_MAX_TERMS];
} t2o_select_job_t;
int t2o_select_u8(const unsigned char* src, unsigned char* out, const t2o_select_job_t* jobs, int J, void* stream);

/* ---- snapping the mask planes of a local edit to the photo's own edges on the device (t2o_refine.hip): the guided filter
 * of He et al. with the photo's luminance as the guide, in INTEGER arithmetic.  Job j reads the (h,w,3) uint8 RGB photo
 * at photo + photo_offset and the (h,w) uint8 plane at src + src_offset and writes (h,w) uint8 at out + out_offset (all
 * three at any byte alignment; no byte outside the plane is written).  radius r in 0..64, eps2 = E in 1..65025 (the
 * regulariser in byte^2 units).  All numbers are integers; // is FLOOR division (numerators can be negative):
 *   I = (69 R + 172 G + 15 B + 128) >> 8                   the guide: t2o_select_u8's luminance L, 0..255
 *   p = the plane's byte
 *   box(v)(y, x) = sum of v[clamp(y+dy, 0, h-1), clamp(x+dx, 0, w-1)] over |dy|, |dx| <= r      replicated borders;
 *                  n = (2r+1)^2 terms everywhere
 *   S_I, S_p, S_II, S_Ip = box(I), box(p), box(I I), box(I p)          each <= 16641 * 65025 < 1.09e9: uint32
 *   cov = n S_Ip - S_I S_p                                             signed 64-bit
 *   var = n S_II - S_I^2 >= 0;  den = var + E n^2 > 0                  64-bit, den < 3.7e13
 *   A = (2 * 1024 * cov + den) // (2 den)                              a in Q10, rounded half up; |A| <= 65281 as
 *                                                                      |a| <= 63.75 / sqrt(E); |numerator| < 9.3e15
 *   B = (2 (1024 S_p - A S_I) + n) // (2 n)                            |B| < 1.7e7: int32
 *   T_A = box(A)   |T_A| <= 1.09e9: int32;     T_B = box(B)   64-bit (a row of 129 B's already passes 2^31)
 *   out = clamp((2 (T_A I + T_B) + 1024 n) // (2 * 1024 * n), 0, 255)
 * Exact consequences: a constant plane c comes out as c for any photo, r and E (cov = 0, A = 0, B = 1024 c); r = 0 is a
 * copy; a constant photo gives A = 0 and a result that depends on the plane alone; flipping photo and plane in both axes
 * flips the output.
 * Four launches cover all jobs (row sums, column sums giving A and B, row sums, column sums giving the byte); every
 * plane byte is read by the first and every destination byte written by the last, so a job may run in place
 * (out + out_offset == src + src_offset) and a source may overlap any destination; photo may be the same buffer as src
 * and out.  jobs: HOST array of 1 <= J <= 4, copied into the kernel arguments.  workspace: DEVICE, 16-byte aligned,
 * t2o_refine_workspace_bytes (20 bytes per pixel with rows padded to 4 pixels; 0 for a job table that t2o_refine_u8
 * would refuse).  No allocation, no host synchronisation, no float, no atomics; deterministic, capturable.  The caller
 * guarantees that offsets and sizes lie inside photo / src / out.
 * T2O_EINVAL, before any launch: null pointers, J outside 1..4, radius outside 0..64, eps2 outside 1..65025,
 * non-positive sizes, h * w >= 2^31, negative offsets, a destination that overlaps (by address) another destination or
 * a photo of the call.  T2O_EWORKSPACE: workspace null, too small or not 16-byte aligned. */
#define T2O_REFINE_MAX_JOBS 4
#define T2O_REFINE_MAX_RADIUS 64
#define T2O_REFINE_MAX_EPS2 65025
typedef struct {
  long long photo_offset, src_offset, out_offset;   /* first byte of the photo / the plane / the destination, counted from photo / src / out */
  int h, w;
  int radius, eps2;
} t2o_refine_job_t;
size_t t2o_refine_workspace_bytes(const t2o_refine_job_t* jobs, int J);
int t2o_refine_u8(const unsigned char* photo, const unsigned char* src, unsigned char* out, const t2o_refine_job_t* jobs, int J,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- the magic wand of a local edit on the device (t2o_region.hip): the CONNECTED region around a seed pixel, by
 * union-find labelling.  Job j reads the (h,w,3) uint8 RGB photo at photo + photo_offset and writes the (h,w) uint8 plane
 * at out + out_offset (both at any byte alignment; no byte outside the plane is written).  Integers only:
 *   (Rs, Gs, Bs) = the photo's bytes at the seed pixel (seed_x, seed_y), READ ON THE DEVICE (no host read)
 *   pass(y, x) <=> max(|R - Rs|, |G - Gs|, |B - Bs|) <= tol                  tol in 0..255; the seed always passes
 *   out(y, x)  =  255 where (y, x) is joined to the seed by a path of passing pixels, else 0
 *                 conn = 4: steps of the path are horizontal or vertical;  conn = 8: diagonal steps too
 * A hard 0/255 plane; t2o_refine_u8 and t2o_feather_u8 soften it.
 * THREE launches cover all jobs, whatever the pictures hold.  The parent array L (int32 per pixel, index i = y w + x) has
 * L[i] < 0 for a pixel that does not pass, L[i] = i for a root and L[i] <= i always.  (1) a workgroup labels a 64 x 64 tile
 * in LDS (runs along rows, min-index unions with the row above) and writes each pixel's parent as the global index of its
 * tile-local root; (2) the pixels of a tile's top row and left column are joined with their passing neighbours across the
 * tile edge: find both roots, atomicMin the larger root's word to the smaller, continue with the returned value where the
 * word was no root any more; (3) one lane per workgroup finds the seed's root, every lane the roots of four neighbouring
 * pixels, and stores one aligned dword (single bytes at the two ends of a misaligned plane).
 * Visibility: in (2) and (3) every access to L is an agent-scope relaxed atomic (served by L2, never by a CU's L1); (1)
 * uses plain stores, which the kernel boundary publishes.
 * Progress: no workgroup waits for another -- no flag, spin, hand-off or grid barrier.  find follows strictly falling
 * indices (every value word i ever holds is <= i, so a stale value cannot lengthen it); a union retries only with an index
 * strictly below the one it held; path compression lowers a word to an ancestor, by atomicMin only.  So L[i] <= i and
 * "same component" are never broken, and a defect could give wrong bytes but never a hang.
 * A root is the smallest index of its component whatever the order of arrival: the output bytes AND the final roots are
 * deterministic (the other words of L are not).
 * photo and out may be one buffer.  jobs: HOST array of 1 <= J <= 4, copied into the kernel arguments; jobs may share a
 * photo.  workspace: DEVICE, 16-byte aligned, t2o_region_workspace_bytes = the sum over the jobs of 4 h w rounded up to a
 * multiple of 16 (0 for a job table that t2o_region_u8 would refuse).  No allocation, no host synchronisation, no float;
 * capturable.  The caller guarantees that offsets and sizes lie inside photo / out.
 * T2O_EINVAL, before any launch: null pointers, J outside 1..4, non-positive sizes, h * w >= 2^31, negative offsets, a
 * seed outside the frame, tol outside 0..255, conn other than 4 or 8, a destination that overlaps (by address) another
 * destination or a photo of the call.  T2O_EWORKSPACE: workspace null, too small or not 16-byte aligned. */
#define T2O_REGION_MAX_JOBS 4
typedef struct {
  long long photo_offset, out_offset;  /* first byte of the photo / the destination, counted from photo / out */
  int h, w;
  int seed_x, seed_y;
  int tol, conn;                       /* 0..255; 4 or 8 */
} t2o_region_job_t;
size_t t2o_region_workspace_bytes(const t2o_region_job_t* jobs, int J);
int t2o_region_u8(const unsigned char* photo, unsigned char* out, const t2o_region_job_t* jobs, int J,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- removing a region of a photo on the device (t2o_fill.hip): the pixels under a plane replaced by a PUSH-PULL FILL
 * from the pixels around them.  A classical, exact, deterministic smooth fill: it suits sky, walls and blurred
 * backgrounds, synthesises no texture, and is NOT the reference's inpaint_obj operator (a network).  Job j reads the
 * (h,w,3) uint8 RGB photo P at photo + photo_offset and the (h,w) uint8 plane M at plane + plane_offset and writes (h,w,3)
 * uint8 at out + out_offset (all three at any byte alignment; no byte outside the destination is written).  Integers
 * only; // is FLOOR division:
 *   known(y, x) <=> M = 0                                  only fully kept pixels are sources
 *   levels      level 0 is the picture; level k+1 has size (ceil(h_k / 2), ceil(w_k / 2)), down to 1 x 1 = level K;
 *               colours are carried in sixteenths: 0..4080, uint16
 *   pull        C_0 = 16 P where known.  A cell of level k+1 has the children (2y+a, 2x+b), a, b in {0, 1}, that lie inside
 *               level k; n = the number of known ones; the cell is known <=> n > 0;
 *               C_{k+1} = (sum of C_k over the known children + n // 2) // n, per channel
 *   push        F_K = C_K; for k = K-1 .. 0: F_k = C_k where the cell is known, otherwise U_k, the 9/3/3/1 tent over F_{k+1}:
 *               Y = y >> 1, X = x >> 1, Yn = clamp(Y + (y odd ? 1 : -1), 0, h_{k+1} - 1), Xn likewise,
 *               U = (9 F[Y,X] + 3 F[Y,Xn] + 3 F[Yn,X] + F[Yn,Xn] + 8) >> 4
 *   result      fill = (F_0 + 8) >> 4;  out = P where M = 0, otherwise out = (P (255 - M) + fill M + 127) // 255.
 *               If the top cell is unknown (no pixel has M = 0) then out = P everywhere: decided on the device, no host read.
 * Exact consequences: kept pixels come out byte for byte; M == 0 everywhere is a copy; every filled channel lies within
 * [min, max] of that channel over the known pixels (rounding half up cannot leave the range); a surround of one colour
 * fills the hole with exactly that colour, whatever lies under the hole; transposing photo and plane transposes the output;
 * a picture with one known pixel is filled with that pixel's colour.  (Flips are NO symmetry: the pyramid is anchored at the
 * top-left.)  A feathered or refined plane has M > 0 in its soft band, so softening a selection also keeps the object's
 * anti-aliased rim out of the sources.
 * T2O_FILL_LAUNCHES = THREE launches cover all jobs, whatever the pictures hold.  (1) pull: a workgroup per 64 x 64 tile
 * (tiles start at multiples of 64, so child pairs stay inside a tile up to level 6) reads photo and plane once, builds levels
 * 1..6 in LDS and stores them in the workspace, 8 bytes per cell (3 x uint16 + known): about 8/3 bytes per pixel.  (2) top: ONE
 * workgroup per job pulls levels 7..K and pushes K..6 through the workspace, __threadfence() + __syncthreads() between two
 * levels, F in arrays of its own, every array on a 128-byte line of its own; the known field of C_K's cell is the "empty" flag.
 * (3) push + blend: a workgroup per tile; a tile without a byte M > 0, or any tile of an empty job, copies its bytes -- or
 * returns at once when the job is in place; another reads the 3 x 3 neighbourhood of F_6 and a one-cell halo of levels 5..1
 * (enough: a halo cell's tent always leans towards the tile), pushes down in LDS and stores aligned dwords, single bytes at the
 * two ends of a misaligned row range.  Pass (3) reads level-0 bytes of its own tile only, so a job may run IN PLACE:
 * out + out_offset == photo + photo_offset.
 * No workgroup waits for another (no flag, no spin, no grid barrier); every loop bound is fixed by the sizes alone; no
 * atomics, no float, no scratch, no inline assembly; no allocation, no host synchronisation; capturable, deterministic.
 * jobs: HOST array of 1 <= J <= 4, copied into the kernel arguments; jobs may share a photo or a plane.  workspace: DEVICE,
 * 16-byte aligned, t2o_fill_workspace_bytes (the arrays above, each rounded up to 128 bytes, plus 112 to round the base up;
 * 0 for a job table that t2o_fill_u8 would refuse).  The caller guarantees that offsets and sizes lie inside photo / plane / out.
 * T2O_EINVAL, before any launch: null pointers, J outside 1..4, non-positive sizes, 3 h w >= 2^31, a side above 4194240
 * (65535 tiles), negative offsets, a destination that overlaps (by address) another destination, a plane of the call, or a photo of the call -- except the
 * job's OWN photo at exactly its own address, the in-place case (a photo that another job of the call also reads is that
 * job's photo too: it cannot be a destination).  T2O_EWORKSPACE: workspace null, too small or not 16-byte aligned. */
#define T2O_FILL_MAX_JOBS 4
#define T2O_FILL_LAUNCHES 3
typedef struct {
  long long photo_offset, plane_offset, out_offset;   /* first byte of the photo / the plane / the destination, counted from photo / plane / out */
  int h, w;
} t2o_fill_job_t;
size_t t2o_fill_workspace_bytes(const t2o_fill_job_t* jobs, int J);
int t2o_fill_u8(const unsigned char* photo, const unsigned char* plane, unsigned char* out, const t2o_fill_job_t* jobs, int J,
                void* workspace, size_t workspace_bytes, void* stream);

/* ---- the metrics of the test loop in one call: utils/eval.py:50-60 (ImageEvaluator.update: input / output L1 and SSIM),
 * utils/ssim/__init__.py:20-40 (the SSIM itself) and test_seq2seqL1.py:60-74 (the END-image select and the two L1
 * distances the loop averages).  imgs: HOST array of 1 <= T <= 8 device pointers to (B,C,H,W) step images, first: device
 * int64 (B) -- the conventions of t2o_end_select_l1_fwd; the output image of sample b is imgs[first[b]][b], read where it
 * lies (a first[b] outside [0,T) counts as T-1).  out4 (device, usually a row of a caller-owned table):
 *   out4[0] = mean |input - target|     out4[2] = SSIM(input, target)
 *   out4[1] = mean |out - target|       out4[3] = SSIM(out, target)
 * the SSIM values being the reference's size_average=True value (the mean of t2o_ssim_fwd's per-sample means); with
 * with_ssim == 0 slots 2 and 3 are written as 0 and no Gaussian pass runs.  Two launches: one workgroup per 32 x 32 tile
 * of a plane reads the three images once (with halo) and writes four partials; a finalize adds them in a fixed order.
 * Deterministic, no float atomics.  workspace: t2o_eval_metrics_workspace_bytes(B,C,H,W). */
size_t t2o_eval_metrics_workspace_bytes(int B, int C, int H, int W);
int t2o_eval_metrics(const float* input, const float* const* imgs, int T, const long long* first,
                     const float* target, float* out4, int with_ssim,
                     void* workspace, size_t workspace_bytes, int B, int C, int H, int W, void* stream);

/* ---- torch.var(torch.cat(ends), dim=0).mean() of test_variance (test_seq2seqL1.py:130-133) from the step images ----
 * imgs: HOST array of R*T device pointers, request r's step t = imgs[r*T+t], (B,row) floats; first: HOST array of R
 * device pointers to int64 (B).  R <= 16, T <= 8, N = R*B >= 2.  For element p of a row the samples are the N values
 * imgs[r*T+first[r][b]][b*row+p]; their unbiased variance is taken in two passes (mean, then squared deviations over
 * N-1) and out[0] = the mean over the row's elements.  Two launches, deterministic; row is any positive size.
 * workspace: t2o_end_select_var_mean_workspace_bytes(row). */
size_t t2o_end_select_var_mean_workspace_bytes(size_t row);
int t2o_end_select_var_mean(const float* const* imgs, const long long* const* first, int R, int T, int B,
                            size_t row, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- local-edit masks on the device (t2o_mask.hip): GIER's COCO run-length masks, resized and unioned without a
 * native-size plane, and the per-step mask of a masked episode chosen from the operator the decoder has just picked ----
 * t2o_rle_union_u8: resize_and_union_mask of data/GIER/GIER.py:288-307 for n_jobs output planes in ONE launch.  A mask is
 * COCO run lengths (column-major over [h, w], zeros first) given as CUMULATIVE run ends: mask m's are
 * ends[first_end .. first_end + n_runs), the last one h * w.  Job j writes the (out_h, out_w) uint8 plane at byte
 * out_offset of `out` (any alignment; planes may abut; no byte outside a plane is written): pixel (oy, ox) is the SUM, over
 * the masks sel[first_sel .. first_sel + n_sel), of the mask's value at source pixel sy = min(floor(oy * (h / out_h)), h - 1),
 * sx likewise (double; OpenCV's INTER_NEAREST rule) -- a count, as the reference's masks.sum(0): overlapping masks give 2, a
 * repeated index counts twice, an empty selection gives 0; the sum saturates at 255.
 * The four tables lie back to back in one buffer: n_jobs t2o_union_job_t, n_masks t2o_rle_mask_t, n_sel ints, n_ends
 * unsigned ints.  host_tables: the buffer as the HOST holds it (read here, for the checks); dev_tables: the same bytes on the
 * DEVICE (read by the kernel); both 8-byte aligned.  T2O_EINVAL, before any launch: null pointers, n_jobs outside 1..65535,
 * sizes that are not positive, h * w >= 2^31, run ends that decrease or do not end at h * w, runs outside the run array, a
 * selection index outside the mask table, a selection outside the list, a plane outside [0, out_bytes).
 * No allocation, no host synchronisation, capturable, deterministic. */
typedef struct {
  unsigned int first_end;             /* index of the mask's first cumulative run end */
  int n_runs, h, w;
} t2o_rle_mask_t;
typedef struct {
  int first_sel, n_sel;
  int out_h, out_w;
  long long out_offset;
} t2o_union_job_t;
int t2o_rle_union_u8(const void* host_tables, const void* dev_tables, int n_jobs, int n_masks, int n_sel, long long n_ends,
                     unsigned char* out, long long out_bytes, void* stream);

/* get_gt_mask of models/actor.py:78-98 from device values.  planes: (N,H,W) uint8; slot: (B,V) int32, a plane number or -1;
 * pred_op: (B) int64; out: (B,1,H,W) fp32 = float(planes[slot[b][pred_op[b]]]), all ones where the slot is -1 (or not a
 * plane number) or pred_op[b] lies outside [0, V): no entry means a global edit.  One launch, any H, W >= 1, B <= 65535;
 * planes may be NULL when N = 0. */
int t2o_mask_select(const unsigned char* planes, const int* slot, const long long* pred_op, float* out, int N, int B, int V,
                    int H, int W, void* stream);

/* ---- per-sample operators under the uint8 mask planes (t2o_apply_planes.hip): t2o_mask_select + t2o_apply_fwd / _bwd
 * (mask_ch = 1) as ONE call that reads the planes where they lie.  For sample b the mask is m = float(planes[k][y][x]) with
 * k = slot[b * V + pred_op[b]], and m = 1 everywhere when pred_op[b] lies outside [0, V) or k is not a plane number
 * (outside [0, N)): t2o_mask_select's rule.  m is a COUNT (0, 1, 2, ...), not divided by 255.  Then exactly t2o_apply_*:
 * out = clamp(process(x) * m + x * (1 - m), 0, 1), op_id[b] the executor index (-1 = identity, returned as is), sharpness
 * reads unmasked neighbours; param rows of >= 24 floats.  No (B,1,H,W) fp32 mask exists anywhere: the forward moves 25
 * bytes per pixel instead of 33 and the backward keeps nothing but img, param and the ids.
 * planes: (N,H,W) uint8, packed (plane k starts at byte k * H * W: no alignment is assumed), NULL only when N = 0;
 * slot: (B,V) int32; pred_op: (B) int64; any H, W >= 1.  gimg may be NULL; workspace: t2o_workspace_bytes(B, H, W).
 * out, gimg and gparam are BIT-IDENTICAL to t2o_mask_select followed by t2o_apply_fwd / t2o_apply_bwd: the same per-pixel
 * programs with only the mask fetch replaced, the same launch geometry, partial-sum layout and finalisation kernel.
 * T2O_EINVAL: null pointers (planes with N > 0), N < 0, B, V, H or W not positive, H * W >= 2^31, strides below 24;
 * T2O_EWORKSPACE: workspace null or too small.  Enqueue only: no allocation, no synchronisation, capturable, deterministic. */
int t2o_apply_planes_fwd(const int* op_id, const long long* pred_op, const unsigned char* planes, const int* slot, int N, int V,
                         const float* img, const float* param, int param_stride, float* out, int B, int H, int W, void* stream);
int t2o_apply_planes_bwd(const int* op_id, const long long* pred_op, const unsigned char* planes, const int* slot, int N, int V,
                         const float* img, const float* param, int param_stride, const float* gout, float* gimg, float* gparam,
                         int gparam_stride, void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* T2ONET_HIP_H */
