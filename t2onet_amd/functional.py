"""torch.autograd bridges to the HIP library: device pointers + the current HIP stream go
straight to the C ABI; torch only owns the memory and the autograd graph.

Every function requires CUDA(HIP) fp32 tensors and raises otherwise -- there is no CPU path.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

OP_NPARAM = (1, 1, 1, 24, 1, 8, 1, 1)
PARAM_PAD = 24
_workspaces = {}


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream(device=None):
    """The current HIP stream of `device` as a raw handle.  torch.cuda.current_stream() costs ~10 us per
    call (device-index resolution, Stream object); the raw getter the compilers use costs ~0.3 us."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device() if device is None or device.index is None else device.index)
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()      # plain ints: ctypes converts them for c_void_p arguments


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError('t2onet_amd: expected fp32 tensors on the GPU (got %s on %s); '
                               'there is no CPU implementation' % (t.dtype, t.device))


def _img(t):
    if t.dim() != 4 or t.shape[1] != 3:
        raise ValueError('image must be (B,3,H,W), got %s' % (tuple(t.shape),))
    return t.contiguous()


def _mask(mask, img):
    if mask is None:
        return None, 0
    B, _, H, W = img.shape
    if mask.dim() != 4 or mask.shape[0] != B or mask.shape[1] not in (1, 3) or tuple(mask.shape[2:]) != (H, W):
        mask = mask.expand(B, mask.shape[1] if mask.shape[1] in (1, 3) else 3, H, W)
    return mask.contiguous(), mask.shape[1]


_ws_need = {}


def _scratch(need, device, cache=None, floor=1 << 20):
    """Per-(device, stream) scratch of at least `need` bytes, grown on demand; kernels on one stream run in order, so one
    buffer per stream is enough.  cache / floor: a caller that keeps buffers of its own (_feather_workspace)."""
    if cache is None:
        cache = _workspaces
    if torch.cuda.is_current_stream_capturing():
        # inside a hipGraph capture the buffer's address is baked into the graph: a private allocation from the graph's
        # pool (a cached buffer could be replaced -- freed -- by a later, larger request on the same stream)
        return torch.empty(max(need, floor), dtype=torch.uint8, device=device)
    key = (device.index, _stream(device))
    ws = cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, floor), dtype=torch.uint8, device=device)
        cache[key] = ws
    return ws


def workspace(B, H, W, device):
    """The scratch of the operator / loss kernels for images of this shape (t2o_workspace_bytes)."""
    need = _ws_need.get((B, H, W))
    if need is None:
        need = _ws_need[(B, H, W)] = _lib.load().t2o_workspace_bytes(B, H, W)
    return _scratch(need, device)


class _OperatorFn(torch.autograd.Function):
    """clamp(process(img, param) * mask + img * (1 - mask), 0, 1) for one operator."""

    @staticmethod
    def forward(ctx, img, param, mask, op):
        _need_gpu(img, param, mask)
        img = _img(img)
        param = param.contiguous()
        mask, mask_ch = _mask(mask, img)
        B, _, H, W = img.shape
        out = torch.empty_like(img)
        rc = _lib.load().t2o_op_fwd(op, _ptr(img), _ptr(param), param.shape[1], _ptr(mask), mask_ch, _ptr(out),
                                    B, H, W, _stream(img.device))
        _lib.check(rc, 't2o_op_fwd')
        ctx.save_for_backward(img, param, mask)
        ctx.op, ctx.mask_ch = op, mask_ch
        return out

    @staticmethod
    def backward(ctx, gout):
        img, param, mask = ctx.saved_tensors
        B, _, H, W = img.shape
        gout = gout.contiguous()
        gimg = torch.empty_like(img) if ctx.needs_input_grad[0] else None
        # the finalize kernel writes every column of an operator's own (B, n) rows
        gparam = torch.empty_like(param) if ctx.op in (0, 1, 2, 3, 5, 6) and param.shape[1] == OP_NPARAM[ctx.op] \
            else torch.zeros_like(param)
        ws = workspace(B, H, W, img.device)
        rc = _lib.load().t2o_op_bwd(ctx.op, _ptr(img), _ptr(param), param.shape[1], _ptr(mask), ctx.mask_ch,
                                    _ptr(gout), _ptr(gimg), _ptr(gparam), gparam.shape[1], _ptr(ws), ws.numel(),
                                    B, H, W, _stream(img.device))
        _lib.check(rc, 't2o_op_bwd')
        return gimg, gparam, None, None


def operator_apply(op, img, param, mask=None):
    """One operator over a (sub)batch (models/operators.py:128-130, fused)."""
    return _OperatorFn.apply(img, param, mask, int(op))


class _ApplyFn(torch.autograd.Function):
    """Per-sample operators in one launch (replaces models/actor.py:100-114,:244-259)."""

    @staticmethod
    def forward(ctx, img, param, mask, op_id):
        _need_gpu(img, param, mask)
        if op_id.dtype != torch.int32 or not op_id.is_cuda:
            raise RuntimeError('op_id must be an int32 GPU tensor')
        img = _img(img)
        param = param.contiguous()
        op_id = op_id.contiguous()
        mask, mask_ch = _mask(mask, img)
        B, _, H, W = img.shape
        if param.shape != (B, PARAM_PAD):
            raise ValueError('param must be (B,24)')
        out = torch.empty_like(img)
        rc = _lib.load().t2o_apply_fwd(_ptr(op_id), _ptr(img), _ptr(param), PARAM_PAD, _ptr(mask), mask_ch,
                                       _ptr(out), B, H, W, _stream(img.device))
        _lib.check(rc, 't2o_apply_fwd')
        ctx.save_for_backward(img, param, mask, op_id)
        ctx.mask_ch = mask_ch
        return out

    @staticmethod
    def backward(ctx, gout):
        img, param, mask, op_id = ctx.saved_tensors
        B, _, H, W = img.shape
        gout = gout.contiguous()
        gimg = torch.empty_like(img) if ctx.needs_input_grad[0] else None
        gparam = torch.zeros_like(param)
        ws = workspace(B, H, W, img.device)
        rc = _lib.load().t2o_apply_bwd(_ptr(op_id), _ptr(img), _ptr(param), PARAM_PAD, _ptr(mask), ctx.mask_ch,
                                       _ptr(gout), _ptr(gimg), _ptr(gparam), PARAM_PAD, _ptr(ws), ws.numel(),
                                       B, H, W, _stream(img.device))
        _lib.check(rc, 't2o_apply_bwd')
        return gimg, gparam, None, None


def apply_per_sample(op_id, img, param, mask=None):
    """op_id (B,) int32 on the GPU (executor index, -1 = identity); param (B,24)."""
    return _ApplyFn.apply(img, param, mask, op_id)


class _L1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        _need_gpu(pred, target)
        pred, target = pred.contiguous(), target.contiguous()
        if pred.shape != target.shape:
            raise ValueError('l1_loss: shape mismatch')
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        n = pred.numel()
        ws = workspace(max(1, n // (3 * 64 * 64) + 1), 64, 64, pred.device)
        rc = _lib.load().t2o_l1_fwd(_ptr(pred), _ptr(target), _ptr(loss), n, _ptr(ws), ws.numel(), _stream(pred.device))
        _lib.check(rc, 't2o_l1_fwd')
        ctx.save_for_backward(pred, target)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        pred, target = ctx.saved_tensors
        gloss = gloss.contiguous().to(torch.float32)
        gpred = torch.empty_like(pred)
        rc = _lib.load().t2o_l1_bwd(_ptr(pred), _ptr(target), _ptr(gloss), _ptr(gpred), pred.numel(), _stream(pred.device))
        _lib.check(rc, 't2o_l1_bwd')
        return gpred, None


def l1_loss(pred, target):
    """mean |pred - target| (experiments/t2onet/train_seq2seqL1.py:85)."""
    return _L1Fn.apply(pred, target)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _EndSelectL1Fn(torch.autograd.Function):
    """mean |imgs[first[b]][b] - target[b]| over the list of step images (t2o_end_select_l1_*): no (B,T,3,H,W) stack."""

    @staticmethod
    def forward(ctx, first, target, *imgs):
        _need_gpu(target, *imgs)
        imgs = [t.contiguous() for t in imgs]
        target = target.contiguous()
        if any(t.shape != target.shape for t in imgs):
            raise ValueError('end_select_l1: shape mismatch')
        B = target.shape[0]
        row = target.numel() // B
        first = first.to(torch.int64).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=target.device)
        n = target.numel()
        ws = workspace(max(1, n // (3 * 64 * 64) + 1), 64, 64, target.device)
        rc = _lib.load().t2o_end_select_l1_fwd(_ptr_array(imgs), len(imgs), _ptr(first), _ptr(target), _ptr(loss), B, row, _ptr(ws),
                                               ws.numel(), _stream(target.device))
        _lib.check(rc, 't2o_end_select_l1_fwd')
        ctx.save_for_backward(first, target, *imgs)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        first, target = ctx.saved_tensors[:2]
        imgs = list(ctx.saved_tensors[2:])
        gloss = gloss.contiguous().to(torch.float32)
        grads = [torch.empty_like(t) for t in imgs]
        B = target.shape[0]
        rc = _lib.load().t2o_end_select_l1_bwd(_ptr_array(imgs), _ptr_array(grads), len(imgs), _ptr(first), _ptr(target), _ptr(gloss), B,
                                               target.numel() // B, _stream(target.device))
        _lib.check(rc, 't2o_end_select_l1_bwd')
        return (None, None) + tuple(grads)


def end_select_l1(imgs, first, target):
    """L1 between each sample's image of step first[b] (imgs: list of T (B,3,H,W) step images) and the target."""
    return _EndSelectL1Fn.apply(first, target, *imgs)


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, context):
        _need_gpu(q, context)
        q, context = q.contiguous(), context.contiguous()
        B, L, D = context.shape
        attn = torch.empty(B, L, dtype=torch.float32, device=q.device)
        mix = torch.empty(B, D, dtype=torch.float32, device=q.device)
        rc = _lib.load().t2o_attn_fwd(_ptr(q), _ptr(context), _ptr(attn), _ptr(mix), B, L, D, _stream(q.device))
        _lib.check(rc, 't2o_attn_fwd')
        ctx.save_for_backward(q, context, attn)
        return mix, attn

    @staticmethod
    def backward(ctx, gmix, gattn):
        q, context, attn = ctx.saved_tensors
        B, L, D = context.shape
        gmix = gmix.contiguous()
        gattn = None if gattn is None else gattn.contiguous()
        gq = torch.empty_like(q)
        gctx = torch.empty_like(context)
        rc = _lib.load().t2o_attn_bwd(_ptr(q), _ptr(context), _ptr(attn), _ptr(gmix), _ptr(gattn), _ptr(gq),
                                      _ptr(gctx), B, L, D, _stream(q.device))
        _lib.check(rc, 't2o_attn_bwd')
        return gq, gctx


def attention_core(q, context):
    """q (B,D), context (B,L,D) -> (mix (B,D), attn (B,L)); softmax over all L rows
    (models/attention.py:37-40)."""
    return _AttnFn.apply(q, context)


def choose_op(logp, op_mask, explore_prob, sample=True, u=None):
    """Next operator of the free-running decode (models/actor.py:222-236) in one launch (t2o_choose_op): probabilities
    from logp (B,n) with the exploration floor, masked by op_mask (B,n) and renormalised, one Categorical draw per
    sample (sample=True: uniform numbers from torch's generator) or the arg-max; op_mask's chosen entries are cleared in
    place.  u: this step's (B) uniform numbers when the caller drew all steps' at once (one launch per episode instead
    of one per step).  Returns (pred_op (B,1) int64 operator-vocabulary ids, exec_op (B) int32 executor indices = id - 3)."""
    _need_gpu(logp, op_mask)
    B, n = op_mask.shape
    logp = logp.detach().reshape(B, n).contiguous()
    if not op_mask.is_contiguous():
        raise ValueError('choose_op: op_mask must be contiguous (it is updated in place)')
    if not sample:
        u = None
    elif u is None:
        u = torch.rand(B, device=logp.device, dtype=torch.float32)
    pred = torch.empty(B, 1, dtype=torch.int64, device=logp.device)
    exe = torch.empty(B, dtype=torch.int32, device=logp.device)
    rc = _lib.load().t2o_choose_op(_ptr(logp), _ptr(op_mask), _ptr(u), float(explore_prob), _ptr(pred), _ptr(exe), B, n, _stream(logp.device))
    _lib.check(rc, 't2o_choose_op')
    return pred, exe


def _is_nhwc(x):
    """4-D activations stored channels-last with a channel count the NHWC kernels take (power of two in [4, 1024])."""
    C = x.shape[1]
    return (x.dim() == 4 and C >= 4 and C <= 1024 and (C & (C - 1)) == 0 and x.shape[2] * x.shape[3] > 1
            and x.is_contiguous(memory_format=torch.channels_last))


class _BnReluFn(torch.autograd.Function):
    """relu(batch_norm(x) (+ res)) with batch statistics (training mode), running stats updated in place.
    Channels-last activations stay channels-last (t2o_bn_relu_nhwc_*); anything else runs on NCHW planes."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, running_mean, running_var, momentum, eps, relu=True, partial=None):
        _need_gpu(x, res, weight, bias)
        nhwc = _is_nhwc(x)
        if not relu and not nhwc:
            raise RuntimeError('batch norm without the activation is only built for channels-last activations')
        fmt = torch.channels_last if nhwc else torch.contiguous_format
        x = x.contiguous(memory_format=fmt)
        res = None if res is None else res.contiguous(memory_format=fmt)
        N, C = x.shape[0], x.shape[1]
        HW = x.numel() // (N * C)
        lib = _lib.load()
        out = torch.empty_like(x)                              # preserves the memory format
        save_mean = torch.empty(C, dtype=torch.float32, device=x.device)
        save_invstd = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = _bn_workspace(lib, N, C, x.device, nhwc, HW)
        if nhwc and partial is not None:                       # statistics from the producing convolution's accumulators
            if partial.dim() != 3 or partial.shape[1] != 2 or partial.shape[2] != C or not partial.is_contiguous():
                raise ValueError('batch_norm_relu: partial must be a contiguous (rows, 2, C) tensor')
            rc = lib.t2o_bn_relu_nhwc_fwd_partials(_ptr(x), _ptr(res), _ptr(weight), _ptr(bias), _ptr(running_mean),
                                                   _ptr(running_var), _ptr(save_mean), _ptr(save_invstd), _ptr(out),
                                                   float(momentum), float(eps), 1 if relu else 0, _ptr(partial),
                                                   partial.shape[0], _ptr(ws), ws.numel(), N * HW, C, _stream(x.device))
        elif nhwc:
            rc = lib.t2o_bn_relu_nhwc_fwd(_ptr(x), _ptr(res), _ptr(weight), _ptr(bias), _ptr(running_mean), _ptr(running_var),
                                          _ptr(save_mean), _ptr(save_invstd), _ptr(out), float(momentum), float(eps),
                                          1 if relu else 0, _ptr(ws), ws.numel(), N * HW, C, _stream(x.device))
        else:
            rc = lib.t2o_bn_relu_fwd(_ptr(x), _ptr(res), _ptr(weight), _ptr(bias), _ptr(running_mean), _ptr(running_var),
                                     _ptr(save_mean), _ptr(save_invstd), _ptr(out), float(momentum), float(eps),
                                     _ptr(ws), ws.numel(), N, C, HW, _stream(x.device))
        _lib.check(rc, 't2o_bn_relu_fwd')
        ctx.save_for_backward(x, out if (res is not None and relu) else None, weight, bias, save_mean, save_invstd)
        ctx.has_res = res is not None
        ctx.nhwc = nhwc
        ctx.relu = bool(relu)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, bias, save_mean, save_invstd = ctx.saved_tensors
        N, C = x.shape[0], x.shape[1]
        HW = x.numel() // (N * C)
        lib = _lib.load()
        dy = dy.contiguous(memory_format=torch.channels_last if ctx.nhwc else torch.contiguous_format)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if ctx.has_res and ctx.needs_input_grad[1] else None
        dweight = torch.empty_like(weight)
        dbias = torch.empty_like(bias)
        ws = _bn_workspace(lib, N, C, x.device, ctx.nhwc, HW)
        if ctx.nhwc:
            rc = lib.t2o_bn_relu_nhwc_bwd(_ptr(x), _ptr(y), _ptr(dy), _ptr(weight), _ptr(bias), _ptr(save_mean),
                                          _ptr(save_invstd), _ptr(dx), _ptr(dres), _ptr(dweight), _ptr(dbias),
                                          1 if ctx.has_res else 0, 1 if ctx.relu else 0, _ptr(ws), ws.numel(), N * HW, C,
                                          _stream(x.device))
        else:
            rc = lib.t2o_bn_relu_bwd(_ptr(x), _ptr(y), _ptr(dy), _ptr(weight), _ptr(bias), _ptr(save_mean), _ptr(save_invstd),
                                     _ptr(dx), _ptr(dres), _ptr(dweight), _ptr(dbias), 1 if ctx.has_res else 0,
                                     _ptr(ws), ws.numel(), N, C, HW, _stream(x.device))
        _lib.check(rc, 't2o_bn_relu_bwd')
        return dx, dres, dweight, dbias, None, None, None, None, None, None


_bn_ws = {}


def _bn_workspace(lib, N, C, device, nhwc=False, HW=1):
    key = (device.index, _stream(device), N, C, nhwc)
    ws = _bn_ws.get(key)
    if ws is None:
        nbytes = lib.t2o_bn_nhwc_workspace_bytes(N * HW, C) if nhwc else lib.t2o_bn_workspace_bytes(N, C)
        ws = _bn_ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def batch_norm_relu(x, bn, residual=None, relu=True, count=True, partial=None):
    """relu(bn(x) (+ residual)) for a torch.nn.BatchNorm2d `bn` in TRAINING mode on the GPU: batch
    statistics, running statistics and num_batches_tracked updated as nn.BatchNorm2d does
    (models/actor_resnet.py:38-44, :99-100).  One statistics pass + one fused normalise/add/ReLU pass.
    relu=False: plain bn(x) (channels-last only: the shortcut branch).  count=False: the caller advances
    num_batches_tracked itself (the encoder does it for all its layers with one launch).  partial: (rows, 2, C)
    per-tile sums / sums of squares of x from the convolution that produced it (conv3x3(..., want_stats=True)):
    the statistics pass over x is skipped (channels-last only)."""
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError('batch_norm_relu: affine BatchNorm2d with running statistics and a fixed momentum only')
    if count:
        bn.num_batches_tracked.add_(1)
    return _BnReluFn.apply(x, residual, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, relu, partial)


HEAD_OPS = (0, 1, 2, 3, 5, 6, 7)          # executor indices with a parameter head on this path (4 = inpaint: none)


def _ptr_table(tensors_by_op):
    """8 device pointers indexed by executor index (entry 4 null) as a ctypes array: the C ABI copies them into
    the kernel arguments."""
    arr = (ctypes.c_void_p * 8)()
    for op, t in tensors_by_op.items():
        arr[op] = t.data_ptr()
    return arr


class _ParamHeadsFn(torch.autograd.Function):
    """param (B,24) = regressor_op(fc2_op(lrelu(fc1_op(features)))) with op = op_ids[b]: one launch forward, two
    backward (t2o_param_heads_*), instead of every head on the whole batch + gather."""

    @staticmethod
    def forward(ctx, features, op_ids, consts, into_grad, *flat):
        _need_gpu(features, *flat)
        # into_grad: the backward ADDS the heads' gradients to the parameters' existing .grad tensors inside its
        # kernel and hands autograd no gradient for them (a trainer with persistent, pre-zeroed gradient buffers)
        ctx.grad_targets = None
        if into_grad and all(t.grad is not None and t.grad.is_contiguous() and t.grad.dtype == torch.float32
                             and t.grad.shape == t.shape and t.is_contiguous() for t in flat):
            ctx.grad_targets = [t.grad for t in flat]
        ctx.param_objs = flat
        features = features.contiguous()
        B, D = features.shape
        flat = [t.contiguous() for t in flat]
        tabs = [{op: flat[4 * k + j] for k, op in enumerate(HEAD_OPS)} for j in range(4)]
        hidden = torch.empty(B, D, dtype=torch.float32, device=features.device)
        raw = torch.empty(B, PARAM_PAD, dtype=torch.float32, device=features.device)
        param = torch.empty(B, PARAM_PAD, dtype=torch.float32, device=features.device)
        rc = _lib.load().t2o_param_heads_fwd(_ptr(op_ids), _ptr(features), _ptr_table(tabs[0]), _ptr_table(tabs[1]),
                                             _ptr_table(tabs[2]), _ptr_table(tabs[3]), _ptr(hidden), _ptr(raw), _ptr(param),
                                             consts[0], consts[1], consts[2], consts[3], B, D, _stream(features.device))
        _lib.check(rc, 't2o_param_heads_fwd')
        ctx.save_for_backward(features, op_ids, hidden, raw, *flat)
        ctx.consts = consts
        return param

    @staticmethod
    def backward(ctx, gparam):
        features, op_ids, hidden, raw = ctx.saved_tensors[:4]
        flat = ctx.saved_tensors[4:]
        B, D = features.shape
        tabs = [{op: flat[4 * k + j] for k, op in enumerate(HEAD_OPS)} for j in range(4)]
        # (in place only while every parameter still carries the gradient tensor seen by the forward)
        acc = ctx.grad_targets is not None and all(p.grad is g for p, g in zip(ctx.param_objs, ctx.grad_targets))
        grads = ctx.grad_targets if acc else [torch.empty_like(t) for t in flat]
        gtabs = [{op: grads[4 * k + j] for k, op in enumerate(HEAD_OPS)} for j in range(4)]
        gctx = torch.empty_like(features)
        dpre = torch.empty_like(features)
        c = ctx.consts
        rc = _lib.load().t2o_param_heads_bwd_acc(_ptr(op_ids), _ptr(features), _ptr_table(tabs[0]), _ptr_table(tabs[1]),
                                                 _ptr_table(tabs[2]), _ptr_table(tabs[3]), _ptr(hidden), _ptr(raw),
                                                 _ptr(gparam.contiguous()), _ptr(gctx), _ptr(dpre), _ptr_table(gtabs[0]),
                                                 _ptr_table(gtabs[1]), _ptr_table(gtabs[2]), _ptr_table(gtabs[3]),
                                                 c[0], c[1], c[2], c[3], B, D, 1 if acc else 0, _stream(features.device))
        _lib.check(rc, 't2o_param_heads_bwd_acc')
        return (gctx, None, None, None) + (tuple(None for _ in flat) if acc else tuple(grads))


def param_heads(features, op_ids, heads, consts, into_grad=False):
    """heads: {executor index: (fc1.weight, fc1.bias, fc2.weight, fc2.bias)} for HEAD_OPS; consts =
    (brightness_range, saturation lo, saturation hi, sharpness_range); op_ids (B,) int32 on the GPU.
    into_grad: the backward adds the heads' gradients to the parameters' existing .grad tensors itself (inside its
    kernel) instead of returning them to autograd -- only for a caller that zeroes those .grad tensors before every
    backward and reads them afterwards (t2onet_amd.train.Trainer); torch.autograd.grad then sees no gradient for them."""
    flat = [t for op in HEAD_OPS for t in heads[op]]
    return _ParamHeadsFn.apply(features, op_ids, tuple(float(v) for v in consts), bool(into_grad), *flat)




def conv3x3_wgrad(x, dy):
    """Weight gradient of a 3x3 stride-1 padding-1 convolution on the fp32 matrix cores (t2o_conv3x3_wgrad_nhwc).
    x (N,Ci,H,W), dy (N,Co,H,W), both channels-last; returns dw (Co,Ci,3,3) channels-last."""
    return _conv_wgrad('conv3x3_wgrad', x, dy, 1, 'channels must be multiples of 64, the width a multiple of 4')


_conv_zeros = {}


def _conv_workspace(device, need):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _conv_zeros and not torch.cuda.is_current_stream_capturing():
        # a block of zeros the kernels read their padding from (never written): saves clearing a region per call
        z = _conv_zeros[idx] = torch.zeros(64 << 10, dtype=torch.uint8, device=device)
        torch.cuda.current_stream(device).synchronize()
        _lib.check(_lib.load().t2o_conv_set_zero_region(idx, _ptr(z), z.numel()), 't2o_conv_set_zero_region')
    # a fresh allocation per call (the caching allocator makes it cheap; inside a captured graph it costs nothing at
    # replay).  A workspace cached per stream and grown on demand was baked into captured graphs and then freed by a
    # later, larger request on the same stream handle -- graphs of another trainer kept replaying into freed memory.
    return torch.empty(need, dtype=torch.uint8, device=device)


def _zero_block(device):
    """The persistent 64 KiB block of zeros registered with the library (padding source of the LDS-DMA kernels)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _conv_zeros:
        _conv_workspace(device, 256)
    return _conv_zeros[idx]


def _nhwc_empty(N, C, H, W, device):
    return torch.empty((N, C, H, W), dtype=torch.float32, device=device, memory_format=torch.channels_last)


def _conv_fwd(who, x, weight, stride, want_stats, hint):
    """The body of conv3x3_forward (stride 1) and conv3x3s2_forward (stride 2)."""
    _need_gpu(x, weight)
    N, Ci, Hi, Wi = x.shape
    Co = weight.shape[0]
    if stride == 2 and (Hi % 2 or Wi % 2):
        raise ValueError('%s: the image size must be even' % who)
    Ho, Wo = Hi // stride, Wi // stride
    x = x.contiguous(memory_format=torch.channels_last)
    weight = weight.contiguous(memory_format=torch.channels_last)
    lib = _lib.load()
    need = (lib.t2o_conv3x3_fwd_workspace_bytes if stride == 1 else lib.t2o_conv3x3s2_fwd_workspace_bytes)(N, Ho, Wo, Ci, Co)
    if need == 0:
        raise RuntimeError('%s: unsupported shape (%s)' % (who, hint))
    ws = _conv_workspace(x.device, need)
    y = _nhwc_empty(N, Co, Ho, Wo, x.device)
    if want_stats:
        stats = torch.empty((lib.t2o_conv3x3_fwd_stats_rows(N, Ho, Wo, Co, stride), 2, Co), dtype=torch.float32, device=x.device)
        rc = lib.t2o_conv3x3_fwd_stats_nhwc(_ptr(x), _ptr(weight), _ptr(y), _ptr(stats), _ptr(ws), ws.numel(), N, Ho, Wo, Ci, Co, stride,
                                            _stream(x.device))
        _lib.check(rc, 't2o_conv3x3_fwd_stats_nhwc')
        return y, stats
    name = 't2o_conv3x3_fwd_nhwc' if stride == 1 else 't2o_conv3x3s2_fwd_nhwc'    # (the _stats entry refuses a null `stats`)
    _lib.check(getattr(lib, name)(_ptr(x), _ptr(weight), _ptr(y), _ptr(ws), ws.numel(), N, Ho, Wo, Ci, Co, _stream(x.device)), name)
    return y


def _conv_dgrad(who, dy, weight, stride, hint):
    """The body of conv3x3_dgrad (stride 1) and conv3x3s2_dgrad (stride 2: dy is the strided side)."""
    _need_gpu(dy, weight)
    N, Co, Ho, Wo = dy.shape
    Ci = weight.shape[1]
    dy = dy.contiguous(memory_format=torch.channels_last)
    weight = weight.contiguous(memory_format=torch.channels_last)
    lib = _lib.load()
    need = (lib.t2o_conv3x3_dgrad_workspace_bytes if stride == 1 else lib.t2o_conv3x3s2_dgrad_workspace_bytes)(N, Ho, Wo, Ci, Co)
    if need == 0:
        raise RuntimeError('%s: unsupported shape (%s)' % (who, hint))
    ws = _conv_workspace(dy.device, need)
    dx = _nhwc_empty(N, Ci, stride * Ho, stride * Wo, dy.device)
    name = 't2o_conv3x3_dgrad_nhwc' if stride == 1 else 't2o_conv3x3s2_dgrad_nhwc'
    _lib.check(getattr(lib, name)(_ptr(dy), _ptr(weight), _ptr(dx), _ptr(ws), ws.numel(), N, Ho, Wo, Ci, Co, _stream(dy.device)), name)
    return dx


def _conv_wgrad(who, x, dy, stride, hint):
    """The body of conv3x3_wgrad (stride 1) and conv3x3s2_wgrad (stride 2): t2o_conv3x3_wgrad_acc_nhwc, not accumulating --
    what the two stride-named entry points run."""
    _need_gpu(x, dy)
    N, Co, Ho, Wo = dy.shape
    Ci = x.shape[1]
    if stride == 2 and tuple(x.shape) != (N, Ci, 2 * Ho, 2 * Wo):
        raise ValueError('%s: x must be (N, Ci, 2 Ho, 2 Wo)' % who)
    x = x.contiguous(memory_format=torch.channels_last)
    dy = dy.contiguous(memory_format=torch.channels_last)
    lib = _lib.load()
    need = (lib.t2o_conv3x3_wgrad_workspace_bytes if stride == 1 else lib.t2o_conv3x3s2_wgrad_workspace_bytes)(N, Ho, Wo, Ci, Co)
    if need == 0:
        raise RuntimeError('%s: unsupported shape (%s)' % (who, hint))
    ws = _conv_workspace(x.device, need)
    dw = _nhwc_empty(Co, Ci, 3, 3, x.device)
    rc = lib.t2o_conv3x3_wgrad_acc_nhwc(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), ws.numel(), N, Ho, Wo, Ci, Co, stride, 0, _stream(x.device))
    _lib.check(rc, 't2o_conv3x3_wgrad_acc_nhwc')
    return dw


def conv3x3_forward(x, weight, want_stats=False):
    """conv2d(x, weight, None, 1, 1) on the fp32 matrix cores (t2o_conv3x3_fwd_nhwc).  x (N,Ci,H,W) and weight
    (Co,Ci,3,3) channels-last; returns y (N,Co,H,W) channels-last.  want_stats: returns (y, stats) with stats
    (rows, 2, Co) = per pixel tile the channels' sums and sums of squares of y (t2o_conv3x3_fwd_stats_nhwc), the
    input of batch_norm_relu(..., partial=stats)."""
    return _conv_fwd('conv3x3_forward', x, weight, 1, want_stats, 'Ci % 32, Co % 64, W % 8 must be 0')


def conv3x3_dgrad(dy, weight):
    """Data gradient of conv2d(x, weight, None, 1, 1) (t2o_conv3x3_dgrad_nhwc).  dy (N,Co,H,W) and weight (Co,Ci,3,3)
    channels-last; returns dx (N,Ci,H,W) channels-last."""
    return _conv_dgrad('conv3x3_dgrad', dy, weight, 1, 'Co % 32, Ci % 64, W % 8 must be 0')


def conv3x3s2_dgrad(dy, weight):
    """Data gradient of conv2d(x, weight, None, stride 2, padding 1) for an even-sized x (t2o_conv3x3s2_dgrad_nhwc).
    dy (N,Co,Ho,Wo) and weight (Co,Ci,3,3) channels-last; returns dx (N,Ci,2Ho,2Wo) channels-last."""
    return _conv_dgrad('conv3x3s2_dgrad', dy, weight, 2, 'Co % 32, Ci % 64, Wo % 8 must be 0 -- or Ci = 3, Co = 32 / 64')


def conv3x3s2_forward(x, weight, want_stats=False):
    """conv2d(x, weight, None, stride 2, padding 1) for an even-sized x (t2o_conv3x3s2_fwd_nhwc).  x (N,Ci,2Ho,2Wo)
    and weight (Co,Ci,3,3) channels-last; returns y (N,Co,Ho,Wo) channels-last (want_stats: as conv3x3_forward)."""
    return _conv_fwd('conv3x3s2_forward', x, weight, 2, want_stats, 'Ci % 32, Co % 64, Wo % 8 must be 0')


def stem_forward(x, weight, want_stats=False):
    """conv2d(x, weight, None, stride 2, padding 1) for the encoder's stem: 3 input channels, 32 / 64 output channels
    (t2o_stem_fwd_nhwc).  x (N,3,2Ho,2Wo), weight (Co,3,3,3) channels-last; returns y (N,Co,Ho,Wo) channels-last, with
    want_stats also the (rows, 2, Co) partial sums for batch_norm_relu(..., partial=)."""
    _need_gpu(x, weight)
    N, Ci, Hi, Wi = x.shape
    Co = weight.shape[0]
    if Ci != 3 or Co not in (32, 64):
        raise ValueError('stem_forward: 3 input channels, 32 or 64 output channels')
    Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2                      # (odd sizes: full-resolution inference images)
    x = x.contiguous(memory_format=torch.channels_last)
    weight = weight.contiguous(memory_format=torch.channels_last)
    lib = _lib.load()
    y = torch.empty((N, Co, Ho, Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    stats = torch.empty((lib.t2o_stem_fwd_stats_rows(N, Ho, Wo), 2, Co), dtype=torch.float32, device=x.device) if want_stats else None
    rc = lib.t2o_stem_fwd_any(_ptr(x), _ptr(weight), _ptr(y), _ptr(stats), N, Hi, Wi, Co, 0, _stream(x.device))
    _lib.check(rc, 't2o_stem_fwd_any')
    return (y, stats) if want_stats else y


def stem_wgrad(x, dy):
    """Weight gradient of the stem convolution (t2o_stem_wgrad_nhwc): x (N,3,2Ho,2Wo), dy (N,Co,Ho,Wo), Co = 32 / 64,
    both channels-last; returns dw (Co,3,3,3) channels-last.  Deterministic."""
    _need_gpu(x, dy)
    N, Co, Ho, Wo = dy.shape
    if tuple(x.shape) != (N, 3, 2 * Ho, 2 * Wo) or Co not in (32, 64):
        raise ValueError('stem_wgrad: x must be (N, 3, 2 Ho, 2 Wo) and dy have 32 or 64 channels')
    x = x.contiguous(memory_format=torch.channels_last)
    dy = dy.contiguous(memory_format=torch.channels_last)
    lib = _lib.load()
    ws = torch.empty(lib.t2o_stem_wgrad_workspace_bytes(N, Ho, Wo, Co), dtype=torch.uint8, device=x.device)
    dw = torch.empty((Co, 3, 3, 3), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    rc = lib.t2o_stem_wgrad_nhwc(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), ws.numel(), N, Ho, Wo, Co, _stream(x.device))
    _lib.check(rc, 't2o_stem_wgrad_nhwc')
    return dw


def conv3x3s2_wgrad(x, dy):
    """Weight gradient of conv2d(x, w, None, stride 2, padding 1) (t2o_conv3x3s2_wgrad_nhwc).  x (N,Ci,2Ho,2Wo),
    dy (N,Co,Ho,Wo), both channels-last; returns dw (Co,Ci,3,3) channels-last."""
    return _conv_wgrad('conv3x3s2_wgrad', x, dy, 2, 'channels must be multiples of 64, Wo a multiple of 4')


def conv3x3s2_supported(x, weight, stride, padding):
    """The stride-2 layers whose data gradient runs on the own kernels: channels-last fp32 on the GPU, 3x3 / stride 2 /
    padding 1, even image size; either Ci a multiple of 64, Co of 32 and an output width that is a multiple of 8
    (matrix cores), or the 3-channel stem with 32 / 64 output channels."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and tuple(weight.shape[2:]) == (3, 3)
            and tuple(stride) == (2, 2) and tuple(padding) == (1, 1) and x.is_contiguous(memory_format=torch.channels_last)):
        return False
    if weight.shape[1] == 3 and (x.shape[2] % 2 or x.shape[3] % 2) and torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        return False                                           # (the stem's GRADIENT kernels want an even image; its forward takes any)
    if weight.shape[1] == 3:                                   # the stem: a streaming kernel (no matrix-core shape)
        return weight.shape[0] in (32, 64)
    return weight.shape[0] % 64 == 0 and weight.shape[1] % 64 == 0


class _Conv3x3S2Fn(torch.autograd.Function):
    """conv2d(x, w, 3x3, stride 2, padding 1) on the hand-written kernels, all three directions (a stem with an odd-sized
    image and gradients keeps the library call: its gradient kernels want an even image)."""

    @staticmethod
    def forward(ctx, x, weight, want_stats=False):
        ctx.save_for_backward(x, weight)
        even = x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
        own = weight.shape[1] % 32 == 0 and weight.shape[0] % 64 == 0 and x.shape[3] % 16 == 0 and even
        stem = weight.shape[1] == 3 and weight.shape[0] in (32, 64)
        fwd = conv3x3s2_forward if own else stem_forward if stem else None
        slow = (lambda: conv3x3_any_forward(x, weight, 2)) if weight.shape[1] % 32 == 0 else \
            (lambda: torch.nn.functional.conv2d(x, weight, None, 2, 1))
        if want_stats:                                       # (y, stats); stats None where the any-size kernel computes y
            y, stats = fwd(x, weight, True) if fwd else (slow(), None)
            if stats is not None:
                ctx.mark_non_differentiable(stats)
            return y, stats
        return fwd(x, weight) if fwd else slow()

    @staticmethod
    def backward(ctx, dy, _gstats=None):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous(memory_format=torch.channels_last)
        is_stem = weight.shape[1] == 3
        even = x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
        fast_d = even and (is_stem or dy.shape[3] % 8 == 0)
        own = ctx.needs_input_grad[0] and fast_d
        own_w = (ctx.needs_input_grad[1] and weight.shape[0] % 64 == 0 and weight.shape[1] % 64 == 0
                 and dy.shape[3] % 4 == 0 and even)
        stem_w = ctx.needs_input_grad[1] and is_stem and weight.shape[0] in (32, 64)
        any_d = ctx.needs_input_grad[0] and not own and not is_stem
        any_w = ctx.needs_input_grad[1] and not own_w and not stem_w and not is_stem
        mask = [ctx.needs_input_grad[0] and not own and not any_d, ctx.needs_input_grad[1] and not own_w and not stem_w and not any_w, False]
        dx = dw = None
        if mask[0] or mask[1]:                               # (only a 3-channel stem on an odd-sized image)
            dx, dw, _ = torch.ops.aten.convolution_backward(dy, x, weight, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, mask)
        if own:
            dx = conv3x3s2_dgrad(dy, weight)
        elif any_d:
            dx = conv3x3_any_dgrad(dy, weight, x.shape[2:], 2)
        if own_w:
            dw = conv3x3s2_wgrad(x, dy)
        elif stem_w:
            dw = stem_wgrad(x, dy)
        elif any_w:
            dw = conv3x3_any_wgrad(x, dy, 2)
        return dx, dw, None


def conv3x3s2(x, weight, want_stats=False):
    """want_stats: (y, stats or None) -- see conv3x3_forward."""
    return _Conv3x3S2Fn.apply(x, weight, want_stats)


def conv3x3_supported(x, weight, stride, padding):
    """Layers the matrix-core convolution kernels take: channels-last fp32 activations on the GPU, 3x3 / stride 1 /
    padding 1, channel counts multiples of 64, image width a multiple of 4 (every BasicBlock convolution of the
    encoder except the strided ones, for inputs of 32 pixels and more)."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and tuple(weight.shape[2:]) == (3, 3)
            and tuple(stride) == (1, 1) and tuple(padding) == (1, 1) and weight.shape[0] % 64 == 0
            and weight.shape[1] % 64 == 0 and x.is_contiguous(memory_format=torch.channels_last))


def _own_direct(x):
    """The forward / data-gradient kernel wants W % 8 == 0 (a DMA piece of 8 pixels inside one image row)."""
    return x.shape[3] % 8 == 0


class _Conv3x3Fn(torch.autograd.Function):
    """conv2d(x, w, 3x3, stride 1, padding 1) on the hand-written MFMA kernels (t2o_conv.hip)."""

    @staticmethod
    def forward(ctx, x, weight, want_stats=False):
        ctx.save_for_backward(x, weight)
        own = _own_direct(x)
        if want_stats:                                      # (y, stats); stats None where the any-size kernel computes y
            y, stats = conv3x3_forward(x, weight, True) if own else (conv3x3_any_forward(x, weight, 1), None)
            if stats is not None:
                ctx.mark_non_differentiable(stats)
            return y, stats
        return conv3x3_forward(x, weight) if own else conv3x3_any_forward(x, weight, 1)

    @staticmethod
    def backward(ctx, dy, _gstats=None):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = None
        if ctx.needs_input_grad[0]:
            if _own_direct(x):
                dx = conv3x3_dgrad(dy, weight)
            else:
                dx = conv3x3_any_dgrad(dy, weight, x.shape[2:], 1)
        dw = None
        if ctx.needs_input_grad[1]:
            if x.shape[3] % 4 == 0:
                dw = conv3x3_wgrad(x, dy)
            else:
                dw = conv3x3_any_wgrad(x, dy, 1)
        return dx, dw, None


def conv3x3(x, weight, want_stats=False):
    """want_stats: (y, stats or None) -- see conv3x3_forward."""
    return _Conv3x3Fn.apply(x, weight, want_stats)


class _SequenceFn(torch.autograd.Function):
    """A known operator list with every intermediate materialised + L1 on the last output."""

    @staticmethod
    def forward(ctx, img, params, target, ops):
        _need_gpu(img, params, target)
        img, params, target = _img(img), params.contiguous(), _img(target)
        B, _, H, W = img.shape
        K = len(ops)
        if params.shape != (K, B, PARAM_PAD):
            raise ValueError('params must be (K,B,24)')
        acts = torch.empty((K,) + tuple(img.shape), dtype=torch.float32, device=img.device)
        loss = torch.empty((), dtype=torch.float32, device=img.device)
        ws = workspace(B, H, W, img.device)
        c_ops = (ctypes.c_int * K)(*ops)
        rc = _lib.load().t2o_sequence_fwd(c_ops, K, _ptr(img), _ptr(params), _ptr(target), _ptr(acts), _ptr(loss),
                                          _ptr(ws), ws.numel(), B, H, W, _stream(img.device))
        _lib.check(rc, 't2o_sequence_fwd')
        ctx.save_for_backward(img, params, target, acts)
        ctx.ops = tuple(ops)
        ctx.mark_non_differentiable(acts)
        return loss, acts

    @staticmethod
    def backward(ctx, gloss, _gacts):
        img, params, target, acts = ctx.saved_tensors
        B, _, H, W = img.shape
        K = len(ctx.ops)
        gloss = gloss.contiguous().to(torch.float32)
        gimg = torch.empty_like(img) if ctx.needs_input_grad[0] else None
        gparams = torch.zeros_like(params)
        gbuf = torch.empty((2,) + tuple(img.shape), dtype=torch.float32, device=img.device)
        ws = workspace(B, H, W, img.device)
        c_ops = (ctypes.c_int * K)(*ctx.ops)
        rc = _lib.load().t2o_sequence_bwd(c_ops, K, _ptr(img), _ptr(params), _ptr(target), _ptr(acts), _ptr(gloss),
                                          _ptr(gimg), _ptr(gparams), _ptr(gbuf), _ptr(ws), ws.numel(), B, H, W,
                                          _stream(img.device))
        _lib.check(rc, 't2o_sequence_bwd')
        return gimg, gparams, None, None


def sequence_l1(img, ops, params, target):
    """Apply ops[k] with params[k] (K,B,24) in order; returns (mean |out - target|, acts (K,B,3,H,W))."""
    return _SequenceFn.apply(img, params, target, [int(o) for o in ops])


_prepared_chains = {}
_CHAIN_JIT = True        # (module switch for the tests; no environment knob)


def prepare_fused_sequence(ops):
    """Run-time specialisation of the fused chain kernels for this operator list (t2o_fused_sequence_prepare: hipRTC,
    ~1 s per new list, code objects cached on disk).  Returns True when the list now runs on compile-time-specialised
    kernels (ahead-of-time or run-time compiled), False when the machine has no hipRTC (run-time-loop kernels stay)."""
    key = tuple(int(o) for o in ops)
    got = _prepared_chains.get(key)
    if got is None:
        lib = _lib.load()
        c_ops = (ctypes.c_int * max(len(key), 1))(*key)
        rc = lib.t2o_fused_sequence_prepare(c_ops, len(key))
        if rc == 0:
            got = True
        else:
            # no libhiprtc on this machine (status 2), a compile error, an unreadable cached code object ...: specialisation
            # is an optimisation -- warn once for anything but the expected "no hipRTC", remember the outcome (no retry per
            # call) and let the run-time-loop kernels serve this list
            got = False
            if rc != 2:
                import warnings
                warnings.warn('t2o_fused_sequence_prepare(%s) failed (status %d: %s); using the run-time-loop kernels'
                              % (list(key), rc, lib.t2o_last_error().decode('utf-8', 'replace')))
        _prepared_chains[key] = got
    return got


class _FusedSequenceFn(torch.autograd.Function):
    """A known operator list with runs of pointwise operators fused in registers; only the
    final image (and the images around each sharpness) exist in HBM."""

    @staticmethod
    def forward(ctx, img, params, target, ops):
        _need_gpu(img, params, target)
        img, params, target = _img(img), params.contiguous(), _img(target)
        B, _, H, W = img.shape
        K = len(ops)
        if params.shape != (K, B, PARAM_PAD):
            raise ValueError('params must be (K,B,24)')
        lib = _lib.load()
        c_ops = (ctypes.c_int * max(K, 1))(*ops)
        nbuf = lib.t2o_fused_sequence_buffers(c_ops, K)
        if nbuf < 0:
            raise RuntimeError('unsupported operator in sequence %s' % (ops,))
        if _CHAIN_JIT and tuple(ops) not in _prepared_chains and not torch.cuda.is_current_stream_capturing():
            prepare_fused_sequence(ops)                        # first use of this list: specialise its chain kernels
        seg = torch.empty((max(nbuf, 1),) + tuple(img.shape), dtype=torch.float32, device=img.device)
        out = torch.empty_like(img)
        loss = torch.empty((), dtype=torch.float32, device=img.device)
        ws = workspace(B, H, W, img.device)
        rc = lib.t2o_fused_sequence_fwd(c_ops, K, _ptr(img), _ptr(params), _ptr(target), _ptr(out), _ptr(loss),
                                        _ptr(seg), _ptr(ws), ws.numel(), B, H, W, _stream(img.device))
        _lib.check(rc, 't2o_fused_sequence_fwd')
        ctx.save_for_backward(img, params, target, seg)
        ctx.ops = tuple(ops)
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    def backward(ctx, gloss, _gout):
        img, params, target, seg = ctx.saved_tensors
        B, _, H, W = img.shape
        K = len(ctx.ops)
        gloss = gloss.contiguous().to(torch.float32)
        gimg = torch.empty_like(img) if ctx.needs_input_grad[0] else None
        gparams = torch.empty_like(params)
        gbuf = torch.empty((2,) + tuple(img.shape), dtype=torch.float32, device=img.device)
        ws = workspace(B, H, W, img.device)
        c_ops = (ctypes.c_int * max(K, 1))(*ctx.ops)
        rc = _lib.load().t2o_fused_sequence_bwd(c_ops, K, _ptr(img), _ptr(params), _ptr(target), _ptr(gloss), None,
                                                _ptr(gimg), _ptr(gparams), _ptr(seg), _ptr(gbuf), _ptr(ws), ws.numel(),
                                                B, H, W, _stream(img.device))
        _lib.check(rc, 't2o_fused_sequence_bwd')
        return gimg, gparams, None, None


def fused_sequence_l1(img, ops, params, target):
    """Like sequence_l1 but fused: returns (mean |out - target|, out (B,3,H,W))."""
    return _FusedSequenceFn.apply(img, params, target, [int(o) for o in ops])


def fused_sequence_l1_value_grad(img, ops, params, target, gloss=None, want_image=False, want_image_grad=True):
    """loss = mean |sequence(img) - target| AND its gradients in one call, outside autograd (the inner loop of a
    parameter fit or a planner step: execute K times + L1Loss + backward, executors/executor.py:33-55,
    utils/beam_search.py:65-91).  t2o_fused_sequence_l1_value_grad: the last segment's forward is not launched -- its
    backward kernels produce the loss (and the image) too -- so BASELINE configs[1]'s list takes 3 launches instead of 4
    and a list without sharpness ONE.  Gradients and image bit-identical to fused_sequence_l1(...) + backward, the loss
    equal up to summation order.

    params (K,B,24); gloss: () tensor scaling the gradients (default 1).  Returns (loss (), gimg (B,3,H,W) or None,
    gparams (K,B,24), out (B,3,H,W) or None)."""
    _need_gpu(img, params, target)
    img, params, target = _img(img.detach()), params.detach().contiguous(), _img(target.detach())
    ops = [int(o) for o in ops]
    B, _, H, W = img.shape
    K = len(ops)
    if params.shape != (K, B, PARAM_PAD):
        raise ValueError('params must be (K,B,24)')
    lib = _lib.load()
    c_ops = (ctypes.c_int * max(K, 1))(*ops)
    nbuf = lib.t2o_fused_sequence_buffers(c_ops, K)
    if nbuf < 0:
        raise RuntimeError('unsupported operator in sequence %s' % (ops,))
    if _CHAIN_JIT and tuple(ops) not in _prepared_chains and not torch.cuda.is_current_stream_capturing():
        prepare_fused_sequence(ops)
    dev = img.device
    gloss = torch.ones((), dtype=torch.float32, device=dev) if gloss is None else gloss.detach().contiguous().to(torch.float32)
    # one allocation for the scratch images: segment boundaries, the two gradient buffers, and (sharpness on the tile
    # kernels, W % 4 != 0: the call falls back to forward + backward) the final image
    scratch = torch.empty((max(nbuf, 1) + 2,) + tuple(img.shape), dtype=torch.float32, device=dev)
    seg, gbuf = scratch[:max(nbuf, 1)], scratch[max(nbuf, 1):]
    out = torch.empty_like(img) if want_image or W % 4 else None
    gimg = torch.empty_like(img) if want_image_grad else None
    gparams = torch.empty_like(params)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ws = workspace(B, H, W, dev)
    rc = lib.t2o_fused_sequence_l1_value_grad(c_ops, K, _ptr(img), _ptr(params), _ptr(target), _ptr(gloss), _ptr(out),
                                              _ptr(loss), _ptr(gimg), _ptr(gparams), _ptr(seg), _ptr(gbuf), _ptr(ws),
                                              ws.numel(), B, H, W, _stream(dev))
    _lib.check(rc, 't2o_fused_sequence_l1_value_grad')
    return loss, gimg, gparams, (out if want_image else None)


def _planner_masks(who, masks, mask_index, J, imgs):
    """The (masks, mask_index) keywords of the two planner calls, checked HERE so that a wrong plane or index is a Python
    error and never a GPU fault -> (planes or None, n_mask, ctypes index array)."""
    index = [-1] * J if mask_index is None else [int(k) for k in mask_index]
    if len(index) != J:
        raise ValueError('%s: one mask index per job (%d for %d jobs)' % (who, len(index), J))
    n = 0
    if masks is not None:
        if not (torch.is_tensor(masks) and masks.is_cuda and masks.dtype == torch.uint8 and masks.dim() == 3 and masks.is_contiguous()):
            raise ValueError('%s: masks must be a contiguous (N,H,W) uint8 GPU tensor' % who)
        if masks.device != imgs.device or tuple(masks.shape[-2:]) != tuple(imgs.shape[-2:]):
            raise ValueError('%s: masks %s on %s do not match the images %s on %s' % (
                who, tuple(masks.shape), masks.device, tuple(imgs.shape), imgs.device))
        n = masks.shape[0]
    if any(k < -1 or k >= n for k in index):
        raise ValueError('%s: mask_index must lie in [-1, %d) (-1 = no mask), got %s' % (who, n, index))
    return (masks if n else None), n, (ctypes.c_int * max(J, 1))(*index)


def candidates_multi_l1(ops, img_index, imgs, target, params, masks=None, mask_index=None):
    """loss[j, c] = mean |execute(imgs[img_index[j]], ops[j], params[j, c]) - target| for J jobs x C candidates in
    ONE launch (t2o_op_candidates_multi_l1).  ops / img_index: python ints; imgs (n,3,H,W); params (J,C,n).
    masks (N,H,W) uint8 on the images' device + mask_index (python ints, -1 = none): job j's candidates are blended under
    plane mask_index[j], m = float(byte) -- execute(..., mask=plane.float()) -- by t2o_op_candidates_multi_l1_masked."""
    _need_gpu(imgs, target, params)
    imgs = imgs.reshape(-1, 3, *imgs.shape[-2:]).contiguous()
    target = target.reshape(3, *target.shape[-2:]).contiguous()
    params = params.contiguous()
    J, C = params.shape[0], params.shape[1]
    H, W = imgs.shape[-2:]
    lib = _lib.load()
    if masks is not None or mask_index is not None:
        planes, n_mask, c_mask = _planner_masks('candidates_multi_l1', masks, mask_index, J, imgs)
    loss = torch.empty(J, C, dtype=torch.float32, device=imgs.device)
    ws = torch.empty(max(lib.t2o_candidates_multi_workspace_bytes(J, C, H, W), 4), dtype=torch.uint8, device=imgs.device)
    c_ops = (ctypes.c_int * J)(*[int(o) for o in ops])
    c_idx = (ctypes.c_int * J)(*[int(i) for i in img_index])
    if masks is not None or mask_index is not None:
        rc = lib.t2o_op_candidates_multi_l1_masked(c_ops, c_idx, c_mask, J, _ptr(imgs), imgs.shape[0], _ptr(planes), n_mask,
                                                   _ptr(target), _ptr(params), C, params.shape[2], _ptr(loss), _ptr(ws),
                                                   ws.numel(), H, W, _stream(imgs.device))
        _lib.check(rc, 't2o_op_candidates_multi_l1_masked')
        return loss
    rc = lib.t2o_op_candidates_multi_l1(c_ops, c_idx, J, _ptr(imgs), imgs.shape[0], _ptr(target), _ptr(params), C,
                                        params.shape[2], _ptr(loss), _ptr(ws), ws.numel(), H, W, _stream(imgs.device))
    _lib.check(rc, 't2o_op_candidates_multi_l1')
    return loss


FIT_MAX_JOBS = 64


def fit_multi_l1(ops, img_index, imgs, targets, target_index, params0, steps=300, lr=2e-2, check_every=50, tol=1e-6,
                 betas=(0.9, 0.999), eps=1e-8, masks=None, mask_index=None):
    """Adam on the parameters of J <= 64 jobs at once, entirely on the device (t2o_fit_multi_l1_adam; with masks (N,H,W)
    uint8 + mask_index, as in candidates_multi_l1, t2o_fit_multi_l1_adam_masked: job j is fitted under its plane): job j fits
    operator ops[j] on imgs[img_index[j]] against targets[target_index[j]] under mean |execute - target|, starting
    from params0[j].  ops / img_index / target_index: python ints; imgs (n,3,H,W); targets (m,3,H,W); params0 (J,n<=24).
    torch.optim.Adam's update and the serial fit's stop rule (check_every <= 0: none), two launches per iteration, no
    host synchronisation.  Returns (params (J,24) zero padded, dist (J,) = the loss at those parameters)."""
    _need_gpu(imgs, targets, params0)
    imgs = imgs.detach().reshape(-1, 3, *imgs.shape[-2:]).contiguous()
    targets = targets.detach().reshape(-1, 3, *targets.shape[-2:]).contiguous()
    if imgs.shape[-2:] != targets.shape[-2:]:
        raise ValueError('images and targets must have one size')
    J = len(ops)
    if not (len(img_index) == len(target_index) == J == params0.shape[0]) or params0.dim() != 2 or params0.shape[1] > PARAM_PAD:
        raise ValueError('one (operator, image index, target index, parameter row of at most 24) per job')
    H, W = imgs.shape[-2:]
    dev = imgs.device
    if params0.shape[1] == PARAM_PAD:
        params = params0.detach().contiguous().clone()                   # (a device copy, no kernel)
    else:
        params = torch.zeros(J, PARAM_PAD, dtype=torch.float32, device=dev)
        params[:, :params0.shape[1]] = params0.detach()
    dist = torch.empty(J, dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws = torch.empty(max(lib.t2o_fit_multi_workspace_bytes(J, H, W), 8), dtype=torch.uint8, device=dev)
    c_ops = (ctypes.c_int * max(J, 1))(*[int(o) for o in ops])
    c_img = (ctypes.c_int * max(J, 1))(*[int(i) for i in img_index])
    c_tgt = (ctypes.c_int * max(J, 1))(*[int(i) for i in target_index])
    if masks is not None or mask_index is not None:
        planes, n_mask, c_mask = _planner_masks('fit_multi_l1', masks, mask_index, J, imgs)
        rc = lib.t2o_fit_multi_l1_adam_masked(c_ops, c_img, c_tgt, c_mask, J, _ptr(imgs), imgs.shape[0], _ptr(targets),
                                              targets.shape[0], _ptr(planes), n_mask, _ptr(params), _ptr(dist), _ptr(ws),
                                              ws.numel(), H, W, int(steps), float(lr), float(betas[0]), float(betas[1]),
                                              float(eps), int(check_every), float(tol), _stream(dev))
        _lib.check(rc, 't2o_fit_multi_l1_adam_masked')
        return params, dist
    rc = lib.t2o_fit_multi_l1_adam(c_ops, c_img, c_tgt, J, _ptr(imgs), imgs.shape[0], _ptr(targets), targets.shape[0],
                                   _ptr(params), _ptr(dist), _ptr(ws), ws.numel(), H, W, int(steps), float(lr),
                                   float(betas[0]), float(betas[1]), float(eps), int(check_every), float(tol), _stream(dev))
    _lib.check(rc, 't2o_fit_multi_l1_adam')
    return params, dist


class _SsimFn(torch.autograd.Function):
    """out (B) = per-sample mean of the SSIM map; backward = t2o_ssim_bwd (closed form, one launch)."""

    @staticmethod
    def forward(ctx, img1, img2):
        B, C, H, W = img1.shape
        lib = _lib.load()
        out = torch.empty(B, dtype=torch.float32, device=img1.device)
        ws = torch.empty(max(lib.t2o_ssim_workspace_bytes(B, C, H, W), 4), dtype=torch.uint8, device=img1.device)
        rc = lib.t2o_ssim_fwd(_ptr(img1), _ptr(img2), _ptr(out), _ptr(ws), ws.numel(), B, C, H, W, _stream(img1.device))
        _lib.check(rc, 't2o_ssim_fwd')
        ctx.save_for_backward(img1, img2)
        return out

    @staticmethod
    def backward(ctx, gout):
        img1, img2 = ctx.saved_tensors
        B, C, H, W = img1.shape
        g1 = torch.empty_like(img1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(img2) if ctx.needs_input_grad[1] else None
        if g1 is None and g2 is None:
            return None, None
        gout = gout.contiguous().float()
        rc = _lib.load().t2o_ssim_bwd(_ptr(img1), _ptr(img2), _ptr(gout), _ptr(g1), _ptr(g2), B, C, H, W, _stream(img1.device))
        _lib.check(rc, 't2o_ssim_bwd')
        return g1, g2


def ssim(img1, img2, size_average=True):
    """SSIM of utils/ssim/__init__.py (11x11 Gaussian, sigma 1.5).  Returns a scalar (size_average) or one value per sample.
    Differentiable w.r.t. both images (t2o_ssim_bwd): `1 - ssim(pred, target)` is usable as a loss, as the reference's SSIM
    module is under autograd (utils/ssim/__init__.py:43-66)."""
    _need_gpu(img1, img2)
    if img1.shape != img2.shape or img1.dim() != 4:
        raise ValueError('ssim expects two (B,C,H,W) tensors of the same shape')
    if img1.dtype != torch.float32 or img2.dtype != torch.float32:
        raise ValueError('ssim expects fp32 images')
    out = _SsimFn.apply(img1.contiguous(), img2.contiguous())
    return out.mean() if size_average else out


def _first_steps(first, B, device, what):
    if not (torch.is_tensor(first) and first.is_cuda and first.dtype == torch.int64 and tuple(first.shape) == (B,)):
        raise ValueError('%s: first must be an int64 GPU tensor of shape (%d,)' % (what, B))
    if first.device != device:
        raise ValueError('%s: tensors on different devices' % what)
    return first.contiguous()


def eval_metrics(input, imgs, first, target, out=None, with_ssim=True):
    """The four numbers the test loop takes per batch (utils/eval.py:50-60, test_seq2seqL1.py:60-74) in ONE call
    (t2o_eval_metrics): [mean |input - target|, mean |out - target|, SSIM(input, target), SSIM(out, target)] with
    out[b] = imgs[first[b]][b] -- imgs the list of T <= 8 (B,C,H,W) step images of an episode (episode_forward(...,
    stack=False)), first (B) int64 on the GPU (train.first_end_step), read where the images lie.  with_ssim=False: the two
    SSIM slots are 0 and no Gaussian pass runs.  out: a contiguous fp32 GPU tensor of 4 elements to fill (a row of a table);
    a new (4,) tensor otherwise.  No host synchronisation."""
    imgs = list(imgs)
    _need_gpu(input, target, out, *imgs)
    if target.dim() != 4 or input.shape != target.shape or any(t.shape != target.shape for t in imgs):
        raise ValueError('eval_metrics: input, target and every step image must be (B,C,H,W) tensors of one shape')
    B, C, H, W = target.shape
    dev = target.device
    first = _first_steps(first, B, dev, 'eval_metrics')
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=dev)
    elif not (out.is_contiguous() and out.numel() == 4):
        raise ValueError('eval_metrics: out must be a contiguous fp32 GPU tensor of 4 elements')
    if any(t.device != dev for t in [input, out] + imgs):
        raise ValueError('eval_metrics: tensors on different devices')
    input, target = input.detach().contiguous(), target.detach().contiguous()
    imgs = [t.detach().contiguous() for t in imgs]
    lib = _lib.load()
    ws = _scratch(lib.t2o_eval_metrics_workspace_bytes(B, C, H, W), dev)
    rc = lib.t2o_eval_metrics(_ptr(input), _ptr_array(imgs), len(imgs), _ptr(first), _ptr(target), _ptr(out), 1 if with_ssim else 0,
                              _ptr(ws), ws.numel(), B, C, H, W, _stream(dev))
    _lib.check(rc, 't2o_eval_metrics')
    return out


def end_select_var_mean(lists, firsts, out=None):
    """torch.var(torch.cat(ends), dim=0).mean() of test_variance (test_seq2seqL1.py:130-133) in ONE call
    (t2o_end_select_var_mean): lists = R <= 16 lists of T <= 8 step images (B, ...) -- one episode per request on the same
    batch -- firsts = R (B) int64 GPU tensors; ends[r][b] = lists[r][firsts[r][b]][b] is read where it lies.  out: a
    contiguous fp32 GPU tensor of 1 element to fill (an entry of a table); a new 0-d tensor otherwise.  No host
    synchronisation."""
    lists = [list(l) for l in lists]
    firsts = list(firsts)
    flat = [t for l in lists for t in l]
    _need_gpu(out, *flat)
    if not flat or len(firsts) != len(lists) or any(len(l) != len(lists[0]) for l in lists):
        raise ValueError('end_select_var_mean: R lists of T step images each and R first-step tensors')
    shape, dev = flat[0].shape, flat[0].device
    if len(shape) < 1 or any(t.shape != shape or t.device != dev for t in flat):
        raise ValueError('end_select_var_mean: every step image must have one shape (B, ...) and one device')
    B = shape[0]
    row = flat[0].numel() // max(B, 1)
    firsts = [_first_steps(f, B, dev, 'end_select_var_mean') for f in firsts]
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=dev)
    elif not (out.is_contiguous() and out.numel() == 1 and out.device == dev):
        raise ValueError('end_select_var_mean: out must be a contiguous fp32 GPU tensor of 1 element on the images\' device')
    flat = [t.detach().contiguous() for t in flat]
    lib = _lib.load()
    ws = _scratch(lib.t2o_end_select_var_mean_workspace_bytes(row), dev)
    rc = lib.t2o_end_select_var_mean(_ptr_array(flat), _ptr_array(firsts), len(lists), len(lists[0]), B, row, _ptr(out), _ptr(ws),
                                     ws.numel(), _stream(dev))
    _lib.check(rc, 't2o_end_select_var_mean')
    return out


def candidates_l1(op, img, target, params):
    """loss[c] = mean |execute(img, op, params[c]) - target| for C candidate rows, one launch.
    img/target (1,3,H,W) or (3,H,W); params (C,n).  Per-pixel operators only (not sharpness)."""
    _need_gpu(img, target, params)
    img = img.reshape(3, *img.shape[-2:]).contiguous()
    target = target.reshape(3, *target.shape[-2:]).contiguous()
    params = params.contiguous()
    C = params.shape[0]
    H, W = img.shape[-2:]
    lib = _lib.load()
    loss = torch.empty(C, dtype=torch.float32, device=img.device)
    ws = torch.empty(max(lib.t2o_candidates_workspace_bytes(C, H, W), 4), dtype=torch.uint8, device=img.device)
    rc = lib.t2o_op_candidates_l1(int(op), _ptr(img), _ptr(target), _ptr(params), C, params.shape[1], _ptr(loss),
                                  _ptr(ws), ws.numel(), H, W, _stream(img.device))
    _lib.check(rc, 't2o_op_candidates_l1')
    return loss


# ---- round 3: entry points of the encoder's explicit schedule (encoder.py), exposed for tests and tools ----------------
def conv_weight_transform(weight, taps, flip):
    """wt (Ci, taps, Co) from a channels-last (Co, Ci, kh, kw) weight (t2o_conv_weight_transform)."""
    _need_gpu(weight)
    Co, Ci = weight.shape[0], weight.shape[1]
    w = weight.contiguous(memory_format=torch.channels_last)
    wt = torch.empty(Ci * taps * Co, dtype=torch.float32, device=weight.device)
    _lib.check(_lib.load().t2o_conv_weight_transform(_ptr(w), _ptr(wt), Co, Ci, taps, 1 if flip else 0, _stream(weight.device)),
               't2o_conv_weight_transform')
    return wt


def conv3x3_dgrad_pre(dy, wt, Ci, addend=None):
    """t2o_conv3x3_dgrad_pre_nhwc: dy (N,Co,H,W) channels-last, wt = conv_weight_transform(w, 9, True); addend (N,Ci,H,W)
    channels-last or None is added in the epilogue.  Returns dx (N,Ci,H,W) channels-last."""
    _need_gpu(dy, wt, addend)
    N, Co, H, W = dy.shape
    dy = dy.contiguous(memory_format=torch.channels_last)
    addend = None if addend is None else addend.contiguous(memory_format=torch.channels_last)
    ws = _conv_workspace(dy.device, 64 << 10)
    dx = torch.empty((N, Ci, H, W), dtype=torch.float32, device=dy.device, memory_format=torch.channels_last)
    rc = _lib.load().t2o_conv3x3_dgrad_pre_nhwc(_ptr(dy), _ptr(wt), _ptr(addend), _ptr(dx), _ptr(ws), ws.numel(), N, H, W, Ci, Co,
                                                _stream(dy.device))
    _lib.check(rc, 't2o_conv3x3_dgrad_pre_nhwc')
    return dx


def conv1x1s2_forward(x, weight):
    """conv2d(x, weight, None, stride 2) for a 1x1 weight (Co,Ci,1,1): x (N,Ci,H,W) channels-last -> y (N,Co,(H+1)//2,(W+1)//2)."""
    _need_gpu(x, weight)
    N, Ci, H, W = x.shape
    Co = weight.shape[0]
    x = x.contiguous(memory_format=torch.channels_last)
    w = weight.reshape(Co, Ci).contiguous()
    y = torch.empty((N, Co, (H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    _lib.check(_lib.load().t2o_conv1x1s2_fwd_nhwc(_ptr(x), _ptr(w), _ptr(y), N, H, W, Ci, Co, _stream(x.device)), 't2o_conv1x1s2_fwd_nhwc')
    return y


def conv1x1s2_dgrad_acc(dy, weight, dx):
    """dx[:, :, ::2, ::2] += data gradient of the 1x1 stride-2 convolution, in place (dx (N,Ci,H,W) channels-last)."""
    _need_gpu(dy, weight, dx)
    N, Ci, H, W = dx.shape
    Co = weight.shape[0]
    if not dx.is_contiguous(memory_format=torch.channels_last):
        raise ValueError('conv1x1s2_dgrad_acc: dx must be channels-last (it is updated in place)')
    dy = dy.contiguous(memory_format=torch.channels_last)
    wt = conv_weight_transform(weight.reshape(Co, Ci, 1, 1), 1, False)
    _lib.check(_lib.load().t2o_conv1x1s2_dgrad_acc_nhwc(_ptr(dy), _ptr(wt), _ptr(dx), N, H, W, Ci, Co, _stream(dx.device)),
               't2o_conv1x1s2_dgrad_acc_nhwc')
    return dx


def conv1x1s2_wgrad(x, dy, into=None):
    """Weight gradient (Co,Ci,1,1) of the 1x1 stride-2 convolution; into: an existing gradient tensor that is added to."""
    _need_gpu(x, dy, into)
    N, Ci, H, W = x.shape
    Co = dy.shape[1]
    x = x.contiguous(memory_format=torch.channels_last)
    dy = dy.contiguous(memory_format=torch.channels_last)
    lib = _lib.load()
    need = lib.t2o_conv1x1s2_wgrad_workspace_bytes(N, H, W, Ci, Co)
    if need == 0:
        raise RuntimeError('conv1x1s2_wgrad: unsupported shape (channel counts must be multiples of 64)')
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    dw = into if into is not None else torch.empty((Co, Ci, 1, 1), dtype=torch.float32, device=x.device)
    rc = lib.t2o_conv1x1s2_wgrad_nhwc(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), need, N, H, W, Ci, Co, 1 if into is not None else 0,
                                      _stream(x.device))
    _lib.check(rc, 't2o_conv1x1s2_wgrad_nhwc')
    return dw


def stem_planar(x, weight, dy=None, want='fwd', into=None):
    """The stem kernels on an NCHW image (t2o_stem_fwd / _wgrad / _dgrad with planar = 1).  want = 'fwd': (y, stats);
    'wgrad': dw (Co,3,3,3) channels-last (into: added to); 'dgrad': dx (N,3,2Ho,2Wo) NCHW (into: added to)."""
    lib = _lib.load()
    Co = weight.shape[0]
    w = weight.contiguous(memory_format=torch.channels_last)
    if want == 'dgrad':
        N, _, Ho, Wo = dy.shape
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = into if into is not None else torch.empty((N, 3, 2 * Ho, 2 * Wo), dtype=torch.float32, device=dy.device)
        _lib.check(lib.t2o_stem_dgrad(_ptr(dy), _ptr(w), _ptr(dx), N, Ho, Wo, Co, 1, 1 if into is not None else 0, _stream(dy.device)),
                   't2o_stem_dgrad')
        return dx
    x = x.contiguous()
    N, _, Hi, Wi = x.shape
    Ho, Wo = Hi // 2, Wi // 2
    if want == 'fwd':
        y = torch.empty((N, Co, Ho, Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        stats = torch.empty((lib.t2o_stem_fwd_stats_rows(N, Ho, Wo), 2, Co), dtype=torch.float32, device=x.device)
        _lib.check(lib.t2o_stem_fwd(_ptr(x), _ptr(w), _ptr(y), _ptr(stats), N, Ho, Wo, Co, 1, _stream(x.device)), 't2o_stem_fwd')
        return y, stats
    dy = dy.contiguous(memory_format=torch.channels_last)
    need = lib.t2o_stem_wgrad_workspace_bytes(N, Ho, Wo, Co)
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    dw = into if into is not None else torch.empty((Co, 3, 3, 3), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    _lib.check(lib.t2o_stem_wgrad(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), need, N, Ho, Wo, Co, 1, 1 if into is not None else 0,
                                  _stream(x.device)), 't2o_stem_wgrad')
    return dw


def _ld(t, what):
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] != 1 and t.stride(0) < t.shape[1]):
        raise ValueError('%s must be a 2-D fp32 matrix with contiguous rows (a column slice of a larger one is fine)' % what)
    return max(t.stride(0), t.shape[1])                    # (one row: its stride is never used and may be anything, 0 after expand())


def gemm(A, B, out=None, a_kmajor=False, b_kmajor=False, accumulate=False):
    """out (M,N) [+]= op(A) op(B) on this library's general matrix-core GEMM (t2o_gemm: one fixed reduction order per shape, the
    same bits on every machine -- the products the framework's BLAS used to pick a kernel for).  A is (M,K), or (K,M) with
    a_kmajor (a `dy^T x` product sums over the rows of both operands); B is (N,K) -- nn.Linear's weight layout -- or (K,N) with
    b_kmajor.  Operands and `out` may be column slices of larger matrices."""
    _need_gpu(A, B, out)
    if out is not None and out.device != A.device:
        raise ValueError('gemm: out is on %s, the operands on %s' % (out.device, A.device))
    K, M = (A.shape[0], A.shape[1]) if a_kmajor else (A.shape[1], A.shape[0])
    Kb, N = (B.shape[0], B.shape[1]) if b_kmajor else (B.shape[1], B.shape[0])
    if K != Kb:
        raise ValueError('gemm: contraction lengths differ (%d vs %d)' % (K, Kb))
    if out is None:
        if accumulate:
            raise ValueError('gemm: accumulate needs `out`')
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    elif tuple(out.shape) != (M, N):
        raise ValueError('gemm: out is %s, the product (%d, %d)' % (tuple(out.shape), M, N))
    if M == 0 or N == 0:
        return out
    if K == 0:
        return out if accumulate else out.zero_()
    rc = _lib.load().t2o_gemm(_ptr(A), _ptr(B), _ptr(out), M, N, K, _ld(A, 'gemm: A'), _ld(B, 'gemm: B'), _ld(out, 'gemm: out'),
                              1 if a_kmajor else 0, 1 if b_kmajor else 0, 1 if accumulate else 0, _stream(A.device))
    _lib.check(rc, 't2o_gemm')
    return out


def colsum(X, out=None, accumulate=False):
    """out (N) [+]= the column sums of X (R,N) in a fixed order (t2o_colsum): bias gradients."""
    _need_gpu(X, out)
    R, N = X.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=X.device)
    elif out.device != X.device:
        raise ValueError('colsum: out is on %s, X on %s' % (out.device, X.device))
    if not (out.dim() == 1 and out.numel() == N and out.is_contiguous() and out.dtype == torch.float32):
        raise ValueError('colsum: out must be a dense fp32 vector of %d' % N)
    if R == 0:
        return out if accumulate else out.zero_()
    _lib.check(_lib.load().t2o_colsum(_ptr(X), _ptr(out), R, N, _ld(X, 'colsum: X'), 1 if accumulate else 0, _stream(X.device)), 't2o_colsum')
    return out


class _LstmLayerFn(torch.autograd.Function):
    """One (bi)directional LSTM layer over zero-padded rows with per-sample lengths (t2o_lstm_layer_fwd / _bwd): the
    input GEMM for all steps and directions, the step kernels, and -- backward -- the weight / bias / input gradients as
    GEMMs over all steps.  Weights in nn.LSTM's layout; `dirs` tuples of (w_ih, w_hh, b_ih, b_hh) flattened."""

    @staticmethod
    def forward(ctx, x, lengths, has_bias, *w):
        _need_gpu(x, *w)
        D = len(w) // (4 if has_bias else 2)
        per = 4 if has_bias else 2
        w_ih = [w[per * d] for d in range(D)]
        w_hh = [w[per * d + 1] for d in range(D)]
        B, L, E = x.shape
        H = w_hh[0].shape[1]
        dev = x.device
        x = x.contiguous()
        wih_cat = torch.cat(w_ih, 0) if D > 1 else w_ih[0]                     # (D*4H, E)
        gi = gemm(x.view(B * L, E), wih_cat).view(B, L, -1)                    # (B, L, D*4H): x W_ih^T for all steps and directions
        whh_t = torch.stack([t.view(4, H, H).permute(2, 1, 0) for t in w_hh], 0).contiguous()     # (D, H(k), H(j), 4 gates)
        b_ih = torch.stack([w[per * d + 2] for d in range(D)], 0).contiguous() if has_bias else None
        b_hh = torch.stack([w[per * d + 3] for d in range(D)], 0).contiguous() if has_bias else None
        out = torch.empty(B, L, D * H, dtype=torch.float32, device=dev)
        hnew = torch.empty(L, D, B, H, dtype=torch.float32, device=dev)
        cnew = torch.empty(L, D, B, H, dtype=torch.float32, device=dev)
        gates = torch.empty(L, D, B, 4 * H, dtype=torch.float32, device=dev)
        lengths = lengths.to(device=dev, dtype=torch.int64).contiguous()
        rc = _lib.load().t2o_lstm_layer_fwd(_ptr(gi), _ptr(whh_t), _ptr(b_ih), _ptr(b_hh), _ptr(lengths), _ptr(out), _ptr(hnew),
                                            _ptr(cnew), _ptr(gates), B, L, H, D, _stream(dev))
        _lib.check(rc, 't2o_lstm_layer_fwd')
        last = [L - 1, 0]
        h_n = torch.stack([hnew[last[d], d] for d in range(D)], 0)
        c_n = torch.stack([cnew[last[d], d] for d in range(D)], 0)
        ctx.save_for_backward(x, lengths, wih_cat, hnew, cnew, gates, *w_hh)
        ctx.meta = (B, L, E, H, D, has_bias)
        ctx.params = w
        ctx.acc = all(_persistent_grad(p) for p in w)
        return out, h_n, c_n

    @staticmethod
    def backward(ctx, dout, dhn, dcn):
        x, lengths, wih_cat, hnew, cnew, gates = ctx.saved_tensors[:6]
        w_hh = ctx.saved_tensors[6:]
        B, L, E, H, D, has_bias = ctx.meta
        dev = x.device
        whh = torch.stack([t.view(H, 4, H).permute(0, 2, 1) for t in w_hh], 0).contiguous()       # (D, 4H/4, H(k), 4 columns)
        dgates = torch.empty(L, D, B, 4 * H, dtype=torch.float32, device=dev)
        carry = torch.empty(D, B, H, dtype=torch.float32, device=dev)
        dc = torch.empty(D, B, H, dtype=torch.float32, device=dev)
        dout = None if dout is None else dout.contiguous()
        dhn = None if dhn is None else dhn.contiguous()
        dcn = None if dcn is None else dcn.contiguous()
        rc = _lib.load().t2o_lstm_layer_bwd(_ptr(whh), _ptr(lengths), _ptr(cnew), _ptr(gates), _ptr(dout), _ptr(dhn), _ptr(dcn),
                                            _ptr(dgates), _ptr(carry), _ptr(dc), B, L, H, D, _stream(dev))
        _lib.check(rc, 't2o_lstm_layer_bwd')
        dgi = dgates.permute(2, 0, 1, 3).reshape(B * L, D * 4 * H)             # rows (b, t), columns (d, gate): gi's layout
        dx = gemm(dgi, wih_cat, b_kmajor=True).view(B, L, E) if ctx.needs_input_grad[0] else None
        dbias = colsum(dgi) if has_bias else None
        per = 4 if has_bias else 2

        def steps_of(d):
            """(dgates, h_prev) over the steps that have a previous state, as (rows, .) matrices: contiguous per direction"""
            dg = (dgates[1:, d] if d == 0 else dgates[:-1, d]).reshape((L - 1) * B, 4 * H)
            hp = (hnew[:-1, d] if d == 0 else hnew[1:, d]).reshape((L - 1) * B, H)
            return dg, hp
        if ctx.acc and all(_persistent_grad(q) for q in ctx.params):           # parameter gradients added in place by the GEMMs
            p, x2 = ctx.params, x.reshape(B * L, E)
            for d in range(D):
                gemm(dgi[:, d * 4 * H:(d + 1) * 4 * H], x2, out=p[per * d].grad, a_kmajor=True, b_kmajor=True, accumulate=True)
                if L > 1:
                    dg, hp = steps_of(d)
                    gemm(dg, hp, out=p[per * d + 1].grad, a_kmajor=True, b_kmajor=True, accumulate=True)
            if has_bias:
                torch._foreach_add_([p[per * d + k].grad for d in range(D) for k in (2, 3)],
                                    [dbias[d * 4 * H:(d + 1) * 4 * H] for d in range(D) for _ in (2, 3)])
            return (dx, None, None) + (None,) * len(p)
        dwih = gemm(dgi, x.reshape(B * L, E), a_kmajor=True, b_kmajor=True)    # (D*4H, E)
        grads = []
        for d in range(D):
            # dW_hh = sum_t dgates[t]^T h_prev(t): h_prev of time t is the state after t-1 (direction 0) / t+1 (direction 1)
            if L > 1:
                dg, hp = steps_of(d)
                dwhh = gemm(dg, hp, a_kmajor=True, b_kmajor=True)
            else:
                dwhh = torch.zeros_like(w_hh[d])
            grads += [dwih[d * 4 * H:(d + 1) * 4 * H], dwhh]
            if has_bias:
                grads += [dbias[d * 4 * H:(d + 1) * 4 * H], dbias[d * 4 * H:(d + 1) * 4 * H]]
        return (dx, None, None) + tuple(grads)


def lstm_layer(x, lengths, dirs):
    """x (B,L,E) zero-padded rows, lengths (B) on any device, dirs = [(w_ih, w_hh, b_ih, b_hh) or (w_ih, w_hh)] per
    direction (nn.LSTM's parameters of one layer).  Returns (out (B,L,D*H) zero at pads, h_n (D,B,H), c_n (D,B,H))."""
    has_bias = len(dirs[0]) == 4
    flat = [t for d in dirs for t in d]
    return _LstmLayerFn.apply(x, lengths, has_bias, *flat)


# ---- 3x3 convolutions for any image size (t2o_conv_generic.hip): what the LDS-DMA kernels cannot take ------------------
def conv3x3_any_forward(x, weight, stride=1):
    """conv2d(x, weight, None, stride, 1) for any H, W (Ci % 32 == 0, Co % 64 == 0): gathered-row kernel."""
    _need_gpu(x, weight)
    N, Ci, H, W = x.shape
    Co = weight.shape[0]
    x = x.contiguous(memory_format=torch.channels_last)
    weight = weight.contiguous(memory_format=torch.channels_last)
    y = torch.empty((N, Co, (H - 1) // stride + 1, (W - 1) // stride + 1), dtype=torch.float32, device=x.device,
                    memory_format=torch.channels_last)
    rc = _lib.load().t2o_conv3x3_any_fwd_nhwc(_ptr(x), _ptr(weight), _ptr(y), N, H, W, Ci, Co, stride, _stream(x.device))
    _lib.check(rc, 't2o_conv3x3_any_fwd_nhwc')
    return y


def conv3x3_any_dgrad(dy, weight, in_hw, stride=1, addend=None):
    """Data gradient of conv2d(x, weight, None, stride, 1) for an x of spatial size in_hw = (H, W); dy channels-last."""
    _need_gpu(dy, weight, addend)
    N, Co = dy.shape[0], dy.shape[1]
    Ci = weight.shape[1]
    H, W = in_hw
    dy = dy.contiguous(memory_format=torch.channels_last)
    wt = conv_weight_transform(weight, 9, stride == 1)
    addend = None if addend is None else addend.contiguous(memory_format=torch.channels_last)
    dx = torch.empty((N, Ci, H, W), dtype=torch.float32, device=dy.device, memory_format=torch.channels_last)
    rc = _lib.load().t2o_conv3x3_any_dgrad_nhwc(_ptr(dy), _ptr(wt), _ptr(addend), _ptr(dx), N, H, W, Ci, Co, stride, _stream(dy.device))
    _lib.check(rc, 't2o_conv3x3_any_dgrad_nhwc')
    return dx


def conv3x3_any_wgrad(x, dy, stride=1, into=None):
    """Weight gradient (Co,Ci,3,3) channels-last of conv2d(x, w, None, stride, 1) for any image size; into: added to."""
    _need_gpu(x, dy, into)
    N, Ci, H, W = x.shape
    Co = dy.shape[1]
    x = x.contiguous(memory_format=torch.channels_last)
    dy = dy.contiguous(memory_format=torch.channels_last)
    lib = _lib.load()
    need = lib.t2o_conv3x3_any_wgrad_workspace_bytes(N, H, W, Ci, Co, stride)
    if need == 0:
        raise RuntimeError('conv3x3_any_wgrad: unsupported shape (channel counts must be multiples of 64)')
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    dw = into if into is not None else torch.empty((Co, Ci, 3, 3), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    rc = lib.t2o_conv3x3_any_wgrad_nhwc(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), need, N, H, W, Ci, Co, stride, 1 if into is not None else 0,
                                        _stream(x.device))
    _lib.check(rc, 't2o_conv3x3_any_wgrad_nhwc')
    return dw


class _Conv1x1S2Fn(torch.autograd.Function):
    """conv2d(x, w, None, stride 2) for a 1x1 weight: the shortcut branch on this library's kernels (t2o_conv1x1.hip)."""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return conv1x1s2_forward(x, weight)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.zeros_like(x, memory_format=torch.channels_last)
            conv1x1s2_dgrad_acc(dy, weight, dx)
        if ctx.needs_input_grad[1]:
            dw = conv1x1s2_wgrad(x, dy).view_as(weight)
        return dx, dw


def conv1x1s2(x, weight):
    return _Conv1x1S2Fn.apply(x, weight)


def conv1x1s2_supported(x, conv):
    w = conv.weight
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and conv.bias is None and tuple(w.shape[2:]) == (1, 1)
            and tuple(conv.stride) == (2, 2) and tuple(conv.padding) == (0, 0) and w.shape[0] % 64 == 0 and w.shape[1] % 64 == 0
            and x.is_contiguous(memory_format=torch.channels_last))


# ---- dense layers of the decoder with in-place gradient accumulation ----------------------------------------------------
# The decoder's Linear layers and LSTM cells are library GEMMs with M = 64; what this adds is bookkeeping: with persistent
# gradient buffers (the Trainer's flat buffer) the weight gradient is accumulated BY the GEMM that computes it (beta = 1)
# and the bias gradient by one GEMV, so autograd hands out no parameter gradient and launches no accumulation kernel --
# ~120 tiny launches per train step (each costs ~5 us of GPU time, inside a hipGraph as much as outside).
_ACC = {}        # id(parameter) -> (weak reference to it, the .grad tensor registered for it)


def enable_grad_accumulation(params):
    """Opt in (Trainer / FlatGradients): the backward kernels of these parameters ADD into their current, persistent
    .grad tensors and autograd is handed no parameter gradient.  Never inferred from `.grad is not None`: a caller that
    runs forward, `optimizer.zero_grad()` (set_to_none) and then backward must get ordinary autograd gradients."""
    import weakref
    for p in params:
        if p.grad is not None and p.grad.dtype == torch.float32 and p.grad.shape == p.shape and p.grad.stride() == p.stride():
            _ACC[id(p)] = (weakref.ref(p), p.grad)


def disable_grad_accumulation(params=None):
    for key in ([id(p) for p in params] if params is not None else list(_ACC)):
        _ACC.pop(key, None)


def _persistent_grad(p):
    """True while `p` is registered AND still carries the registered gradient tensor (checked again at backward time)."""
    e = _ACC.get(id(p))
    return e is not None and e[0]() is p and p.grad is e[1]

_ones_cache = {}


def _ones(n, device):
    key = (n, device)
    t = _ones_cache.get(key)
    if t is None or torch.cuda.is_current_stream_capturing():
        t = torch.ones(n, dtype=torch.float32, device=device)
        if not torch.cuda.is_current_stream_capturing():
            _ones_cache[key] = t
    return t


class _LinearAccFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.params = (weight, bias)
        ctx.acc = _persistent_grad(weight) and (bias is None or _persistent_grad(bias))
        if not x.is_cuda:                                     # (host tensors: the data-parallel logic's gloo tests)
            return torch.addmm(bias, x, weight.t()) if bias is not None else x @ weight.t()
        x = x.contiguous()
        if bias is None:
            return gemm(x, weight)
        return gemm(x, weight, out=bias.detach().unsqueeze(0).repeat(x.shape[0], 1), accumulate=True)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        weight, bias = ctx.params
        dy = dy.contiguous()
        if not dy.is_cuda:
            dx = dy @ w if ctx.needs_input_grad[0] else None
            if ctx.acc and _persistent_grad(weight) and (bias is None or _persistent_grad(bias)):
                weight.grad.addmm_(dy.t(), x)
                if bias is not None:
                    bias.grad.addmv_(dy.t(), _ones(dy.shape[0], dy.device))
                return dx, None, None
            return dx, dy.t() @ x, (dy.sum(0) if bias is not None else None)
        x = x.contiguous()
        dx = gemm(dy, w, b_kmajor=True) if ctx.needs_input_grad[0] else None
        if ctx.acc and _persistent_grad(weight) and (bias is None or _persistent_grad(bias)):
            gemm(dy, x, out=weight.grad, a_kmajor=True, b_kmajor=True, accumulate=True)
            if bias is not None:
                colsum(dy, out=bias.grad, accumulate=True)
            return dx, None, None
        return dx, gemm(dy, x, a_kmajor=True, b_kmajor=True), (colsum(dy) if bias is not None else None)


def linear_acc(x, weight, bias=None):
    """F.linear(x, weight, bias) for 2-D x; with persistent .grad buffers the backward adds the parameter gradients in place."""
    return _LinearAccFn.apply(x, weight, bias)


class _LstmCellAccFn(torch.autograd.Function):
    """torch.lstm_cell (one step of nn.LSTM, gate order i, f, g, o) as two GEMMs + the framework's fused gate kernel, with the
    parameter gradients accumulated in place by the GEMMs of the backward (persistent .grad buffers)."""

    @staticmethod
    def forward(ctx, x, h, c, w_ih, w_hh, b_ih, b_hh):
        ig, hg = (gemm(x.contiguous(), w_ih), gemm(h.contiguous(), w_hh)) if x.is_cuda else (x @ w_ih.t(), h @ w_hh.t())
        hy, cy, ws = torch.ops.aten._thnn_fused_lstm_cell(ig, hg, c, b_ih, b_hh)
        ctx.save_for_backward(x, h, c, cy, ws, w_ih, w_hh)
        ctx.params = (w_ih, w_hh, b_ih, b_hh)
        ctx.acc = all(_persistent_grad(p) for p in ctx.params if p is not None)
        return hy, cy

    @staticmethod
    def backward(ctx, ghy, gcy):
        x, h, c, cy, ws, w_ih, w_hh = ctx.saved_tensors
        p_ih, p_hh, b_ih, b_hh = ctx.params
        has_bias = b_ih is not None
        gg, gcx, gb = torch.ops.aten._thnn_fused_lstm_cell_backward_impl(ghy, gcy, c, cy, ws, has_bias)
        own = gg.is_cuda
        if own:
            gg, x, h = gg.contiguous(), x.contiguous(), h.contiguous()
        dx = (gemm(gg, w_ih, b_kmajor=True) if own else gg @ w_ih) if ctx.needs_input_grad[0] else None
        dh = (gemm(gg, w_hh, b_kmajor=True) if own else gg @ w_hh) if ctx.needs_input_grad[1] else None
        if ctx.acc and all(_persistent_grad(p) for p in ctx.params if p is not None):
            if own:
                gemm(gg, x, out=p_ih.grad, a_kmajor=True, b_kmajor=True, accumulate=True)
                gemm(gg, h, out=p_hh.grad, a_kmajor=True, b_kmajor=True, accumulate=True)
            else:
                p_ih.grad.addmm_(gg.t(), x)
                p_hh.grad.addmm_(gg.t(), h)
            if has_bias:
                torch._foreach_add_([b_ih.grad, b_hh.grad], [gb, gb])
            return dx, dh, gcx, None, None, None, None
        if own:
            return dx, dh, gcx, gemm(gg, x, a_kmajor=True, b_kmajor=True), gemm(gg, h, a_kmajor=True, b_kmajor=True), (gb if has_bias else None), (gb if has_bias else None)
        return dx, dh, gcx, gg.t() @ x, gg.t() @ h, (gb if has_bias else None), (gb if has_bias else None)


def lstm_cell_acc(x, h, c, w_ih, w_hh, b_ih=None, b_hh=None):
    return _LstmCellAccFn.apply(x, h, c, w_ih, w_hh, b_ih, b_hh)


# ---- Winograd F(2x2,3x3) for the stride-1 3x3 convolutions of the deep stages (t2o_winograd.hip) -----------------------
def wino_weight(w_taps_last, Cn, Ck):
    """(Cn,3,3,Ck) filter bank (channels-last conv weight, or the mirrored transpose from conv_weight_transform) -> U (16,Cn,Ck)."""
    U = torch.empty((16, Cn, Ck), dtype=torch.float32, device=w_taps_last.device)
    _lib.check(_lib.load().t2o_wino_weight_transform(_ptr(w_taps_last), _ptr(U), Cn, Ck, _stream(U.device)), 't2o_wino_weight_transform')
    return U


def gemm_nt_batched(A, B, M=None):
    """C[b] (M,N) = A[b][:M] @ B[b]^T for dense fp32 A (batches, rows >= M, K), B (batches, N, K): this library's matrix-core
    kernel (t2o_gemm_nt_batched; N % 64 == 0, K % 32 == 0)."""
    batches, rows, K = A.shape
    M = rows if M is None else M
    if A.stride(2) != 1 or A.stride(1) != K or A.stride(0) % K:
        raise ValueError('gemm_nt_batched: A must have dense rows (a row range of a larger (batches, R, K) tensor is fine)')
    rows = A.stride(0) // K                                # rows per plane of the tensor A lives in
    N = B.shape[1]
    C = torch.empty((batches, M, N), dtype=torch.float32, device=A.device)
    _lib.check(_lib.load().t2o_gemm_nt_batched(_ptr(A), _ptr(B), _ptr(C), batches, M, N, K, rows, _stream(A.device)), 't2o_gemm_nt_batched')
    return C


def _plane_rows(t, what):
    """Rows per plane of the (batches, R, width) tensor a row-range view t (batches, rows, width) lives in."""
    width = t.shape[2]
    if t.stride(2) != 1 or t.stride(1) != width or t.stride(0) % width or t.stride(0) < t.shape[1] * width:
        raise ValueError('%s must have dense rows (a row range of a larger (batches, R, width) tensor is fine)' % what)
    return t.stride(0) // width


def gemm_tn_batched(A, B):
    """(splits, batches, M, N) pieces of C[b] = A[b]^T @ B[b] for A (batches, rows, M), B (batches, rows, N) (rows % 256 == 0,
    M, N % 128 == 0: t2o_gemm_tn_batched); the caller adds the pieces in order (t2o_wino_dw_transform does).  A and B may be
    row ranges of larger tensors (the first passes of encoder.WgradArena's arenas)."""
    batches, rows, M = A.shape
    N = B.shape[2]
    lib = _lib.load()
    ldA, ldB = _plane_rows(A, 'gemm_tn_batched: A'), _plane_rows(B, 'gemm_tn_batched: B')
    splits = lib.t2o_gemm_tn_splits(batches, rows, M, N)
    if splits <= 0:
        raise RuntimeError('gemm_tn_batched: M, N must be multiples of 128 and the row count of 256 (got %d x %d over %d rows)' % (M, N, rows))
    C = torch.empty((splits, batches, M, N), dtype=torch.float32, device=A.device)
    _lib.check(lib.t2o_gemm_tn_batched_ld(_ptr(A), _ptr(B), _ptr(C), batches, rows, ldA, ldB, M, N, splits, _stream(A.device)),
               't2o_gemm_tn_batched_ld')
    return C


def wino_input(x, N, H, W, out=None):
    """x (N,H,W,C) -> V (16, Tpad, C): the transformed 4x4 input patches of the T = N*H/2*W/2 output tiles, zero rows up to
    Tpad = t2o_wino_padded_tiles (a multiple of 256).  out: a (16, Tpad, C) row range of a larger (16, R, C) tensor to write
    into (encoder.WgradArena: the passes of a train step side by side)."""
    lib = _lib.load()
    C = x.shape[-1]
    if out is None:
        V = torch.empty((16, lib.t2o_wino_padded_tiles(N, H, W), C), dtype=torch.float32, device=x.device)
        _lib.check(lib.t2o_wino_input_transform(_ptr(x), _ptr(V), N, H, W, C, _stream(x.device)), 't2o_wino_input_transform')
        return V
    _lib.check(lib.t2o_wino_input_transform_ld(_ptr(x), _ptr(out), N, H, W, C, out.stride(0) // C, _stream(x.device)), 't2o_wino_input_transform_ld')
    return out


def wino_wgrad_nhwc(V, dy, dw, N, H, W, accumulate):
    """dw (Co,3,3,Ci) (+)= weight gradient of the convolution whose transformed input is V (16,Tpad,Ci), for dy (N,H,W,Co)."""
    lib = _lib.load()
    st = _stream(dy.device)
    Co, Ci = dy.shape[-1], V.shape[2]
    Ad = torch.empty((16, V.shape[1], Co), dtype=torch.float32, device=dy.device)
    _lib.check(lib.t2o_wino_dy_transform(_ptr(dy), _ptr(Ad), N, H, W, Co, st), 't2o_wino_dy_transform')
    dU = gemm_tn_batched(Ad, V.contiguous())              # 16 GEMMs over the tiles (Co x T) x (T x Ci), in `splits` pieces
    _lib.check(lib.t2o_wino_dw_transform(_ptr(dU), _ptr(dw), Co, Ci, dU.shape[0], 1 if accumulate else 0, st), 't2o_wino_dw_transform')


def wino_backward_nhwc(dy, Vx, Ud, dw, dx, N, H, W, addend, accumulate, ad_out=None, uc=None):
    """Both gradients of a Winograd layer from one pass over dy (N,H,W,Co): dx (N,H,W,Ci) = data gradient (+ addend) with
    Ud (16,Ci,Co) the transformed mirrored filter, dw (Co,3,3,Ci) (+)= weight gradient with Vx (16,Tpad,Ci) the forward's
    transformed input.  ad_out: a (16, Tpad, Co) row range of a larger tensor that receives A dY A^T instead -- the weight
    gradient is then NOT formed here (encoder.WgradArena forms it once over all passes of the train step)."""
    lib = _lib.load()
    dev = dy.device
    st = _stream(dev)
    Co, Ci = dy.shape[-1], Vx.shape[2]
    Tpad = Vx.shape[1]
    if uc is not None and lib.t2o_wino_fused_supported(N, H, W, Co, Ci):
        # uc = the mirrored filter in the on-chip kernel's layout: the data gradient in ONE launch; only A dY A^T (the weight
        # gradient's operand) is still formed by a transform pass
        Ad = ad_out if ad_out is not None else torch.empty((16, Tpad, Co), dtype=torch.float32, device=dev)
        _lib.check(lib.t2o_wino_dy_transform_ld(_ptr(dy), _ptr(Ad), N, H, W, Co, Ad.stride(0) // Co, st), 't2o_wino_dy_transform_ld')
        wino_fused_conv_nhwc(dy, uc, N, H, W, addend, False, out=dx)
        if ad_out is None and not wino_dw_from(Ad, Vx.contiguous(), dw, accumulate):
            raise RuntimeError('wino_backward_nhwc: no split for %d tile rows' % Tpad)
        return
    Vd = torch.empty((16, Tpad, Co), dtype=torch.float32, device=dev)
    if ad_out is None:
        Ad = torch.empty((16, Tpad, Co), dtype=torch.float32, device=dev)
        _lib.check(lib.t2o_wino_dy_transforms(_ptr(dy), _ptr(Vd), _ptr(Ad), N, H, W, Co, st), 't2o_wino_dy_transforms')
    else:
        _lib.check(lib.t2o_wino_dy_transforms_ld(_ptr(dy), _ptr(Vd), _ptr(ad_out), N, H, W, Co, ad_out.stride(0) // Co, st), 't2o_wino_dy_transforms_ld')
    M = gemm_nt_batched(Vd, Ud, N * (H // 2) * (W // 2))
    _lib.check(lib.t2o_wino_output_transform(_ptr(M), _ptr(addend), _ptr(dx), None, N, H, W, Ci, st), 't2o_wino_output_transform')
    if ad_out is None:
        if not wino_dw_from(Ad, Vx.contiguous(), dw, accumulate):       # (.contiguous(): Vx may be a row range of an arena)
            raise RuntimeError('wino_backward_nhwc: no split for %d tile rows' % Tpad)


def wino_dw_from(Ad, V, dw, accumulate):
    """dw (Co,3,3,Ci) (+)= G^T [sum over the tile rows of Ad (16,R,Co)^T V (16,R,Ci)] G; False when the row count has no valid
    split (the caller then goes piece by piece)."""
    lib = _lib.load()
    Co, Ci = Ad.shape[2], V.shape[2]
    if lib.t2o_gemm_tn_splits(16, Ad.shape[1], Co, Ci) <= 0:
        return False
    dU = gemm_tn_batched(Ad, V)
    _lib.check(lib.t2o_wino_dw_transform(_ptr(dU), _ptr(dw), Co, Ci, dU.shape[0], 1 if accumulate else 0, _stream(dw.device)), 't2o_wino_dw_transform')
    return True


def wino_conv_nhwc(x, U, N, H, W, addend=None, want_stats=False, out=None, keep_v=None, v_out=None, uc=None):
    """x (N,H,W,Ci) NHWC buffer, U (16,Co,Ci) -> y (N,H,W,Co) (+ addend) [, stats rows for the batch norm that follows].
    keep_v: a list that receives V (the weight gradient reuses it: wino_wgrad_nhwc); v_out: where V is to be written
    (wino_input's `out`)."""
    lib = _lib.load()
    dev = x.device
    st = _stream(dev)
    Co = U.shape[1]
    if uc is not None and lib.t2o_wino_fused_supported(N, H, W, x.shape[-1], Co):
        # uc = U in the on-chip kernel's layout: the convolution in ONE launch; V is formed only when the weight gradient
        # will want it (keep_v / v_out)
        if keep_v is not None or v_out is not None:
            V = wino_input(x, N, H, W, v_out)
            if keep_v is not None:
                keep_v.append(V)
        return wino_fused_conv_nhwc(x, uc, N, H, W, addend, want_stats, out=out)
    V = wino_input(x, N, H, W, v_out)
    if keep_v is not None:
        keep_v.append(V)
    M = gemm_nt_batched(V, U, N * (H // 2) * (W // 2))    # 16 GEMMs (T x Ci) x (Ci x Co)
    y = out if out is not None else torch.empty((N, H, W, Co), dtype=torch.float32, device=dev)
    stats = torch.empty((lib.t2o_wino_stats_rows(N, H, W, Co), 2, Co), dtype=torch.float32, device=dev) if want_stats else None
    _lib.check(lib.t2o_wino_output_transform(_ptr(M), _ptr(addend), _ptr(y), _ptr(stats), N, H, W, Co, st), 't2o_wino_output_transform')
    return y, stats


def wino_u_chunked(U):
    """U (16,Cn,Ck) -> the chunk-major layout (Ck/8, 16, Cn, 8) the on-chip Winograd kernel streams (t2o_wino_u_chunked)."""
    _, Cn, Ck = U.shape
    Uc = torch.empty((Ck // 8, 16, Cn, 8), dtype=torch.float32, device=U.device)
    _lib.check(_lib.load().t2o_wino_u_chunked(_ptr(U), _ptr(Uc), Cn, Ck, _stream(U.device)), 't2o_wino_u_chunked')
    return Uc


def wino_fused_conv_nhwc(x, Uc, N, H, W, addend=None, want_stats=False, out=None):
    """x (N,H,W,Ci) NHWC buffer, Uc = wino_u_chunked(U) -> y (N,H,W,Co) (+ addend) [, stats rows]: Winograd F(2x2,3x3) in ONE
    launch, V and M never leave the chip (t2o_wino_fused_conv_nhwc; H, W multiples of 16, Co of 64)."""
    lib = _lib.load()
    dev = x.device
    Ci, Co = Uc.shape[0] * 8, Uc.shape[2]
    if not (x.is_contiguous() and x.numel() == N * H * W * Ci and Uc.is_contiguous()):
        raise ValueError('wino_fused_conv_nhwc: x must be a dense (N,H,W,%d) buffer and Uc dense' % Ci)
    if addend is not None and not (addend.is_contiguous() and addend.numel() == N * H * W * Co):
        raise ValueError('wino_fused_conv_nhwc: addend must be a dense (N,H,W,%d) buffer' % Co)
    if out is not None and not (out.is_contiguous() and out.numel() == N * H * W * Co):
        raise ValueError('wino_fused_conv_nhwc: out must be a dense (N,H,W,%d) buffer' % Co)
    y = out if out is not None else torch.empty((N, H, W, Co), dtype=torch.float32, device=dev)
    stats = torch.empty((lib.t2o_wino_fused_stats_rows(N, H, W), 2, Co), dtype=torch.float32, device=dev) if want_stats else None
    zeros = _zero_block(dev)
    _lib.check(lib.t2o_wino_fused_conv_nhwc(_ptr(x), _ptr(Uc), _ptr(addend), _ptr(y), _ptr(stats), _ptr(zeros), N, H, W, Ci, Co, _stream(dev)),
               't2o_wino_fused_conv_nhwc')
    return y, stats


def wino_fused_wgrad_nhwc(x, dy, dw, n_img, H, W, accumulate):
    """dw (Co,3,3,Ci) (+)= weight gradient of the stride-1 3x3 convolution for x (n_img,H,W,Ci), dy (n_img,H,W,Co) NHWC buffers, in
    the Winograd domain with both transforms on chip (t2o_wino_fused_wgrad_nhwc).  False when the shape is not taken (H, W
    multiples of 16, channel counts multiples of 64 up to 512)."""
    lib = _lib.load()
    dev = x.device
    Ci, Co = x.shape[-1], dy.shape[-1]
    if not lib.t2o_wino_fused_wgrad_supported(n_img, H, W, Ci, Co):
        return False
    if not (x.is_contiguous() and x.numel() == n_img * H * W * Ci and dy.is_contiguous() and dy.numel() == n_img * H * W * Co):
        raise ValueError('wino_fused_wgrad_nhwc: x and dy must be dense (n_img,H,W,C) buffers')
    if not (dw.numel() == Co * 9 * Ci and (dw.is_contiguous() or (dw.dim() == 4 and dw.is_contiguous(memory_format=torch.channels_last)))):
        raise ValueError('wino_fused_wgrad_nhwc: dw must be a dense (Co,3,3,Ci) buffer (a channels-last convolution weight)')
    need = lib.t2o_wino_fused_wgrad_workspace_bytes(n_img, H, W, Ci, Co)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = lib.t2o_wino_fused_wgrad_nhwc(_ptr(x), _ptr(dy), _ptr(dw), _ptr(_zero_block(dev)), _ptr(ws), need, n_img, H, W, Ci, Co,
                                       1 if accumulate else 0, _stream(dev))
    _lib.check(rc, 't2o_wino_fused_wgrad_nhwc')
    return True


def conv3x3_winograd(x, weight, addend=None):
    """conv2d(x, weight, None, 1, 1) (+ addend) through the Winograd pipeline; x (N,Ci,H,W) any layout, returns channels_last."""
    _need_gpu(x, weight)
    N, Ci, H, W = x.shape
    Co = weight.shape[0]
    xh = x.permute(0, 2, 3, 1).contiguous()
    U = wino_weight(weight.permute(0, 2, 3, 1).contiguous(), Co, Ci)
    ad = None if addend is None else addend.permute(0, 2, 3, 1).contiguous()
    y, _ = wino_conv_nhwc(xh, U, N, H, W, ad)
    return y.permute(0, 3, 1, 2)


# ---- image I/O (t2o_image_io.hip): the data step's resize + layout conversion, and its inverse for writing images ----

IMAGE_DESC = np.dtype([('offset', '<i8'), ('h', '<i4'), ('w', '<i4')])       # t2o_image_desc_t, field for field


def _u8_hwc(img):
    a = img.numpy() if torch.is_tensor(img) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('image must be uint8 (H,W,3), got %s %s' % (a.dtype, a.shape))
    return np.ascontiguousarray(a)


def pack_u8(images, pads=None, pin=None):
    """Pack uint8 (H,W,3) images (arrays or CPU tensors; None = an absent image, a zero output) back to back into ONE
    byte buffer headed by their descriptor table.  Returns (buffer, descs): a 1-D uint8 CPU tensor -- pinned when `pin`
    (default: when a GPU is there; pass False inside DataLoader workers) -- and a numpy view of its first 16 n bytes as
    IMAGE_DESC records, offsets counted from the buffer's first byte.  pads[i] unused bytes go in front of image i."""
    n = len(images)
    if n == 0:
        raise ValueError('pack_u8: no images')
    arrays = [None if im is None else _u8_hwc(im) for im in images]
    pads = [0] * n if pads is None else [int(p) for p in pads]
    pos, offsets = IMAGE_DESC.itemsize * n, []
    for a, pad in zip(arrays, pads):
        pos += pad
        offsets.append(pos)
        pos += 0 if a is None else a.size
    buffer = torch.empty(pos, dtype=torch.uint8, pin_memory=torch.cuda.is_available() if pin is None else bool(pin))
    flat = buffer.numpy()
    descs = flat[:IMAGE_DESC.itemsize * n].view(IMAGE_DESC)
    end = IMAGE_DESC.itemsize * n
    for i, (a, off) in enumerate(zip(arrays, offsets)):
        flat[end:off] = 0
        descs[i] = (off, 0, 0) if a is None else (off, a.shape[0], a.shape[1])
        if a is not None:
            flat[off:off + a.size] = a.reshape(-1)
            end = off + a.size
    return buffer, descs


def image_descs(descs, nbytes):
    """`descs` (IMAGE_DESC records, or their (n,4) int32 form, array or tensor) as a checked IMAGE_DESC array: every
    image must lie inside a buffer of `nbytes` bytes -- the kernel reads where the table points."""
    d = descs.numpy() if torch.is_tensor(descs) else np.asarray(descs)
    if d.dtype != IMAGE_DESC:
        if d.dtype != np.int32 or d.ndim != 2 or d.shape[1] != 4:
            raise ValueError('descriptors: IMAGE_DESC records or an (n,4) int32 array')
        d = np.ascontiguousarray(d).view(IMAGE_DESC)
    d = np.ascontiguousarray(d.reshape(-1))
    if d.size == 0:
        raise ValueError('descriptors: empty table')
    off, h, w = d['offset'], d['h'].astype(np.int64), d['w'].astype(np.int64)
    absent = (h == 0) & (w == 0)
    ok = absent | ((h > 0) & (w > 0) & (off >= 0) & (off + 3 * h * w <= nbytes))
    if not ok.all():
        raise ValueError('descriptor %d points outside the %d-byte buffer or has a bad size' % (int(np.argmin(ok)), nbytes))
    return d


def _resize_launch(dev_buffer, table_ptr, n, h, w, out=None):
    """One t2o_resize_u8_to_f32 launch on the current stream: images in `dev_buffer`, n descriptors at device address table_ptr."""
    dev = dev_buffer.device
    if out is None:
        out = torch.empty(n, 3, h, w, dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, 3, h, w)):
        raise ValueError('out must be a contiguous fp32 GPU tensor of shape %s' % ((n, 3, h, w),))
    rc = _lib.load().t2o_resize_u8_to_f32(_ptr(dev_buffer), table_ptr, n, h, w, _ptr(out), _stream(dev))
    _lib.check(rc, 't2o_resize_u8_to_f32')
    return out


def upload_packed(buffer, descs, device=None):
    """The packed buffer on the device (ONE host-to-device copy; none if it is there already) and the device address of
    its descriptor table: the buffer's head when pack_u8 laid it out, else a second, small upload of `descs`.
    Returns (device buffer, table address, checked descriptors, keep-alive)."""
    buffer = torch.from_numpy(buffer) if isinstance(buffer, np.ndarray) else buffer
    if buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous():
        raise ValueError('packed buffer must be a contiguous 1-D uint8 tensor')
    descs = image_descs(descs, buffer.numel())
    head = IMAGE_DESC.itemsize * descs.size
    if device is None:
        device = buffer.device if buffer.is_cuda else torch.device('cuda', torch.cuda.current_device())
    in_head = (not buffer.is_cuda and buffer.numel() >= head
               and np.array_equal(buffer[:head].numpy().view(IMAGE_DESC), descs))
    dev_buffer = buffer if buffer.is_cuda else buffer.to(device, non_blocking=True)
    if in_head and dev_buffer.data_ptr() % 8 == 0:
        return dev_buffer, dev_buffer.data_ptr(), descs, None
    table = torch.from_numpy(descs.view(np.uint8)).to(dev_buffer.device, non_blocking=True)
    return dev_buffer, table.data_ptr(), descs, table


def resize_u8(images, size, device=None, out=None):
    """The loaders' cv2.resize + transpose + / 255 (utils/visual_utils.py:6-31) for a batch of decoded images on the GPU:
    (n,3,h,w) fp32 in [0,1], bit for bit data.resize_linear_u8(img, h, w).astype(float32).transpose(2,0,1) / 255.
    images: a list of uint8 (H,W,3) arrays / CPU tensors of any sizes (None = absent: zeros), or an already packed
    (buffer, descs) pair (pack_u8, data.collate_raw); size: int or (h, w).  One pinned buffer, one upload, one launch on
    the current stream; nothing waits on the host."""
    h, w = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if h <= 0 or w <= 0:
        raise ValueError('resize_u8: size must be positive')
    packed = isinstance(images, tuple) and len(images) == 2 and getattr(images[0], 'ndim', 0) == 1
    buffer, descs = images if packed else pack_u8(images)
    dev_buffer, table_ptr, descs, keep = upload_packed(buffer, descs, device)
    return _resize_launch(dev_buffer, table_ptr, int(descs.size), h, w, out)


def to_u8_hwc(t, out=None):
    """(N,3,H,W) or (3,H,W) fp32 GPU tensor in [0,1] -> (N,H,W,3) uint8 GPU tensor = (t * 255) truncated, the rounding of
    utils/visual_utils.py:50-58; equals (t * 255).permute(0,2,3,1).cpu().numpy().astype(uint8).  out: optional contiguous
    uint8 GPU tensor of N H W 3 elements (any alignment)."""
    _need_gpu(t)
    t = t.detach()
    t = t.reshape(-1, 3, *t.shape[-2:]) if t.dim() in (3, 4) and t.shape[-3] == 3 else None
    if t is None:
        raise ValueError('to_u8_hwc: expected (N,3,H,W) or (3,H,W)')
    t = t.contiguous()
    N, _, H, W = t.shape
    if out is None:
        out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=t.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == N * H * W * 3):
        raise ValueError('out must be a contiguous uint8 GPU tensor of %d elements' % (N * H * W * 3))
    rc = _lib.load().t2o_f32_to_u8_hwc(_ptr(t), N, H, W, _ptr(out), _stream(t.device))
    _lib.check(rc, 't2o_f32_to_u8_hwc')
    return out.view(N, H, W, 3)


# ---- resident set (t2o_resident.hip): a batch gathered out of a device-resident store of resized 8-bit pictures ----

GATHER_MAX_K = 8


def _need_gpu_as(t, dtype, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise RuntimeError('t2onet_amd: %s must be a contiguous %s tensor on the GPU (got %s on %s); there is no CPU '
                           'implementation' % (what, dtype, getattr(t, 'dtype', type(t)), getattr(t, 'device', 'the host')))


def _gather(who, max_k, items, store, slots, index, size, rows, out):
    """The one implementation behind gather_u8 and gather_items_u8 (`who`; items: the entry point takes rows, and the
    messages say so): the tensors, the size, K against max_k, one device, `out` allocated or held against the shapes, then
    the launch of t2o_<who>_to_f32.  Returns (img_x, img_ys) or, with rows, (img_x, img_ys, out_rows)."""
    _need_gpu_as(store, torch.uint8, 'store')
    _need_gpu_as(slots, torch.int64, 'slots')
    _need_gpu_as(index, torch.int64, 'index')
    if rows is not None:
        _need_gpu_as(rows, torch.int32, 'rows')
    h, w = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if store.dim() != 1 or slots.dim() != 2 or index.dim() != 1 or index.numel() == 0 or h <= 0 or w <= 0:
        raise ValueError('%s: store (bytes,), slots (N,K), index (B,) with B > 0, positive size' % who)
    N, K = slots.shape
    if not 1 <= K <= max_k or N == 0:
        raise ValueError('%s: slots must be (N,K) with N > 0 and 1 <= K <= %d' % (who, max_k))
    B, dev = index.numel(), store.device
    if rows is not None and (rows.dim() != 2 or rows.shape[0] != N or rows.shape[1] == 0):
        raise ValueError('%s: rows must be (N,V) with the N of slots and V > 0' % who)
    V = 0 if rows is None else rows.shape[1]
    if slots.device != dev or index.device != dev or (rows is not None and rows.device != dev):
        raise ValueError('%s: store, slots%s must lie on one device' % (who, ', index and rows' if items else ' and index'))
    shapes = [(B, 3, h, w), (B, K - 1, 3, h, w)] + ([(B, V)] if V else [])
    dtypes = [torch.float32, torch.float32, torch.int32]
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in zip(shapes, dtypes))
    else:
        out = tuple(out)
        if len(out) != len(shapes) or not all(torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == d and t.is_contiguous()
                                              and tuple(t.shape) == s for t, s, d in zip(out, shapes, dtypes)):
            raise ValueError('%s: out must be contiguous %s' % (who, 'GPU tensors of shapes %s (fp32, fp32, int32)' % (shapes,) if items
                                                                 else 'fp32 tensors of shapes %s and %s' % tuple(shapes)))
    entry = 't2o_%s_to_f32' % who
    rc = getattr(_lib.load(), entry)(_ptr(store), _ptr(slots), _ptr(index), N, K, B, h, w, _ptr(out[0]), _ptr(out[1]) if K > 1 else None,
                                     *((_ptr(rows), V, _ptr(out[2]) if V else None) if items else ()), _stream(dev))
    _lib.check(rc, entry)
    return out


def gather_u8(store, slots, index, size, out=None):
    """The pictures of the items `index` names out of a resident store, as the loaders' fp32 tensors: (img_x (B,3,h,w),
    img_ys (B,K-1,3,h,w)), each picture .astype(float32).transpose(2,0,1) / 255, an absent one zeros.
    store: 1-D uint8 GPU tensor; slots: (N,K) int64 GPU tensor, the byte offset of picture (i, k) in the store -- a
    multiple of 16 -- or -1; index: (B,) int64 GPU tensor, read on the device (values in [0, N): the caller's promise,
    nothing reads them back); size: int or (h, w), the pictures' size.  out: an (img_x, img_ys) pair to write into -- a
    captured launch keeps serving new batches through the same three tensors.  One launch on the current stream."""
    if out is not None:
        img_x, img_ys = out
        _need_gpu(img_x, img_ys)
    return _gather('gather_u8', GATHER_MAX_K, False, store, slots, index, size, None, out)


GATHER_ITEMS_MAX_K = 16


def gather_items_u8(store, slots, index, size, rows=None, out=None):
    """gather_u8 for items of up to 16 pictures whose slots may be shared between items (t2o_gather_items_u8_to_f32; for
    K <= 8 the same bits as gather_u8), and with `rows` -- an (N,V) int32 GPU table -- also out_rows (B,V) int32 =
    rows[index], written by the SAME launch (an index outside [0, N) gives a row of -1).  Returns (img_x, img_ys) or
    (img_x, img_ys, out_rows).  out: the tensors to write into, a pair or, with rows, a triple."""
    return _gather('gather_items_u8', GATHER_ITEMS_MAX_K, True, store, slots, index, size, rows, out)


# ---- 8-bit replay (t2o_replay.hip): a known operator list on uint8 pictures at their native size ----

REPLAY_MAX_JOBS, REPLAY_MAX_STEPS = 64, 8


class ReplayJob(ctypes.Structure):
    """t2o_replay_job_t of include/t2onet_hip.h (field for field)."""
    _fields_ = [('src_offset', ctypes.c_longlong), ('out_offset', ctypes.c_longlong), ('h', ctypes.c_int), ('w', ctypes.c_int),
                ('steps', ctypes.c_int), ('ops', ctypes.c_int * REPLAY_MAX_STEPS)]


def replay_jobs(jobs):
    """jobs: a sequence of (src_offset, out_offset, h, w, ops) with ops a list of executor indices (-1 = identity) ->
    the ctypes array t2o_replay_u8 takes.  `steps` is len(ops) even beyond 8, so that the library is the one to refuse it."""
    arr = (ReplayJob * len(jobs))()
    for c, (src_offset, out_offset, h, w, ops) in zip(arr, jobs):
        c.src_offset, c.out_offset, c.h, c.w, c.steps = int(src_offset), int(out_offset), int(h), int(w), len(ops)
        for k, op in enumerate(list(ops)[:REPLAY_MAX_STEPS]):
            c.ops[k] = int(op)
    return arr


def replay_status(rc, what='t2o_replay_u8'):
    """The library's status as an exception carrying its text: invalid argument -> ValueError, unsupported operator list ->
    NotImplementedError, anything else -> RuntimeError."""
    if rc == 0:
        return
    msg = '%s failed (status %d): %s' % (what, rc, _lib.load().t2o_last_error().decode('utf-8', 'replace'))
    raise {1: ValueError, 2: NotImplementedError}.get(rc, RuntimeError)(msg)


REPLAY_MAX_MASKS, REPLAY_SHARPNESS = 4, 6             # (the executor index of the sharpness, data.ACTIONS)


def replay_mask_table(jobs):
    """The (J, 8) per-step mask indices of `jobs` (6-tuples, see replay_u8_masked) as the ctypes int array
    t2o_replay_u8_masked takes: -1 where a job's mask_of is shorter than 8."""
    arr = (ctypes.c_int * (REPLAY_MAX_STEPS * len(jobs)))(*([-1] * (REPLAY_MAX_STEPS * len(jobs))))
    for j, job in enumerate(jobs):
        for k, i in enumerate(list(job[5])[:REPLAY_MAX_STEPS]):
            arr[REPLAY_MAX_STEPS * j + k] = int(i)
    return arr


def _replay(who, masked, src_u8, jobs, params, masks_u8=None, mask_offsets=(), out=None, five_ok=False):
    """replay_u8, replay_u8_masked and replay_u8_stencils: who = the C entry point without its t2o_; masked: jobs carry mask_of
    and the entry point takes masks; five_ok: a 5-tuple job names no mask.  Checked here, so that a wrong offset or size is a
    Python error and never a GPU fault: the source, every job against source and output, `out` (allocated to fit when None),
    params, and with masks their number, their buffer, each mask_of against its list and each named mask against the buffer."""
    if not (torch.is_tensor(src_u8) and src_u8.is_cuda and src_u8.dtype == torch.uint8 and src_u8.is_contiguous()):
        raise ValueError('%s: src must be a contiguous uint8 GPU tensor' % who)
    jobs = [tuple(j) for j in jobs]
    for j, (so, _, h, w) in enumerate(job[:4] for job in jobs):
        if h > 0 and w > 0 and not (0 <= so and so + 3 * h * w <= src_u8.numel()):
            raise ValueError('%s: job %d reads outside the %d-byte source' % (who, j, src_u8.numel()))
    need = max([job[1] + 3 * job[2] * job[3] for job in jobs if job[2] > 0 and job[3] > 0] or [1])
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=src_u8.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.device == src_u8.device):
        raise ValueError('%s: out must be a contiguous uint8 GPU tensor on the source\'s device' % who)
    elif out.numel() < need or any(job[1] < 0 for job in jobs):
        raise ValueError('%s: a job writes outside the %d-byte output' % (who, out.numel()))
    if params is not None:
        _need_gpu(params)
        params = params.contiguous()
        if tuple(params.shape) != (len(jobs), REPLAY_MAX_STEPS, PARAM_PAD):
            raise ValueError('%s: params must be (J, 8, 24), got %s' % (who, tuple(params.shape)))
    if not masked:
        tables = (replay_jobs(jobs), len(jobs), _ptr(params))
    else:
        if five_ok:
            for j, job in enumerate(jobs):
                if len(job) not in (5, 6):
                    raise ValueError('%s: job %d has %d fields, 5 or 6 are taken' % (who, j, len(job)))
            jobs = [job if len(job) == 6 else job + ([-1] * len(job[4]),) for job in jobs]
        mask_offsets = [int(o) for o in mask_offsets]
        if len(mask_offsets) > REPLAY_MAX_MASKS:
            raise ValueError('%s: at most 4 masks per launch, got %d' % (who, len(mask_offsets)))
        if mask_offsets and not (torch.is_tensor(masks_u8) and masks_u8.is_cuda and masks_u8.dtype == torch.uint8
                                 and masks_u8.is_contiguous() and masks_u8.device == src_u8.device):
            raise ValueError('%s: masks must be a contiguous uint8 GPU tensor on the source\'s device' % who)
        for j, (_, _, h, w, ops, mask_of) in enumerate(jobs):
            if len(mask_of) > len(ops):
                raise ValueError('%s: job %d names %d masks for %d steps' % (who, j, len(mask_of), len(ops)))
            for i in mask_of if h > 0 and w > 0 else ():             # (an empty picture: the library refuses it)
                if 0 <= i < len(mask_offsets) and not (0 <= mask_offsets[i] and mask_offsets[i] + h * w <= masks_u8.numel()):
                    raise ValueError('%s: job %d reads mask %d outside the %d-byte mask buffer' % (who, j, i, masks_u8.numel()))
        offs = (ctypes.c_longlong * max(len(mask_offsets), 1))(*mask_offsets)
        tables = (replay_jobs([j[:5] for j in jobs]), replay_mask_table(jobs), len(jobs), _ptr(params),
                  _ptr(masks_u8) if mask_offsets else None, offs, len(mask_offsets))
    rc = getattr(_lib.load(), 't2o_' + who)(_ptr(src_u8), _ptr(out), *tables, _stream(src_u8.device))
    replay_status(rc, 't2o_' + who)
    return out


def replay_u8(src_u8, jobs, params, out=None):
    """Apply known (operator, parameter) lists to uint8 (h,w,3) RGB pictures at their native size, bytes in and bytes out,
    in ONE launch (t2o_replay_u8): job j = (src_offset, out_offset, h, w, ops) reads its picture at byte src_offset of the
    1-D uint8 GPU tensor src_u8 (any alignment; jobs may share a source), applies ops[k] with params[j, k] ((J,8,24) fp32
    GPU; None when no job applies an operator) as Operator.execute does with specified_param, and writes at byte out_offset of
    `out` (allocated to fit when None).  The bytes equal resize_u8 at the picture's size -> operator_apply per step ->
    to_u8_hwc.  Returns out (1-D uint8)."""
    return _replay('replay_u8', False, src_u8, jobs, params, out=out)


def replay_u8_masked(src_u8, jobs, params, masks_u8, mask_offsets, out=None):
    """replay_u8 with Operator.execute's mask operand -- a LOCAL edit at native size, ONE launch (t2o_replay_u8_masked):
    job j = (src_offset, out_offset, h, w, ops, mask_of), mask_of[k] being an index into mask_offsets or -1; mask i is an
    (h, w) uint8 plane of the job's own size at byte mask_offsets[i] of the 1-D uint8 GPU tensor masks_u8 (any alignment,
    at most 4, shared by the jobs): 0 leaves a pixel, 255 applies the operator, values between feather the edge.  Step k
    computes clamp(o * m + x * (1 - m), 0, 1) with m = byte / 255 where it names a mask, clamp(o, 0, 1) where it names
    none.  The bytes equal resize_u8 at the picture's size -> operator_apply(op, x, param, mask (1,1,h,w) fp32) per step ->
    to_u8_hwc.  Returns out (1-D uint8)."""
    return _replay('replay_u8_masked', True, src_u8, jobs, params, masks_u8, mask_offsets, out)


def replay_u8_stencils(src_u8, jobs, params, masks_u8=None, mask_offsets=(), out=None):
    """replay_u8 / replay_u8_masked for lists with ANY number of sharpness steps, ONE launch (t2o_replay_u8_stencils):
    jobs are 5-tuples (src_offset, out_offset, h, w, ops) as for replay_u8 or 6-tuples with mask_of as for
    replay_u8_masked (a 5-tuple names no mask); masks_u8 / mask_offsets as there, None / () for a global edit.  Every
    sharpness reads the four neighbours of the image in front of it, zero outside the picture; a masked one blends with
    its input at the centre.  The bytes equal resize_u8 at the picture's size -> operator_apply(op, x, param[, mask]) per
    step -> to_u8_hwc.  Lists with at most one sharpness give replay_u8's / replay_u8_masked's bytes, at a higher cost
    (the window is recomputed on a ring of one pixel per sharpness).  Returns out (1-D uint8)."""
    return _replay('replay_u8_stencils', True, src_u8, jobs, params, masks_u8, mask_offsets, out, five_ok=True)


def replay_u8_pick(jobs):
    """The name of the wrapper that serves a launch of `jobs` (a list) -- THE rule, held here only: replay_u8_stencils for the whole
    launch when some job repeats the sharpness, else the cheaper kernel: replay_u8_masked for 6-tuple jobs, else replay_u8."""
    if any(sum(op == REPLAY_SHARPNESS for op in job[4]) >= 2 for job in jobs):
        return 'replay_u8_stencils'
    return 'replay_u8_masked' if any(len(job) == 6 for job in jobs) else 'replay_u8'


def replay_u8_any(src_u8, jobs, params, masks_u8=None, mask_offsets=(), out=None):
    """replay_u8, replay_u8_masked or replay_u8_stencils, whichever replay_u8_pick names for `jobs`, with that wrapper's
    arguments and result.  (The wrappers are looked up by name at call time.)"""
    jobs = [tuple(j) for j in jobs]
    name = replay_u8_pick(jobs)
    return globals()[name](src_u8, jobs, params, *((out,) if name == 'replay_u8' else (masks_u8, mask_offsets, out)))


# ---- local-edit masks (t2o_mask.hip): run-length masks resized and unioned on the device; the per-step mask select ----

RLE_MASK = np.dtype([('first_end', '<u4'), ('n_runs', '<i4'), ('h', '<i4'), ('w', '<i4')])                    # t2o_rle_mask_t
UNION_JOB = np.dtype([('first_sel', '<i4'), ('n_sel', '<i4'), ('out_h', '<i4'), ('out_w', '<i4'), ('out_offset', '<i8')])   # t2o_union_job_t


class RleTables(object):
    """The packed tables of a t2o_rle_union_u8 launch: .host (1-D uint8 CPU tensor, pinned when a GPU is there) = jobs, masks,
    selection, cumulative run ends back to back, then `extra` (int32 values that travel in the same upload), .counts =
    (n_jobs, n_masks, n_sel, n_ends), .need = bytes of output the jobs cover, .dev = the device copy once uploaded."""

    def __init__(self, host, counts, need, extra_at, extra_n):
        self.host, self.counts, self.need, self.extra_at, self.extra_n, self.dev = host, counts, need, extra_at, extra_n, None

    def upload(self, device=None):
        if self.dev is None:
            if device is None:
                device = torch.device('cuda', torch.cuda.current_device())
            self.dev = self.host.to(device, non_blocking=True)
        return self.dev

    def extra(self):
        return self.dev[self.extra_at:self.extra_at + 4 * self.extra_n].view(torch.int32)


def pack_rle_union(masks, jobs, extra=None, pin=None):
    """masks: COCO RLE dicts {'size': [h, w], 'counts': string or list} or (counts, h, w) tuples; jobs: (mask indices,
    out_offset, out_h, out_w) per output plane -> RleTables.  Parsing (gier.rle_counts) and the running sums happen here."""
    from .gier import rle_counts
    ends, mrec, first = [], np.zeros(len(masks), RLE_MASK), 0
    for i, m in enumerate(masks):
        if isinstance(m, dict):
            counts, h, w = rle_counts(m), int(m['size'][0]), int(m['size'][1])
        else:
            counts, h, w = np.asarray(m[0], dtype=np.int64).astype(np.uint32), int(m[1]), int(m[2])
        ends.append(np.cumsum(counts, dtype=np.uint64).astype(np.uint32))
        mrec[i] = (first, len(counts), h, w)
        first += len(counts)
    jrec, sel = np.zeros(len(jobs), UNION_JOB), []
    need = 1
    for i, (ids, off, oh, ow) in enumerate(jobs):
        jrec[i] = (len(sel), len(ids), int(oh), int(ow), int(off))
        sel.extend(int(k) for k in ids)
        need = max(need, int(off) + max(int(oh), 0) * max(int(ow), 0))
    sel = np.asarray(sel, dtype=np.int32)
    ends = np.concatenate(ends) if ends else np.zeros(0, np.uint32)
    extra = np.zeros(0, np.int32) if extra is None else np.ascontiguousarray(extra, dtype=np.int32).reshape(-1)
    parts = [jrec.view(np.uint8), mrec.view(np.uint8), sel.view(np.uint8), ends.view(np.uint8), extra.view(np.uint8)]
    total = sum(p.size for p in parts)
    host = torch.empty(max(total, 8), dtype=torch.uint8, pin_memory=torch.cuda.is_available() if pin is None else bool(pin))
    flat, pos = host.numpy(), 0
    for p in parts:
        flat[pos:pos + p.size] = p.reshape(-1)
        pos += p.size
    return RleTables(host, (len(jobs), len(masks), int(sel.size), int(ends.size)), need, total - 4 * extra.size, int(extra.size))


def rle_union_u8(masks, jobs=None, device=None, out=None, extra=None):
    """resize_and_union_mask (data/GIER/GIER.py:288-307) for every plane of a batch in ONE launch, from run lengths
    (t2o_rle_union_u8): job j = (mask indices, out_offset, out_h, out_w) writes, at byte out_offset of the 1-D uint8 GPU
    tensor `out` (allocated to fit when None; any alignment, planes may abut), the uint8 plane whose pixel (oy, ox) is the
    SUM over the job's masks of the mask's value at the source pixel edit.nearest_index names -- a count: overlapping masks
    give 2, a repeated index counts twice, an empty list gives zeros; saturating at 255.  masks: RLE dicts / (counts, h, w)
    tuples, or an RleTables from pack_rle_union (jobs is then None; already uploaded tables are launched as they are, e.g.
    inside a graph capture).  One pinned buffer, one upload, one launch on the current stream; nothing waits on the host.
    extra: int32 values to ride in the same upload; returns (out, their device copy) then, else out."""
    tables = masks if isinstance(masks, RleTables) else pack_rle_union(masks, jobs, extra)
    if tables.dev is None:
        tables.upload(device if device is not None else (out.device if out is not None else None))
    dev = tables.dev.device
    if out is None:
        out = torch.empty(tables.need, dtype=torch.uint8, device=dev)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.device == dev):
        raise ValueError('rle_union_u8: out must be a contiguous uint8 GPU tensor on the tables\' device')
    n_jobs, n_masks, n_sel, n_ends = tables.counts
    rc = _lib.load().t2o_rle_union_u8(tables.host.data_ptr(), tables.dev.data_ptr(), n_jobs, n_masks, n_sel, n_ends, _ptr(out),
                                      out.numel(), _stream(dev))
    replay_status(rc, 't2o_rle_union_u8')
    return (out, tables.extra()) if extra is not None else out


def mask_select(planes, slot, pred_op):
    """Actor.get_gt_mask from device values (t2o_mask_select): planes (N,H,W) uint8, slot (B,V) int32 -- a plane number or
    -1 --, pred_op (B,) or (B,1) int64, all on the GPU -> (B,1,H,W) fp32 = float(planes[slot[b][pred_op[b]]]), all ones where
    the slot is -1 or the operator lies outside [0, V): no entry means a global edit.  One launch, no host read."""
    pred_op = _plane_args('mask_select', planes, slot, pred_op)
    N, H, W = planes.shape
    B, V = slot.shape
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=planes.device)
    rc = _lib.load().t2o_mask_select(_ptr(planes) if N else None, _ptr(slot), _ptr(pred_op), _ptr(out), N, B, V, H, W,
                                     _stream(planes.device))
    replay_status(rc, 't2o_mask_select')
    return out


PlaneMask = collections.namedtuple('PlaneMask', 'planes slot pred_op')
PlaneMask.__doc__ = """The mask of one masked step as the device holds it: planes (N,H,W) uint8 and slot (B,V) int32 of a gier.MaskTable,
pred_op (B,) or (B,1) int64 the operator vocabulary id each sample chose.  Executor.execute_per_sample takes one as `mask`:
apply_planes then reads the bytes where they lie instead of a (B,1,H,W) fp32 tensor from mask_select."""


def _plane_args(who, planes, slot, pred_op, img=None):
    """The argument checks of mask_select and apply_planes (which also has the images they must belong to) -> pred_op (B,)."""
    if not (planes.is_cuda and planes.dtype == torch.uint8 and planes.dim() == 3 and planes.is_contiguous()):
        raise RuntimeError('%s: planes must be a contiguous (N,H,W) uint8 GPU tensor; there is no CPU implementation' % who)
    if not (slot.is_cuda and slot.dtype == torch.int32 and slot.dim() == 2 and slot.is_contiguous()):
        raise RuntimeError('%s: slot must be a contiguous (B,V) int32 GPU tensor' % who)
    pred_op = pred_op.detach().reshape(-1)
    if not (pred_op.is_cuda and pred_op.dtype == torch.int64 and pred_op.is_contiguous() and pred_op.numel() == slot.shape[0]):
        raise RuntimeError('%s: pred_op must be a contiguous int64 GPU tensor of B elements' % who)
    if img is not None and (slot.shape[0] != img.shape[0] or tuple(planes.shape[1:]) != tuple(img.shape[2:])):
        raise ValueError('%s: planes %s / slot %s do not belong to images %s' % (who, tuple(planes.shape), tuple(slot.shape), tuple(img.shape)))
    return pred_op


class _ApplyPlanesFn(torch.autograd.Function):
    """apply_per_sample under mask_select's mask without the fp32 mask (t2o_apply_planes_fwd / _bwd): saves img, param and
    the ids; the backward reads the same bytes again."""

    @staticmethod
    def forward(ctx, img, param, planes, slot, pred_op, op_id):
        _need_gpu(img, param)
        if op_id.dtype != torch.int32 or not op_id.is_cuda:
            raise RuntimeError('op_id must be an int32 GPU tensor')
        img = _img(img)
        param = param.contiguous()
        op_id = op_id.contiguous()
        pred_op = _plane_args('apply_planes', planes, slot, pred_op, img)
        B, _, H, W = img.shape
        if param.shape != (B, PARAM_PAD):
            raise ValueError('param must be (B,24)')
        N, V = planes.shape[0], slot.shape[1]
        out = torch.empty_like(img)
        rc = _lib.load().t2o_apply_planes_fwd(_ptr(op_id), _ptr(pred_op), _ptr(planes) if N else None, _ptr(slot), N, V, _ptr(img),
                                              _ptr(param), PARAM_PAD, _ptr(out), B, H, W, _stream(img.device))
        _lib.check(rc, 't2o_apply_planes_fwd')
        ctx.save_for_backward(img, param, planes, slot, pred_op, op_id)
        return out

    @staticmethod
    def backward(ctx, gout):
        img, param, planes, slot, pred_op, op_id = ctx.saved_tensors
        B, _, H, W = img.shape
        N, V = planes.shape[0], slot.shape[1]
        gout = gout.contiguous()
        gimg = torch.empty_like(img) if ctx.needs_input_grad[0] else None
        gparam = torch.zeros_like(param)
        ws = workspace(B, H, W, img.device)
        rc = _lib.load().t2o_apply_planes_bwd(_ptr(op_id), _ptr(pred_op), _ptr(planes) if N else None, _ptr(slot), N, V, _ptr(img),
                                              _ptr(param), PARAM_PAD, _ptr(gout), _ptr(gimg), _ptr(gparam), PARAM_PAD, _ptr(ws),
                                              ws.numel(), B, H, W, _stream(img.device))
        _lib.check(rc, 't2o_apply_planes_bwd')
        return gimg, gparam, None, None, None, None


def apply_planes(op_id, pred_op, img, param, planes, slot):
    """apply_per_sample(op_id, img, param, mask_select(planes, slot, pred_op)) in one launch and bit for bit the same out,
    image and parameter gradients: the kernels read the uint8 planes where they lie (no (B,1,H,W) fp32 mask is written,
    read back or kept for the backward).  op_id (B,) int32 executor indices (-1 = identity), pred_op (B,) / (B,1) int64
    operator vocabulary ids -- the column of `slot` --, planes (N,H,W) uint8, slot (B,V) int32; a count, not divided by 255."""
    return _ApplyPlanesFn.apply(img, param, planes, slot, pred_op, op_id)


# ---- mask feathering (t2o_feather.hip): the soft edge of a local edit, an exact integer Gaussian on uint8 planes ----

FEATHER_MAX_JOBS, FEATHER_MAX_SIGMA, FEATHER_MAX_RADIUS = 4, 64.0, 192


class FeatherJob(ctypes.Structure):
    """t2o_feather_job_t of include/t2onet_hip.h (field for field)."""
    _fields_ = [('src_offset', ctypes.c_longlong), ('out_offset', ctypes.c_longlong), ('h', ctypes.c_int), ('w', ctypes.c_int),
                ('sigma', ctypes.c_double)]


def feather_jobs(jobs):
    """jobs: a sequence of (src_offset, out_offset, h, w, sigma) -> the ctypes array t2o_feather_u8 takes."""
    arr = (FeatherJob * max(len(jobs), 1))()
    for c, (src_offset, out_offset, h, w, sigma) in zip(arr, jobs):
        c.src_offset, c.out_offset, c.h, c.w, c.sigma = int(src_offset), int(out_offset), int(h), int(w), float(sigma)
    return arr


def feather_weights(sigma):
    """The integer Gaussian of t2o_feather_u8 for `sigma`: a numpy uint16 array of R + 1 weights, centre first, with
    w[0] + 2 * sum(w[1:]) = 65536 exactly (t2o_feather_weights; the rule is in include/t2onet_hip.h).  R = 0 -- sigma = 0 or
    at or below about 0.2 -- is the copy, whose single weight 65536 the array holds modulo 2^16: [0]."""
    w = np.zeros(FEATHER_MAX_RADIUS + 1, np.uint16)
    radius = ctypes.c_int(0)
    rc = _lib.load().t2o_feather_weights(float(sigma), w.ctypes.data, ctypes.addressof(radius))
    replay_status(rc, 't2o_feather_weights')
    return w[:radius.value + 1].copy()


_feather_ws = {}


def _feather_workspace(need, device):
    """The intermediate of feather_u8: cached per device and stream like _scratch, but a buffer of its own -- a 24 Mpx plane
    needs 48 MB, which the shared scratch should not be grown to."""
    return _scratch(need, device, _feather_ws, 8)


def feather_u8(buffer, jobs, out=None):
    """Feather uint8 planes on the device in TWO launches, whatever their number (t2o_feather_u8): job j = (src_offset,
    out_offset, h, w, sigma) blurs the (h, w) plane at byte src_offset of the 1-D uint8 GPU tensor `buffer` (any alignment)
    with the exact integer separable Gaussian of standard deviation sigma <= 64 (replicated borders; feather_weights) and
    writes it at byte out_offset of `out` -- of `buffer` itself when out is None: in place where the two offsets agree.  At
    most 4 jobs; their destinations may not overlap each other, a source may overlap any destination.  Returns out."""
    if not (torch.is_tensor(buffer) and buffer.is_cuda and buffer.dtype == torch.uint8 and buffer.is_contiguous()):
        raise ValueError('feather_u8: buffer must be a contiguous uint8 GPU tensor')
    if out is None:
        out = buffer
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.device == buffer.device):
        raise ValueError('feather_u8: out must be a contiguous uint8 GPU tensor on the buffer\'s device')
    jobs = [tuple(j) for j in jobs]
    if not 1 <= len(jobs) <= FEATHER_MAX_JOBS:
        raise ValueError('feather_u8: 1 to 4 jobs per call, got %d' % len(jobs))
    for j, (so, oo, h, w, sigma) in enumerate(jobs):
        if not (h > 0 and w > 0):
            continue                                             # the library refuses it
        if not (0 <= so and so + h * w <= buffer.numel()):
            raise ValueError('feather_u8: job %d reads outside the %d-byte buffer' % (j, buffer.numel()))
        if not (0 <= oo and oo + h * w <= out.numel()):
            raise ValueError('feather_u8: job %d writes outside the %d-byte output' % (j, out.numel()))
    lib = _lib.load()
    table = feather_jobs(jobs)
    need = lib.t2o_feather_workspace_bytes(table, len(jobs))     # 0 for a table the library refuses: it says why below
    ws = _feather_workspace(need, buffer.device)
    rc = lib.t2o_feather_u8(_ptr(buffer), _ptr(out), table, len(jobs), _ptr(ws), ws.numel(), _stream(buffer.device))
    replay_status(rc, 't2o_feather_u8')
    return out


# ---- mask morphology (t2o_morph.hip): a plane's boundary moved by an exact Euclidean distance in pixels ----

MORPH_MAX_JOBS, MORPH_MAX_RADIUS = 4, 64
MORPH_MODES = ('grow', 'shrink', 'border')                   # T2O_MORPH_GROW .. T2O_MORPH_BORDER


class MorphJob(ctypes.Structure):
    """t2o_morph_job_t of include/t2onet_hip.h (field for field)."""
    _fields_ = [('src_offset', ctypes.c_longlong), ('out_offset', ctypes.c_longlong), ('h', ctypes.c_int), ('w', ctypes.c_int),
                ('radius', ctypes.c_int), ('mode', ctypes.c_int)]


def morph_jobs(jobs):
    """jobs: a sequence of (src_offset, out_offset, h, w, radius, mode) -> the ctypes array t2o_morph_u8 takes.  mode: one of
    MORPH_MODES or its index; any other integer goes to the library as it is (it refuses it)."""
    arr = (MorphJob * max(len(jobs), 1))()
    for c, (src_offset, out_offset, h, w, radius, mode) in zip(arr, jobs):
        if isinstance(mode, str):
            if mode not in MORPH_MODES:
                raise ValueError('morph_u8: mode %r is none of %s' % (mode, ', '.join(MORPH_MODES)))
            mode = MORPH_MODES.index(mode)
        c.src_offset, c.out_offset, c.h, c.w, c.radius, c.mode = int(src_offset), int(out_offset), int(h), int(w), int(radius), int(mode)
    return arr


_morph_ws = {}


def _morph_workspace(need, device):
    """The distance fields of morph_u8: cached per device and stream like _feather_workspace, a buffer of its own -- a
    24 Mpx plane needs 24 MB (48 MB for a border), which the shared scratch should not be grown to."""
    return _scratch(need, device, _morph_ws, 8)


def morph_u8(buffer, jobs, out=None):
    """Grow, shrink or border uint8 planes on the device in TWO launches, whatever their number (t2o_morph_u8): job j =
    (src_offset, out_offset, h, w, radius, mode) reads the (h, w) plane at byte src_offset of the 1-D uint8 GPU tensor
    `buffer` (any alignment), takes S = the bytes >= 128, and writes the hard 0 / 255 plane of mode 'grow' (within `radius`
    pixels of S, exact Euclidean distance), 'shrink' (in S and further than radius from every pixel of the frame outside S)
    or 'border' (grown and not shrunk) at byte out_offset of `out` -- of `buffer` itself when out is None: in place where
    the two offsets agree.  radius: a whole number in 0..64.  The frame edge is no edge of the selection.  At most 4 jobs;
    their destinations may not overlap each other, a source may overlap any destination.  Returns out."""
    if not (torch.is_tensor(buffer) and buffer.is_cuda and buffer.dtype == torch.uint8 and buffer.is_contiguous()):
        raise ValueError('morph_u8: buffer must be a contiguous uint8 GPU tensor')
    if out is None:
        out = buffer
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.device == buffer.device):
        raise ValueError('morph_u8: out must be a contiguous uint8 GPU tensor on the buffer\'s device')
    jobs = [tuple(j) for j in jobs]
    if not 1 <= len(jobs) <= MORPH_MAX_JOBS:
        raise ValueError('morph_u8: 1 to 4 jobs per call, got %d' % len(jobs))
    for j, (so, oo, h, w, radius, mode) in enumerate(jobs):
        if radius != int(radius):
            raise ValueError('morph_u8: job %d: the radius %r is not a whole number' % (j, radius))
        if not (h > 0 and w > 0):
            continue                                             # the library refuses it
        if not (0 <= so and so + h * w <= buffer.numel()):
            raise ValueError('morph_u8: job %d reads outside the %d-byte buffer' % (j, buffer.numel()))
        if not (0 <= oo and oo + h * w <= out.numel()):
            raise ValueError('morph_u8: job %d writes outside the %d-byte output' % (j, out.numel()))
    lib = _lib.load()
    table = morph_jobs(jobs)
    need = lib.t2o_morph_workspace_bytes(table, len(jobs))       # 0 for a table the library refuses: it says why below
    ws = _morph_workspace(need, buffer.device)
    rc = lib.t2o_morph_u8(_ptr(buffer), _ptr(out), table, len(jobs), _ptr(ws), ws.numel(), _stream(buffer.device))
    replay_status(rc, 't2o_morph_u8')
    return out


# ---- selections (t2o_select.hip): the mask planes of a local edit computed from a rule, where the photo already lies ----

SELECT_MAX_JOBS, SELECT_MAX_TERMS = 4, 4
SELECT_KINDS = ('lum', 'sat', 'hue', 'linear', 'radial', 'plane')          # T2O_SELECT_LUM .. T2O_SELECT_PLANE


class SelectTerm(ctypes.Structure):
    """t2o_select_term_t of include/t2onet_hip.h (field for field)."""
    _fields_ = [('kind', ctypes.c_int), ('invert', ctypes.c_int), ('p', ctypes.c_int * 4), ('plane_offset', ctypes.c_longlong)]


class SelectJob(ctypes.Structure):
    """t2o_select_job_t of include/t2onet_hip.h (field for field)."""
    _fields_ = [('src_offset', ctypes.c_longlong), ('out_offset', ctypes.c_longlong), ('h', ctypes.c_int), ('w', ctypes.c_int),
                ('n_terms', ctypes.c_int), ('reserved', ctypes.c_int), ('terms', SelectTerm * SELECT_MAX_TERMS)]


def select_jobs(jobs):
    """jobs: a sequence of (src_offset, out_offset, h, w, terms) -> the ctypes array t2o_select_u8 takes.  A term is
    (kind, invert, values...) in the INTEGER units of include/t2onet_hip.h, kind a name of SELECT_KINDS or its number:
    ('lum' | 'sat' | 'hue', invert, lo, hi[, soft]), ('linear', invert, X0, Y0, X1, Y1), ('radial', invert, CX, CY, RI, RO),
    ('plane', invert, byte offset of the plane in src).  `n_terms` is len(terms) even beyond 4, and an unknown number is
    passed on, so that the library is the one to refuse them; a wrong number of values is a ValueError here."""
    arr = (SelectJob * max(len(jobs), 1))()
    for c, (src_offset, out_offset, h, w, terms) in zip(arr, jobs):
        c.src_offset, c.out_offset, c.h, c.w, c.n_terms = int(src_offset), int(out_offset), int(h), int(w), len(terms)
        for t, term in zip(c.terms, list(terms)[:SELECT_MAX_TERMS]):
            kind, invert, values = term[0], term[1], [int(v) for v in term[2:]]
            if isinstance(kind, str):
                if kind not in SELECT_KINDS:
                    raise ValueError('select_u8: %r is not a term kind (one of %s)' % (kind, ', '.join(SELECT_KINDS)))
                kind = SELECT_KINDS.index(kind)
            t.kind, t.invert = int(kind), int(invert)
            name = SELECT_KINDS[t.kind] if 0 <= t.kind < len(SELECT_KINDS) else None
            if name == 'plane':
                if len(values) != 1:
                    raise ValueError('select_u8: a plane term takes one offset, got %r' % (term,))
                t.plane_offset = values[0]
            else:
                if name in ('lum', 'sat', 'hue') and len(values) == 2:
                    values = values + [0]
                if len(values) > 4 or (name is not None and len(values) != (3 if name in ('lum', 'sat', 'hue') else 4)):
                    raise ValueError('select_u8: wrong number of values in term %r' % (term,))
                for k, v in enumerate(values):
                    if not -2 ** 31 <= v < 2 ** 31:
                        raise ValueError('select_u8: a value of term %r does not fit 32 bits' % (term,))
                    t.p[k] = v
    return arr


def select_u8(src_u8, jobs, out=None):
    """Mask planes from a rule in ONE launch (t2o_select_u8): job j = (src_offset, out_offset, h, w, terms) reads the uint8
    (h, w, 3) RGB photo at byte src_offset of the 1-D uint8 GPU tensor src_u8 (any alignment; jobs may share a photo) and
    writes the (h, w) uint8 plane of its selection at byte out_offset of `out` (allocated to fit when None).  terms: 1 to 4
    integer terms as select_jobs takes them, multiplied left to right; a 'plane' term reads an (h, w) plane at its byte offset
    in src_u8.  At most 4 jobs; no destination may overlap another one or, when out is src_u8, anything the call reads.
    Every offset and size is checked here against the tensors, so that a wrong argument is a ValueError and never a GPU
    fault.  Returns out (1-D uint8)."""
    if not (torch.is_tensor(src_u8) and src_u8.is_cuda and src_u8.dtype == torch.uint8 and src_u8.is_contiguous()):
        raise ValueError('select_u8: src must be a contiguous uint8 GPU tensor')
    jobs = [tuple(j) for j in jobs]
    if not 1 <= len(jobs) <= SELECT_MAX_JOBS:
        raise ValueError('select_u8: 1 to 4 jobs per call, got %d' % len(jobs))
    table = select_jobs(jobs)
    live = [(j, c) for j, c in enumerate(table[:len(jobs)]) if c.h > 0 and c.w > 0]          # (an empty plane: the library refuses it)
    for j, c in live:
        if not (0 <= c.src_offset and c.src_offset + 3 * c.h * c.w <= src_u8.numel()):
            raise ValueError('select_u8: job %d reads outside the %d-byte source' % (j, src_u8.numel()))
        for t in c.terms[:min(c.n_terms, SELECT_MAX_TERMS)]:
            if t.kind == SELECT_KINDS.index('plane') and not (0 <= t.plane_offset and t.plane_offset + c.h * c.w <= src_u8.numel()):
                raise ValueError('select_u8: job %d reads a plane term outside the %d-byte source' % (j, src_u8.numel()))
    for j, c in live:                                                                         # before `out` is allocated to fit
        if c.out_offset < 0:
            raise ValueError('select_u8: job %d writes before the output (out_offset %d)' % (j, c.out_offset))
    need = max([c.out_offset + c.h * c.w for _, c in live] or [1])
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=src_u8.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.device == src_u8.device):
        raise ValueError('select_u8: out must be a contiguous uint8 GPU tensor on the source\'s device')
    if out.numel() < need:
        raise ValueError('select_u8: a job writes outside the %d-byte output' % out.numel())
    rc = _lib.load().t2o_select_u8(_ptr(src_u8), _ptr(out), table, len(jobs), _stream(src_u8.device))
    replay_status(rc, 't2o_select_u8')
    return out


# ---- mask refinement (t2o_refine.hip): a plane snapped to the photo's own edges, the guided filter in exact integers ----

REFINE_MAX_JOBS, REFINE_MAX_RADIUS, REFINE_MAX_EPS2, REFINE_LAUNCHES = 4, 64, 65025, 4


class RefineJob(ctypes.Structure):
    """t2o_refine_job_t of include/t2onet_hip.h (field for field)."""
    _fields_ = [('photo_offset', ctypes.c_longlong), ('src_offset', ctypes.c_longlong), ('out_offset', ctypes.c_longlong),
                ('h', ctypes.c_int), ('w', ctypes.c_int), ('radius', ctypes.c_int), ('eps2', ctypes.c_int)]


def refine_jobs(jobs):
    """jobs: a sequence of (photo_offset, src_offset, out_offset, h, w, radius, eps2) -> the ctypes array t2o_refine_u8
    takes.  Integers only; a value that does not fit its field is a ValueError."""
    arr = (RefineJob * max(len(jobs), 1))()
    for c, job in zip(arr, jobs):
        if len(job) != 7:
            raise ValueError('refine_u8: a job is (photo_offset, src_offset, out_offset, h, w, radius, eps2), got %r' % (job,))
        values = [int(v) for v in job]
        if any(v != f for v, f in zip(values, job)):
            raise ValueError('refine_u8: job %r holds a value that is not an integer' % (job,))
        if not all(-2 ** 63 <= v < 2 ** 63 for v in values[:3]) or not all(-2 ** 31 <= v < 2 ** 31 for v in values[3:]):
            raise ValueError('refine_u8: a value of job %r does not fit its field' % (job,))
        c.photo_offset, c.src_offset, c.out_offset, c.h, c.w, c.radius, c.eps2 = values
    return arr


_refine_ws = {}


def _refine_workspace(need, device):
    """The intermediates of refine_u8: cached per device and stream like _feather_workspace, a buffer of its own -- 20 bytes
    per pixel of every plane of the call."""
    return _scratch(need, device, _refine_ws, 16)


def refine_u8(photo_u8, buffer, jobs, out=None):
    """Snap uint8 planes to the edges of their photo on the device in FOUR launches, whatever their number
    (t2o_refine_u8): job j = (photo_offset, src_offset, out_offset, h, w, radius, eps2) runs the exact integer guided filter
    of include/t2onet_hip.h -- guide = the luminance of the (h, w, 3) uint8 RGB photo at byte photo_offset of the 1-D uint8 GPU
    tensor photo_u8, window radius <= 64, regulariser eps2 in 1..65025 (byte^2) -- on the (h, w) plane at byte src_offset of
    the 1-D uint8 GPU tensor `buffer` and writes it at byte out_offset of `out` -- of `buffer` itself when out is None: in
    place where the two offsets agree.  Any byte alignment; photo_u8 may be `buffer`.  At most 4 jobs; a destination may not
    overlap another one or a photo of the call, a source may overlap any destination.  Every offset and size is checked here
    against the tensors, so that a wrong argument is a ValueError and never a GPU fault.  Returns out."""
    def ok(t):
        return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    if not (ok(photo_u8) and ok(buffer)) or photo_u8.device != buffer.device:
        raise ValueError('refine_u8: photo and buffer must be contiguous uint8 GPU tensors on one device')
    if out is None:
        out = buffer
    elif not (ok(out) and out.device == buffer.device):
        raise ValueError('refine_u8: out must be a contiguous uint8 GPU tensor on the buffer\'s device')
    jobs = [tuple(j) for j in jobs]
    if not 1 <= len(jobs) <= REFINE_MAX_JOBS:
        raise ValueError('refine_u8: 1 to 4 jobs per call, got %d' % len(jobs))
    table = refine_jobs(jobs)
    for j, c in enumerate(table[:len(jobs)]):
        if c.out_offset < 0:                                     # before anything is allocated
            raise ValueError('refine_u8: job %d writes before the output (out_offset %d)' % (j, c.out_offset))
        if not (c.h > 0 and c.w > 0):
            continue                                             # the library refuses it
        if not (0 <= c.photo_offset and c.photo_offset + 3 * c.h * c.w <= photo_u8.numel()):
            raise ValueError('refine_u8: job %d reads outside the %d-byte photo buffer' % (j, photo_u8.numel()))
        if not (0 <= c.src_offset and c.src_offset + c.h * c.w <= buffer.numel()):
            raise ValueError('refine_u8: job %d reads outside the %d-byte buffer' % (j, buffer.numel()))
        if not c.out_offset + c.h * c.w <= out.numel():
            raise ValueError('refine_u8: job %d writes outside the %d-byte output' % (j, out.numel()))
    lib = _lib.load()
    need = lib.t2o_refine_workspace_bytes(table, len(jobs))      # 0 for a table the library refuses: it says why below
    ws = _refine_workspace(need, buffer.device)
    rc = lib.t2o_refine_u8(_ptr(photo_u8), _ptr(buffer), _ptr(out), table, len(jobs), _ptr(ws), ws.numel(), _stream(buffer.device))
    replay_status(rc, 't2o_refine_u8')
    return out


# ---- the magic wand (t2o_region.hip): the connected region around a seed pixel, union-find labelling on the device ----

REGION_MAX_JOBS, REGION_LAUNCHES = 4, 3


class RegionJob(ctypes.Structure):
    """t2o_region_job_t of include/t2onet_hip.h (field for field)."""
    _fields_ = [('photo_offset', ctypes.c_longlong), ('out_offset', ctypes.c_longlong), ('h', ctypes.c_int), ('w', ctypes.c_int),
                ('seed_x', ctypes.c_int), ('seed_y', ctypes.c_int), ('tol', ctypes.c_int), ('conn', ctypes.c_int)]


def region_jobs(jobs):
    """jobs: a sequence of (photo_offset, out_offset, h, w, seed_x, seed_y, tol, conn) -> the ctypes array t2o_region_u8
    takes.  Integers only; a value that does not fit its field is a ValueError."""
    arr = (RegionJob * max(len(jobs), 1))()
    for c, job in zip(arr, jobs):
        if len(job) != 8:
            raise ValueError('region_u8: a job is (photo_offset, out_offset, h, w, seed_x, seed_y, tol, conn), got %r' % (job,))
        values = [int(v) for v in job]
        if any(v != f for v, f in zip(values, job)):
            raise ValueError('region_u8: job %r holds a value that is not an integer' % (job,))
        if not all(-2 ** 63 <= v < 2 ** 63 for v in values[:2]) or not all(-2 ** 31 <= v < 2 ** 31 for v in values[2:]):
            raise ValueError('region_u8: a value of job %r does not fit its field' % (job,))
        c.photo_offset, c.out_offset, c.h, c.w, c.seed_x, c.seed_y, c.tol, c.conn = values
    return arr


_region_ws = {}


def _region_workspace(need, device):
    """The parent array of region_u8: cached per device and stream like _refine_workspace, a buffer of its own -- 4 bytes
    per pixel of every job of the call."""
    return _scratch(need, device, _region_ws, 16)


def region_u8(photo_u8, jobs, out=None):
    """The connected region around a seed pixel as a hard 0 / 255 plane, on the device in THREE launches whatever the number
    of jobs and whatever the pictures hold (t2o_region_u8): job j = (photo_offset, out_offset, h, w, seed_x, seed_y, tol,
    conn) reads the (h, w, 3) uint8 RGB photo at byte photo_offset of the 1-D uint8 GPU tensor photo_u8 (jobs may share a
    photo) and writes 255 at byte out_offset + y w + x of `out` (allocated to fit when None) where pixel (y, x) is joined to
    the seed by a path of pixels whose three bytes each differ from the seed's by at most tol (0..255), else 0; conn = 4
    allows horizontal and vertical steps, 8 diagonal ones too.  The seed's bytes are read on the device.  Any byte alignment;
    out may be photo_u8.  At most 4 jobs; a destination may overlap neither another one nor a photo of the call.  The
    labelling is lock-free union-find in which no workgroup waits for another and every loop follows strictly falling
    indices (include/t2onet_hip.h); the bytes are deterministic.  Every offset and size is checked here against the tensors,
    so that a wrong argument is a ValueError and never a GPU fault.  Returns out (1-D uint8)."""
    def ok(t):
        return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    if not ok(photo_u8):
        raise ValueError('region_u8: photo must be a contiguous uint8 GPU tensor')
    jobs = [tuple(j) for j in jobs]
    if not 1 <= len(jobs) <= REGION_MAX_JOBS:
        raise ValueError('region_u8: 1 to 4 jobs per call, got %d' % len(jobs))
    table = region_jobs(jobs)
    live = [(j, c) for j, c in enumerate(table[:len(jobs)]) if c.h > 0 and c.w > 0]          # (an empty plane: the library refuses it)
    for j, c in enumerate(table[:len(jobs)]):                                                # before `out` is allocated to fit
        if c.out_offset < 0:
            raise ValueError('region_u8: job %d writes before the output (out_offset %d)' % (j, c.out_offset))
    for j, c in live:
        if not (0 <= c.photo_offset and c.photo_offset + 3 * c.h * c.w <= photo_u8.numel()):
            raise ValueError('region_u8: job %d reads outside the %d-byte photo buffer' % (j, photo_u8.numel()))
        if not (0 <= c.seed_x < c.w and 0 <= c.seed_y < c.h):
            raise ValueError('region_u8: job %d has its seed (%d, %d) outside the %d x %d frame' % (j, c.seed_x, c.seed_y, c.w, c.h))
    need = max([c.out_offset + c.h * c.w for _, c in live] or [1])
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=photo_u8.device)
    elif not (ok(out) and out.device == photo_u8.device):
        raise ValueError('region_u8: out must be a contiguous uint8 GPU tensor on the photo\'s device')
    if out.numel() < need:
        raise ValueError('region_u8: a job writes outside the %d-byte output' % out.numel())
    lib = _lib.load()
    need = lib.t2o_region_workspace_bytes(table, len(jobs))      # 0 for a table the library refuses: it says why below
    ws = _region_workspace(need, photo_u8.device)
    rc = lib.t2o_region_u8(_ptr(photo_u8), _ptr(out), table, len(jobs), _ptr(ws), ws.numel(), _stream(photo_u8.device))
    replay_status(rc, 't2o_region_u8')
    return out


# ---- removing a region (t2o_fill.hip): the pixels under a plane replaced by an exact integer push-pull fill ----

FILL_MAX_JOBS, FILL_LAUNCHES = 4, 3


class FillJob(ctypes.Structure):
    """t2o_fill_job_t of include/t2onet_hip.h (field for field)."""
    _fields_ = [('photo_offset', ctypes.c_longlong), ('plane_offset', ctypes.c_longlong), ('out_offset', ctypes.c_longlong),
                ('h', ctypes.c_int), ('w', ctypes.c_int)]


def fill_jobs(jobs):
    """jobs: a sequence of (photo_offset, plane_offset, out_offset, h, w) -> the ctypes array t2o_fill_u8 takes.  Integers
    only; a value that does not fit its field is a ValueError."""
    arr = (FillJob * max(len(jobs), 1))()
    for c, job in zip(arr, jobs):
        if len(job) != 5:
            raise ValueError('fill_u8: a job is (photo_offset, plane_offset, out_offset, h, w), got %r' % (job,))
        values = [int(v) for v in job]
        if any(v != f for v, f in zip(values, job)):
            raise ValueError('fill_u8: job %r holds a value that is not an integer' % (job,))
        if not all(-2 ** 63 <= v < 2 ** 63 for v in values[:3]) or not all(-2 ** 31 <= v < 2 ** 31 for v in values[3:]):
            raise ValueError('fill_u8: a value of job %r does not fit its field' % (job,))
        c.photo_offset, c.plane_offset, c.out_offset, c.h, c.w = values
    return arr


_fill_ws = {}


def _fill_workspace(need, device):
    """The pyramid of fill_u8: cached per device and stream like _region_workspace, a buffer of its own -- about 8/3 bytes
    per pixel of every job of the call."""
    return _scratch(need, device, _fill_ws, 16)


def fill_u8(photo_u8, planes_u8, jobs, out=None):
    """Remove what lies under a plane, on the device in THREE launches whatever the number of jobs and whatever the pictures
    hold (t2o_fill_u8): job j = (photo_offset, plane_offset, out_offset, h, w) reads the (h, w, 3) uint8 RGB photo at byte
    photo_offset of the 1-D uint8 GPU tensor photo_u8 and the (h, w) uint8 plane at byte plane_offset of the 1-D uint8 GPU
    tensor planes_u8 (jobs may share either) and writes the photo with every pixel whose plane byte M is > 0 blended, by
    M / 255, with the exact integer push-pull fill of include/t2onet_hip.h from the pixels with M = 0, at byte out_offset of
    `out` (allocated to fit when None); pixels with M = 0 come out byte for byte, and a plane without a 0 leaves the photo as
    it is.  A SMOOTH fill -- sky, walls, blurred backgrounds; it synthesises no texture and is not the reference's inpaint
    network.  Any byte alignment; planes_u8 and out may be photo_u8.  At most 4 jobs; a destination may overlap neither
    another one nor a plane nor a photo of the call, except its own photo at exactly its own address: a job in place.  No
    workgroup waits for another and every loop bound follows from the sizes; the bytes are deterministic.  Every offset and
    size is checked here against the tensors, so that a wrong argument is a ValueError and never a GPU fault.  Returns out
    (1-D uint8)."""
    def ok(t):
        return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    if not (ok(photo_u8) and ok(planes_u8)) or photo_u8.device != planes_u8.device:
        raise ValueError('fill_u8: photo and planes must be contiguous uint8 GPU tensors on one device')
    jobs = [tuple(j) for j in jobs]
    if not 1 <= len(jobs) <= FILL_MAX_JOBS:
        raise ValueError('fill_u8: 1 to 4 jobs per call, got %d' % len(jobs))
    table = fill_jobs(jobs)
    live = [(j, c) for j, c in enumerate(table[:len(jobs)]) if c.h > 0 and c.w > 0]          # (an empty picture: the library refuses it)
    for j, c in enumerate(table[:len(jobs)]):                                                # before `out` is allocated to fit
        if c.out_offset < 0:
            raise ValueError('fill_u8: job %d writes before the output (out_offset %d)' % (j, c.out_offset))
    for j, c in live:
        if not (0 <= c.photo_offset and c.photo_offset + 3 * c.h * c.w <= photo_u8.numel()):
            raise ValueError('fill_u8: job %d reads outside the %d-byte photo buffer' % (j, photo_u8.numel()))
        if not (0 <= c.plane_offset and c.plane_offset + c.h * c.w <= planes_u8.numel()):
            raise ValueError('fill_u8: job %d reads outside the %d-byte plane buffer' % (j, planes_u8.numel()))
    need = max([c.out_offset + 3 * c.h * c.w for _, c in live] or [1])
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=photo_u8.device)
    elif not (ok(out) and out.device == photo_u8.device):
        raise ValueError('fill_u8: out must be a contiguous uint8 GPU tensor on the photo\'s device')
    if out.numel() < need:
        raise ValueError('fill_u8: a job writes outside the %d-byte output' % out.numel())
    lib = _lib.load()
    need = lib.t2o_fill_workspace_bytes(table, len(jobs))        # 0 for a table the library refuses: it says why below
    ws = _fill_workspace(need, photo_u8.device)
    rc = lib.t2o_fill_u8(_ptr(photo_u8), _ptr(planes_u8), _ptr(out), table, len(jobs), _ptr(ws), ws.numel(), _stream(photo_u8.device))
    replay_status(rc, 't2o_fill_u8')
    return out
