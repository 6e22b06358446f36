"""The fused decoder step and feature head (t2o_decoder.hip, decoder_step.py) against the SAME modules run by PyTorch
in fp64 (models/action_decoder.py:38-64, models/attention.py:17-44, models/actor.py:50): every output, every data
gradient and every parameter gradient; the Trainer's deferred weight gradients (one product per weight over the steps
of a train step) against per-step autograd; evaluation mode; the argument validation of the C entry points.  Over the
whole documented domain: every width class (D % 64 == 0 up to 1024, E % 4 == 0, 1 <= V <= 16, 1 <= L <= 64), modules without
biases / affine parameters / running statistics, every output gradient absent, saturated ("confident") parameters."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _close(got, ref, tol, what=''):
    ref = ref.detach().double().cpu()
    scale = float(ref.abs().max()) or 1.0
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), ref.numpy(), rtol=tol, atol=tol * scale, err_msg=what)


def _rel_err(got, ref):
    """max |got - ref| over the largest reference entry: the quantity _close bounds"""
    ref = ref.detach().double()
    return float((got.detach().double() - ref).abs().max()) / (float(ref.abs().max()) or 1.0)


def _decoder(seed, dev=DEV, V=11, E=300, D=512, scale=2.0, no_bias=(), **kw):
    """The actor's decoder layout at width D (2-layer LSTM(E + D -> D), attention, V operator tokens).  `no_bias`: which of
    'rnn', 'vis', 'lo', 'out' are rebuilt with bias=False."""
    from t2onet_amd.action_decoder import Decoder
    torch.manual_seed(seed)
    dec = Decoder(V, 5, E, D // 2, 2, bidirectional=True, use_attention=True, **kw)
    assert dec.hidden_size == D
    if 'rnn' in no_bias:
        dec.rnn = nn.LSTM(E + D, D, 2, batch_first=True, bias=False)
    if 'vis' in no_bias:
        dec.vis_linear = nn.Linear(D, D, bias=False)
    if 'lo' in no_bias:
        dec.attention.linear_out = nn.Linear(2 * D, D, bias=False)
    if 'out' in no_bias:
        dec.out_linear = nn.Linear(D, V, bias=False)
    with torch.no_grad():
        for p in dec.parameters():
            p.mul_(scale)                                        # (livelier activations than the default initialisation)
    return dec.to(dev)


def _reference_step(dec64, prev_op, hidden, enc, feat):
    """The reference's forward_step, literally (action_decoder.py:38-64 with attention.py:17-44), on an fp64 (or fp32) CPU
    copy; every width is the module's own."""
    B = prev_op.shape[0]
    token = dec64.embedding(prev_op)
    vis = F.relu(dec64.vis_linear(feat)).unsqueeze(1)
    out, hidden = dec64.rnn(torch.cat((token, vis), 2), hidden)
    attn = F.softmax(torch.bmm(out, enc.transpose(1, 2)).view(-1, enc.shape[1]), dim=1).view(B, -1, enc.shape[1])
    mix = torch.bmm(attn, enc)
    comb = torch.cat((mix, out), dim=2)
    ctx = torch.tanh(dec64.attention.linear_out(comb.view(-1, 2 * dec64.hidden_size))).view(B, -1, dec64.hidden_size)
    logp = F.log_softmax(dec64.out_linear(ctx.contiguous().view(-1, dec64.hidden_size)), dim=1).view(B, 1, -1)
    return logp, hidden, attn, ctx.squeeze(1)


def _inputs(B, L, seed, V=11, D=512):
    feat = synth.uniform((B, D), seed + 1, 0.0, 1.5)
    h = synth.uniform((2, B, D), seed + 2, -1.0, 1.0)
    c = synth.uniform((2, B, D), seed + 3, -1.0, 1.0)
    enc = synth.uniform((B, L, D), seed + 4, -0.3, 0.3)
    op = (synth.uniform((B, 1), seed + 5, 0.0, 1.0) * V).long().clamp(0, V - 1)
    return feat, h, c, enc, op


def _must_be_fused(monkeypatch, dec, op, hidden, enc, feat):
    """The step must be taken by the fused kernels: a silent fall-back to the per-layer path fails the test."""
    import t2onet_amd.action_decoder as AD
    from t2onet_amd import decoder_step as DS
    assert AD._FUSED_STEP and DS.step_supported(dec, op, hidden, enc, feat)
    monkeypatch.setattr(AD.Decoder, '_rnn_step', lambda *a, **k: pytest.fail('the per-layer path ran'))


def _reference_run(dec, inputs, g, dtype):
    """dec's step in `dtype` on the CPU and the gradients of sum_i <output_i, g_i>.  Returns (module copy, outputs
    [logp, h, c, attn, ctx], input gradients [feat, h, c, enc])."""
    feat, h, c, enc, op = inputs
    ref = copy.deepcopy(dec).to(dtype).cpu()
    ref.zero_grad(set_to_none=True)
    r_in = [t.detach().clone().to(dtype).requires_grad_(True) for t in (feat, h, c, enc)]
    logp, (hn, cn), attn, ctx = _reference_step(ref, op, (r_in[1], r_in[2]), r_in[3], r_in[0])
    gt =[t.to(dtype) for t in g]
    ((logp * gt[0]).sum() + (hn * gt[1]).sum() + (cn * gt[2]).sum() + (ctx * gt[3]).sum()).backward()
    return ref, [t.detach() for t in (logp, hn, cn, attn, ctx)], [t.grad for t in r_in]


def _step_vs_fp64(monkeypatch, dec, B, L, seed, gseed=200, measured=False):
    """One fused step of `dec` against the same modules in fp64: every output, data gradient and parameter gradient.
    `measured`: each tolerance is the larger of the file's (3e-6 forward, 2e-5 gradients) and 4 x the error of the same
    modules run in fp32 on the CPU (another, equally valid fp32 summation order) for that tensor -- for widths and
    magnitudes the file's numbers were never measured at."""
    V, D = dec.output_size, dec.hidden_size
    inputs = _inputs(B, L, seed, V, D)
    feat, h, c, enc, op = inputs
    g = [synth.uniform(s, gseed + i, -1.0, 1.0) for i, s in enumerate([(B, 1, V), (2, B, D), (2, B, D), (B, D)])]
    dec64, outs, grads = _reference_run(dec, inputs, g, torch.float64)
    pnames = [n for n, _ in dec.named_parameters()]
    assert pnames == [n for n, _ in dec64.named_parameters()]
    pgrads = [q.grad for _, q in dec64.named_parameters()]
    tol_o, tol_g, tol_p = [3e-6] * 5, [2e-5] * 4, [2e-5] * len(pgrads)
    if measured:
        dec32, o32, g32 = _reference_run(dec, inputs, g, torch.float32)
        e_o, e_g = [_rel_err(a, r) for a, r in zip(o32, outs)], [_rel_err(a, r) for a, r in zip(g32, grads)]
        e_p = [_rel_err(q.grad, r) for (_, q), r in zip(dec32.named_parameters(), pgrads)]
        print('fp32 CPU modules vs fp64, relative to the largest entry: logp/h/c/attn/ctx %s, d feat/h/c/enc %s, d parameters %s'
              % (['%.2e' % e for e in e_o], ['%.2e' % e for e in e_g], ['%.2e' % e for e in e_p]))
        tol_o, tol_g, tol_p = ([max(3e-6, 4 * e) for e in e_o], [max(2e-5, 4 * e) for e in e_g], [max(2e-5, 4 * e) for e in e_p])
    # fused step
    t_in = [t.to(DEV).requires_grad_(True) for t in (feat, h, c, enc)]
    _must_be_fused(monkeypatch, dec, op.to(DEV), (t_in[1], t_in[2]), t_in[3], t_in[0])
    dec.zero_grad(set_to_none=True)
    logp2, (hn2, cn2), attn2, ctx2 = dec.forward_step(op.to(DEV), (t_in[1], t_in[2]), t_in[3], t_in[0])
    assert logp2.shape == (B, 1, V) and hn2.shape == (2, B, D) and attn2.shape == (B, 1, L) and ctx2.shape == (B, D)
    for got, ref, name, tol in zip((logp2, hn2, cn2, attn2, ctx2), outs, ('logp', 'h', 'c', 'attn', 'ctx'), tol_o):
        _close(got, ref, tol, name)
    gd = [t.to(DEV) for t in g]
    ((logp2 * gd[0]).sum() + (hn2 * gd[1]).sum() + (cn2 * gd[2]).sum() + (ctx2 * gd[3]).sum()).backward()
    for a, b, name, tol in zip(t_in, grads, ('feat', 'h', 'c', 'enc'), tol_g):
        _close(a.grad, b, tol, 'd ' + name)
    for (name, p), q, tol in zip(dec.named_parameters(), pgrads, tol_p):
        assert p.grad is not None, name
        _close(p.grad, q, tol, 'd ' + name)
    return logp2, dec


@pytest.mark.parametrize('B,L', [(64, 17), (8, 5), (4, 12), (37, 9), (1, 3), (70, 4)])
def test_fused_step_matches_fp64_modules(monkeypatch, B, L):
    _step_vs_fp64(monkeypatch, _decoder(5), B, L, 100 + B)


# (D, E, V, L, B): the smallest of everything (V = 1: one logit per row);  a full logit tile, the longest request and a
# row-tile tail;  D no power of two and not a multiple of 256 (k_attn_fwd / k_attn_bwd inside the step, not the _wide
# forms);  E + D = 356 with a K tail (356 % 32 = 4) in layer 0's products;  the upper width
WIDTHS = [(64, 4, 1, 1, 1), (128, 20, 16, 64, 17), (192, 300, 11, 17, 33), (320, 36, 7, 9, 5), (1024, 8, 5, 3, 16)]


@pytest.mark.parametrize('D,E,V,L,B', WIDTHS)
def test_fused_step_over_the_documented_widths(monkeypatch, D, E, V, L, B):
    logp, dec = _step_vs_fp64(monkeypatch, _decoder(5, V=V, E=E, D=D), B, L, 100 + B, measured=D == 1024)
    if V == 1:                                                      # log_softmax of one logit: exactly 0, and no gradient through it
        assert float(logp.abs().max()) == 0.0
        assert float(dec.out_linear.weight.grad.abs().max()) == 0.0 and float(dec.out_linear.bias.grad.abs().max()) == 0.0


@pytest.mark.parametrize('no_bias', [('rnn', 'vis', 'lo', 'out'), ('vis',), ('lo',), ('out',)], ids=lambda t: '-'.join(t))
def test_fused_step_without_biases(monkeypatch, no_bias):
    """nn.LSTM(bias=False) and bias-free Linears: the NULL sides of every `if (bias)` in the step's epilogues.  The
    parameter loop covers exactly the parameters that exist (a gradient for an absent one would have nowhere to go:
    autograd refuses a tensor returned for a None input)."""
    dec = _decoder(5, V=11, E=20, D=128, no_bias=no_bias)
    assert (dec.vis_linear.bias is None) == ('vis' in no_bias) and (dec.attention.linear_out.bias is None) == ('lo' in no_bias)
    assert (dec.out_linear.bias is None) == ('out' in no_bias) and dec.rnn.bias == ('rnn' not in no_bias)
    assert len(list(dec.parameters())) == 15 - sum({'rnn': 4, 'vis': 1, 'lo': 1, 'out': 1}[k] for k in no_bias)
    _step_vs_fp64(monkeypatch, dec, 9, 6, 150)


def test_confident_decoder(monkeypatch):
    """Parameters x 8 (a trained checkpoint's regime rather than an initialised one's): LSTM gates at 0 / 1, tanh at
    +-1, one logit dominating its row of the log-softmax."""
    _step_vs_fp64(monkeypatch, _decoder(5, V=11, E=20, D=128, scale=8.0), 9, 6, 160, measured=True)


def test_evaluation_mode_with_dropout_configured_takes_the_fused_step(monkeypatch):
    """dropout_p / input_dropout_p > 0 are inert under eval(): the fused step takes the decoder and matches fp64; in
    training mode it declines (active dropout is the per-layer path's)."""
    from t2onet_amd import decoder_step as DS
    dec = _decoder(5, V=11, E=20, D=128, input_dropout_p=0.25, dropout_p=0.25)
    assert dec.rnn.dropout == 0.25 and dec.input_dropout.p == 0.25
    feat, h, c, enc, op = (t.to(DEV) for t in _inputs(4, 5, 170, 11, 128))
    dec.train()
    assert not DS.step_supported(dec, op, (h, c), enc, feat)
    dec.eval()
    _step_vs_fp64(monkeypatch, dec, 9, 6, 170)


def test_fused_step_equals_the_per_layer_path(monkeypatch):
    """Same module, fused step on and off (library GEMMs + framework gate kernels): outputs and gradients agree in fp32."""
    import t2onet_amd.action_decoder as AD
    dec = _decoder(7)
    B, L = 16, 9
    feat, h, c, enc, op = _inputs(B, L, 300)
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(AD, '_FUSED_STEP', fused)
        dec.zero_grad(set_to_none=True)
        t_in = [t.to(DEV).requires_grad_(True) for t in (feat, h, c, enc)]
        logp, (hn, cn), _, ctx = dec.forward_step(op.to(DEV), (t_in[1], t_in[2]), t_in[3], t_in[0])
        (logp.sum() * 0.3 + hn.square().sum() + cn.sum() + ctx.square().sum()).backward()
        outs.append([logp, hn, cn, ctx] + [t.grad for t in t_in] + [p.grad.clone() for p in dec.parameters()])
    for a, b in zip(*outs):
        _close(a, b, 2e-5)


_OUTPUTS = ('logp', 'ctx', 'h0n', 'c0n', 'h1n', 'c1n')
_SHARED = {}


def _partial_loss_setup():
    """One decoder, one batch and one weighting per output for all partial-loss cases (built once, never modified)."""
    if not _SHARED:
        B, L = 8, 6
        _SHARED['dec'] = _decoder(9)
        _SHARED['dec64'] = copy.deepcopy(_SHARED['dec']).double().cpu()
        _SHARED['inputs'] = _inputs(B, L, 400)
        _SHARED['g'] = dict(zip(_OUTPUTS, [synth.uniform(s, 410 + i, -1.0, 1.0) for i, s in
                                           enumerate([(B, 1, 11)] + [(B, 512)] * 5)]))
    return _SHARED['dec'], _SHARED['dec64'], _SHARED['inputs'], _SHARED['g']


def _partial_loss_vs_fp64(monkeypatch, loss_of, absent=None):
    """Gradients of loss_of({name: output}) through the fused step (per-layer states in, so that an unused output's
    gradient reaches the step as None -- it does not materialise them) against fp64.  `absent`: the g_* arguments that
    must have reached t2o_decoder_step_bwd as NULL."""
    dec, dec64, (feat, h, c, enc, op), _ = _partial_loss_setup()
    dec.zero_grad(set_to_none=True)
    dec64.zero_grad(set_to_none=True)
    r_in = [t.double().requires_grad_(True) for t in (feat, h, c, enc)]
    logp, (hn, cn), _, ctx = _reference_step(dec64, op, (r_in[1], r_in[2]), r_in[3], r_in[0])
    loss_of(dict(zip(_OUTPUTS, (logp, ctx, hn[0], cn[0], hn[1], cn[1])))).backward()
    hd, cd = h.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
    t_in = [feat.to(DEV).requires_grad_(True), hd, cd, enc.to(DEV).requires_grad_(True)]
    hidden = (list(hd.unbind(0)), list(cd.unbind(0)))
    _must_be_fused(monkeypatch, dec, op.to(DEV), hidden, t_in[3], t_in[0])
    logp2, (hn2, cn2), _, ctx2 = dec.forward_step(op.to(DEV), hidden, t_in[3], t_in[0])
    node = ctx2.grad_fn                                              # the step's autograd node: its argument block outlives backward()
    loss_of(dict(zip(_OUTPUTS, (logp2, ctx2, hn2[0], cn2[0], hn2[1], cn2[1])))).backward()
    if absent is not None:
        assert [n for n in _OUTPUTS if getattr(node.args, 'g_' + n) is None] == list(absent)
    for a, b, name in zip(t_in, r_in, ('feat', 'h', 'c', 'enc')):
        if b.grad is None:
            assert a.grad is None or float(a.grad.abs().max()) == 0.0
        else:
            _close(a.grad, b.grad, 2e-5, 'd ' + name)
    for (name, p), (_, q) in zip(dec.named_parameters(), dec64.named_parameters()):
        if q.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
        else:
            _close(p.grad, q.grad, 2e-5, 'd ' + name)


def test_context_only_and_state_only_gradients(monkeypatch):
    """An episode's last step receives a gradient through its context only; a step whose operator was END may receive
    one through the states only."""
    _partial_loss_vs_fp64(monkeypatch, lambda o: o['ctx'].square().sum(), absent=('logp', 'h0n', 'c0n', 'h1n', 'c1n'))
    # (neither g_logp nor g_ctx: the wrapper hands the step a zero g_ctx)
    _partial_loss_vs_fp64(monkeypatch, lambda o: (o['h0n'] * o['c1n']).sum(), absent=('logp', 'c0n', 'h1n'))


@pytest.mark.parametrize('missing', _OUTPUTS)
def test_each_output_gradient_absent_alone(monkeypatch, missing):
    """A loss over exactly five of the step's six differentiable outputs: the sixth's gradient is NULL in the kernel
    arguments (`a.dh_a ? ...`, `a.dc_next ? ...`, `a.g_ctx ? ...`, no k_dec_logits_bwd without g_logp)."""
    g = _partial_loss_setup()[3]
    _partial_loss_vs_fp64(monkeypatch, lambda o: sum((o[n] * g[n].to(o[n])).sum() for n in _OUTPUTS if n != missing), absent=(missing,))


def test_score_only_gradient(monkeypatch):
    """The loss uses logp alone: d ctx comes from the scores only (g_ctx = NULL) and the states receive nothing."""
    g = _partial_loss_setup()[3]
    _partial_loss_vs_fp64(monkeypatch, lambda o: (o['logp'] * g['logp'].to(o['logp'])).sum(), absent=_OUTPUTS[1:])


def _head_modules(K, D, fc_bias=True, affine=True, track=True, seed=2):
    torch.manual_seed(seed)
    fc, bn = nn.Linear(K, D, bias=fc_bias).to(DEV), nn.BatchNorm1d(D, affine=affine, track_running_stats=track).to(DEV)
    with torch.no_grad():
        if affine:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
        if track:
            bn.running_mean.uniform_(-0.1, 0.1)
            bn.running_var.uniform_(0.5, 1.5)
    return fc, bn


def _head_vs_fp64(monkeypatch, B, K, D, training, fc_bias=True, affine=True, track=True):
    """DS.image_feature against relu(bn(fc(x))) in fp64: the output, every gradient, the running statistics."""
    import t2onet_amd.actor as ACT
    from t2onet_amd import decoder_step as DS
    fc, bn = _head_modules(K, D, fc_bias, affine, track)
    fc64, bn64 = copy.deepcopy(fc).double().cpu(), copy.deepcopy(bn).double().cpu()
    for m in (bn, bn64):
        m.train(training)
    pooled = synth.uniform((B, K), 31, 0.0, 1.0)
    gout = synth.uniform((B, D), 32, -1.0, 1.0)
    x64 = pooled.double().requires_grad_(True)
    ref = F.relu(bn64(fc64(x64)))
    (ref * gout.double()).sum().backward()
    x = pooled.to(DEV).requires_grad_(True)
    assert ACT._FUSED_FEATURE and DS.feature_supported(x, fc, bn)
    monkeypatch.setattr(F, 'batch_norm', lambda *a, **k: pytest.fail('the library batch norm ran'))
    got = DS.image_feature(x, fc, bn)
    # (two rows in training mode: the normalisation divides by half the difference of two nearly equal numbers wherever a
    # column's values are close -- 1 / std up to 1e3 here -- and fp32 rounding of fc's output is amplified accordingly)
    tol = 2e-3 if (training and B == 2) else 3e-5
    _close(got, ref, 3e-6 if tol < 1e-3 else 1e-4)
    (got * gout.to(DEV)).sum().backward()
    _close(x.grad, x64.grad, tol)
    _close(fc.weight.grad, fc64.weight.grad, tol)
    if affine:
        for p, q in ((bn.weight, bn64.weight), (bn.bias, bn64.bias)):
            _close(p.grad, q.grad, tol)
    else:
        assert bn.weight is None and bn.bias is None
    if not fc_bias:
        assert fc.bias is None
    elif training or not track:   # batch statistics remove any shift of the Linear's output: this gradient is zero up to rounding
        # (measured against the batch norm's bias gradient -- the column sums of the gradient that passes the ReLU)
        colsum = bn.bias.grad if affine else (gout.double() * (ref > 0)).sum(0)
        assert float(fc.bias.grad.abs().max()) < (1e-4 if B > 2 else 5e-2) * float(colsum.abs().max()) and float(fc64.bias.grad.abs().max()) < 1e-9
    else:
        _close(fc.bias.grad, fc64.bias.grad, 3e-5)
    if track:               # running statistics exactly as torch updates them
        _close(bn.running_mean, bn64.running_mean, 1e-6)
        _close(bn.running_var, bn64.running_var, 1e-6)
        assert int(bn.num_batches_tracked) == int(bn64.num_batches_tracked) == (1 if training else 0)
    else:
        assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None


@pytest.mark.parametrize('B,training', [(64, True), (8, True), (2, True), (5, False), (1, False)])
def test_feature_head_matches_fp64(monkeypatch, B, training):
    _head_vs_fp64(monkeypatch, B, 512, 512, training)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('B', [16, 17, 32, 33])
def test_feature_head_row_block_thresholds(monkeypatch, B, training):
    """rb_for(): k_dec_feat<1> up to 16 rows, <2> for 17 .. 32 (no other test enters it), <4> from 33."""
    _head_vs_fp64(monkeypatch, B, 512, 512, training)


# (B, K, D): K below one 32-wide chunk and D below one 16-column tile;  a K tail (36 = 32 + 4) with D ending inside its
# second tile;  D = 48 with K over all 16 waves;  K = 100 = 3 chunks + a 4-wide tail.  More than a handful of rows in
# training mode: the batch norm amplifies the rounding of fc's output by 1 / std of a column, which for 2 or 3 rows is
# 1 / (a difference of nearly equal numbers) in some column (the note in _head_vs_fp64).
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('B,K,D', [(5, 4, 4), (7, 36, 20), (9, 512, 48), (6, 100, 512)])
def test_feature_head_k_tails_and_partial_column_tiles(monkeypatch, B, K, D, training):
    _head_vs_fp64(monkeypatch, B, K, D, training)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('fc_bias,affine,track', [(False, True, True), (True, False, True), (True, True, False), (True, False, False),
                                                  (False, False, False)])
def test_feature_head_without_bias_affine_or_running_statistics(monkeypatch, fc_bias, affine, track, training):
    """nn.Linear(bias=False), BatchNorm1d(affine=False), BatchNorm1d(track_running_stats=False) -- which normalises with
    the batch's statistics in eval() too, reads and counts nothing -- and their combinations."""
    _head_vs_fp64(monkeypatch, 6, 36, 20, training, fc_bias, affine, track)


def _tape_vs_autograd(dec, fc, bn, K):
    """A persistent tape (what the Trainer installs): three chained steps + feature heads, weight gradients formed once by
    tape.flush(), against the same chain with private tapes (gradients returned to autograd step by step)."""
    from t2onet_amd import decoder_step as DS
    D, E, V = dec.hidden_size, dec.word_vec_dim, dec.output_size
    B, L, S = 16, 7, 3
    _, h, c, enc, _ = _inputs(B, L, 500, V, D)
    pooled = [synth.uniform((B, K), 510 + s, 0.0, 1.0).to(DEV) for s in range(S)]
    ops = [(synth.uniform((B, 1), 520 + s, 0.0, 1.0) * V).long().clamp(0, V - 1).to(DEV) for s in range(S)]

    class Holder:                                                  # what tape.flush() reads: decoder, vis_encoder.fc, bn1
        pass
    model = Holder()
    model.decoder, model.bn1, model.vis_encoder = dec, bn, Holder()
    model.vis_encoder.fc = fc
    named = list(dec.named_parameters()) + [('fc.' + n, p) for n, p in fc.named_parameters()] + [('bn.' + n, p) for n, p in bn.named_parameters()]
    params = [p for _, p in named]

    def run(tape):
        for p in params:
            p.grad = None
        if bn.track_running_stats:
            bn.reset_running_stats()
        hid = (list(h.to(DEV).unbind(0)), list(c.to(DEV).unbind(0)))
        e = enc.to(DEV).requires_grad_(True)
        loss = 0.0
        for s in range(S):
            assert DS.feature_supported(pooled[s], fc, bn) and DS.step_supported(dec, ops[s], hid, e, pooled[s].new_zeros(B, D))
            feat = DS.image_feature(pooled[s], fc, bn, tape)
            logp, hid, _, ctx = DS.decoder_step(dec, ops[s], hid, e, feat, tape)
            loss = loss + ctx.square().sum() + (logp.sum() * 0.1 if s != 1 else 0.0)     # (step 1: no gradient through its scores)
        loss.backward()
        if tape is not None:
            assert all(p.grad is None for p in params)              # nothing was handed to autograd
            tape.flush(model)
        assert all(p.grad is not None for p in params)
        return [p.grad.clone() for p in params] + [e.grad.clone()]

    ref = run(None)
    tape = DS.DecoderTape(B, D, E, V, K, S + 1, torch.device(DEV), persistent=True)
    got = run(tape)
    names = [n for n, _ in named] + ['enc']
    for a, b, name in zip(got, ref, names):
        if name != 'fc.bias':                                       # (zero in exact arithmetic -- bn removes any shift: rounding noise)
            _close(a, b, 1e-5, name)
    got2 = run(tape)                                                # the tape rewinds: a second train step gives the same
    for a, b, name in zip(got2, ref, names):
        if name != 'fc.bias':
            _close(a, b, 1e-5, name)
    return ref, names


def test_deferred_weight_gradients_equal_per_step_autograd():
    dec = _decoder(11)
    torch.manual_seed(4)
    fc, bn = nn.Linear(512, 512).to(DEV), nn.BatchNorm1d(512).to(DEV)
    _, names = _tape_vs_autograd(dec, fc, bn, 512)
    assert len(names) == 15 + 4 + 1


def test_deferred_weight_gradients_without_biases(monkeypatch):
    """The tape's `p is None` branches: a decoder without any bias, a Linear without one and a batch norm without affine
    parameters through tape.flush() -- against per-step autograd, which in turn is held to fp64 here."""
    dec = _decoder(11, V=11, E=20, D=128, no_bias=('rnn', 'vis', 'lo', 'out'))
    fc, bn = _head_modules(36, 128, fc_bias=False, affine=False, seed=4)
    _, names = _tape_vs_autograd(dec, fc, bn, 36)
    assert len(names) == 8 + 1 + 0 + 1
    _step_vs_fp64(monkeypatch, dec, 16, 7, 500)


def test_zero_grad_between_forward_and_backward_gives_autograd_gradients():
    """The reference's loop (train_seq2seqL1.py:63,86): forward, optimizer.zero_grad() (set_to_none under torch >= 2),
    backward, optimizer.step() with a STOCK optimiser -- every parameter must end up with an ordinary .grad."""
    import t2onet_amd
    from t2onet_amd.actor import Actor
    opt = t2onet_amd.default_options()
    model = Actor(opt).to(DEV)
    model.use_channels_last()
    model.train()
    optim = torch.optim.Adam(model.parameters(), lr=1e-3)
    B = 4
    x = torch.zeros(B, 17, dtype=torch.long)
    x[:, 0], x[:, 1:4], x[:, 4] = 1, 7, 2
    img = synth.images(B, 64, 64, 3).to(DEV)
    for _ in range(2):                                              # (the second pass meets the .grad tensors of the first)
        _, imgs, _, _ = model.episode_forward(x.to(DEV), img, None, reinforce_sample=0)
        loss = (imgs[:, -1] - 0.5).abs().mean()
        optim.zero_grad()
        loss.backward()
        have = [n for n, p in model.named_parameters() if p.grad is not None]
        assert any(n.startswith('vis_encoder.conv1') for n in have) and any(n.startswith('decoder.rnn') for n in have)
        assert any(n.startswith('vis_encoder.fc') for n in have) and any(n.startswith('bn1') for n in have)
        optim.step()
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_argument_validation():
    from t2onet_amd import _lib
    lib = _lib.load()
    a = _lib.DecoderStepArgs()
    assert lib.t2o_decoder_step_fwd(None, None) == 1
    a.B, a.L, a.D, a.E, a.V = 4, 5, 500, 300, 11                    # D % 64 != 0
    assert lib.t2o_decoder_step_fwd(ctypes.byref(a), None) == 1 and b'D % 64' in lib.t2o_last_error()
    a.D = 512
    assert lib.t2o_decoder_step_fwd(ctypes.byref(a), None) == 1 and b'null' in lib.t2o_last_error()
    f = _lib.ImageFeatureArgs()
    f.B, f.K, f.D = 65, 512, 512
    buf = torch.zeros(16, device=DEV)
    for n in ('fc_w', 'pooled', 'fc_out', 'stats', 'feat'):
        setattr(f, n, buf.data_ptr())
    assert lib.t2o_image_feature_fwd(ctypes.byref(f), None) == 1 and b'B <= 64' in lib.t2o_last_error()
    f.B, f.training = 1, 1
    assert lib.t2o_image_feature_fwd(ctypes.byref(f), None) == 1 and b'more than one row' in lib.t2o_last_error()


def _head_args(B, K, D, training=1):
    """An argument block of the feature head's C entry points over fresh tensors (returned with it: it holds raw pointers)."""
    from t2onet_amd import _lib
    t = {'fc_w': synth.uniform((D, K), 61, -0.2, 0.2), 'fc_b': synth.uniform((D,), 62, -0.1, 0.1), 'bn_w': synth.uniform((D,), 63, 0.5, 1.5),
         'bn_b': synth.uniform((D,), 64, -0.3, 0.3), 'pooled': synth.uniform((B, K), 65, 0.0, 1.0), 'g_feat': synth.uniform((B, D), 66, -1.0, 1.0)}
    t = {n: v.to(DEV) for n, v in t.items()}
    for n, shape in (('pooled_copy', (B, K)), ('fc_out', (B, D)), ('stats', (2, D)), ('feat', (B, D)), ('d_fc', (B, D)), ('d_bn', (2, D)),
                     ('d_pooled', (B, K))):
        t[n] = torch.full(shape, 7.0, device=DEV)
    f = _lib.ImageFeatureArgs()
    for n, v in t.items():
        setattr(f, n, v.data_ptr())
    f.momentum, f.eps, f.training, f.B, f.K, f.D = 0.1, 1e-5, training, B, K, D
    return f, t


def test_feature_head_absent_outputs_leave_the_rest_bit_identical():
    """pooled_copy = NULL (no copy for the weight-gradient product) and d_pooled = NULL (a frozen trunk: no data gradient
    product) through the C entry points: everything else is bit-identical to the full call."""
    from t2onet_amd import _lib
    from t2onet_amd.functional import _stream
    lib = _lib.load()
    st = _stream(torch.device(DEV))
    B, K, D = 19, 36, 20                                            # k_dec_feat<2>, a K tail, a partial column tile
    full, tf = _head_args(B, K, D)
    assert lib.t2o_image_feature_fwd(ctypes.byref(full), st) == 0 and lib.t2o_image_feature_bwd(ctypes.byref(full), st) == 0, lib.t2o_last_error()
    assert torch.equal(tf['pooled_copy'], tf['pooled']) and float((tf['d_pooled'] - 7.0).abs().min()) > 0.0
    part, tp = _head_args(B, K, D)
    part.pooled_copy, part.d_pooled = None, None
    assert lib.t2o_image_feature_fwd(ctypes.byref(part), st) == 0 and lib.t2o_image_feature_bwd(ctypes.byref(part), st) == 0, lib.t2o_last_error()
    for n in ('feat', 'fc_out', 'stats', 'd_fc', 'd_bn'):
        assert torch.equal(tp[n], tf[n]), n
    assert float((tp['pooled_copy'] - 7.0).abs().max()) == 0.0 and float((tp['d_pooled'] - 7.0).abs().max()) == 0.0      # untouched


def test_feature_head_refuses_widths_that_are_no_multiple_of_four():
    """D % 4 == 0 is one rule for the forward, the backward and feature_supported (the backward's products read d_fc in
    16-byte pieces): D = 10 is refused by both entry points with the same message, before anything is launched."""
    from t2onet_amd import _lib
    from t2onet_amd import decoder_step as DS
    from t2onet_amd.functional import _stream
    lib = _lib.load()
    st = _stream(torch.device(DEV))
    f, t = _head_args(4, 8, 10)
    assert lib.t2o_image_feature_fwd(ctypes.byref(f), st) == 1
    fwd_msg = lib.t2o_last_error()
    assert b'D % 4 == 0' in fwd_msg
    assert lib.t2o_image_feature_bwd(ctypes.byref(f), st) == 1
    assert lib.t2o_last_error() == fwd_msg
    torch.cuda.synchronize()
    for n in ('fc_out', 'stats', 'feat', 'pooled_copy', 'd_fc', 'd_bn', 'd_pooled'):
        assert float((t[n] - 7.0).abs().max()) == 0.0, n           # nothing ran
    fc, bn = nn.Linear(8, 10).to(DEV), nn.BatchNorm1d(10).to(DEV)
    assert not DS.feature_supported(t['pooled'], fc, bn)
    f12, _t12 = _head_args(4, 8, 12)
    assert lib.t2o_image_feature_fwd(ctypes.byref(f12), st) == 0 and lib.t2o_image_feature_bwd(ctypes.byref(f12), st) == 0, lib.t2o_last_error()
