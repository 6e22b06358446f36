"""The operators' parameter heads (t2o_param_heads_fwd / _bwd_acc, t2o_heads.hip) against the fp64 reference of
tests/step_cases.py, through the C ABI so that hidden, raw and dpre are seen as well.

Forward, random fp32 inputs: every layer inside a bound DERIVED from the kernel's summation depth (step_cases.K_DOT).
Gradients, dyadic inputs (fc1 exact in fp32, no unit on the LeakyReLU kink -- tests/test_step_cases_cpu.py): per tensor,
max |error| / max |fp64| at most 4 x the same figure of the library path (Executor.predict_params_gemm, the reference's own
fp32 arithmetic) on the same inputs, floor 64 u: the 4 x covers the other summation order, the floor tensors the library
happens to get exact.  Both figures as measured on an MI355X are in GRAD_FIGURES."""
import numpy as np
import pytest
import torch

from tests import step_cases as sc

pytestmark = pytest.mark.gpu
U = sc.U

# case: (fused, library) largest relative error over gctx, dpre and the 28 head gradients, in units of u, as measured on an
# MI355X with this file (the assertion recomputes the library's figure on every run, tensor by tensor; these are the
# record).  b128_mixed: the one-element brightness_op.fc2.bias gradient is a sum of 20 terms of either sign that cancels to
# 0.0125 from sum |term| = 11.4 -- both paths lose the same three digits there (fused 421 u, library 140 u on that tensor;
# the next largest tensor of that case: 11 u).
GRAD_FIGURES = {
    'b1': (2.5, 5.8), 'b64_mixed': (3.3, 12.8), 'b65_run6': (4.6, 13.5), 'b128_mixed': (421.1, 140.4), 'b130_run3': (24.3, 13.7),
    'b130_run2': (6.3, 10.6), 'b9_none': (0.0, 0.0), 'b3_all0': (4.6, 3.8), 'b3_all1': (3.0, 5.5), 'b3_all2': (3.4, 3.9),
    'b3_all3': (3.0, 5.5), 'b3_all5': (2.6, 5.1), 'b3_all6': (5.7, 4.4), 'b3_all7': (4.5, 4.8),
}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _tables(tensors):
    import t2onet_amd.functional as T
    return [T._ptr_table({op: tensors[sc.ATTR[op] + '.' + key] for op in sc.HEAD_OPS}) for key in sc.HEAD_KEYS]


def fused(sd, op_ids, ctx, gout, consts, dev, accumulate=0, into=None):
    """Forward + backward through the C ABI on buffers pre-filled with NaN (an element the kernels skip shows).  into: the
    gradient tensors to write / add to.  -> dict of CPU numpy arrays: hidden, raw, param, gctx, dpre, gw{...}."""
    import t2onet_amd.functional as T
    from t2onet_amd import _lib
    lib = _lib.load()
    B = ctx.shape[0]
    w = {k: v.to(dev).contiguous() for k, v in sd.items()}
    ids, x = op_ids.to(dev), ctx.to(dev).contiguous()
    nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    hidden, raw, param = nan(B, sc.D), nan(B, sc.PAD), nan(B, sc.PAD)
    wt = _tables(w)
    c = [float(v) for v in consts]
    st = T._stream(dev)
    rc = lib.t2o_param_heads_fwd(ids.data_ptr(), x.data_ptr(), wt[0], wt[1], wt[2], wt[3], hidden.data_ptr(), raw.data_ptr(),
                                 param.data_ptr(), c[0], c[1], c[2], c[3], B, sc.D, st)
    _lib.check(rc, 't2o_param_heads_fwd')
    out = dict(hidden=hidden, raw=raw, param=param)
    if gout is not None:
        g = gout.to(dev).contiguous()
        gw = into if into is not None else {k: torch.full_like(v, float('nan')) for k, v in w.items()}
        gt = _tables(gw)
        gctx, dpre = nan(B, sc.D), nan(B, sc.D)
        rc = lib.t2o_param_heads_bwd_acc(ids.data_ptr(), x.data_ptr(), wt[0], wt[1], wt[2], wt[3], hidden.data_ptr(), raw.data_ptr(),
                                         g.data_ptr(), gctx.data_ptr(), dpre.data_ptr(), gt[0], gt[1], gt[2], gt[3],
                                         c[0], c[1], c[2], c[3], B, sc.D, accumulate, st)
        _lib.check(rc, 't2o_param_heads_bwd_acc')
        out.update(gctx=gctx, dpre=dpre)
        out['gw'] = {k: v.cpu().numpy() for k, v in gw.items()}
    torch.cuda.synchronize()
    return {k: (v if k == 'gw' else v.cpu().numpy()) for k, v in out.items()}


def library(sd, op_ids, ctx, gout, consts, dev):
    """The same heads through Executor.predict_params_gemm (library GEMMs on the whole batch + gather) and torch autograd in
    fp32 on the GPU; dpre from the same modules run on each operator's own rows."""
    import t2onet_amd
    opt = t2onet_amd.default_options(brightness_range=consts[0], saturation_range=(consts[1], consts[2]), sharpness_range=consts[3])
    ex = t2onet_amd.Executor(opt).to(dev)
    missing = ex.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and all('inpaint' in k for k in missing.missing_keys)
    ids = op_ids.to(dev)
    f = ctx.to(dev).requires_grad_(True)
    g = gout.to(dev)
    p = ex.predict_params_gemm(ids, f)
    (p * g).sum().backward()
    named = dict(ex.named_parameters())
    out = dict(param=p.detach().cpu().numpy(), gctx=f.grad.cpu().numpy(),
               gw={k: (torch.zeros_like(named[k]) if named[k].grad is None else named[k].grad).cpu().numpy() for k in sd})
    dpre = torch.zeros(ctx.shape[0], sc.D, device=dev)
    for op in sc.HEAD_OPS:
        idx = (ids == op).nonzero().flatten()
        if idx.numel() == 0:
            continue
        Op = ex.ops[op]
        pre = Op.fc1(ctx.to(dev)[idx])
        pre.retain_grad()
        par = Op.op_param_regressor(Op.fc2(torch.nn.functional.leaky_relu(pre, 0.01)))
        (par * g[idx, :par.shape[1]]).sum().backward()
        dpre[idx] = pre.grad
    out['dpre'] = dpre.cpu().numpy()
    return out


def rel_errors(got, ref):
    """{tensor: max |got - ref| / max |ref|}; a tensor whose fp64 reference is all zero must be exactly zero (-> 0.0)."""
    errs = {}
    pairs = [('gctx', got['gctx'], ref['gctx']), ('dpre', got['dpre'], ref['dpre'])] + [(k, got['gw'][k], ref['gw'][k]) for k in ref['gw']]
    for name, a, r in pairs:
        assert a.shape == r.shape and np.isfinite(a).all(), name
        top = np.abs(r).max()
        if top == 0.0:
            assert not a.any(), '%s: the reference is exactly zero, the kernel wrote %g' % (name, np.abs(a).max())
            errs[name] = 0.0
        else:
            errs[name] = float(np.abs(a.astype(np.float64) - r).max() / top)
    return errs


@pytest.mark.parametrize('name', [c[0] for c in sc.HEAD_GRAD_CASES])
def test_head_gradients_against_fp64_with_the_library_path_as_yardstick(dev, name):
    sd, op_ids, ctx, gout, consts = sc.head_grad_case(name)
    ref = sc.heads_reference(sd, op_ids, ctx, consts, gout)
    got = fused(sd, op_ids, ctx, gout, consts, dev)
    # fc1 is exact on these inputs: hidden of every unit with pre > 0 IS the fp64 value; below zero one product with 0.01f
    pos = ref['pre'] > 0
    assert np.array_equal(got['hidden'][pos].astype(np.float64), ref['pre'][pos]), 'a mis-indexed row, slice or column'
    neg = ~pos
    assert (np.abs(got['hidden'][neg] - ref['hidden'][neg]) <= 2 * U * np.abs(ref['hidden'][neg])).all()
    none = ((op_ids < 0) | (op_ids == 4)).numpy()
    for k in ('hidden', 'raw', 'param', 'gctx', 'dpre'):
        assert not got[k][none].any(), k                                                  # identity / inpaint rows: zeros
    # forward: raw from exact fc1 -> one dot product's bound; param through the regressor
    _, _, raw_h, e_raw, e_tot = sc.forward_bounds(sd, op_ids, ctx, got['hidden'])
    assert (np.abs(got['raw'] - raw_h) <= e_raw).all()
    for op in sc.HEAD_OPS:
        rows = (op_ids == op).numpy()
        n = sc.N_PARAM[op]
        assert (np.abs(got['param'][rows, :n] - ref['param'][rows, :n])
                <= sc.param_bound_end_to_end(op, ref['raw'][rows, :n], e_tot[rows, :n], consts)).all(), op
        assert not got['param'][rows, n:].any() and not got['raw'][rows, n:].any()
    # gradients: 4 x the library path's error against the same fp64, floor 64 u
    lib = library(sd, op_ids, ctx, gout, consts, dev)
    e_f, e_l = rel_errors(got, ref), rel_errors(lib, ref)
    worst = max(e_f, key=lambda k: e_f[k] / max(4 * e_l[k], 64 * U))
    print('%s: fused max %.1f u (next %.1f u), library max %.1f u; tightest %s: fused %.1f u vs library %.1f u'
          % (name, max(e_f.values()) / U, sorted(e_f.values())[-2] / U, max(e_l.values()) / U, worst, e_f[worst] / U, e_l[worst] / U))
    for k in e_f:
        assert e_f[k] <= max(4 * e_l[k], 64 * U), '%s: fused %.1f u, library %.1f u' % (k, e_f[k] / U, e_l[k] / U)
    # determinism: a second run gives the same bits
    again = fused(sd, op_ids, ctx, gout, consts, dev)
    for k in ('hidden', 'raw', 'param', 'gctx', 'dpre'):
        assert np.array_equal(got[k], again[k]), k
    for k in got['gw']:
        assert np.array_equal(got['gw'][k], again['gw'][k]), k


@pytest.mark.parametrize('scale,B,layout,consts', [(1.0, 130, 'mixed', sc.DEFAULT_CONSTS), (8.0, 130, 'run5', sc.OTHER_CONSTS),
                                                   (8.0, 65, 'run0', sc.DEFAULT_CONSTS), (8.0, 1, 'all2', sc.OTHER_CONSTS),
                                                   (1.0, 64, 'run7', sc.OTHER_CONSTS), (8.0, 128, 'mixed', sc.DEFAULT_CONSTS)])
def test_head_forward_on_random_inputs_inside_the_derived_bounds(dev, scale, B, layout, consts):
    """Default-initialised weights (x1: raw stays small; x8: the regressors bend), random features: hidden against fp64 fc1,
    raw against fp64 fc2 of the kernel's own hidden, param against the fp64 regressor of the kernel's own raw, and param end
    to end against the all-fp64 head through the regressor's derivative."""
    sd = sc.default_init_heads(21 + B, scale)
    op_ids, ctx = sc.op_layout(layout, B), sc.random_features(B, 22 + B)
    ref = sc.heads_reference(sd, op_ids, ctx, consts)
    got = fused(sd, op_ids, ctx, None, consts, dev)
    hid, e_hid, raw_h, e_raw, e_tot = sc.forward_bounds(sd, op_ids, ctx, got['hidden'])
    for k in ('hidden', 'raw', 'param'):
        assert np.isfinite(got[k]).all(), k
    r = [float((np.abs(a - b) / np.maximum(e, 1e-300))[e > 0].max()) if (e > 0).any() else 0.0
         for a, b, e in ((got['hidden'], hid, e_hid), (got['raw'], raw_h, e_raw), (got['raw'], ref['raw'], e_tot))]
    print('x%g B=%d %s: hidden %.3f, raw %.3f, raw end to end %.3f of the bound' % (scale, B, layout, r[0], r[1], r[2]))
    assert (np.abs(got['hidden'] - hid) <= e_hid).all()
    assert (np.abs(got['raw'] - raw_h) <= e_raw).all()
    assert (np.abs(got['raw'] - ref['raw']) <= e_tot).all()
    for op in list(sc.HEAD_OPS) + [-1, 4]:
        rows = (op_ids == op).numpy()
        if not rows.any():
            continue
        if op in (-1, 4):
            assert not got['param'][rows].any() and not got['raw'][rows].any() and not got['hidden'][rows].any()
            continue
        n = sc.N_PARAM[op]
        own = sc.regress64(op, got['raw'][rows, :n].astype(np.float64), consts)
        assert (np.abs(got['param'][rows, :n] - own) <= sc.param_bound(op, consts)).all(), op
        assert (np.abs(got['param'][rows, :n] - ref['param'][rows, :n])
                <= sc.param_bound_end_to_end(op, ref['raw'][rows, :n], e_tot[rows, :n], consts)).all(), op
        assert not got['param'][rows, n:].any() and not got['raw'][rows, n:].any()


def test_saturation_head_at_raw_zero_has_exact_zero_gradients(dev):
    """op 2 with W2 = 0, b2 = 0: raw = 0 sits on the f == 0 branch of the saturation regressor (relu'(0) = 0 on both sides):
    param 0 and gctx of those rows, gW2, gb2 (and through dpre = 0: gW1, gb1) exactly 0; the other heads are untouched."""
    sd, op_ids, ctx, gout, consts = sc.head_grad_case('b130_run2')
    sd['saturation_op.fc2.weight'].zero_()
    sd['saturation_op.fc2.bias'].zero_()
    ref = sc.heads_reference(sd, op_ids, ctx, consts, gout)
    got = fused(sd, op_ids, ctx, gout, consts, dev)
    sat = (op_ids == 2).numpy()
    assert sat.sum() > 64
    for k in ('raw', 'param', 'gctx', 'dpre'):
        assert not got[k][sat].any(), k
    for key in sc.HEAD_KEYS:
        assert not got['gw']['saturation_op.' + key].any(), key
    e = rel_errors(got, ref)
    assert max(e.values()) <= 64 * U and e['brightness_op.fc1.weight'] > 0, e


@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_regressors_saturated_at_raw_30_stay_finite(dev, sign):
    """raw = +-30 (+- 1.2) on the tanh / sigmoid heads: expf(30) must not turn into inf / inf or 0 * inf.  Outputs finite
    and at the fp64 value; the gradients through a regressor whose slope is below exp(-28) are below 1e-9 in fp64 and
    must be finite and as small here (the fp32 slope is exactly 0 or a few 1e-13)."""
    B = 10
    sd = sc.dyadic_heads(7)
    for op in (0, 1, 2, 6, 7):
        sd[sc.ATTR[op] + '.fc2.bias'].fill_(30.0 * sign)
    op_ids = torch.tensor([0, 1, 2, 6, 7] * 2, dtype=torch.int32)
    ctx, gout, consts = sc.dyadic_features(B, 8), sc.gout_of(B, 9), sc.OTHER_CONSTS
    ref = sc.heads_reference(sd, op_ids, ctx, consts, gout)
    got = fused(sd, op_ids, ctx, gout, consts, dev)
    assert np.abs(ref['raw'][:, 0]).min() > 28 and np.abs(ref['raw'][:, 0]).max() < 32
    for k in ('hidden', 'raw', 'param', 'gctx', 'dpre'):
        assert np.isfinite(got[k]).all(), k
    for b, op in enumerate(op_ids.tolist()):
        assert abs(got['param'][b, 0] - ref['param'][b, 0]) <= sc.param_bound(op, consts) + 1e-12, (op, got['param'][b, 0])
    for k in ('gctx', 'dpre'):
        assert np.abs(ref[k]).max() < 1e-9 and np.abs(got[k]).max() < 1e-9, k
    for k, v in got['gw'].items():
        assert np.isfinite(v).all() and np.abs(v).max() < 1e-9 and np.abs(ref['gw'][k]).max() < 1e-9, k


def test_accumulate_twice_is_twice_the_plain_gradient(dev):
    """accumulate = 1 adds into the gradient tensors (every element has one writer): from zeros, two backward calls leave
    exactly 2 x the accumulate = 0 result, bit for bit; gctx and dpre are written, not added."""
    sd, op_ids, ctx, gout, consts = sc.head_grad_case('b65_run6')
    plain = fused(sd, op_ids, ctx, gout, consts, dev)
    acc = {k: torch.zeros_like(v, device=dev) for k, v in sd.items()}
    fused(sd, op_ids, ctx, gout, consts, dev, accumulate=1, into=acc)
    twice = fused(sd, op_ids, ctx, gout, consts, dev, accumulate=1, into=acc)
    assert np.array_equal(twice['gctx'], plain['gctx']) and np.array_equal(twice['dpre'], plain['dpre'])
    for k in plain['gw']:
        assert np.array_equal(twice['gw'][k], 2 * plain['gw'][k]), k
    assert plain['gw']['sharpness_op.fc1.weight'].any() and not plain['gw']['white_op.fc2.weight'].any()
