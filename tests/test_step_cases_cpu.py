"""The references and inputs of tests/step_cases.py, checked without a GPU: the dyadic head inputs are exact in fp32 and
clear of the LeakyReLU kink, the fp64 head reference is cpu_ref.param_head, the derived forward bounds hold for another
fp32 summation order, fp32 torch.optim.Adam stays inside the Adam bounds, and the small helpers mean what they say."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests import step_cases as sc

U = sc.U


@pytest.mark.parametrize('name', [c[0] for c in sc.HEAD_GRAD_CASES])
def test_dyadic_head_inputs_are_exact_in_fp32_and_clear_of_the_kink(name):
    """Every gradient case: fc1 in fp32, summed in two different orders, equals fp64 bit for bit, and min |pre| >= 2^-15 --
    a property of the inputs (no unit excluded), so fp32 and fp64 agree on every LeakyReLU branch."""
    sd, op_ids, ctx, _, _ = sc.head_grad_case(name)
    x32 = ctx.numpy()
    perm = np.random.default_rng(1).permutation(sc.D)
    for op in sc.HEAD_OPS:
        idx = (op_ids == op).nonzero().flatten().numpy()
        if idx.size == 0:
            continue
        w, b = sd[sc.ATTR[op] + '.fc1.weight'].numpy(), sd[sc.ATTR[op] + '.fc1.bias'].numpy()
        exact = x32[idx].astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
        blas = (x32[idx] @ w.T + b).astype(np.float64)                         # the library's blocked order, bias last
        seq = np.broadcast_to(b, (idx.size, sc.D)).copy()                      # bias first, then a shuffled sequential order
        for j in perm:
            seq += x32[idx, j:j + 1] * w[None, :, j]
        assert seq.dtype == np.float32
        assert np.array_equal(blas, exact) and np.array_equal(seq.astype(np.float64), exact)
        assert np.abs(exact).min() >= 2.0 ** -15
        assert 0.3 < exact.std() < 0.7 or idx.size < 3                         # (the pre-activations are not degenerate)


def test_head_reference_is_cpu_ref_param_head_per_sample():
    sd = sc.default_init_heads(5, 8.0)
    op_ids = sc.op_layout('mixed', 40)
    ctx = sc.random_features(40, 6)
    for consts in (sc.DEFAULT_CONSTS, sc.OTHER_CONSTS):
        ref = sc.heads_reference(sd, op_ids, ctx, consts)
        sd64 = {k: v.double() for k, v in sd.items()}
        for b, op in enumerate(op_ids.tolist()):
            row = np.zeros(sc.PAD)
            if op >= 0 and op != 4:
                row[:sc.N_PARAM[op]] = cpu_ref.param_head(sd64, op, ctx[b:b + 1].double(), sc.opt_of(consts), prefix='').numpy()[0]
            np.testing.assert_allclose(ref['param'][b], row, rtol=0, atol=1e-12)      # (fp64 GEMM order: batched vs one row)
    assert np.abs(ref['param']).max() > 0.5


def test_head_reference_gradients_have_the_stated_structure():
    """Rows of op -1 / 4 and heads nobody selected get exact zeros; dpre is LeakyReLU' times W2^T df; a saturation head with
    W2 = b2 = 0 sits at relu'(0) = 0 on both branches: param, gctx, gW2, gb2 all exactly 0."""
    sd, op_ids, ctx, gout, consts = sc.head_grad_case('b64_mixed')
    sd['saturation_op.fc2.weight'].zero_()
    sd['saturation_op.fc2.bias'].zero_()
    ref = sc.heads_reference(sd, op_ids, ctx, consts, gout)
    none = ((op_ids < 0) | (op_ids == 4)).numpy()
    assert none.any() and not ref['gctx'][none].any() and not ref['dpre'][none].any() and not ref['param'][none].any()
    sat = (op_ids == 2).numpy()
    assert sat.any() and not ref['param'][sat].any() and not ref['gctx'][sat].any()
    assert not ref['gw']['saturation_op.fc2.weight'].any() and not ref['gw']['saturation_op.fc2.bias'].any()
    assert ref['gw']['brightness_op.fc1.weight'].any()
    ref1 = sc.heads_reference(*sc.head_grad_case('b3_all7')[:3], sc.DEFAULT_CONSTS, sc.head_grad_case('b3_all7')[3])
    assert not ref1['gw']['brightness_op.fc1.weight'].any() and ref1['gw']['white_op.fc1.weight'].any()


@pytest.mark.parametrize('scale', [1.0, 8.0])
def test_forward_bounds_hold_for_the_library_order_in_fp32(scale):
    """The derived dot-product bound (K = 12) is a worst case over summation orders no deeper than the kernel's: CPU torch
    fp32 (blocked GEMM order, far shallower than 512 sequential adds) must sit inside it, and not by a factor that would
    make the bound meaningless (the largest ratio is printed)."""
    sd = sc.default_init_heads(11, scale)
    B = 65
    op_ids, ctx = sc.op_layout('mixed', B), sc.random_features(B, 12)
    ref = sc.heads_reference(sd, op_ids, ctx, sc.DEFAULT_CONSTS)
    hid32 = np.zeros((B, sc.D), dtype=np.float32)
    raw32 = np.zeros((B, sc.PAD), dtype=np.float32)
    for op in sc.HEAD_OPS:
        idx = (op_ids == op).nonzero().flatten()
        a = sc.ATTR[op]
        h = F.leaky_relu(F.linear(ctx[idx], sd[a + '.fc1.weight'], sd[a + '.fc1.bias']), 0.01)
        hid32[idx.numpy()] = h.numpy()
        raw32[idx.numpy(), :sc.N_PARAM[op]] = F.linear(h, sd[a + '.fc2.weight'], sd[a + '.fc2.bias']).numpy()
    hid, e_hid, raw, e_raw, e_tot = sc.forward_bounds(sd, op_ids, ctx, hid32)
    np.testing.assert_allclose(hid, ref['hidden'], rtol=0, atol=1e-14)
    r_h = np.abs(hid32 - hid) / np.maximum(e_hid, 1e-300)
    r_r = np.abs(raw32 - raw) / np.maximum(e_raw, 1e-300)
    r_t = np.abs(raw32 - ref['raw']) / np.maximum(e_tot, 1e-300)
    print('scale %g: hidden %.3f  raw %.3f  raw end-to-end %.3f of the bound' % (scale, r_h.max(), r_r.max(), r_t.max()))
    assert r_h.max() <= 1.0 and r_r.max() <= 1.0 and r_t.max() <= 1.0
    assert not e_hid[(op_ids == 4).numpy()].any() and not e_tot[(op_ids < 0).numpy()].any()


def test_regressor_slope_sup_dominates_the_derivative():
    f = np.linspace(-6, 6, 241)
    for consts in (sc.DEFAULT_CONSTS, sc.OTHER_CONSTS):
        for op in sc.HEAD_OPS:
            x = torch.tensor(f, dtype=torch.float64, requires_grad=True)
            cpu_ref.regress(op, x, sc.opt_of(consts)).sum().backward()
            sup = sc.regress_slope_sup(op, f, 0.05, consts)
            assert (sup >= np.abs(x.grad.numpy()) - 1e-12).all(), op
            assert (sup <= {0: consts[0], 2: max(abs(consts[1]), abs(consts[2])), 6: consts[3] / 4, 7: 0.25}.get(op, 1.0) + 1e-12).all(), op
            # and the finite difference over the interval is inside sup * width
            lo, hi = (sc.regress64(op, f + s, consts) for s in (-0.05, 0.05))
            assert (np.abs(hi - lo) <= sup * 0.1 + 1e-12).all(), op


@pytest.mark.parametrize('step', [1, 2, 1000])
def test_fp32_torch_adam_stays_inside_the_adam_bounds(step):
    """The per-element bounds of step_cases.adam_reference are rounding counts; fp32 torch.optim.Adam(foreach=False), a
    different but equally valid fp32 evaluation, must satisfy them too (n = 100003, arbitrary state)."""
    for hp in sc.ADAM_HYPERS:
        p, g, m, v = sc.adam_state(100003, 3 + step)
        p1, m1, v1, bnd = sc.adam_reference(p, g, m, v, step, hp)
        tp, tm, tv = sc.torch_adam_step(p, g, m, v, step, hp)
        ratios = {k: float((np.abs(t.astype(np.float64) - r) / np.maximum(bnd[k], 1e-300))[bnd[k] > 0].max())
                  for k, t, r in (('m', tm, m1), ('v', tv, v1), ('p', tp, p1))}
        print('step %d hp %s: error / bound  m %.2f  v %.2f  p %.2f' % (step, hp, ratios['m'], ratios['v'], ratios['p']))
        for k, t, r in (('m', tm, m1), ('v', tv, v1), ('p', tp, p1)):
            assert (np.abs(t.astype(np.float64) - r) <= bnd[k]).all(), (k, ratios)
        still = (g == 0) & (m == 0) & (v == 0)
        assert still.sum() > 1000 and np.array_equal(tp[still], p[still]) and np.array_equal(p1[still], p[still].astype(np.float64))


def test_adam_hyper_parameters_are_the_fp32_values():
    lr, b1, b2, eps = sc.ADAM_DEFAULT
    assert b2 == float(np.float32(0.999)) and b2 != 0.999
    assert float(np.float32(1.0) - np.float32(b2)) == 1.0 - b2                   # 1 - beta2 is exact in fp32
    assert abs((1.0 - b2) / 0.001 - 1.0) > 1e-5                                  # ... and 1.3e-5 off the decimal 0.001


def test_adam_trajectory_yardstick():
    p0, gs = sc.adam_trajectory_inputs()
    p64 = sc.adam_trajectory64(p0, gs, sc.ADAM_DEFAULT)
    p32 = sc.adam_trajectory_torch32(p0, gs, sc.ADAM_DEFAULT)
    err = float(np.abs(p32.astype(np.float64) - p64).max())
    print('fp32 torch Adam after %d steps: max error %.3g (%.2f ulp of max |p|)' % (sc.TRAJ_STEPS, err, err / np.spacing(np.float32(np.abs(p64).max()))))
    assert 0 < err < 1e-5 and np.abs(p64 - p0).max() > 5e-3                      # it moved by >> the error


def test_l1_helpers():
    for n in (1, 5, 4097):
        p, t = sc.l1_pair(n, n)
        want = F.l1_loss(torch.from_numpy(p).double(), torch.from_numpy(t).double()).item()
        assert abs(sc.l1_loss64(p, t) - want) <= 1e-15
        g = sc.l1_grad32(p, t, 3.0)
        assert g.dtype == np.float32 and np.array_equal(g == 0, p == t)
        assert np.array_equal(np.sign(g), np.sign(p.astype(np.float64) - t.astype(np.float64)))
        nz = g[g != 0]
        assert nz.size == 0 or np.abs(np.abs(nz).astype(np.float64) * n / 3.0 - 1).max() <= 3 * U
    assert (sc.l1_pair(4097, 1)[0] == sc.l1_pair(4097, 1)[1]).sum() > 100       # ties are there


@pytest.mark.parametrize('name', [c[0] for c in sc.END_CASES])
def test_end_cases_are_what_they_claim(name):
    _, B, T, shape, _ = next(c for c in sc.END_CASES if c[0] == name)
    imgs, first, tgt = sc.end_case(name)
    assert len(imgs) == T and first.shape == (B,) and first.min() >= 0 and first.max() < T
    pred = sc.end_gather(imgs, first)
    assert pred.shape == tgt.shape == (B,) + shape
    assert B == 1 or np.array_equal(pred[0], tgt[0])
    # every case has something to get wrong: a non-zero loss, non-zero expected gradients, and ties
    g = sc.l1_grad32(pred, tgt, 3.0)
    assert sc.l1_loss64(pred, tgt) > 0.05 and (g != 0).mean() > 0.9 * max(B - 1, 1) / B and (g == 0).any()
    for b in range(B):
        assert np.array_equal(pred[b], imgs[first[b]][b])
    rest = slice(1, None) if B > 1 else slice(None)
    assert (pred[rest] != tgt[rest]).mean() > 0.9 and (pred[rest] == tgt[rest]).sum() > 0


def test_end_cases_cover_one_sample_and_every_step_count():
    shapes = {(B, T) for _, B, T, _, _ in sc.END_CASES}
    assert {(1, 1), (1, 8)} <= shapes and {T for _, T in shapes} >= {1, 2, 8}
    assert max(-(-B * int(np.prod(s)) // 2048) for _, B, _, s, _ in sc.END_CASES) <= 384      # nblk of the bound's comment
    assert max(-(-n // (8192 if n % 4 == 0 else 2048)) for n in sc.L1_SIZES) == 384


def test_fill_bytes_is_the_memset_node_semantics():
    buf = np.full(40, 0xEE, dtype=np.uint8)
    sc.fill_bytes(buf, 3, 0x11223344, 2, 3, height=2, pitch=16)
    want = np.full(40, 0xEE, dtype=np.uint8)
    want[3:9] = [0x44, 0x33] * 3
    want[19:25] = [0x44, 0x33] * 3
    assert np.array_equal(buf, want)
    sc.fill_bytes(buf, 0, 0x1A7, 1, 5)
    assert buf[:5].tolist() == [0xA7] * 5 and buf[5] == 0x44
