"""t2o_adam_step (k_adam, t2o_optim.hip) through the C ABI against the same formulas in fp64, evaluated from the fp32 state
and the fp32 hyper-parameters the ABI receives.  Per-element bounds are rounding counts (step_cases.adam_reference); fp32
torch.optim.Adam satisfies them too (tests/test_step_cases_cpu.py: at most 0.50 of any bound).

Twenty consecutive steps against the fp64 trajectory: the kernel's largest error may be 4 x that of fp32 torch.optim.Adam
against the same trajectory, floor 2 ulp of max |p|.  Measured: see test_adam_twenty_steps_against_the_fp64_trajectory.
One step at 8.4 M floats uses 0.31 / 0.58 / 0.50 of the m / v / p bounds."""
import numpy as np
import pytest
import torch

from tests import step_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def adam_abi(bufs, n, step, hp, offset=0):
    import t2onet_amd.functional as T
    from t2onet_amd import _lib
    p, g, m, v = bufs
    return _lib.load().t2o_adam_step(p.data_ptr() + offset, g.data_ptr(), m.data_ptr(), v.data_ptr(), n, hp[0], hp[1], hp[2], hp[3],
                                     step, T._stream(p.device))


def check_one_step(dev, n, step, hp, seed):
    state = sc.adam_state(n, seed)
    bufs = [torch.from_numpy(a).to(dev) for a in state]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    assert adam_abi(bufs, n, step, hp) == 0
    torch.cuda.synchronize()
    p1, m1, v1, bnd = sc.adam_reference(*(a[:n] for a in state), step, hp)
    gp, gg, gm, gv = (b.cpu().numpy() for b in bufs)
    assert np.array_equal(gg, state[1])
    ratios = {}
    for k, got, ref, old in (('m', gm, m1, state[2]), ('v', gv, v1, state[3]), ('p', gp, p1, state[0])):
        assert np.array_equal(got[n:], old[n:]), '%s: an element past n was written' % k            # guard elements
        err = np.abs(got[:n].astype(np.float64) - ref)
        assert np.isfinite(got[:n]).all() and (err <= bnd[k]).all(), (k, n, step, float((err / np.maximum(bnd[k], 1e-300)).max()))
        ratios[k] = float((err / np.maximum(bnd[k], 1e-300))[bnd[k] > 0].max()) if (bnd[k] > 0).any() else 0.0
    still = (state[1][:n] == 0) & (state[2][:n] == 0) & (state[3][:n] == 0)
    assert np.array_equal(gp[:n][still], state[0][:n][still])                                       # m = v = g = 0: p unchanged
    return ratios


@pytest.mark.parametrize('n', sc.ADAM_SIZES)
def test_adam_one_step_tail_sizes(dev, n):
    """Every n % 4, below and above one float4, one workgroup and several; every step count and hyper-parameter set on each."""
    for i, step in enumerate(sc.ADAM_STEPS):
        for j, hp in enumerate(sc.ADAM_HYPERS):
            check_one_step(dev, n, step, hp, 1000 * n + 10 * i + j)


def test_adam_one_step_grid_stride(dev):
    """More than 4 * 4096 * 256 floats: the launch is capped at 4096 workgroups and every thread loops (the training buffer has
    22 M floats: five passes); 2 * 4 * 4096 * 256 + 1203 has two full passes and a 3-float tail."""
    assert sc.ADAM_BIG > 2 * 4 * 4096 * 256 and sc.ADAM_BIG % 4 == 3
    r = check_one_step(dev, sc.ADAM_BIG, 2, sc.ADAM_DEFAULT, 5)
    print('n=%d step 2: error / bound  m %.2f  v %.2f  p %.2f' % (sc.ADAM_BIG, r['m'], r['v'], r['p']))


def test_adam_twenty_steps_against_the_fp64_trajectory(dev):
    """Measured on an MI355X, max |p - p64| after 20 steps for the three hyper-parameter sets: kernel 2.86e-07, 4.41e-07,
    2.73e-07; fp32 torch.optim.Adam on the CPU the same three numbers (the kernel follows its arithmetic); floor 2.38e-07."""
    p0, gs = sc.adam_trajectory_inputs()
    n = p0.size
    for hp in sc.ADAM_HYPERS:
        p64 = sc.adam_trajectory64(p0, gs, hp)
        yard = float(np.abs(sc.adam_trajectory_torch32(p0, gs, hp).astype(np.float64) - p64).max())
        bufs = [torch.from_numpy(p0.copy()).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
        for t, g in enumerate(gs, 1):
            bufs[1].copy_(torch.from_numpy(g))
            assert adam_abi(bufs, n, t, hp) == 0
        err = float(np.abs(bufs[0].cpu().numpy().astype(np.float64) - p64).max())
        floor = 2 * float(np.spacing(np.float32(np.abs(p64).max())))
        print('hp %s: kernel %.3g, torch fp32 %.3g, floor %.3g' % (hp, err, yard, floor))
        assert err <= max(4 * yard, floor)


def test_adam_refusals(dev):
    from t2onet_amd import _lib
    bufs = [torch.ones(16, device=dev) for _ in range(4)]
    assert adam_abi(bufs, 8, 1, sc.ADAM_DEFAULT, offset=4) == 1 and b'aligned' in _lib.load().t2o_last_error()
    assert adam_abi(bufs, 0, 1, sc.ADAM_DEFAULT) == 1
    assert adam_abi(bufs, 8, 0, sc.ADAM_DEFAULT) == 1
    torch.cuda.synchronize()
    assert all(bool((b == 1).all()) for b in bufs)
