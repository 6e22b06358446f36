"""The sampled operator choice of the free-running decode: k_choose_op (t2o_choose_op, functional.choose_op) against a
plain numpy float64 restatement of models/actor.py:222-236 with actor.sample_categorical's inverse-CDF draw, then the
same choice seen from Actor.episode_forward(reinforce_sample=1) and from the captured whole-step graph.

The kernel sums in fp32, the restatement in fp64, so every input is BUILT to have one answer: draws aimed inside a
category keep 2e-5 from its edges (the fp32 running sum over n <= 32 terms is off by at most ~32 * 2^-24 = 2e-6), exact
boundaries use weights and thresholds that are dyadic fractions.  The conditions on the inputs (margins, the frequency
test's seed, ambiguity caps) are asserted on the restatement alone in tests without the `gpu` mark, and again by the
GPU tests before they look at the kernel.  No case is excluded at run time.

Every kernel call of this file goes through check_outputs(): pred_op (B,1) int64, exec_op (B) int32 == pred_op - 3,
op_mask afterwards == op_mask before with exactly the chosen entry cleared, never a masked operator in a row that has a
live one, index 0 in a row that has none."""
import functools

import numpy as np
import pytest
import torch

from t2onet_amd.actor import OP_MASK

gpu = pytest.mark.gpu
U_TOP = float(np.float32(1.0) - np.float32(2.0 ** -24))        # the largest fp32 below 1
FRACTIONS = (0.02, 0.5, 0.98)
EXPLORES = (0.0, 0.05, 1.0)
AMBIGUOUS = 1e-5
NEG_INF = float('-inf')


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
def probabilities(lp, m, e):
    """p = (exp(lp) (1 - e) + e) m, p /= (sum p + 1e-30), in float64.  lp: the fp32 values the kernel reads."""
    m = np.asarray(m, np.float64)
    lp = np.asarray(lp, np.float64).reshape(m.shape)
    e = float(np.float32(e))                                   # the C ABI takes the exploration floor as a float
    with np.errstate(under='ignore'):
        p = (np.exp(lp) * (1.0 - e) + e) * m
    return p / (p.sum(1, keepdims=True) + 1e-30)


def restate(lp, m, e, u=None):
    """The choice per row: with u the first index whose cumulative weight exceeds u * sum p, the arg-max if none does;
    without u the first maximal index."""
    p = probabilities(lp, m, e)
    best = p.argmax(1)
    if u is None:
        return best
    cdf = np.cumsum(p, 1)
    idx = (cdf <= np.asarray(u, np.float64).reshape(-1, 1) * cdf[:, -1:]).sum(1)
    return np.where(idx >= p.shape[1], best, idx)


def boundary_distance(lp, m, e, u):
    """min_k |u * sum p - cdf_k| per row."""
    cdf = np.cumsum(probabilities(lp, m, e), 1)
    return np.abs(cdf - np.asarray(u, np.float64).reshape(-1, 1) * cdf[:, -1:]).min(1)


def neighbours(lp_row, m_row, e, u, tol=AMBIGUOUS):
    """The live categories within tol of the threshold of one row: the two beside the boundary an ambiguous draw sits on."""
    p = probabilities(lp_row[None], m_row[None], e)[0]
    live = np.flatnonzero(np.asarray(m_row) > 0)
    cl = np.cumsum(p[live])
    thr = float(u) * cl[-1]
    lo = min(int((cl <= thr - tol).sum()), len(live) - 1)
    hi = min(int((cl <= thr + tol).sum()), len(live) - 1)
    return set(int(k) for k in live[lo:hi + 1])


def log_softmax(v):
    v = np.asarray(v, np.float64)
    return (v - np.log(np.exp(v).sum(-1, keepdims=True))).astype(np.float32)


def interior_targets(lp, m, e):
    """Every live category k with p_k >= 1e-3 of every row, three times: u = (cdf_{k-1} + f p_k) / sum p, computed in
    float64 and rounded to fp32.  Returns (row index, k, u) arrays."""
    p = probabilities(lp, m, e)
    cdf = np.cumsum(p, 1)
    rows, ks, us = [], [], []
    for r in range(p.shape[0]):
        for k in range(p.shape[1]):
            if m[r, k] > 0 and p[r, k] >= 1e-3:
                for f in FRACTIONS:
                    rows.append(r), ks.append(k), us.append((cdf[r, k] - p[r, k] + f * p[r, k]) / cdf[r, -1])
    return np.array(rows), np.array(ks), np.array(us, np.float64).astype(np.float32)


def random_masks(rng, R, n):
    m = rng.integers(0, 2, (R, n)).astype(np.float32)
    for r in range(R):
        while m[r].sum() < min(2, n):
            m[r, rng.integers(0, n)] = 1.0
    return m


def expand(lp, m, e, at_least=300):
    """The interior targets of the rows, one sample each, tiled to at_least samples: (lp, m, u, k) per sample."""
    rows, k, u = interior_targets(lp, m, e)
    reps = -(-at_least // len(rows))
    rows, k, u = np.tile(rows, reps), np.tile(k, reps), np.tile(u, reps)
    return np.ascontiguousarray(lp[rows]), np.ascontiguousarray(m[rows]), u, k


@functools.lru_cache(None)
def interior_case(n, e):
    rng = np.random.default_rng(1000 + 37 * n + int(round(100 * e)))
    R = {1: 2, 2: 8, 11: 10, 32: 6}[n]
    spread = np.where(np.arange(R) % 2, 8.0, 1.0)[:, None]     # odd rows: probabilities over three decades, down to the 1e-3 floor
    lp = log_softmax(rng.random((R, n)) * spread)
    m = random_masks(rng, R, n)
    if n >= 11:
        m[0, 0] = m[0, -1] = 0.0                               # masked entries before the first and after the last live one
        m[0, 1:3] = 1.0
        m[1, :3] = 1.0                                         # ids below 3: negative executor indices
    if n == 11:
        m[2] = OP_MASK
    return expand(lp, m, e)


@functools.lru_cache(None)
def extreme_case(e):
    """logp = -inf and -1e4 on live entries (weight 0 at e = 0, weight e otherwise), one of them between two positive
    ones; a row with all its mass on one entry."""
    rng = np.random.default_rng(77)
    lp = log_softmax(rng.random((6, 11)))
    lp[:, 4] = NEG_INF
    lp[:, 6] = -1e4
    lp[3, 0] = lp[3, 10] = NEG_INF
    lp[5, :] = NEG_INF
    lp[5, 7] = 0.0
    m = np.ones((6, 11), np.float32)
    m[1] = OP_MASK
    m[2, 5] = 0.0                                              # live zero-weight 4 and 6 around a masked entry
    return expand(lp, m, e)


def check_interior_inputs(lp, m, e, u, k):
    """The restatement run on the fp32-rounded u still returns the targeted category, 1.9e-5 (2e-5 less the rounding
    of u) from the nearest boundary."""
    assert len(k) >= 300 and np.array_equal(restate(lp, m, e, u), k)
    assert float(boundary_distance(lp, m, e, u).min()) >= 1.9e-5
    assert bool((m[np.arange(len(k)), k] == 1).all())


@pytest.mark.parametrize('e', EXPLORES)
@pytest.mark.parametrize('n', [1, 2, 11, 32])
def test_interior_inputs_are_unambiguous(n, e):
    lp, m, u, k = interior_case(n, e)
    check_interior_inputs(lp, m, e, u, k)
    assert k.min() == 0 and k.max() == n - 1                   # ids below 3 (negative executor indices) up to the last one


@pytest.mark.parametrize('e', EXPLORES)
def test_extreme_inputs_are_unambiguous(e):
    lp, m, u, k = extreme_case(e)
    check_interior_inputs(lp, m, e, u, k)
    zero_weight = np.isin(k, (4, 6)) | ((lp[np.arange(len(k)), k] == NEG_INF))
    assert bool(zero_weight.any()) == (e > 0)                  # weight e: targeted; weight 0: never a target
    if e == 0:
        assert set(k[np.all(lp[:, [0, 1]] == NEG_INF, 1)]) == {7}      # the one-entry row


# ---------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------
def dev():
    return torch.device('cuda:0')


def check_outputs(pred, exe, before, after):
    B, n = before.shape
    assert tuple(pred.shape) == (B, 1) and pred.dtype == torch.int64
    assert tuple(exe.shape) == (B,) and exe.dtype == torch.int32
    assert bool(((pred >= 0) & (pred < n)).all())
    assert torch.equal(exe, (pred.view(-1) - 3).to(torch.int32))
    assert torch.equal(after, before.clone().scatter_(1, pred, 0.0))
    has_live = before.sum(1) > 0
    chosen_was = before.gather(1, pred).view(-1)
    assert bool((chosen_was[has_live] == 1).all()), 'a masked operator was chosen'
    assert bool((pred.view(-1)[~has_live] == 0).all())


def choose(lp, m, e, u=None, sample=True):
    """functional.choose_op on numpy inputs; the outputs and the mask update are checked, the choices returned."""
    import t2onet_amd.functional as T
    lp_t = torch.tensor(np.asarray(lp, np.float32), device=dev())          # copies: the cases are shared between tests
    m_t = torch.tensor(np.asarray(m, np.float32), device=dev())
    u_t = None if u is None else torch.tensor(np.asarray(u, np.float32), device=dev())
    before = m_t.clone()
    pred, exe = T.choose_op(lp_t, m_t, e, sample, u_t)
    check_outputs(pred, exe, before, m_t)
    return pred.view(-1).cpu().numpy()


def batch_sizes(total):
    return (1, 63, 64, 65, total)                              # one thread, the wave edge, two workgroups, several


@gpu
@pytest.mark.parametrize('e', EXPLORES)
@pytest.mark.parametrize('n', [1, 2, 11, 32])
def test_interior_draws_hit_every_category(n, e):
    lp, m, u, k = interior_case(n, e)
    check_interior_inputs(lp, m, e, u, k)
    for B in batch_sizes(len(k)):
        got = choose(lp[:B], m[:B], e, u[:B])
        assert np.array_equal(got, k[:B]), (B, np.flatnonzero(got != k[:B])[:8])


@gpu
@pytest.mark.parametrize('e', EXPLORES)
def test_extreme_log_probabilities(e):
    lp, m, u, k = extreme_case(e)
    check_interior_inputs(lp, m, e, u, k)
    got = choose(lp, m, e, u)
    assert np.array_equal(got, k), np.flatnonzero(got != k)[:8]


def boundary_cases():
    """explore = 1: the weights are the mask itself; 2, 4, 8, 16 live entries: every cumulative value and u = j / count are
    exact in fp32 and in float64.  u = j / count is the j-th boundary: a cumulative weight equal to the threshold does not
    exceed it, so the (j+1)-th live entry is drawn.  Masked entries lead and trail each row."""
    rng = np.random.default_rng(5)
    lps, ms, us, ks = [], [], [], []
    for n, count in [(4, 2), (11, 4), (11, 8), (32, 8), (32, 16), (20, 16)]:
        for trial in range(2):
            live = np.sort(rng.choice(np.arange(1, n - 1), count, replace=False))
            m = np.zeros(32, np.float32)
            m[live] = 1.0
            lp = np.full(32, NEG_INF, np.float32)
            lp[:n] = log_softmax(rng.random(n))
            for j in range(count):
                lps.append(lp), ms.append(m), us.append(j / count), ks.append(live[j])
            lps.append(lp), ms.append(m), us.append(U_TOP), ks.append(live[-1])
    return np.stack(lps), np.stack(ms), np.array(us, np.float32), np.array(ks)


def test_boundary_inputs_are_exact():
    lp, m, u, k = boundary_cases()
    steps = u.astype(np.float64) * m.sum(1)                    # u = j / count exactly, or the largest fp32 below 1
    assert bool(((steps == np.round(steps)) | (u == np.float32(U_TOP))).all())
    assert np.array_equal(restate(lp, m, 1.0, u), k)
    assert bool((m[:, 0] == 0).all() and (m[np.arange(len(k)), k] == 1).all())
    op = np.array([OP_MASK] * 2, np.float32)
    assert list(restate(np.zeros((2, 11)), op, 1.0, np.array([0.0, U_TOP]))) == [2, 9]


@gpu
def test_exact_boundaries_take_the_next_live_entry():
    lp, m, u, k = boundary_cases()
    assert np.array_equal(choose(lp, m, 1.0, u), k)            # rows padded to n = 32 with masked entries
    for n in (4, 11, 20):                                      # the same rows at their own width
        sel = np.flatnonzero(m[:, n:].sum(1) == 0)
        assert np.array_equal(choose(lp[sel, :n], m[sel, :n], 1.0, u[sel]), k[sel]), n
    # the actor's own mask: u = 0 skips the masked entries in front, u = 1 - 2^-24 the one behind
    op = np.array([OP_MASK] * 4, np.float32)
    lp11 = log_softmax(np.random.default_rng(6).random((4, 11)))
    for e in EXPLORES:
        assert list(choose(lp11, op, e, np.array([0.0, U_TOP, 0.0, U_TOP]))) == [2, 9, 2, 9], e


@gpu
def test_all_masked_rows_and_single_live_rows():
    lp = log_softmax(np.random.default_rng(8).random((70, 11)))
    m = np.zeros((70, 11), np.float32)
    m[1::2, 10] = 1.0                                          # odd rows: one live entry, the last
    m[1, 10], m[1, 0] = 0.0, 1.0
    want = np.where(m.sum(1) > 0, m.argmax(1), 0)
    for e in EXPLORES:
        for u in (None, np.zeros(70), np.full(70, 0.5), np.full(70, U_TOP)):
            assert np.array_equal(choose(lp, m, e, u), want), e  # (check_outputs: an all-masked row's mask is unchanged)


def argmax_case(n, e):
    """The largest live probability lifted so that the runner-up is at least 1e-3 (relative) below it."""
    rng = np.random.default_rng(300 + n)
    lp = log_softmax(rng.random((130, n)))
    m = random_masks(rng, 130, n)
    m[0] = 0.0
    m[0, n - 1] = m[0, n // 2] = 1.0
    top = probabilities(lp, m, e).argmax(1)
    lp[np.arange(130), top] += np.float32(0.1)
    return lp, m


def check_argmax_inputs(lp, m, e):
    p = np.sort(probabilities(lp, m, e), 1)
    assert float(((p[:, -1] - p[:, -2]) / p[:, -1]).min()) >= 1e-3


@pytest.mark.parametrize('e', [0.0, 0.05])
@pytest.mark.parametrize('n', [2, 11, 32])
def test_argmax_inputs_have_a_clear_winner(n, e):
    check_argmax_inputs(*argmax_case(n, e), e)


@gpu
@pytest.mark.parametrize('e', [0.0, 0.05])
@pytest.mark.parametrize('n', [2, 11, 32])
def test_argmax_matches_the_restatement(n, e):
    lp, m = argmax_case(n, e)
    check_argmax_inputs(lp, m, e)
    want = restate(lp, m, e)
    assert len(set(want)) > 1
    assert np.array_equal(choose(lp, m, e, None, sample=False), want)
    u =np.random.default_rng(9).random(130, dtype=np.float32)
    assert np.array_equal(choose(lp, m, e, u, sample=False), want)               # sample=False ignores a supplied u
    assert np.array_equal(choose(lp, m, e, np.zeros(130), sample=False), want)


@gpu
def test_argmax_ties_give_the_lowest_live_index():
    rng = np.random.default_rng(10)
    for n in (1, 11, 32):
        lp = log_softmax(rng.random((66, n)))
        m = random_masks(rng, 66, n)
        m[0] = 1.0
        if n == 11:
            m[1] = OP_MASK
        assert np.array_equal(choose(lp, m, 1.0, None, sample=False), m.argmax(1)), n


@gpu
def test_exact_extremes():
    """exp(0) = 1 and exp(-inf) = 0 are exact: weights (1, 0, 1) on live entries 3, 4, 5 at explore = 0 give the boundary
    0.5 exactly; the zero-weight entry between them (and those in front) is never drawn.  One entry with all the mass."""
    lp = np.full((8, 11), NEG_INF, np.float32)
    lp[:4, 3] = lp[:4, 5] = 0.0
    lp[4:, 7] = 0.0
    lp[7, 2] = -1e4
    m = np.ones((8, 11), np.float32)
    u = np.array([0.0, 0.5, U_TOP, np.float32(0.5) - np.float32(2.0 ** -25), 0.0, 0.5, U_TOP, 0.25], np.float32)
    want = np.array([3, 5, 5, 3, 7, 7, 7, 7])
    assert np.array_equal(restate(lp, m, 0.0, u), want)
    assert np.array_equal(choose(lp, m, 0.0, u), want)
    assert np.array_equal(choose(lp, m, 0.0, None, sample=False), np.array([3, 3, 3, 3, 7, 7, 7, 7]))


@gpu
@pytest.mark.parametrize('B', [1, 63, 65])
def test_rows_past_the_batch_are_untouched(B):
    """Raw C entry on buffers one row longer than B, every extra row poisoned: a thread past the batch writes nothing.  Then
    the wrapper on the first B rows of an over-allocated mask, and logp given as (B,1,n)."""
    import t2onet_amd.functional as T
    from t2onet_amd import _lib
    lp, m, u, k = interior_case(11, 0.05)
    lp_t = torch.as_tensor(np.concatenate([lp[:B], np.zeros((1, 11), np.float32)])).to(dev())
    m_t = torch.as_tensor(np.concatenate([m[:B], np.full((1, 11), 7.0, np.float32)])).to(dev())
    u_t = torch.as_tensor(np.concatenate([u[:B], [0.5]]).astype(np.float32)).to(dev())
    pred = torch.full((B + 1, 1), -77, dtype=torch.int64, device=dev())
    exe = torch.full((B + 1,), -77, dtype=torch.int32, device=dev())
    before = m_t.clone()
    rc = _lib.load().t2o_choose_op(lp_t.data_ptr(), m_t.data_ptr(), u_t.data_ptr(), 0.05, pred.data_ptr(), exe.data_ptr(), B, 11,
                                   T._stream(dev()))
    assert rc == 0
    check_outputs(pred[:B], exe[:B], before[:B], m_t[:B])
    assert np.array_equal(pred[:B].view(-1).cpu().numpy(), k[:B])
    assert int(pred[B]) == -77 and int(exe[B]) == -77 and torch.equal(m_t[B], before[B])
    m_t.copy_(before)
    view = m_t[:B]
    assert view.is_contiguous()
    p2, e2 = T.choose_op(lp_t[:B].view(B, 1, 11), view, 0.05, True, u_t[:B])
    check_outputs(p2, e2, before[:B], view)
    assert torch.equal(p2, pred[:B]) and torch.equal(m_t[B], before[B])


@gpu
def test_executor_index_is_the_id_minus_three():
    m = np.eye(11, dtype=np.float32)                           # row r can only choose r
    got = choose(np.zeros((11, 11), np.float32), m, 0.05, np.full(11, 0.5))
    assert list(got) == list(range(11))                        # (check_outputs: exec_op == pred_op - 3, here -3 .. 7)


@gpu
def test_wrapper_rejects_what_the_kernel_cannot_take():
    import t2onet_amd.functional as T
    lp = torch.zeros(4, 11, device=dev())
    wide = torch.ones(4, 22, device=dev())
    with pytest.raises(ValueError, match='contiguous'):
        T.choose_op(lp, wide[:, ::2], 0.05, False)
    assert bool((wide == 1).all())
    with pytest.raises(RuntimeError, match='1..32 operator tokens'):
        T.choose_op(torch.zeros(2, 33, device=dev()), torch.ones(2, 33, device=dev()), 0.05, False)
    with pytest.raises(RuntimeError, match='no CPU'):
        T.choose_op(torch.zeros(2, 11), torch.ones(2, 11), 0.05, False)


def check_invalid_arguments(lp, m, u, pred, exe, stream):
    """n_cls = 33, B = 0 and a null pointer: T2O_EINVAL with the documented message (the caller checks nothing was written)."""
    from t2onet_amd import _lib
    lib = _lib.load()
    T2O_EINVAL = 1
    args = [lp.data_ptr(), m.data_ptr(), u.data_ptr(), 0.05, pred.data_ptr(), exe.data_ptr()]
    assert lib.t2o_choose_op(*args, 2, 33, stream) == T2O_EINVAL
    assert lib.t2o_last_error() == b'choose_op: 1..32 operator tokens'
    assert lib.t2o_choose_op(*args, 0, 11, stream) == T2O_EINVAL
    assert lib.t2o_last_error() == b'choose_op: 1..32 operator tokens'
    assert lib.t2o_choose_op(*args, 2, 0, stream) == T2O_EINVAL
    for hole in (0, 1, 4, 5):                                  # logp, op_mask, pred_op, exec_op (u may be null: arg-max)
        holed = list(args)
        holed[hole] = None
        assert lib.t2o_choose_op(*holed, 2, 11, stream) == T2O_EINVAL
        assert lib.t2o_last_error() == b'choose_op: null pointer'


def test_invalid_arguments_are_refused_without_a_device():
    lp, m, u = torch.zeros(2, 33), torch.ones(2, 33), torch.zeros(2)
    pred, exe = torch.full((2,), -77, dtype=torch.int64), torch.full((2,), -77, dtype=torch.int32)
    check_invalid_arguments(lp, m, u, pred, exe, None)         # (host memory: a launch would not get this far unnoticed)
    assert bool((m == 1).all() and (pred == -77).all() and (exe == -77).all())


@gpu
def test_invalid_arguments_launch_nothing():
    import t2onet_amd.functional as T
    lp, m, u = torch.zeros(2, 33, device=dev()), torch.ones(2, 33, device=dev()), torch.zeros(2, device=dev())
    pred = torch.full((2,), -77, dtype=torch.int64, device=dev())
    exe = torch.full((2,), -77, dtype=torch.int32, device=dev())
    check_invalid_arguments(lp, m, u, pred, exe, T._stream(dev()))
    torch.cuda.synchronize()
    assert bool((m == 1).all() and (pred == -77).all() and (exe == -77).all())


# ---------------------------------------------------------------------------------------------------------------
# frequencies
# ---------------------------------------------------------------------------------------------------------------
FREQ_B, FREQ_SEED, FREQ_E = 1 << 18, 2024, 0.05
FREQ_AMBIGUOUS_CAP = FREQ_B * 11 * 2e-5 * 3                    # three times the expected count of |u sum p - cdf_k| < 1e-5


@functools.lru_cache(None)
def frequency_case():
    lp = log_softmax(np.random.default_rng(FREQ_SEED + 1).random((1, 11)))
    m = np.array([OP_MASK], np.float32)
    u = np.random.default_rng(FREQ_SEED).random(FREQ_B, dtype=np.float32)
    p = probabilities(lp, m, FREQ_E)[0]
    cdf = np.cumsum(p)
    thr = u.astype(np.float64) * cdf[-1]
    idx = (cdf[None, :] <= thr[:, None]).sum(1)
    assert int(idx.max()) < 11
    near = (np.abs(cdf[None, :] - thr[:, None]) < AMBIGUOUS).any(1)
    return lp, m, u, p, idx, near


def check_frequencies(choice, p):
    counts = np.bincount(choice, minlength=11)
    sigma = np.sqrt(FREQ_B * p * (1.0 - p))
    assert bool((np.abs(counts - FREQ_B * p) <= 5.0 * sigma).all()), (counts, FREQ_B * p, sigma)
    assert bool((counts[np.array(OP_MASK) == 0] == 0).all())


def test_frequency_inputs_meet_their_conditions():
    """The seed's own draws pass the 5-sigma test on the restatement, and few enough of them sit on a boundary."""
    lp, m, u, p, idx, near = frequency_case()
    assert abs(p.sum() - 1.0) < 1e-12 and float(u.max()) < 1.0
    check_frequencies(idx, p)
    assert 0 < int(near.sum()) <= FREQ_AMBIGUOUS_CAP


@gpu
def test_draw_frequencies_follow_the_probabilities():
    import t2onet_amd.functional as T
    lp, m, u, p, idx, near = frequency_case()
    check_frequencies(idx, p)
    assert int(near.sum()) <= FREQ_AMBIGUOUS_CAP
    lp_t = torch.as_tensor(lp).to(dev()).expand(FREQ_B, 11).contiguous()
    m_t = torch.as_tensor(m).to(dev()).expand(FREQ_B, 11).contiguous()
    before = m_t.clone()
    pred, exe = T.choose_op(lp_t, m_t, FREQ_E, True, torch.as_tensor(u).to(dev()))
    check_outputs(pred, exe, before, m_t)
    got = pred.view(-1).cpu().numpy()
    check_frequencies(got, p)
    differ = got != idx
    assert not bool((differ & ~near).any()), np.flatnonzero(differ & ~near)[:8]
    for b in np.flatnonzero(differ):
        assert int(got[b]) in neighbours(lp[0], m[0], FREQ_E, u[b]), (b, got[b], idx[b], u[b])


@gpu
def test_wrapper_draws_from_the_seeded_generator():
    """sample=True without u: the wrapper's own torch.rand -- the same seed gives the same draws, another seed others (flat
    distribution over the 7 live operators, B = 256: equal by chance with probability 7^-256)."""
    import t2onet_amd.functional as T
    lp = torch.as_tensor(log_softmax(np.random.default_rng(12).random((256, 11)))).to(dev())
    base = torch.tensor([OP_MASK] * 256, device=dev())
    runs = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        m = base.clone()
        pred, exe = T.choose_op(lp, m, 1.0, True, None)
        check_outputs(pred, exe, base, m)
        runs.append(pred.clone())
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    assert len(set(runs[0].view(-1).tolist())) == 7


# ---------------------------------------------------------------------------------------------------------------
# the sampled decode of the actor
# ---------------------------------------------------------------------------------------------------------------
def spy_on(monkeypatch, inner=None):
    """functional.choose_op (or `inner` in its place) recorded per decoder step: logp, the mask before, u, the outputs."""
    import t2onet_amd.functional as T
    inner = T.choose_op if inner is None else inner
    calls = []

    def spy(logp, op_mask, explore_prob, sample=True, u=None):
        rec = {'logp': logp.detach().clone(), 'before': op_mask.clone(), 'u': u, 'explore': explore_prob, 'sample': sample}
        rec['pred'], rec['exe'] = inner(logp, op_mask, explore_prob, sample, u)
        rec['after'] = op_mask.clone()
        calls.append(rec)
        return rec['pred'], rec['exe']
    monkeypatch.setattr(T, 'choose_op', spy)
    return calls


def episode(seed, reinforce_sample=1):
    from oracle import synth
    from tests.test_gpu_actor_extra import make_model, B, H, W, L
    model, opt = make_model(dev())
    model.train()
    x = synth.requests(B, L, 41).to(dev())
    img = synth.images(B, H, W, 42).to(dev())
    torch.manual_seed(seed)
    _, imgs, ops, _ = model.episode_forward(x, img, None, reinforce_sample=reinforce_sample)
    return opt, imgs.detach(), ops


def check_recorded_calls(calls, opt, B):
    """Every recorded call against the restatement; returns the (step, row) pairs of ambiguous draws (a threshold within 1e-5
    of a boundary), where the kernel may take either neighbour."""
    assert len(calls) == opt.decoder_max_len
    ambiguous = []
    for t, c in enumerate(calls):
        check_outputs(c['pred'], c['exe'], c['before'], c['after'])
        lp = c['logp'].reshape(B, -1).cpu().numpy()
        m = c['before'].cpu().numpy()
        u = c['u'].cpu().numpy()
        assert c['sample'] is True and c['explore'] == opt.explore_prob and u.shape == (B,) and float(u.max()) < 1.0
        got = c['pred'].view(-1).cpu().numpy()
        want = restate(lp, m, opt.explore_prob, u)
        near = boundary_distance(lp, m, opt.explore_prob, u) < AMBIGUOUS
        for b in range(B):
            if near[b]:
                ambiguous.append((t, b))
                assert int(got[b]) in neighbours(lp[b], m[b], opt.explore_prob, u[b]), (t, b)
            else:
                assert got[b] == want[b], (t, b, got[b], want[b], u[b])
    assert len(ambiguous) <= 1, ambiguous
    return ambiguous


def check_episode_ops(ops, opt):
    live = {k for k, v in enumerate(OP_MASK) if v}
    for row in ops.cpu().tolist():
        assert len(set(row)) == len(row) == opt.decoder_max_len and set(row) <= live, row


@gpu
def test_sampled_episode_draws_match_the_restatement(monkeypatch):
    from tests.test_gpu_actor_extra import B
    calls = spy_on(monkeypatch)
    opt, imgs, ops = episode(seed=5)
    check_recorded_calls(calls, opt, B)
    check_episode_ops(ops, opt)
    assert torch.equal(ops, torch.cat([c['pred'] for c in calls], 1))
    # the uniform numbers are drawn once per episode: step t sees row t of ONE (decoder_max_len, B) tensor
    draws = calls[0]['u']._base
    assert draws is not None and tuple(draws.shape) == (opt.decoder_max_len, B) and draws.dtype == torch.float32
    for t, c in enumerate(calls):
        assert c['u']._base is draws and c['u'].data_ptr() == draws[t].data_ptr() and torch.equal(c['u'], draws[t])
    assert len({tuple(row) for row in draws.cpu().tolist()}) == opt.decoder_max_len
    # the same seed: the same operators and images, bit for bit; another seed: other draws
    first = len(calls)
    opt, imgs2, ops2 = episode(seed=5)
    assert torch.equal(ops2, ops) and torch.equal(imgs2, imgs)
    assert torch.equal(calls[first]['u']._base, draws)
    opt, imgs3, ops3 = episode(seed=6)
    assert not torch.equal(calls[2 * first]['u']._base, draws)
    check_episode_ops(ops3, opt)


@gpu
def test_argmax_episode_passes_no_uniform_numbers(monkeypatch):
    from tests.test_gpu_actor_extra import B
    calls = spy_on(monkeypatch)
    opt, imgs, ops = episode(seed=5, reinforce_sample=0)
    assert len(calls) == opt.decoder_max_len
    for c in calls:
        assert c['u'] is None and c['sample'] is False
        check_outputs(c['pred'], c['exe'], c['before'], c['after'])
        lp, m = c['logp'].reshape(B, -1).cpu().numpy(), c['before'].cpu().numpy()
        p = np.sort(probabilities(lp, m, opt.explore_prob), 1)
        clear = (p[:, -1] - p[:, -2]) / p[:, -1] >= 1e-3
        got = c['pred'].view(-1).cpu().numpy()
        assert np.array_equal(got[clear], restate(lp, m, opt.explore_prob)[clear])
    check_episode_ops(ops, opt)


def fallback_choice(logp, op_mask, explore_prob, sample=True, u=None):
    """The framework branch of Actor.episode_decode (the `else:` beside the fused choice) with the draw of
    actor.sample_categorical made from the supplied uniform numbers."""
    B, n = op_mask.shape
    probs = torch.exp(logp.detach()).reshape(B, n)
    probs = probs * (1 - explore_prob) + explore_prob
    probs = probs * op_mask
    probs = probs / (probs.sum(1, keepdim=True) + 1e-30)
    if sample:
        cdf = probs.cumsum(1)
        idx = (cdf <= u.view(B, 1) * cdf[:, -1:]).sum(1, keepdim=True)
        pred_op = torch.where(idx >= n, probs.argmax(1, keepdim=True), idx)
    else:
        pred_op = probs.topk(1)[1].view(B, -1)
    op_mask.scatter_(1, pred_op, 0.0)
    return pred_op, (pred_op.view(-1) - 3).to(torch.int32)


@gpu
def test_fused_choice_equals_the_fallback_formula(monkeypatch):
    from tests.test_gpu_actor_extra import B
    calls = spy_on(monkeypatch)
    opt, imgs, ops = episode(seed=5)
    ambiguous = check_recorded_calls(calls, opt, B)
    monkeypatch.undo()
    other = spy_on(monkeypatch, fallback_choice)
    opt, imgs_f, ops_f = episode(seed=5)
    assert len(other) == len(calls) and torch.equal(other[0]['u']._base, calls[0]['u']._base)
    if torch.equal(ops_f, ops):
        assert torch.equal(imgs_f, imgs)
        return
    # the two may part at the one ambiguous draw only (training-mode batch norm then spreads the difference over the batch)
    assert len(ambiguous) == 1
    t, b = ambiguous[0]
    assert torch.equal(ops_f[:, :t], ops[:, :t]) and torch.equal(imgs_f[:, :t], imgs[:, :t])
    same = torch.ones(B, dtype=torch.bool)
    same[b] = False
    assert torch.equal(ops_f[same, t], ops[same, t])
    c = calls[t]
    assert int(ops_f[b, t]) in neighbours(c['logp'].reshape(B, -1)[b].cpu().numpy(), c['before'][b].cpu().numpy(), opt.explore_prob,
                                          float(c['u'][b]))


# ---------------------------------------------------------------------------------------------------------------
# the captured whole-step graph
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_every_replay_of_the_step_graph_draws_other_operators():
    """explore_prob = 1: every draw is uniform over the operators still unused.  Four replays of the captured step on the same
    batch with frozen weights must not all choose the same (B, decoder_max_len) operators -- a graph that replayed one frozen
    draw would (by chance: 2520^-8 per pair of replays at B = 8)."""
    import copy
    import t2onet_amd
    from oracle import synth
    from t2onet_amd.actor import Actor
    from t2onet_amd.train import Trainer
    opt = t2onet_amd.default_options()
    opt.explore_prob = 1.0
    torch.manual_seed(43)
    model = Actor(opt).to(dev()).train()
    model.use_channels_last()
    B, H, W = 8, 256, 256
    img = synth.images(B, H, W, 101).to(dev())
    tgt = synth.images(B, H, W, 102).to(dev())
    x = synth.requests(B, 17, 103).to(dev())
    lengths = (x != 0).sum(1).cpu()
    tr = Trainer(model, opt, lr=0.0, graph_step=True)
    seen = []
    for _ in range(4):
        tr.episode_step(x, img, tgt, lengths=lengths)
        assert tr.graph_step and len(tr._step_graphs) == 1, 'the whole-step graph was not used'
        ops = next(iter(tr._step_graphs.values())).ops.clone()
        assert tuple(ops.shape) == (B, opt.decoder_max_len) and ops.dtype == torch.int64
        check_episode_ops(ops, opt)
        seen.append(ops)
    assert not all(torch.equal(seen[0], s) for s in seen[1:]), seen[0]
