"""functional.l1_loss and functional.end_select_l1 (k_l1_* / k_end_l1_* in t2o_kernels.hip) against fp64.

Forward: all terms are non-negative, so the relative error is a rounding count -- at most 32 adds per thread (8 iterations
x float4), 8 levels of block reduction, ceil(nblk / 256) strided adds and 8 more levels in the finaliser, then the
subtraction inside |p - t|, 1 / n and the last product: (52 + ceil(nblk / 256)) u.  nblk <= 384 here (54 u), so 64 u is asserted.
Backward: exact.  sign(p - t) * fl32(gloss * fl32(1 / fl32(n))) bit for bit, 0 at ties, and every step image that was not
selected gets an all-zero gradient."""
import ctypes

import numpy as np
import pytest
import torch

from tests import step_cases as sc

pytestmark = pytest.mark.gpu
GLOSS = 3.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.mark.parametrize('n', sc.L1_SIZES)
def test_l1_loss_against_fp64(dev, n):
    """n % 4 != 0 runs the scalar kernels (2048 floats per workgroup), else the float4 ones (8192); 8192 / 8196 and 2048 /
    2049 are their one-to-two workgroup edges; 64 x 3 x 128 x 128 leaves 384 partial sums: the finaliser's second pass."""
    import t2onet_amd.functional as T
    p, t = sc.l1_pair(n, 100 + n % 997)
    pred = torch.from_numpy(p).to(dev).requires_grad_(True)
    loss = T.l1_loss(pred, torch.from_numpy(t).to(dev))
    (g,) = torch.autograd.grad(loss * GLOSS, pred)
    want = sc.l1_loss64(p, t)
    err = abs(float(loss.detach()) - want) / want if want else abs(float(loss.detach()))
    print('n=%d: loss relative error %.2f u' % (n, err / sc.U))
    assert err <= sc.L1_REL_BOUND
    assert np.array_equal(g.cpu().numpy(), sc.l1_grad32(p, t, GLOSS))


@pytest.mark.parametrize('name', [c[0] for c in sc.END_CASES])
def test_end_select_l1_against_fp64(dev, name):
    import t2onet_amd.functional as T
    imgs, first, tgt = sc.end_case(name)
    pred = sc.end_gather(imgs, first)
    want = sc.l1_loss64(pred, tgt)
    d_imgs = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in imgs]
    d_tgt = torch.from_numpy(tgt).to(dev)
    loss = T.end_select_l1(d_imgs, torch.from_numpy(first).to(dev), d_tgt)
    grads = torch.autograd.grad(loss * GLOSS, d_imgs)
    assert abs(float(loss.detach()) - want) <= sc.L1_REL_BOUND * want
    # the identity the kernel promises: same partition and order as l1_loss on the gathered tensor
    assert torch.equal(loss, T.l1_loss(torch.from_numpy(pred).to(dev), d_tgt))
    gsel = sc.l1_grad32(pred, tgt, GLOSS)
    assert want > 0 and gsel.any() and (gsel == 0).any()                 # something to get wrong, and ties
    assert len(first) == 1 or not gsel[0].any()                          # B > 1: sample 0 has pred == target everywhere
    for t, g in enumerate(grads):
        exp = np.zeros_like(gsel)
        exp[first == t] = gsel[first == t]
        assert np.array_equal(g.cpu().numpy(), exp), 'step image %d' % t


def test_end_select_l1_from_operator_tokens_with_and_without_end(dev):
    """train.end_l1_loss: first END token per sample, the last step where there is none (T = 5, scalar path: row 3 * 5 * 7)."""
    from t2onet_amd.train import end_l1_loss, first_end_step
    rng = np.random.default_rng(5)
    B, Tn, shape = 6, 5, (3, 5, 7)
    imgs = [rng.random((B,) + shape, dtype=np.float32) for _ in range(Tn)]
    tgt = rng.random((B,) + shape, dtype=np.float32)
    ops = torch.tensor([[5, 2, 4, 4, 4], [2, 3, 3, 3, 3], [3, 4, 5, 6, 8], [3, 4, 5, 6, 2], [3, 2, 2, 2, 2], [4, 4, 2, 5, 2]], device=dev)
    first = first_end_step(ops, 2).cpu().numpy()
    assert first.tolist() == [1, 0, 4, 4, 1, 2]
    d_imgs = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in imgs]
    loss = end_l1_loss(d_imgs, ops, 2, torch.from_numpy(tgt).to(dev))
    grads = torch.autograd.grad(loss * GLOSS, d_imgs)
    pred = sc.end_gather(imgs, first)
    want = sc.l1_loss64(pred, tgt)
    assert abs(float(loss.detach()) - want) <= sc.L1_REL_BOUND * want
    gsel = sc.l1_grad32(pred, tgt, GLOSS)
    for t, g in enumerate(grads):
        exp = np.zeros_like(gsel)
        exp[first == t] = gsel[first == t]
        assert np.array_equal(g.cpu().numpy(), exp)


def test_end_select_l1_refusals(dev):
    """T = 0, T = 9, a shape mismatch, and -- through the C ABI -- a workspace smaller than the partial sums."""
    import t2onet_amd.functional as T
    from t2onet_amd import _lib
    B, shape = 2, (3, 4, 4)
    tgt = torch.zeros((B,) + shape, device=dev)
    first = torch.zeros(B, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match='1 <= T <= 8'):
        T.end_select_l1([], first, tgt)
    with pytest.raises(RuntimeError, match='1 <= T <= 8'):
        T.end_select_l1([tgt.clone() for _ in range(9)], first, tgt)
    with pytest.raises(ValueError, match='shape mismatch'):
        T.end_select_l1([tgt.clone(), torch.zeros(B, 3, 4, 5, device=dev)], first, tgt)
    lib = _lib.load()
    big = torch.zeros(3, 3 * 64 * 64, device=dev)                        # 36864 floats: 5 partial sums = 20 bytes
    one = torch.ones(3, 3 * 64 * 64, device=dev)
    f3 = torch.zeros(3, dtype=torch.int64, device=dev)
    loss = torch.full((), 7.0, device=dev)
    ws = torch.zeros(64, dtype=torch.uint8, device=dev)
    arr = (ctypes.c_void_p * 1)(one.data_ptr())
    st = T._stream(dev)
    assert lib.t2o_end_select_l1_fwd(arr, 1, f3.data_ptr(), big.data_ptr(), loss.data_ptr(), 3, 3 * 64 * 64, ws.data_ptr(), 16, st) == 3
    assert b'workspace' in lib.t2o_last_error()
    assert lib.t2o_end_select_l1_fwd(arr, 1, f3.data_ptr(), big.data_ptr(), loss.data_ptr(), 3, 3 * 64 * 64, None, 64, st) == 3
    assert float(loss) == 7.0                                            # refused before any launch
    assert lib.t2o_end_select_l1_fwd(arr, 1, f3.data_ptr(), big.data_ptr(), loss.data_ptr(), 3, 3 * 64 * 64, ws.data_ptr(), 20, st) == 0
    assert abs(float(loss) - 1.0) <= sc.L1_REL_BOUND                     # |1 - 0| everywhere: the accepted call did run
