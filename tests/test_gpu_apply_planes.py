"""functional.apply_planes on the device against the path it replaces, mask_select + apply_per_sample: out, image gradient
and parameter gradient bit for bit (torch.equal), at every shape where the per-sample launch changes path.  The two-launch
path is the one tests/test_gpu_operator_masks.py holds to fp64, so no tolerance and no clamp-edge allowance appear here."""
import numpy as np
import pytest
import torch

from tests import apply_planes_cases as AP

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(stack, slot, pred_op):
    # the planes sit at an ODD byte of their buffer: torch allocations are 256-byte aligned, the kernels may assume nothing
    buf = torch.zeros(stack.size + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = torch.from_numpy(np.ascontiguousarray(stack).reshape(-1)).to(DEV)
    planes = buf[1:].view(stack.shape)
    return planes, torch.from_numpy(slot).to(DEV), torch.from_numpy(pred_op).to(DEV)


def _run(fn, img, param, gout, want_gimg=True):
    x = img.clone().requires_grad_(want_gimg)
    p = param.clone().requires_grad_(True)
    out = fn(x, p)
    out.backward(gout)
    return out.detach(), (x.grad if want_gimg else None), p.grad


def _both(stack, slot, pred_op, H, W, want_gimg=True):
    from t2onet_amd import functional as T
    planes, slot, pred_op = _dev(stack, slot, pred_op)
    img, param, gout = (t.to(DEV) for t in AP.tensors(H, W))
    op_id = torch.from_numpy(AP.OP_ID).to(DEV)
    got = _run(lambda x, p: T.apply_planes(op_id, pred_op, x, p, planes, slot), img, param, gout, want_gimg)
    want = _run(lambda x, p: T.apply_per_sample(op_id, x, p, T.mask_select(planes, slot, pred_op)), img, param, gout, want_gimg)
    return got, want


def _assert_equal(got, want, tag):
    for name, g, w in zip(('out', 'gimg', 'gparam'), got, want):
        if w is None:
            assert g is None, (tag, name)
            continue
        assert torch.isfinite(w).all(), (tag, name)
        assert torch.equal(g, w), (tag, name, float((g - w).abs().max()))


@pytest.mark.parametrize('shape', AP.SHAPES)
def test_planes_equal_select_then_apply_bit_for_bit(shape):
    H, W = shape
    stack = AP.planes(H, W)
    got, want = _both(stack, AP.slots('mixed'), AP.PRED_OP, H, W)
    _assert_equal(got, want, ('mixed', shape))
    assert float(want[2].abs().max()) > 0                                     # the parameter gradients are not trivially zero
    got, want = _both(stack, AP.slots('mixed'), AP.pred_op_outside(), H, W)
    _assert_equal(got, want, ('pred_op = V', shape))


@pytest.mark.parametrize('shape', AP.SHAPES)
def test_without_an_image_gradient(shape):
    H, W = shape
    got, want = _both(AP.planes(H, W), AP.slots('mixed'), AP.PRED_OP, H, W, want_gimg=False)
    assert got[1] is None
    _assert_equal(got, want, ('no gimg', shape))


@pytest.mark.parametrize('shape', AP.SHAPES)
def test_no_planes_at_all(shape):
    """N = 0: the plane pointer is NULL, every slot that names a plane names one that does not exist."""
    H, W = shape
    got, want = _both(AP.planes(H, W)[:0], AP.slots('mixed'), AP.PRED_OP, H, W)
    _assert_equal(got, want, ('N = 0', shape))


@pytest.mark.parametrize('shape', AP.SHAPES)
def test_every_slot_minus_one_is_the_unmasked_call(shape):
    from t2onet_amd import functional as T
    H, W = shape
    planes, slot, pred_op = _dev(AP.planes(H, W), AP.slots('none'), AP.PRED_OP)
    img, param, gout = (t.to(DEV) for t in AP.tensors(H, W))
    op_id = torch.from_numpy(AP.OP_ID).to(DEV)
    got = _run(lambda x, p: T.apply_planes(op_id, pred_op, x, p, planes, slot), img, param, gout)
    want = _run(lambda x, p: T.apply_per_sample(op_id, x, p, None), img, param, gout)
    _assert_equal(got, want, ('all -1', shape))


def test_the_masks_act_and_the_executor_routes_a_plane_mask():
    import t2onet_amd
    from t2onet_amd import functional as T
    H, W = AP.SHAPES[0]
    planes, slot, pred_op = _dev(AP.planes(H, W), AP.slots('mixed'), AP.PRED_OP)
    img, param, _ = (t.to(DEV) for t in AP.tensors(H, W))
    op_id = torch.from_numpy(AP.OP_ID).to(DEV)
    ex = t2onet_amd.Executor(t2onet_amd.default_options()).to(DEV)
    with torch.no_grad():
        out, par = ex.execute_per_sample(img, op_id, T.PlaneMask(planes, slot, pred_op.view(-1, 1)), specified_param=param)
        plain, _ = ex.execute_per_sample(img, op_id, None, specified_param=param)
        two, _ = ex.execute_per_sample(img, op_id, T.mask_select(planes, slot, pred_op), specified_param=param)
    assert par is param and torch.equal(out, two) and not torch.equal(out, plain)
    assert torch.equal(out[0, :, 0], img[0, :, 0])                            # brightness under the box: row 0 lies outside it
    with pytest.raises(ValueError):
        T.apply_planes(op_id, pred_op, img[:, :, :-1], param, planes, slot)   # planes of another size
