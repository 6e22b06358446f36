"""No-GPU checks of the byte-plane per-sample operators (t2o_apply_planes.hip): the block programs walked with the uint8
fetch (PlaneU8) against the same programs walked with the fp32 fetch fed float(byte) (tests/host_emul/emul_apply_planes.cpp,
g++ -ffp-contract=off) -- outputs, image gradients and per-block parameter partials bit for bit --, the status codes of the
two C entry points, and train_cli's --load_mask flag."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import apply_planes_cases as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emul():
    out = os.path.join(ROOT, 'tests', '_build')
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, 'libt2o_emul_apply_planes.so')
    src = os.path.join(ROOT, 'tests', 'host_emul', 'emul_apply_planes.cpp')
    deps = [src] + [os.path.join(ROOT, 't2onet_amd', 'csrc', h) for h in ('t2o_pixel_math.h', 't2o_block_programs.h', 't2o_plane_programs.h')]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = '%s.tmp.%d' % (so, os.getpid())
        subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-o', tmp, src])
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    lib.emul_apply_planes_rows.argtypes = [ctypes.c_int] * 3
    lib.emul_apply_planes.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 7 + [ctypes.c_int] * 3
    return lib


def _walk(emul, stack, slot, pred_op, mask_f32, img, param, gout, H, W):
    rows = emul.emul_apply_planes_rows(AP.B, H, W)
    out, gimg = np.full((AP.B, 3, H, W), np.nan, np.float32), np.full((AP.B, 3, H, W), np.nan, np.float32)
    partials = np.zeros((AP.B, rows, 24), np.float32)
    # the planes packed into a buffer that starts at an ODD address: no alignment may be assumed
    buf = np.zeros(stack.size + 8, np.uint8)
    off = 1 if buf.ctypes.data % 2 == 0 else 2
    packed = buf[off:off + stack.size]
    packed[:] = stack.reshape(-1)
    rc = emul.emul_apply_planes(AP.OP_ID.ctypes.data, pred_op.ctypes.data, packed.ctypes.data if stack.size else None, slot.ctypes.data,
                                len(stack), AP.V, None if mask_f32 is None else mask_f32.ctypes.data, img.ctypes.data, param.ctypes.data,
                                gout.ctypes.data, out.ctypes.data, gimg.ctypes.data, partials.ctypes.data, AP.B, H, W)
    assert rc == 0
    return out, gimg, partials


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('shape', AP.SHAPES)
def test_byte_fetch_walks_to_the_same_bits_as_the_fp32_fetch(emul, shape):
    H, W = shape
    img, param, gout = (np.ascontiguousarray(t.numpy()) for t in AP.tensors(H, W))
    stack = AP.planes(H, W)
    cases = [('mixed', AP.slots('mixed'), AP.PRED_OP, stack), ('pred_op = V', AP.slots('mixed'), AP.pred_op_outside(), stack),
             ('every slot -1', AP.slots('none'), AP.PRED_OP, stack), ('N = 0', AP.slots('mixed'), AP.PRED_OP, stack[:0])]
    for name, slot, pred_op, planes in cases:
        mask = AP.select_host(planes, slot, pred_op)
        got = _walk(emul, planes, slot, pred_op, None, img, param, gout, H, W)
        want = _walk(emul, planes, slot, pred_op, mask, img, param, gout, H, W)
        for what, g, w in zip(('out', 'gimg', 'partials'), got, want):
            assert not np.isnan(w).any(), (name, what)
            assert _same_bits(g, w), (name, what, shape)
    # the masks act: the mixed table's output differs from the all-ones one
    ones = _walk(emul, stack, AP.slots('none'), AP.PRED_OP, None, img, param, gout, H, W)[0]
    mixed = _walk(emul, stack, AP.slots('mixed'), AP.PRED_OP, None, img, param, gout, H, W)[0]
    assert not np.array_equal(ones, mixed)


# ------------------------------------------------------------------ C ABI without a device
@pytest.fixture(scope='module')
def lib():
    from t2onet_amd import build, _lib
    build.build()
    return _lib.load()


def test_entry_points_reject_bad_arguments_without_a_device(lib):
    buf = torch.zeros(1 << 16)
    p = buf.data_ptr()
    B, H, W, N, V = 2, 8, 12, 3, 11
    need = lib.t2o_workspace_bytes(B, H, W)
    assert 0 < need <= buf.numel() * 4

    def fwd(op_id=p, pred_op=p, planes=p, slot=p, N=N, V=V, img=p, param=p, stride=24, out=p, B=B, H=H, W=W):
        return lib.t2o_apply_planes_fwd(op_id, pred_op, planes, slot, N, V, img, param, stride, out, B, H, W, None)

    def bwd(op_id=p, pred_op=p, planes=p, slot=p, N=N, V=V, img=p, param=p, stride=24, gout=p, gimg=p, gparam=p, gstride=24, ws=p,
            ws_bytes=need, B=B, H=H, W=W):
        return lib.t2o_apply_planes_bwd(op_id, pred_op, planes, slot, N, V, img, param, stride, gout, gimg, gparam, gstride, ws, ws_bytes,
                                        B, H, W, None)
    for call, names in ((fwd, ('op_id', 'pred_op', 'slot', 'img', 'param', 'out')), (bwd, ('op_id', 'pred_op', 'slot', 'img', 'param', 'gout'))):
        for name in names:
            assert call(**{name: None}) == 1, name                           # T2O_EINVAL
            assert b'null' in lib.t2o_last_error() or b'param' in lib.t2o_last_error()
        assert call(planes=None) == 1 and b'plane' in lib.t2o_last_error()   # planes == NULL with N > 0
        assert call(N=-1) == 1 and call(V=0) == 1 and call(stride=23) == 1
        for kw in (dict(B=0), dict(H=0), dict(W=0), dict(B=-1), dict(H=-3), dict(W=-2)):
            assert call(**kw) == 1, kw
            assert b'positive' in lib.t2o_last_error()
        assert call(planes=None, N=0) in (0, 4)                              # accepted up to the launch
    assert bwd(ws=None, ws_bytes=0) == 3 and bwd(ws_bytes=need - 1) == 3     # T2O_EWORKSPACE
    assert b'workspace' in lib.t2o_last_error()
    assert bwd(gstride=23) == 1
    assert bwd(gimg=None) in (0, 4)                                          # the image gradient is optional


def test_functional_refuses_host_tensors():
    from t2onet_amd import functional as T
    with pytest.raises(RuntimeError):
        T.apply_planes(torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), torch.zeros(1, 3, 2, 2), torch.zeros(1, 24),
                       torch.zeros(1, 2, 2, dtype=torch.uint8), torch.zeros(1, 11, dtype=torch.int32))
    assert T.PlaneMask._fields == ('planes', 'slot', 'pred_op')


def test_train_cli_load_mask_flag():
    from t2onet_amd import train_cli
    assert train_cli.parse_args(['--synthetic']).load_mask is False
    assert train_cli.parse_args(['--dataset', 'GIER', '--load_mask']).load_mask is True
    with pytest.raises(SystemExit):
        train_cli.parse_args(['--synthetic', '--load_mask'])                 # only GIER annotates regions
    with pytest.raises(SystemExit):
        train_cli.parse_args(['--load_mask'])
