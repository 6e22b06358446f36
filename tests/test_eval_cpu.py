"""No-GPU checks of the evaluation kernels (t2o_eval.hip): the metrics tile program and the variance program, compiled for the
host from the shared header (tests/host_emul/emul_eval.cpp) and run over whole planes / rows, against the oracle's SSIM and
fp64 means; the status codes of the four C entry points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import cpu_ref, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 5, 7), (2, 3, 33, 70), (1, 3, 48, 40)]
VAR_SHAPES = [(2, 1, 105), (4, 1, 3 * 33 * 70), (2, 3, 3 * 48 * 40)]


@pytest.fixture(scope='module')
def emul():
    out = os.path.join(ROOT, 'tests', '_build')
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, 'libt2o_emul_eval.so')
    src = os.path.join(ROOT, 'tests', 'host_emul', 'emul_eval.cpp')
    deps = [src] + [os.path.join(ROOT, 't2onet_amd', 'csrc', h) for h in ('t2o_eval_math.h', 't2o_block_programs.h', 't2o_pixel_math.h')]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = '%s.tmp.%d' % (so, os.getpid())
        subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-o', tmp, src])
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    assert lib.emul_eval_lds_floats() == 3 * 42 * 43 + 8 * 42 * 33
    return lib


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def metric_case(shape, T, seed=0):
    """input, T step images, first (mixed, the last step among them), target for a (B,C,H,W) case, as float32 arrays."""
    B, C, H, W = shape
    pick = lambda s: np.ascontiguousarray(synth.images(B, H, W, s)[:, :C].numpy())
    first = np.array([(T - 1 - 3 * b) % T for b in range(B)], np.int64)        # b = 0: the last step
    return pick(seed + 1), [pick(seed + 10 + t) for t in range(T)], first, pick(seed + 2)


def expected_metrics(inp, imgs, first, tgt):
    """[fp64 mean |in - tgt|, fp64 mean |out - tgt|, oracle SSIM(in, tgt), oracle SSIM(out, tgt)] on the gathered images."""
    out = np.stack([imgs[min(int(f), len(imgs) - 1) if f >= 0 else len(imgs) - 1][b] for b, f in enumerate(first)])
    l1 = lambda a: float(np.abs(a.astype(np.float64) - tgt.astype(np.float64)).mean())
    ss = lambda a: float(cpu_ref.ssim(torch.from_numpy(a), torch.from_numpy(tgt)))
    return [l1(inp), l1(out), ss(inp), ss(out)]


def run_metrics(lib, inp, imgs, first, tgt, with_ssim=1):
    B, C, H, W = tgt.shape
    out4 = np.full(4, np.nan, np.float32)
    rc = lib.emul_eval_metrics(inp.ctypes.data_as(ctypes.c_void_p), _ptrs(imgs), len(imgs), first.ctypes.data_as(ctypes.c_void_p),
                               tgt.ctypes.data_as(ctypes.c_void_p), out4.ctypes.data_as(ctypes.c_void_p), with_ssim, B, C, H, W)
    assert rc == 0
    return out4


def check_metrics(got, want):
    assert abs(float(got[0]) - want[0]) < 1e-6 and abs(float(got[1]) - want[1]) < 1e-6, (got, want)
    np.testing.assert_allclose(got[2:], want[2:], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('T', [1, 5])
@pytest.mark.parametrize('shape', SHAPES)
def test_metrics_tile_program_against_the_oracle(emul, shape, T):
    inp, imgs, first, tgt = metric_case(shape, T)
    if T > 1:
        assert int(first[0]) == T - 1
    want = expected_metrics(inp, imgs, first, tgt)
    got = run_metrics(emul, inp, imgs, first, tgt)
    check_metrics(got, want)
    # without SSIM: slots 2 and 3 are 0, slots 0 and 1 the same bits
    plain = run_metrics(emul, inp, imgs, first, tgt, with_ssim=0)
    assert plain[2] == 0.0 and plain[3] == 0.0 and np.array_equal(plain[:2], got[:2])


def test_metrics_step_outside_the_table_counts_as_the_last(emul):
    inp, imgs, first, tgt = metric_case((2, 3, 33, 70), 5)
    wild = np.array([5 + 2, -1], np.int64)
    last = np.array([4, 4], np.int64)
    assert np.array_equal(run_metrics(emul, inp, imgs, wild, tgt), run_metrics(emul, inp, imgs, last, tgt))


def var_case(R, B, row, T=3, seed=0):
    """R lists of T (B,row) step images = clip(base + U(-0.1, 0.1)) around one base image per sample, and R first tensors."""
    rng = np.random.default_rng(100 + seed + row)
    base = rng.random((B, row))
    lists = [[np.clip(base + rng.uniform(-0.1, 0.1, (B, row)), 0, 1).astype(np.float32) for _ in range(T)] for _ in range(R)]
    firsts = [np.array([(r + 2 * b + T - 1) % T for b in range(B)], np.int64) for r in range(R)]
    return lists, firsts


def expected_variance(lists, firsts):
    ends = np.concatenate([np.stack([l[int(f[b])][b] for b in range(len(f))]) for l, f in zip(lists, firsts)]).astype(np.float64)
    return float(ends.var(axis=0, ddof=1).mean())


@pytest.mark.parametrize('R,B,row', VAR_SHAPES)
def test_variance_program_against_fp64(emul, R, B, row):
    lists, firsts = var_case(R, B, row)
    want = expected_variance(lists, firsts)
    assert want > 1e-3                                                   # (about 3.1e-3 for B = 1; more across samples)
    flat = [t for l in lists for t in l]
    for V in (0, 1) + ((2,) if row % 2 == 0 else ()):                     # the width the entry point picks, and narrower ones
        out = np.full(1, np.nan, np.float32)
        rc = emul.emul_end_select_var_mean(_ptrs(flat), _ptrs(firsts), R, len(lists[0]), B, ctypes.c_size_t(row), V,
                                           out.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0
        np.testing.assert_allclose(float(out[0]), want, rtol=1e-5)


def _library():
    from t2onet_amd import build, _lib
    if os.path.exists(build.hipcc_path()):
        build.build()
    elif not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libt2onet_hip.so is absent and there is no hipcc to build it')
    return _lib.load()


def test_status_codes_before_any_launch():
    """Every refusal returns before a launch: the pointers below are host memory and no device is needed."""
    lib = _library()
    assert lib.t2o_abi_version() == 4
    p = torch.zeros(64).data_ptr()
    one = (ctypes.c_void_p * 8)(*([p] * 8))
    many = (ctypes.c_void_p * 136)(*([p] * 136))
    big = 1 << 20

    def metrics(input=p, imgs=one, T=1, first=p, target=p, out4=p, ws=p, ws_bytes=big, B=1, C=3, H=8, W=8):
        return lib.t2o_eval_metrics(input, imgs, T, first, target, out4, 1, ws, ws_bytes, B, C, H, W, None)
    assert lib.t2o_eval_metrics_workspace_bytes(1, 3, 8, 8) == 4 * 3 * 4
    assert lib.t2o_eval_metrics_workspace_bytes(2, 3, 33, 70) == 4 * 2 * 3 * 6 * 4
    for kw in (dict(input=None), dict(imgs=None), dict(first=None), dict(target=None), dict(out4=None)):
        assert metrics(**kw) == 1 and b'null' in lib.t2o_last_error()
    assert metrics(imgs=(ctypes.c_void_p * 8)(p, None), T=2) == 1 and b'null' in lib.t2o_last_error()
    assert metrics(T=0) == 1 and metrics(T=9) == 1 and b'T <= 8' in lib.t2o_last_error()
    assert metrics(B=0) == 1 and metrics(C=0) == 1 and metrics(H=-1) == 1 and metrics(W=0) == 1
    assert metrics(ws=None) == 3 and metrics(ws_bytes=4 * 3 * 4 - 1) == 3 and b'workspace' in lib.t2o_last_error()
    assert metrics(B=1 << 16, C=1 << 10, H=1024, W=1024) == 2 and b'2^31' in lib.t2o_last_error()

    def variance(imgs=many, first=one, R=2, T=5, B=1, row=105, out=p, ws=p, ws_bytes=big):
        return lib.t2o_end_select_var_mean(imgs, first, R, T, B, row, out, ws, ws_bytes, None)
    assert lib.t2o_end_select_var_mean_workspace_bytes(105) == 4 and lib.t2o_end_select_var_mean_workspace_bytes(1025) == 8
    for kw in (dict(imgs=None), dict(first=None), dict(out=None)):
        assert variance(**kw) == 1 and b'null' in lib.t2o_last_error()
    assert variance(imgs=(ctypes.c_void_p * 10)(p, None)) == 1 and variance(first=(ctypes.c_void_p * 2)(p, None)) == 1
    assert variance(T=0) == 1 and variance(T=9) == 1
    assert variance(R=0) == 1 and variance(R=17, T=8) == 1 and b'R <= 16' in lib.t2o_last_error()
    assert variance(R=1, B=1) == 1 and b'fewer than two' in lib.t2o_last_error()          # N = 1
    assert variance(B=0) == 1 and variance(row=0) == 1
    assert variance(ws=None) == 3 and variance(row=4096, ws_bytes=3) == 3 and b'workspace' in lib.t2o_last_error()
    # the Python surface refuses CPU tensors, the table row included
    import t2onet_amd.functional as T
    img = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match='no CPU'):
        T.eval_metrics(img, [img], torch.zeros(1, dtype=torch.int64), img)
    with pytest.raises(RuntimeError, match='no CPU'):
        T.end_select_var_mean([[img], [img]], [torch.zeros(1, dtype=torch.int64)] * 2, out=torch.zeros(1))
