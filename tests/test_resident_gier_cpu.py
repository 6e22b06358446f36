"""No-GPU checks of the resident-item gather (t2o_resident_items.hip): the thread program of t2o_resident_items_math.h,
compiled for the host (tests/host_emul/emul_resident_items.cpp) and run for every thread of the flat grid -- picture
workgroups and the appended row workgroups -- against the numpy statement and, for K <= 8, against the emulation of the
existing gather; the status codes of the C entry point; the --resident_gier flag.  One fp32 division of an integer and an
int32 copy: every comparison is exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import resident_gier_cases as GC
from tests.resident_cases import aligned_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('t2o_resident_items_math.h', 't2o_resident_math.h', 't2o_image_math.h')


def build_emulation(stem):
    """tests/host_emul/<stem>.cpp as tests/_build/libt2o_<stem>.so (g++), rebuilt when a source is newer."""
    out = os.path.join(ROOT, 'tests', '_build')
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, 'libt2o_%s.so' % stem)
    src = os.path.join(ROOT, 'tests', 'host_emul', stem + '.cpp')
    deps = [src] + [os.path.join(ROOT, 't2onet_amd', 'csrc', h) for h in HEADERS]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = '%s.tmp.%d' % (so, os.getpid())
        subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-o', tmp, src])
        os.replace(tmp, so)
    return ctypes.CDLL(so)


@pytest.fixture(scope='module')
def emul():
    lib = build_emulation('emul_resident_items')
    lib.emul_gather_items_u8_to_f32.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2
    return lib


@pytest.fixture(scope='module')
def emul_gather():
    lib = build_emulation('emul_resident')
    lib.emul_gather_u8_to_f32.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    return lib


ROW_GUARD = -77


def guarded_outputs(B, K, V, h, w, shift):
    """(whole, img_x, img_ys, rows_whole, out_rows): NaN-filled picture outputs cut out of one buffer, `shift` floats past a
    16-byte boundary, with spare floats around and between them; an int32 buffer of ROW_GUARD with the row output in its
    middle.  No thread may touch the spare elements."""
    nx, ny = B * 3 * h * w, B * (K - 1) * 3 * h * w
    whole = aligned_bytes(4 * (nx + ny + 24), 0).view(np.float32)
    whole[:] = np.nan
    x = whole[8 + shift:8 + shift + nx]
    y = whole[16 + shift + nx:16 + shift + nx + ny]
    rows_whole = np.full(B * V + 10, ROW_GUARD, np.int32)
    r = rows_whole[5:5 + B * V]
    return whole, x.reshape(B, 3, h, w), y.reshape(B, K - 1, 3, h, w), rows_whole, r.reshape(B, V)


@pytest.mark.parametrize('V', GC.VS)
@pytest.mark.parametrize('K', GC.KS)
@pytest.mark.parametrize('size', GC.SIZES)
def test_thread_program_against_numpy(emul, emul_gather, size, K, V):
    h, w = size
    store, slots = GC.case(h, w, K)
    table = GC.rows(V)
    assert store.ctypes.data % 16 == 0 and (slots[slots >= 0] % 16 == 0).all()
    for which, index in GC.index_vectors().items():
        B = len(index)
        want_x, want_ys = GC.expected(h, w, K, which)
        for shift in ((0, 1, 3) if which == 'repeat' else (0,)):        # planes at every alignment a tensor view can have
            whole, x, ys, rows_whole, out_rows = guarded_outputs(B, K, V, h, w, shift)
            grid = ctypes.c_longlong(0)
            rc = emul.emul_gather_items_u8_to_f32(store.ctypes.data, slots.ctypes.data, index.ctypes.data, GC.N, K, B, h, w,
                                                  x.ctypes.data, ys.ctypes.data if K > 1 else None, table.ctypes.data if V else None,
                                                  V, out_rows.ctypes.data if V else None, ctypes.addressof(grid))
            assert rc == 0
            # the flat grid: the existing entry's picture workgroups, then the row workgroups
            assert grid.value == B * K * ((h * w + 1023) // 1024) + (B * V + 255) // 256
            assert not np.isnan(x).any() and not np.isnan(ys).any()     # every element written
            np.testing.assert_array_equal(x, want_x)
            np.testing.assert_array_equal(ys, want_ys)
            assert np.isnan(whole).sum() == 24                          # and nothing outside the two tensors was
            np.testing.assert_array_equal(out_rows, GC.expected_rows(V, which))
            assert (rows_whole[:5] == ROW_GUARD).all() and (rows_whole[5 + B * V:] == ROW_GUARD).all()
            for b, i in enumerate(index):                               # absent columns and bad indices: exactly 0 / -1
                if not 0 <= i < GC.N:
                    assert not x[b].any() and not ys[b].any() and (out_rows[b] == -1).all()
                    continue
                for k in range(1, K):
                    if slots[i, k] < 0:
                        assert not ys[b, k - 1].any()
        if K <= 8 and which != 'bad':                                   # the existing gather's emulation: the same bits
            _, x2, ys2, _, _ = guarded_outputs(B, K, 0, h, w, 0)
            assert emul_gather.emul_gather_u8_to_f32(store.ctypes.data, slots.ctypes.data, index.ctypes.data, GC.N, K, B, h, w,
                                                     x2.ctypes.data, ys2.ctypes.data if K > 1 else None) == 0
            assert x.tobytes() == x2.tobytes() and ys.tobytes() == ys2.tobytes()


def test_items_that_share_slots_get_the_same_pictures(emul):
    """The cases' sharing, said outright: items 1 and 2 are one pair; items 0 and 1 differ in the target only."""
    h, w, K = 5, 7, 10
    store, slots = GC.case(h, w, K)
    index = np.array([0, 1, 2], np.int64)
    _, x, ys, _, _ = guarded_outputs(3, K, 0, h, w, 0)
    assert emul.emul_gather_items_u8_to_f32(store.ctypes.data, slots.ctypes.data, index.ctypes.data, GC.N, K, 3, h, w,
                                            x.ctypes.data, ys.ctypes.data, None, 0, None, None) == 0
    assert len(np.unique(slots[slots >= 0])) < (slots >= 0).sum()
    np.testing.assert_array_equal(x[0], x[1])
    np.testing.assert_array_equal(ys[0, :K - 2], ys[1, :K - 2])
    assert (ys[0, K - 2] != ys[1, K - 2]).any()
    np.testing.assert_array_equal(ys[1], ys[2])


def _library():
    from t2onet_amd import build, _lib
    if os.path.exists(build.hipcc_path()):
        build.build()
    elif not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libt2onet_hip.so is absent and there is no hipcc to build it')
    return _lib.load()


def test_status_codes_before_any_launch():
    """Every refusal returns before a launch: all pointers below are host memory and no device is needed."""
    import torch
    from t2onet_amd import functional as T
    lib = _library()
    assert lib.t2o_abi_version() == 4
    p = aligned_bytes(256, 0).ctypes.data

    def gather(store=p, slots=p, index=p, N=6, K=10, B=2, h=4, w=4, x=p, ys=p, rows=p, V=3, out_rows=p):
        return lib.t2o_gather_items_u8_to_f32(store, slots, index, N, K, B, h, w, x, ys, rows, V, out_rows, None)
    for kw in (dict(store=None), dict(slots=None), dict(index=None), dict(x=None), dict(ys=None)):
        assert gather(**kw) == 1 and b'null' in lib.t2o_last_error()
    for kw in (dict(N=0), dict(K=0), dict(B=0), dict(h=0), dict(w=0), dict(N=-1), dict(K=-2), dict(B=-1), dict(h=-4), dict(w=-4)):
        assert gather(**kw) == 1 and b'positive' in lib.t2o_last_error()
    assert gather(K=17) == 1 and b'at most 16' in lib.t2o_last_error()
    assert gather(V=-1) == 1 and b'negative' in lib.t2o_last_error()
    assert gather(V=-1, rows=None, out_rows=None) == 1 and b'negative' in lib.t2o_last_error()
    for kw in (dict(out_rows=None), dict(rows=None), dict(V=0), dict(V=0, rows=None), dict(V=0, out_rows=None),
               dict(rows=None, out_rows=None)):
        assert gather(**kw) == 1 and b'do not agree' in lib.t2o_last_error()
    for kw in (dict(store=p + 4), dict(slots=p + 4), dict(index=p + 4), dict(x=p + 2), dict(ys=p + 1), dict(rows=p + 2), dict(out_rows=p + 1)):
        assert gather(**kw) == 1 and b'aligned' in lib.t2o_last_error()
    # 2^31 - 1 workgroups: B K ceil(h w / 1024) + ceil(B V / 256) -- one more is refused (the largest grid itself would launch)
    none = dict(rows=None, V=0, out_rows=None)
    assert gather(B=1 << 20, K=16, h=1024, w=128, **none) == 1 and b'2^31' in lib.t2o_last_error()
    assert gather(B=1 << 30, K=2, h=1, w=1, **none) == 1 and b'2^31' in lib.t2o_last_error()
    # the pictures alone fit (2^31 - 16 workgroups); the 2^19 row workgroups of V = 1 push the grid over
    B = (1 << 27) - 1
    assert gather(B=B, K=16, h=1, w=1, V=1) == 1 and b'2^31' in lib.t2o_last_error()
    assert gather(B=1 << 30, K=1, h=1, w=1, V=1 << 30) == 1 and b'2^31' in lib.t2o_last_error()
    # the existing entry keeps its own bound
    assert lib.t2o_gather_u8_to_f32(p, p, p, 6, 9, 2, 4, 4, p, p, None) == 1 and b'at most 8' in lib.t2o_last_error()
    # the Python surface refuses CPU tensors
    with pytest.raises(RuntimeError, match='no CPU'):
        T.gather_items_u8(torch.zeros(64, dtype=torch.uint8), torch.zeros(1, 10, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 2)


def test_grid_overflow_is_counted_with_the_row_workgroups(emul):
    """The entry point's own check, asked for the grid alone: the largest B whose picture AND row workgroups number at most
    2^31 - 1 passes with exactly that count, the next B is refused -- although its picture workgroups alone would fit."""
    emul.emul_items_grid.restype = ctypes.c_longlong
    emul.emul_items_grid.argtypes = [ctypes.c_int] * 6
    limit = (1 << 31) - 1
    for K, h, w, V in ((1, 1, 1, 1), (16, 1, 1, 11), (10, 40, 30, 11), (3, 33, 31, 300)):
        def grid(B):
            return B * K * ((h * w + 1023) // 1024) + (B * V + 255) // 256
        lo, hi = 1, limit                                               # grid(lo) <= limit < grid(hi + 1)
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if grid(mid) <= limit else (lo, mid - 1)
        assert emul.emul_items_grid(6, K, lo, h, w, V) == grid(lo) <= limit
        assert lo * K * ((h * w + 1023) // 1024) < grid(lo)
        assert emul.emul_items_grid(6, K, lo + 1, h, w, V) == -1 and (lo + 1) * K * ((h * w + 1023) // 1024) <= limit
    assert emul.emul_items_grid(6, 1, limit, 1, 1, 0) == limit          # no rows: the existing entry's bound
    assert emul.emul_items_grid(6, 17, 1, 1, 1, 0) == -1 and emul.emul_items_grid(6, 16, 1, 1, 1, -1) == -1


def test_resident_gier_flag():
    from t2onet_amd import train_cli
    a = train_cli.parse_args(['--dataset', 'GIER', '--resident_gier'])
    assert a.resident_gier and not a.load_mask and not a.resident
    assert train_cli.parse_args(['--dataset', 'GIER', '--resident_gier', '--load_mask']).load_mask
    assert not train_cli.parse_args(['--dataset', 'GIER']).resident_gier and not train_cli.parse_args([]).resident_gier
    for bad in (['--resident_gier'], ['--resident_gier', '--dataset', 'FiveK'],
                ['--dataset', 'GIER', '--resident_gier', '--synthetic'], ['--dataset', 'GIER', '--resident_gier', '--device_resize'],
                ['--dataset', 'GIER', '--resident_gier', '--resident'], ['--resident', '--dataset', 'GIER']):
        with pytest.raises(SystemExit):
            train_cli.parse_args(bad)
