"""No-GPU checks of the resident-set gather (t2o_resident.hip): the thread program of t2o_resident_math.h, compiled for the
host (tests/host_emul/emul_resident.cpp) and run for every thread of the grid, against the numpy statement; the byte round
trip the store's build rests on; the status codes of the C entry point; the --resident flag.  One fp32 division of an
integer: every comparison is exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import resident_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emul():
    out = os.path.join(ROOT, 'tests', '_build')
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, 'libt2o_emul_resident.so')
    src = os.path.join(ROOT, 'tests', 'host_emul', 'emul_resident.cpp')
    deps = [src] + [os.path.join(ROOT, 't2onet_amd', 'csrc', h) for h in ('t2o_resident_math.h', 't2o_image_math.h')]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = '%s.tmp.%d' % (so, os.getpid())
        subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-o', tmp, src])
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    lib.emul_gather_u8_to_f32.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    return lib


def nan_outputs(B, K, h, w, shift):
    """(whole, img_x, img_ys): NaN-filled outputs cut out of one buffer, `shift` floats past a 16-byte boundary, with spare
    floats around and between them that no thread may touch."""
    nx, ny = B * 3 * h * w, B * (K - 1) * 3 * h * w
    whole = RC.aligned_bytes(4 * (nx + ny + 24), 0).view(np.float32)
    whole[:] = np.nan
    x = whole[8 + shift:8 + shift + nx]
    y = whole[16 + shift + nx:16 + shift + nx + ny]
    return whole, x.reshape(B, 3, h, w), y.reshape(B, K - 1, 3, h, w)


@pytest.mark.parametrize('which', ['one', 'repeat', 'batch64'])
@pytest.mark.parametrize('size', RC.SIZES)
def test_thread_program_against_numpy(emul, size, which):
    h, w = size
    store, slots, _ = RC.case(h, w)
    index = RC.index_vectors()[which]
    want_x, want_ys = RC.expected(h, w, which)
    assert store.ctypes.data % 16 == 0 and (slots[slots >= 0] % 16 == 0).all()
    for shift in ((0, 1, 3) if h * w < 4096 else (0,)):                 # planes at every alignment a tensor view can have
        whole, x, ys = nan_outputs(len(index), RC.K, h, w, shift)
        rc = emul.emul_gather_u8_to_f32(store.ctypes.data, slots.ctypes.data, index.ctypes.data, RC.N, RC.K, len(index), h, w,
                                        x.ctypes.data, ys.ctypes.data)
        assert rc == 0
        assert not np.isnan(x).any() and not np.isnan(ys).any()         # every element written
        np.testing.assert_array_equal(x, want_x)
        np.testing.assert_array_equal(ys, want_ys)
        for b, i in enumerate(index):                                   # absent columns are exactly 0
            for k in range(1, RC.K):
                if slots[i, k] < 0:
                    assert not ys[b, k - 1].any()
        assert np.isnan(whole).sum() == 24                              # and nothing outside the two tensors was


def test_an_unaligned_slot_and_a_bad_index_stay_inside_their_bounds(emul):
    """Not ResidentFiveK's layout, but the program's own promise: a slot off the dword grid is read byte by byte, an index
    outside [0, N) reads nothing and gives zeros."""
    h, w = 5, 7
    store, slots, pictures = RC.case(h, w)
    moved = RC.aligned_bytes(store.size + 16, RC.GUARD)
    moved[1:1 + store.size] = store
    off = slots.copy()
    off[off >= 0] += 1
    index = np.array([3, RC.N, -1, 0], np.int64)
    whole, x, ys = nan_outputs(4, RC.K, h, w, 0)
    assert emul.emul_gather_u8_to_f32(moved.ctypes.data, off.ctypes.data, index.ctypes.data, RC.N, RC.K, 4, h, w, x.ctypes.data, ys.ctypes.data) == 0
    for b, i in enumerate(index):
        for k in range(RC.K):
            got = x[b] if k == 0 else ys[b, k - 1]
            pic = pictures.get((int(i), k))
            want = np.zeros((3, h, w), np.float32) if pic is None else pic.astype(np.float32).transpose(2, 0, 1) / np.float32(255)
            np.testing.assert_array_equal(got, want)


def test_byte_round_trip_in_fp32():
    """The store holds to_u8_hwc of the resized fp32 picture: trunc((b / 255) * 255) must give b back for all 256 bytes."""
    b = np.arange(256, dtype=np.uint8)
    unit = b.astype(np.float32) / np.float32(255)
    assert unit.dtype == np.float32
    back = (unit * np.float32(255)).astype(np.uint8)
    np.testing.assert_array_equal(back, b)
    import torch
    t = torch.arange(256, dtype=torch.float32) / 255.0
    assert torch.equal((t * 255.0).to(torch.uint8), torch.arange(256, dtype=torch.uint8))


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
    p = RC.aligned_bytes(256, 0).ctypes.data

    def gather(store=p, slots=p, index=p, N=6, K=7, B=2, h=4, w=4, x=p, ys=p):
        return lib.t2o_gather_u8_to_f32(store, slots, index, N, K, B, h, w, x, ys, None)
    for kw in (dict(store=None), dict(slots=None), dict(index=None), dict(x=None), dict(ys=None)):
        assert gather(**kw) == 1 and b'null' in lib.t2o_last_error()
    for kw in (dict(N=0), dict(K=0), dict(B=0), dict(h=0), dict(w=0), dict(N=-1), dict(K=-2), dict(B=-1), dict(h=-4), dict(w=-4)):
        assert gather(**kw) == 1 and b'positive' in lib.t2o_last_error()
    assert gather(K=9) == 1 and b'at most 8' in lib.t2o_last_error()
    for kw in (dict(store=p + 4), dict(slots=p + 4), dict(index=p + 4), dict(x=p + 2), dict(ys=p + 1)):
        assert gather(**kw) == 1 and b'aligned' in lib.t2o_last_error()
    # 2^31 - 1 workgroups: B K ceil(h w / 1024) -- one more is refused (the largest grid itself would launch)
    assert gather(B=1 << 20, K=8, h=1024, w=256) == 1 and b'2^31' in lib.t2o_last_error()
    assert gather(B=1 << 30, K=2, h=1, w=1) == 1 and b'2^31' in lib.t2o_last_error()
    # the Python surface refuses CPU tensors
    with pytest.raises(RuntimeError, match='no CPU'):
        T.gather_u8(torch.zeros(64, dtype=torch.uint8), torch.zeros(1, 7, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 2)


def test_resident_flag():
    from t2onet_amd import train_cli
    assert train_cli.parse_args(['--resident']).resident and not train_cli.parse_args([]).resident
    assert train_cli.parse_args(['--resident', '--device_resize', '--device_eval']).resident
    for bad in (['--resident', '--synthetic'], ['--resident', '--dataset', 'GIER']):
        with pytest.raises(SystemExit):
            train_cli.parse_args(bad)


def test_epoch_orders_without_a_device():
    """The order is the host's seeded permutation: another one per epoch, the same one per seed, ranks disjoint and level."""
    import torch
    from t2onet_amd import data
    a, b = data.epoch_order(11, 10, 0), data.epoch_order(11, 10, 1)
    assert sorted(a.tolist()) == list(range(11)) and a.tolist() != b.tolist()
    assert torch.equal(a, data.epoch_order(11, 10, 0)) and torch.equal(a, torch.randperm(11, generator=torch.Generator().manual_seed(10)))
    r0, r1 = data.epoch_order(11, 10, 3, 0, 2), data.epoch_order(11, 10, 3, 1, 2)
    assert len(r0) == len(r1) == 5 and not set(r0.tolist()) & set(r1.tolist())
    assert data.resident_slot_bytes(16) == 768 and data.resident_slot_bytes(33) == 3280 and data.resident_slot_bytes(33) % 16 == 0
