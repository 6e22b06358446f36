"""No-GPU checks of the mask kernels (t2o_mask.hip): the thread programs of t2o_mask_math.h, compiled for the host
(tests/host_emul/emul_mask.cpp) and run for every thread of the grid, against the numpy oracle (decode, nearest_index, sum);
the select program against Actor.get_gt_mask; the status codes of the two C entry points.  Integers throughout: every
comparison is exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import mask_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emul():
    out = os.path.join(ROOT, 'tests', '_build')
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, 'libt2o_emul_mask.so')
    src = os.path.join(ROOT, 'tests', 'host_emul', 'emul_mask.cpp')
    deps = [src] + [os.path.join(ROOT, 't2onet_amd', 'csrc', h) for h in ('t2o_mask_math.h', 't2o_pixel_math.h')]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = '%s.tmp.%d' % (so, os.getpid())
        subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-o', tmp, src])
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    lib.emul_rle_union_u8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_longlong]
    lib.emul_mask_select.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5
    return lib


def aligned_bytes(n, fill):
    """n bytes whose first one lies at a 16-byte boundary (so that a job's offset IS its alignment)."""
    raw = np.full(n + 16, fill, np.uint8)
    at = (-raw.ctypes.data) % 16
    return raw[at:at + n]


def run_union(lib, rles, jobs, total):
    from t2onet_amd import functional as T
    tables = T.pack_rle_union(rles, jobs, pin=False)
    host = aligned_bytes(tables.host.numel(), 0)
    host[:] = tables.host.numpy()
    buf = aligned_bytes(total, MC.GUARD)
    n_jobs, n_masks, n_sel, n_ends = tables.counts
    rc = lib.emul_rle_union_u8(host.ctypes.data, n_jobs, n_masks, n_sel, n_ends, buf.ctypes.data, total)
    assert rc == 0
    return buf


@pytest.mark.parametrize('align', [0, 1, 2, 3])
@pytest.mark.parametrize('src', MC.SRC_SIZES)
def test_union_program_against_the_numpy_oracle(emul, src, align):
    planes, rles, jobs, total = MC.source_case(src, align)
    assert {off % 4 for _, off, _, _ in jobs} == {0, 1, 2, 3}
    want = MC.expected_buffer(planes, jobs, total)                      # guard bytes around every plane included
    if src[0] >= 33:                                                    # overlapping and repeated masks are counted
        inside = np.concatenate([want[off:off + oh * ow] for _, off, oh, ow in jobs])
        assert inside.max() == 3 and (inside == 2).any()
    np.testing.assert_array_equal(run_union(emul, rles, jobs, total), want)


@pytest.mark.parametrize('n_jobs', [1, 7, 64])
def test_union_program_mixed_sizes_in_one_call(emul, n_jobs):
    planes, rles, jobs, total = MC.mixed_case(n_jobs)
    np.testing.assert_array_equal(run_union(emul, rles, jobs, total), MC.expected_buffer(planes, jobs, total))


def test_union_saturates_at_255(emul):
    planes, rles = MC.mask_set(7, 5)
    jobs, total = MC.layout([([1] * 300, 5, 9)])
    got = run_union(emul, rles, jobs, total)
    off = jobs[0][1]
    assert (got[off:off + 45] == 255).all() and (got[:off] == MC.GUARD).all() and (got[off + 45:] == MC.GUARD).all()


def select_case(H, W, seed=0):
    """B = 5, V = 11: operators present, absent, END, out of range (both sides); one plane holding a count of 2."""
    rng = np.random.default_rng(seed)
    B, V = 5, 11
    planes = (rng.random((4, H, W)) < 0.5).astype(np.uint8)
    planes[3] += (rng.random((H, W)) < 0.5).astype(np.uint8)             # 0 / 1 / 2
    mask_dict = [{'3': [planes[0].astype(np.float32)[None]], '9': [planes[1].astype(np.float32)[None]]}, {},
                 {'6': [planes[2].astype(np.float32)[None]]}, {'8': [planes[3].astype(np.float32)[None]]}, {'4': [planes[0].astype(np.float32)[None]]}]
    ops = np.array([9, 5, 2, 8, 4], np.int64)                            # present, absent (no dict), END, present (count 2), present
    wild = np.array([11, -1, 6, 1 << 40, 3], np.int64)                   # out of range, negative, present, far out, absent
    return B, V, planes, mask_dict, ops, wild


@pytest.mark.parametrize('H,W', [(1, 1), (33, 47), (32, 32)])
def test_select_program_against_get_gt_mask(emul, H, W):
    from t2onet_amd import default_options
    from t2onet_amd.actor import Actor
    from t2onet_amd.gier import MaskTable
    B, V, planes, mask_dict, ops, wild = select_case(H, W)
    slot = np.full((B, V), -1, np.int32)
    table_planes = []
    for b, entry in enumerate(mask_dict):
        for key, v in entry.items():
            slot[b, int(key)] = len(table_planes)
            table_planes.append(np.asarray(v[0][0], np.uint8))
    stack = np.ascontiguousarray(np.stack(table_planes))
    actor = Actor.__new__(Actor)                                         # get_gt_mask uses no state
    img = torch.zeros(B, 3, H, W)
    for chosen in (ops, wild):
        want = Actor.get_gt_mask(actor, img, mask_dict, chosen.reshape(B, 1))[:, :1].numpy()
        np.testing.assert_array_equal(want, MC.gt_mask_reference(mask_dict, chosen, H, W) if chosen is ops else want)
        for shift in (0, 1, 2, 3):                                       # every 16-byte alignment of the output
            raw = aligned_bytes(4 * (B * H * W + 8), 0).view(np.float32)
            raw[:] = -7.0
            out = raw[shift:shift + B * H * W]
            rc = emul.emul_mask_select(stack.ctypes.data, slot.ctypes.data, chosen.ctypes.data, out.ctypes.data, len(stack), B, V, H, W)
            assert rc == 0
            np.testing.assert_array_equal(out.reshape(B, 1, H, W), want)
            assert (raw[:shift] == -7.0).all() and (raw[shift + B * H * W:] == -7.0).all()


def _library():
    from t2onet_amd import build, _lib
    if os.path.exists(build.hipcc_path()):
        build.build()
    elif not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libt2onet_hip.so is absent and there is no hipcc to build it')
    return _lib.load()


def test_status_codes_before_any_launch():
    """Every refusal returns before a launch: all pointers below are host memory and no device is needed."""
    from t2onet_amd import functional as T
    lib = _library()
    assert lib.t2o_abi_version() == 4
    planes, rles = MC.mask_set(7, 5)
    out = aligned_bytes(64, 0)

    def union(masks=None, jobs=None, out_ptr=out.ctypes.data, out_bytes=64, edit=None, null_tables=False, n_jobs=None):
        t = T.pack_rle_union(rles if masks is None else masks, [([4, 5], 3, 5, 9)] if jobs is None else jobs, pin=False)
        host = aligned_bytes(t.host.numel(), 0)
        host[:] = t.host.numpy()
        if edit is not None:
            edit(host, t)
        n, m, s, e = t.counts
        p = None if null_tables else host.ctypes.data
        return lib.t2o_rle_union_u8(p, p, n if n_jobs is None else n_jobs, m, s, e, out_ptr, out_bytes, None)
    assert union(null_tables=True) == 1 and b'null' in lib.t2o_last_error()
    assert union(out_ptr=None) == 1 and b'null' in lib.t2o_last_error()
    assert union(n_jobs=0) == 1 and union(n_jobs=65536) == 1 and b'65535' in lib.t2o_last_error()
    assert union(out_bytes=0) == 1
    # h * w >= 2^31 (the runs agree with the size: only the size is refused)
    big = [(np.array([1 << 31], np.int64), 1 << 16, 1 << 15)]
    assert union(masks=big, jobs=[([0], 0, 2, 2)]) == 1 and b'2^31' in lib.t2o_last_error()
    # a last cumulative end that is not h * w; run ends that decrease
    assert union(masks=[(np.array([30, 4]), 7, 5)], jobs=[([0], 0, 2, 2)]) == 1 and b'add up' in lib.t2o_last_error()
    assert union(masks=[(np.array([36]), 7, 5)], jobs=[([0], 0, 2, 2)]) == 1 and b'add up' in lib.t2o_last_error()

    def decreasing(host, t):
        ends = host[24 + 16:24 + 16 + 4 * 4].view(np.uint32)              # 1 job, 1 mask, 0 selections: the ends follow
        ends[1] = ends[0] - 1
    assert union(masks=[(np.array([10, 5, 10, 10]), 7, 5)], jobs=[([], 0, 2, 2)], edit=decreasing) == 1 and b'decrease' in lib.t2o_last_error()
    # a selection index outside the mask table, on either side
    assert union(jobs=[([6], 0, 5, 9)]) == 1 and b'selection index' in lib.t2o_last_error()
    assert union(jobs=[([-1], 0, 5, 9)]) == 1 and b'selection index' in lib.t2o_last_error()
    # sizes that are not positive: output planes and masks
    assert union(jobs=[([0], 0, 0, 9)]) == 1 and union(jobs=[([0], 0, 5, -1)]) == 1 and b'positive' in lib.t2o_last_error()
    assert union(masks=[(np.array([0]), 0, 5)], jobs=[([0], 0, 2, 2)]) == 1 and b'positive' in lib.t2o_last_error()
    assert union(masks=[(np.zeros(0), 7, 5)], jobs=[([0], 0, 2, 2)]) == 1 and b'positive' in lib.t2o_last_error()
    # a plane outside the output buffer
    assert union(jobs=[([0], 20, 5, 9)]) == 1 and union(jobs=[([0], -1, 5, 9)]) == 1 and b'outside the output' in lib.t2o_last_error()

    p = out.ctypes.data

    def select(planes=p, slot=p, op=p, o=p, N=1, B=1, V=11, H=2, W=2):
        return lib.t2o_mask_select(planes, slot, op, o, N, B, V, H, W, None)
    for kw in (dict(slot=None), dict(op=None), dict(o=None), dict(planes=None)):
        assert select(**kw) == 1 and b'null' in lib.t2o_last_error()
    assert select(B=0) == 1 and select(V=0) == 1 and select(H=0) == 1 and select(W=-3) == 1 and select(N=-1) == 1
    assert select(H=1 << 16, W=1 << 15) == 1 and b'2^31' in lib.t2o_last_error()
    assert select(o=p + 2) == 1 and b'aligned' in lib.t2o_last_error()
    # the Python surface refuses CPU tensors
    with pytest.raises(RuntimeError, match='no CPU'):
        T.mask_select(torch.zeros(1, 2, 2, dtype=torch.uint8), torch.zeros(1, 11, dtype=torch.int32), torch.zeros(1, dtype=torch.int64))
