"""No-GPU checks of the masked planner path: the per-pixel masked term of t2o_pixel_math.h (masked_l1_term) walked over the
pixels as the two masked kernels walk them (tests/host_emul/emul_planner_mask.cpp, g++) against fp64 autograd of the
oracle's masked operator; the status codes of the two masked C entry points; plan_cli's GIER record writer and flags.

Tolerances are those of tests/test_block_programs_cpu.py::test_fused_l1, the operator + L1 form of the same pixel math
against the same fp64 oracle: loss 1e-6 absolute, parameter gradient rtol 1e-4 / atol 1e-7."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import cpu_ref, synth
from tests import planner_mask_cases as PM

OPT = cpu_ref.default_opt()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emul():
    out = os.path.join(ROOT, 'tests', '_build')
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, 'libt2o_emul_planner_mask.so')
    src = os.path.join(ROOT, 'tests', 'host_emul', 'emul_planner_mask.cpp')
    deps = [src] + [os.path.join(ROOT, 't2onet_amd', 'csrc', h) for h in ('t2o_pixel_math.h', 't2o_block_programs.h')]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = '%s.tmp.%d' % (so, os.getpid())
        subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-o', tmp, src])
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    lib.emul_fit_eval_masked.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.emul_cand_masked.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def _oracle64(op, img, p, mask_u8, tgt):
    """loss and parameter gradient of the oracle's masked operator + l1_loss in fp64; the mask value is float(byte)."""
    pp = p.double().clone().requires_grad_(True)
    m = None if mask_u8 is None else torch.from_numpy(mask_u8.astype(np.float64)).view(1, 1, *mask_u8.shape)
    loss = cpu_ref.l1_loss(cpu_ref.operator_apply(op, img.double(), pp, m, OPT), tgt.double())
    loss.backward()
    g = pp.grad if pp.grad is not None else torch.zeros_like(pp)
    return loss.item(), g.numpy()[0]


@pytest.mark.parametrize('shape', PM.SHAPES[:2])
@pytest.mark.parametrize('op', [0, 1, 2, 3, 5, 6])
def test_masked_pixel_term_against_fp64_autograd(emul, op, shape):
    H, W = shape
    img, tgt = synth.images(1, H, W, 11), synth.images(1, H, W, 12)
    n = cpu_ref.OP_NPARAM[op]
    stack = PM.planes(H, W)
    buf = np.zeros(stack.size + 1, np.uint8)                             # the planes packed: plane 1 starts at an odd byte for odd H W
    flat = buf[:stack.size]
    flat[:] = stack.reshape(-1)
    for si, setting in enumerate(['mid', 'strong']):
        p = synth.op_params(op, 1, 900 + 10 * op + si, setting)
        prow = np.zeros(24, np.float32)
        prow[:n] = p[0].numpy()
        for k, name in enumerate([None] + PM.PLANES):
            mask = None if name is None else stack[k - 1]
            ptr = None if name is None else flat[(k - 1) * H * W:].ctypes.data
            want_loss, want_g = _oracle64(op, img, p, mask, tgt)
            loss = ctypes.c_double()
            grad = np.zeros(24, np.float32)
            i32, t32 = np.ascontiguousarray(img[0].numpy()), np.ascontiguousarray(tgt[0].numpy())
            assert emul.emul_fit_eval_masked(op, i32.ctypes.data, t32.ctypes.data, prow.ctypes.data, ptr, H, W, ctypes.addressof(loss),
                                             grad.ctypes.data) == 0
            tag = 'op%d %s %s %s' % (op, shape, setting, name)
            assert abs(loss.value - want_loss) < 1e-6, tag
            np.testing.assert_allclose(grad[:n], want_g, rtol=1e-4, atol=1e-7, err_msg=tag)
            assert np.all(grad[n:] == 0)
            if name == 'zeros':
                assert np.all(grad == 0), tag                            # g_z carries the factor m: exactly zero
            if op != 6:                                                  # the sweep's thread functions: the same value
                sweep = ctypes.c_double()
                assert emul.emul_cand_masked(op, i32.ctypes.data, t32.ctypes.data, prow.ctypes.data, 24, ptr, H, W, ctypes.addressof(sweep)) == 0
                assert abs(sweep.value - want_loss) < 1e-6, tag


def test_white_under_a_mask(emul):
    """`white` has no parameter: the sweep's value under every plane against the oracle."""
    H, W = PM.SHAPES[1]
    img, tgt = synth.images(1, H, W, 13), synth.images(1, H, W, 14)
    stack = PM.planes(H, W)
    prow = np.zeros(24, np.float32)
    i32, t32 = np.ascontiguousarray(img[0].numpy()), np.ascontiguousarray(tgt[0].numpy())
    for k, name in enumerate(PM.PLANES):
        m = torch.from_numpy(stack[k].astype(np.float64)).view(1, 1, H, W)
        want = cpu_ref.l1_loss(cpu_ref.operator_apply(7, img.double(), torch.zeros(1, 1, dtype=torch.float64), m, OPT), tgt.double()).item()
        got = ctypes.c_double()
        plane = np.ascontiguousarray(stack[k])
        assert emul.emul_cand_masked(7, i32.ctypes.data, t32.ctypes.data, prow.ctypes.data, 24, plane.ctypes.data, H, W, ctypes.addressof(got)) == 0
        assert abs(got.value - want) < 1e-6, name


# ------------------------------------------------------------------ C ABI without a device
@pytest.fixture(scope='module')
def lib():
    from t2onet_amd import build, _lib
    build.build()
    return _lib.load()


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_masked_symbols_and_workspace_sizes(lib):
    for name in ('t2o_op_candidates_multi_l1_masked', 't2o_candidates_multi_masked_workspace_bytes', 't2o_fit_multi_l1_adam_masked',
                 't2o_fit_multi_masked_workspace_bytes'):
        assert hasattr(lib, name), name
    assert lib.t2o_abi_version() == 4
    fit, cand = lib.t2o_fit_multi_masked_workspace_bytes, lib.t2o_candidates_multi_masked_workspace_bytes
    assert fit(0, 8, 8) == 0 and fit(1, 0, 8) == 0 and cand(0, 64, 8, 8) == 0 and cand(1, 64, 0, 8) == 0
    for ws in (lambda J, h, w: fit(J, h, w), lambda J, h, w: cand(J, 64, h, w)):
        sizes = [ws(J, 128, 128) for J in (1, 2, 9, 63, 64)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))                 # monotone in J
        hw = [ws(9, h, w) for h, w in ((1, 1), (37, 53), (64, 64), (128, 128), (256, 256), (600, 900))]
        assert all(a <= b for a, b in zip(hw, hw[1:])) and hw[0] < hw[-1]                    # monotone in H W
    assert fit(9, 37, 53) == lib.t2o_fit_multi_workspace_bytes(9, 37, 53)
    assert cand(9, 64, 37, 53) == lib.t2o_candidates_multi_workspace_bytes(9, 64, 37, 53)


def test_masked_fit_rejects_bad_arguments_without_a_device(lib):
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    H = W = 8
    need = lib.t2o_fit_multi_masked_workspace_bytes(2, H, W)
    assert need <= buf.numel() * 4

    def call(ops=_ints(3, 6), img=_ints(0, 1), tgt=_ints(0, 0), mk=_ints(0, -1), J=2, imgs=p, n_img=2, targets=p, n_target=1, masks=p,
             n_mask=2, params=p, dist=p, ws=p, ws_bytes=need, steps=3):
        return lib.t2o_fit_multi_l1_adam_masked(ops, img, tgt, mk, J, imgs, n_img, targets, n_target, masks, n_mask, params, dist, ws,
                                                ws_bytes, H, W, steps, 2e-2, 0.9, 0.999, 1e-8, 50, 1e-6, None)
    for kw in (dict(ops=None), dict(img=None), dict(tgt=None), dict(mk=None), dict(imgs=None), dict(targets=None), dict(params=None),
               dict(dist=None)):
        assert call(**kw) == 1, kw
        assert b'null' in lib.t2o_last_error()
    assert call(J=0) == 1 and call(J=-1) == 1
    assert call(ops=_ints(*[3] * 65), img=_ints(*[0] * 65), tgt=_ints(*[0] * 65), mk=_ints(*[-1] * 65), J=65) == 1
    for bad in (4, 7, 8, -1, 99):                                        # what the unmasked fit refuses, with its status
        assert call(ops=_ints(3, bad)) == 2, bad
    assert call(img=_ints(0, 2)) == 1 and call(tgt=_ints(0, 1)) == 1
    assert call(mk=_ints(0, -2)) == 1 and call(mk=_ints(2, -1)) == 1 and call(mk=_ints(0, 0), n_mask=0) == 1
    assert b'mask_index' in lib.t2o_last_error()
    assert call(masks=None) == 1 and b'null' in lib.t2o_last_error()     # an index >= 0 needs the planes
    assert call(ws=None, ws_bytes=0) == 3 and call(ws_bytes=need - 1) == 3
    assert b'workspace' in lib.t2o_last_error()
    assert call(steps=-1) == 1
    # null planes with every index -1: accepted up to the launch (no argument or workspace status)
    assert call(masks=None, n_mask=0, mk=_ints(-1, -1)) in (0, 4)


def test_masked_sweep_rejects_bad_arguments_without_a_device(lib):
    buf = torch.zeros(8192)
    p = buf.data_ptr()
    H = W = 8
    C = 5
    need = lib.t2o_candidates_multi_masked_workspace_bytes(2, C, H, W)
    assert 0 < need <= buf.numel() * 4

    def call(ops=_ints(0, 3), img=_ints(0, 1), mk=_ints(1, -1), J=2, imgs=p, n_img=2, masks=p, n_mask=2, target=p, params=p, stride=24,
             loss=p, ws=p, ws_bytes=need):
        return lib.t2o_op_candidates_multi_l1_masked(ops, img, mk, J, imgs, n_img, masks, n_mask, target, params, C, stride, loss, ws,
                                                     ws_bytes, H, W, None)
    for kw in (dict(ops=None), dict(img=None), dict(mk=None), dict(imgs=None), dict(target=None), dict(params=None), dict(loss=None)):
        assert call(**kw) == 1, kw
        assert b'null' in lib.t2o_last_error()
    assert call(J=0) == 1 and call(J=-1) == 1
    assert call(ops=_ints(*[0] * 65), img=_ints(*[0] * 65), mk=_ints(*[-1] * 65), J=65) == 1
    for bad in (4, 6, 8, -1, 99):                                        # what the unmasked sweep refuses, with its status
        assert call(ops=_ints(0, bad)) == 2, bad
    assert call(img=_ints(0, 2)) == 1 and call(stride=8) == 1
    assert call(mk=_ints(-2, -1)) == 1 and call(mk=_ints(0, 2)) == 1 and call(mk=_ints(0, -1), n_mask=0) == 1
    assert b'mask_index' in lib.t2o_last_error()
    assert call(masks=None) == 1 and b'null' in lib.t2o_last_error()
    assert call(ws=None, ws_bytes=0) == 3 and call(ws_bytes=need - 1) == 3
    assert call(masks=None, n_mask=0, mk=_ints(-1, -1)) in (0, 4)


# ------------------------------------------------------------------ plan_cli --dataset GIER: records and flags
def _smooth(seed, size=64):
    g = torch.Generator().manual_seed(seed)
    small = torch.rand(1, 3, size // 8, size // 8, generator=g)
    return torch.nn.functional.interpolate(small, size=(size, size), mode='bilinear', align_corners=False).clamp(0, 1)


def test_written_gier_records_are_what_gierdatasetact_reads(tmp_path):
    """plan_cli.write_gier_record fed a hand-made planner result for every pair of the synthetic tree: GIERDatasetAct.get_act
    must return the operator ids, the parameters (max-abs rule for the curves, 0 for `white`) and exactly the edit images of
    the kept steps; 'local operators' is stored and ignored by the reader; an existing record is found again by its path."""
    from tests import gier_tree
    from t2onet_amd import gier, plan_cli
    data_dir, vocab_dir, _, _ = gier_tree.write_tree(str(tmp_path), n_train=4, n_val=1)
    save_dir = str(tmp_path / 'GIER_actions_set_1')
    rng = np.random.default_rng(5)
    color = [float(v) for v in rng.random(24) * 0.5 + 0.75]
    tone = [float(v) for v in rng.random(8) * 0.5 + 0.75]
    best = [('brightness', [0.4], 0.20), ('color', color, 0.12), ('white', [0.0], 0.08), ('tone', tone, 0.0799), ('sharpness', [0.4], 0.05)]
    other = [('contrast', [-0.1], 0.25)]
    init = 0.30
    # drops / init: 0.333, 0.267, 0.133, 0.0003 (not more than 1 %: stop) -> 3 steps are kept
    want_ops = np.array([1, 0 + 3, 3 + 3, 7 + 3, 2, 0, 0, 0, 0, 0])
    want_params = np.zeros((8, 24), dtype=np.float32)
    want_params[0, 0] = 0.4
    want_params[1] = np.array(color) / max(color)
    index = gier.GIER(data_dir, vocab_dir, 'train', 'valid', False, 3, 64)
    names = {i: index.op_data[i]['input'].split('_')[0] for i in range(len(index))}
    assert plan_cli.gier_todo(save_dir, names) == [0, 1, 2, 3]
    for i in range(len(index)):
        name = names[i]
        assert plan_cli.gier_todo(save_dir, names) == list(range(i, 4))      # resume: what has a record is skipped
        imgs = [_smooth(10 * i + k) for k in range(5)]
        assert not os.path.exists(plan_cli.gier_record_path(save_dir, name))
        info = plan_cli.write_gier_record(save_dir, name, ['a request', 'another'], init, [best, other], [imgs, imgs[:1]], _smooth(100 + i),
                                          _smooth(200 + i), ['brightness', 'white'])
        assert plan_cli.gier_record_path(save_dir, name) == os.path.join(save_dir, name, 'acts.json')
        with open(plan_cli.gier_record_path(save_dir, name)) as f:
            rec = json.load(f)
        assert rec == json.loads(json.dumps(info))
        assert set(rec) == {'request', 'init distance', 'operation sequence', 'local operators'}
        assert rec['local operators'] == ['brightness', 'white'] and rec['request'] == ['a request', 'another']
        assert [s[0] for s in rec['operation sequence'][0]] == [b[0] for b in best] and rec['operation sequence'][1] == [['contrast', [-0.1], 0.25]]
        assert rec['operation sequence'][0][2] == ['white', [0.0], 0.08]
        assert sorted(os.listdir(os.path.join(save_dir, name))) == ['acts.json'] + ['edit%d.jpg' % k for k in range(5)] + ['input.jpg', 'target.jpg']
    assert plan_cli.gier_todo(save_dir, names) == [] and plan_cli.gier_todo(save_dir, names, overwrite=True) == [0, 1, 2, 3]
    os.rename(plan_cli.gier_record_path(save_dir, names[2]), plan_cli.gier_record_path(save_dir, names[2]) + '.tmp')
    assert plan_cli.gier_todo(save_dir, names) == [2]                        # a record still under its temporary name is not done
    os.rename(plan_cli.gier_record_path(save_dir, names[2]) + '.tmp', plan_cli.gier_record_path(save_dir, names[2]))
    ds = gier.GIERDatasetAct(data_dir, vocab_dir, save_dir, 'train', 'valid', False, 3, 64)
    assert len(ds) > 0
    for item in range(len(ds)):
        ops, params, imgs = ds.get_act(item)
        assert np.array_equal(ops, want_ops) and np.allclose(params, want_params, atol=1e-7)
        assert all(float(imgs[k].abs().max()) > 0 for k in range(3)) and float(imgs[3:].abs().max()) == 0.0
        d = ds[item]
        assert d['output'].shape == (9, 3, 64, 64) and np.array_equal(d['operations'], want_ops)


def test_plan_cli_flags():
    from t2onet_amd import plan_cli
    d = plan_cli.parse_args([])
    assert (d.dataset, d.img_size, d.session, d.max_step, d.local) == ('FiveK', 128, 1, 6, False)      # the FiveK defaults, untouched
    g = plan_cli.parse_args(['--dataset', 'GIER'])
    assert (g.dataset, g.data_dir, g.vocab_dir, g.data_mode, g.session, g.img_size, g.local, g.overwrite) == (
        'GIER', 'data/GIER', 'data/language', 'global', 3, 256, False, False)
    loc = plan_cli.parse_args(['--dataset', 'GIER', '--local', '--img_size', '64', '--pairs_per_batch', '4', '--data_mode', 'valid', '--overwrite'])
    assert loc.local and loc.img_size == 64 and loc.pairs_per_batch == 4 and loc.data_mode == 'valid' and loc.overwrite
    assert plan_cli.GIER_LOCAL_OPERATIONS == [0, 1, 2, 3, 5, 6, 7] and plan_cli.OPERATIONS == [0, 1, 2, 3, 5, 6]
    with pytest.raises(SystemExit):
        plan_cli.parse_args(['--local'])                                 # FiveK has no masks
