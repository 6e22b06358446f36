"""No-GPU checks of the batched planner fit's C ABI (argument validation, workspace size) and of the action-set
generator's record writer (t2onet_amd/plan_cli.py): what it writes is what data.FiveKAct reads."""
import ctypes
import io
import json
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def lib():
    from t2onet_amd import build, _lib
    build.build()
    return _lib.load()


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_fit_symbols_and_workspace_size(lib):
    assert lib.t2o_fit_multi_l1_adam is not None and lib.t2o_fit_multi_workspace_bytes is not None
    assert lib.t2o_abi_version() == 4
    ws = lib.t2o_fit_multi_workspace_bytes
    assert ws(0, 128, 128) == 0 and ws(1, 0, 128) == 0 and ws(1, 128, 0) == 0
    sizes = [ws(J, 128, 128) for J in (1, 2, 9, 63, 64)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))                 # monotone in J
    hw = [ws(9, h, w) for h, w in ((1, 1), (37, 53), (64, 64), (128, 128), (256, 256), (600, 900))]
    assert all(a <= b for a, b in zip(hw, hw[1:])) and hw[0] < hw[-1]                    # monotone in H W
    # room for Adam's two moments of every padded parameter at the very least
    assert ws(64, 1, 1) >= 64 * 2 * 24 * 4


def test_fit_rejects_bad_arguments_without_a_device(lib):
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    H = W = 8
    need = lib.t2o_fit_multi_workspace_bytes(2, H, W)
    assert need <= buf.numel() * 4

    def call(ops=_ints(3, 6), img=_ints(0, 1), tgt=_ints(0, 0), J=2, imgs=p, n_img=2, targets=p, n_target=1, params=p, dist=p,
             ws=p, ws_bytes=need, steps=3):
        return lib.t2o_fit_multi_l1_adam(ops, img, tgt, J, imgs, n_img, targets, n_target, params, dist, ws, ws_bytes, H, W, steps,
                                         2e-2, 0.9, 0.999, 1e-8, 50, 1e-6, None)
    # null pointers
    for kw in (dict(ops=None), dict(img=None), dict(tgt=None), dict(imgs=None), dict(targets=None), dict(params=None), dict(dist=None)):
        assert call(**kw) == 1, kw
        assert b'null' in lib.t2o_last_error()
    # J outside 1..64
    assert call(J=0) == 1 and call(J=-1) == 1
    assert call(ops=_ints(*[3] * 65), img=_ints(*[0] * 65), tgt=_ints(*[0] * 65), J=65) == 1
    # inpaint has no parameter to fit; 7 (white) neither; unknown operators
    for bad in (4, 7, 8, -1, 99):
        assert call(ops=_ints(3, bad)) == 2, bad
    # indices out of range
    assert call(img=_ints(0, 2)) == 1 and call(img=_ints(-1, 0)) == 1
    assert call(tgt=_ints(0, 1)) == 1 and call(tgt=_ints(-1, 0)) == 1
    # workspace missing / too small
    assert call(ws=None, ws_bytes=0) == 3
    assert call(ws_bytes=need - 1) == 3
    assert b'workspace' in lib.t2o_last_error()
    # negative iteration count
    assert call(steps=-1) == 1


def _smooth(seed, size=128):
    g = torch.Generator().manual_seed(seed)
    small = torch.rand(1, 3, size // 8, size // 8, generator=g)
    return torch.nn.functional.interpolate(small, size=(size, size), mode='bilinear', align_corners=False).clamp(0, 1)


def _jpeg_roundtrip(t):
    """The tensor through PIL's JPEG encoder at PIL's default quality, in this test -- not through the writer under test."""
    from PIL import Image
    u8 = (t.reshape(3, *t.shape[-2:]).permute(1, 2, 0) * 255).numpy().astype(np.uint8)
    bio = io.BytesIO()
    Image.fromarray(u8).save(bio, format='JPEG')
    back = np.asarray(Image.open(io.BytesIO(bio.getvalue())).convert('RGB'), dtype=np.float32) / 255.0
    return torch.from_numpy(back.transpose(2, 0, 1))


def test_written_records_are_what_fivekact_reads(tmp_path):
    """plan_cli.write_record fed a hand-made planner result: two surviving sequences, the best one with a 24-parameter
    step and a third step that improves by less than 1 % of the initial distance.  data.parse_action_record / FiveKAct
    must return the operator ids, padded parameters and truncation that analyze_traj prescribes for these numbers (worked
    out by hand below), and the reloaded edit images must be within JPEG error of the tensors handed to the writer.

    JPEG bound: the same tensors encoded in this test by PIL at its DEFAULT quality and decoded again; a writer that
    encodes at no less than that quality from the reference's 8-bit rounding stays within that error plus one grey level
    (the truncation to 8 bits), in the mean and in the maximum."""
    from tests import fivek_tree
    from t2onet_amd import data, plan_cli
    img_dir, anno_dir, act_dir, _ = fivek_tree.write_tree(str(tmp_path), n_train=4, n_val=1)
    rng = np.random.default_rng(5)
    color = [float(v) for v in rng.random(24) * 0.5 + 0.75]
    tone = [float(v) for v in rng.random(8) * 0.5 + 0.75]
    best = [('brightness', [0.2], 0.20), ('color', color, 0.12), ('tone', tone, 0.1195), ('sharpness', [0.4], 0.08)]
    other = [('contrast', [-0.1], 0.25), ('saturation', [7.0], 0.21)]
    init = 0.30
    # drops / init: 0.333, 0.267, 0.0017 (not more than 1 %: stop), ... -> 2 steps are kept
    want_ops = np.array([1, 0 + 3, 3 + 3, 2, 0, 0, 0])
    want_params = np.zeros((5, 24), dtype=np.float32)
    want_params[0, 0] = 0.2
    want_params[1] = np.array(color) / max(color)
    for i in range(4):
        imgs = [_smooth(10 * i + k) for k in range(4)]
        x, y = _smooth(100 + i), _smooth(200 + i)
        info = plan_cli.write_record(act_dir, 'train', i, 'make it %d' % i, init, [best, other], [imgs, imgs[:2]], x, y)
        with open(os.path.join(act_dir, 'train%d' % i, '%05d.json' % i)) as f:
            rec = json.load(f)
        assert rec == json.loads(json.dumps(info))
        assert set(rec) == {'request', 'init distance', 'operation sequence'} and rec['request'] == 'make it %d' % i
        assert len(rec['operation sequence']) == 2 and [s[0] for s in rec['operation sequence'][0]] == [b[0] for b in best]
        assert rec['operation sequence'][0][1][1] == color and rec['operation sequence'][1][1] == ['saturation', [7.0], 0.21]
        ops, params, n = data.parse_action_record(rec)
        assert n == 2 and np.array_equal(ops, want_ops)
        assert params.shape == (5, 24) and np.allclose(params, want_params, atol=1e-7)
        for name in ('input.jpg', 'target.jpg', 'edit0.jpg', 'edit1.jpg', 'edit2.jpg', 'edit3.jpg'):
            assert os.path.exists(os.path.join(act_dir, 'train%d' % i, name)), name
    ds = data.FiveKAct(img_dir, anno_dir, act_dir, 'train', 1, 128)
    for i in range(4):
        _, imgs_y, _, ops, params, req = ds[i]
        assert np.array_equal(ops, want_ops) and np.allclose(params, want_params, atol=1e-7) and req == 'make it %d' % i
        assert float(imgs_y[2:5].abs().max()) == 0.0                                  # truncated steps are not loaded
        for k in range(2):
            t = _smooth(10 * i + k)[0]
            ref = (_jpeg_roundtrip(t) - t).abs()
            got = (imgs_y[k] - t).abs()
            print('item %d edit%d: max err %.4f (bound %.4f), mean err %.5f (bound %.5f)' % (
                i, k, got.max(), ref.max() + 1 / 255, got.mean(), ref.mean() + 1 / 255))
            assert got.max() <= ref.max() + 1 / 255 and got.mean() <= ref.mean() + 1 / 255
    # the saturation value beyond +-5 of the other sequence would be replaced by 0 (FiveKdataset.py:86-116) if it led
    rec['operation sequence'] = rec['operation sequence'][::-1]
    ops, params, n = data.parse_action_record(rec)
    assert n == 2 and list(ops[:4]) == [1, 1 + 3, 2 + 3, 2] and params[0, 0] == np.float32(-0.1) and params[1, 0] == 0.0


def test_tensor2img_rounds_like_the_reference():
    """utils/visual_utils.py:50-58: * 255 and truncation to uint8 (no rounding to nearest), channels last; RGB here."""
    from t2onet_amd import plan_cli
    t = torch.tensor([0.0, 0.5, 0.999, 1.0, 0.25, 0.75]).view(1, 3, 1, 2)
    out = plan_cli.tensor2img(t)
    assert out.dtype == np.uint8 and out.shape == (1, 2, 3)
    assert out[0, 0].tolist() == [0, 254, 63] and out[0, 1].tolist() == [127, 255, 191]
