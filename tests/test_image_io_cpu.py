"""No-GPU checks of the device data step (t2o_image_io.hip): the kernels' per-pixel program, compiled for the host from
the shared header, against data.resize_linear_u8 and the numpy conversions EXACTLY; argument validation of the two C-ABI
entry points; the packing of raw batches."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (16, 24), (37, 53), (3, 501)]
OUTPUTS = [(1, 1), (8, 12), (13, 17), (31, 17), (2, 8), (64, 64)]


@pytest.fixture(scope='module')
def emul():
    out = os.path.join(ROOT, 'tests', '_build')
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, 'libt2o_emul_image.so')
    src = os.path.join(ROOT, 'tests', 'host_emul', 'emul_image.cpp')
    deps = [src, os.path.join(ROOT, 't2onet_amd', 'csrc', 't2o_image_math.h')]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = '%s.tmp.%d' % (so, os.getpid())
        subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-o', tmp, src])
        os.replace(tmp, so)
    return ctypes.CDLL(so)


def source_images(shape, seed):
    """Random bytes, all 0 and all 255 of one (H, W)."""
    h, w = shape
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)]


def numpy_path(img, oh, ow):
    from t2onet_amd import data
    return data.resize_linear_u8(img, oh, ow).astype(np.float32).transpose(2, 0, 1) / 255.0


def _emul_resize(lib, img, oh, ow):
    img = np.ascontiguousarray(img)
    out = np.full((3, oh, ow), np.nan, np.float32)
    rc = lib.emul_resize_u8_f32(img.ctypes.data_as(ctypes.c_void_p), img.shape[0], img.shape[1], oh, ow,
                                out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


@pytest.mark.parametrize('src', SOURCES)
def test_block_program_equals_numpy_resize(emul, src):
    for k, img in enumerate(source_images(src, 11 + 97 * SOURCES.index(src))):
        for oh, ow in OUTPUTS:
            got, want = _emul_resize(emul, img, oh, ow), numpy_path(img, oh, ow)
            assert want.dtype == np.float32
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (src, (oh, ow), k)


def test_block_program_all_byte_values(emul):
    """The /255 conversion over every byte value (a same-size source is a plain convert)."""
    img = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3) % 256
    img = img.astype(np.uint8)
    got = _emul_resize(emul, img, 16, 16)
    assert np.array_equal(got.view(np.uint32), numpy_path(img, 16, 16).view(np.uint32))
    assert len(np.unique(img)) == 256


def edge_values():
    """k/255, the neighbouring floats on both sides of each, 0 and 1 -- clipped to [0, 1]."""
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    v = np.concatenate([k, np.nextafter(k, np.float32(-1.0)), np.nextafter(k, np.float32(2.0)), np.float32([0.0, 1.0])])
    return np.clip(v, 0.0, 1.0).astype(np.float32)


def test_block_program_inverse_conversion(emul):
    rng = np.random.default_rng(5)
    v = np.concatenate([edge_values(), rng.random(4096, dtype=np.float32)])
    want = torch.from_numpy(v).mul(255).numpy().astype(np.uint8)
    got = np.full(v.size, 77, np.uint8)
    assert emul.emul_unit_to_u8(v.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(v.size), got.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(got, want)
    assert np.array_equal(want, (v * np.float32(255.0)).astype(np.uint8))


def test_cabi_validates_before_any_device_call():
    from t2onet_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert lib.t2o_abi_version() == 4
    p = torch.zeros(64).data_ptr()
    for args in ((None, p, 1, 4, 4, p), (p, None, 1, 4, 4, p), (p, p, 1, 4, 4, None), (p, p, 0, 4, 4, p), (p, p, -1, 4, 4, p),
                 (p, p, 1, 0, 4, p), (p, p, 1, 4, 0, p), (p, p, 1, -3, 4, p), (p, p, 1, 4, -3, p)):
        assert lib.t2o_resize_u8_to_f32(*args, None) == 1, args
        assert b'resize_u8_to_f32' in lib.t2o_last_error()
    for args in ((None, 1, 4, 4, p), (p, 1, 4, 4, None), (p, 0, 4, 4, p), (p, -1, 4, 4, p), (p, 1, 0, 4, p), (p, 1, 4, 0, p),
                 (p, 1, -1, 4, p), (p, 1, 4, -1, p)):
        assert lib.t2o_f32_to_u8_hwc(*args, None) == 1, args
        assert b'f32_to_u8_hwc' in lib.t2o_last_error()
    assert lib.t2o_f32_to_u8_hwc(None, 1, 4, 4, p, None) == 1 and b'null' in lib.t2o_last_error()


def test_pack_u8_layout_and_descriptor_checks():
    import t2onet_amd.functional as T
    imgs = [a[0] for a in (source_images(s, 3) for s in SOURCES[:5])]
    buffer, descs = T.pack_u8(imgs[:2] + [None] + imgs[2:], pads=[1, 2, 0, 3, 0, 0], pin=False)
    assert ctypes.sizeof(ctypes.c_longlong) + 2 * ctypes.sizeof(ctypes.c_int) == T.IMAGE_DESC.itemsize == 16
    flat = buffer.numpy()
    assert np.array_equal(flat[:16 * 6].view(T.IMAGE_DESC), descs)
    pos = 16 * 6
    for d, im, pad in zip(descs, imgs[:2] + [None] + imgs[2:], [1, 2, 0, 3, 0, 0]):
        pos += pad
        assert d['offset'] == pos
        if im is None:
            assert (d['h'], d['w']) == (0, 0)
            continue
        assert (d['h'], d['w']) == im.shape[:2]
        assert np.array_equal(flat[pos:pos + im.size].reshape(im.shape), im)
        pos += im.size
    assert pos == flat.size
    assert np.array_equal(T.image_descs(descs.view(np.int32).reshape(-1, 4), flat.size), descs)
    bad = descs.copy()
    bad['offset'][5] += 1                                   # the last image would end one byte past the buffer
    with pytest.raises(ValueError, match='outside'):
        T.image_descs(bad, flat.size)
    bad = descs.copy()
    bad['h'][0] = -1
    with pytest.raises(ValueError):
        T.image_descs(bad, flat.size)
    with pytest.raises(ValueError):
        T.pack_u8([np.zeros((4, 4), np.uint8)], pin=False)


def test_collate_raw_on_a_generated_tree(tmp_path):
    from PIL import Image
    import t2onet_amd.functional as T
    from t2onet_amd import data
    from tests import fivek_tree
    img_dir, anno_dir, act_dir, _ = fivek_tree.write_tree(str(tmp_path), n_train=4, n_val=2)
    raw = data.FiveKAct(img_dir, anno_dir, act_dir, 'train', 1, 16, raw=True)
    ref = data.FiveKAct(img_dir, anno_dir, act_dir, 'train', 1, 16)
    items = [raw[i] for i in range(4)]
    steps = []
    for i, it in enumerate(items):
        img_x, imgs, x, ops, params, req = it
        n = int((ops > 2).sum())
        steps.append(n)
        assert img_x.dtype == np.uint8 and img_x.shape[2] == 3 and len(imgs) == 6
        assert [im is None for im in imgs] == [False] * n + [True] * (5 - n) + [False]
        pil = np.asarray(Image.open(os.path.join(act_dir, 'train%d' % i, 'edit0.jpg')).convert('RGB'))
        assert np.array_equal(imgs[0], pil) and np.array_equal(img_x, data.decode_image(os.path.join(img_dir, 'train%d_in.jpg' % i)))
        np.testing.assert_array_equal(ops, ref[i][3])
        np.testing.assert_array_equal(params, ref[i][4])
    assert min(steps) < 5                                    # unused steps occur
    batch = data.collate_raw(items)
    assert batch['items'] == 4 and batch['buffer'].dtype == torch.uint8 and tuple(batch['descs'].shape) == (28, 4)
    descs = T.image_descs(batch['descs'], batch['buffer'].numel())
    flat = batch['buffer'].numpy()
    order = [it[0] for it in items] + [im for it in items for im in it[1]]
    pos = 16 * 28
    for d, im in zip(descs, order):
        assert d['offset'] == pos                            # back to back, behind the table
        if im is None:
            assert (d['h'], d['w']) == (0, 0)
        else:
            assert (d['h'], d['w']) == im.shape[:2] and np.array_equal(flat[pos:pos + im.size].reshape(im.shape), im)
            pos += im.size
    assert pos == flat.size
    want = next(iter(torch.utils.data.DataLoader(ref, batch_size=4)))
    for got, exp in zip(batch['rest'], want[2:]):
        assert torch.equal(got, exp) if torch.is_tensor(exp) else list(got) == list(exp)
    val = data.FiveK(img_dir, anno_dir, 'val', 1, raw=True)
    a, b, x, req = val[1]
    assert a.shape == (96, 144, 3) and b.dtype == np.uint8 and req == 'make it 1'
    vb = data.collate_raw([val[1]])
    assert tuple(vb['descs'].shape) == (2, 4) and vb['descs'][0].tolist()[2:] == [96, 144]
    assert data.short_side_size(96, 144, 24) == (24, 36)
