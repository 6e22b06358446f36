"""No-GPU checks of the MASKED 8-bit replay (t2o_replay_mask.hip): the kernel's tile program, compiled for the host from the
shared header (tests/host_emul/emul_replay_mask.cpp) and run for whole pictures, against the fp32 oracle with masks byte
by byte; the degenerate masks against the unmasked emulation; the C entry point's status codes; the nearest-neighbour
index rule of the proxy mask; the --mask option of the edit command."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import replay_cases as RC
from tests import replay_mask_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A
HEADERS = ('t2o_replay_mask_math.h', 't2o_replay_math.h', 't2o_pixel_math.h', 't2o_image_math.h')


def _compile(stem):
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
    lib = _compile('emul_replay_mask')
    assert lib.emul_replay_mask_tile() == RC.TILE
    assert lib.emul_replay_mask_lds_bytes() < 32 * 1024              # four staged masks beside the unmasked kernel's 21 KB
    assert lib.emul_replay_mask_args_bytes() <= 4096                 # the job table travels in the kernel arguments
    return lib


@pytest.fixture(scope='module')
def emul_plain():
    return _compile('emul_replay')                                   # the unmasked tile program


def _c_ints(values, n=8, fill=0):
    return (ctypes.c_int * n)(*([int(v) for v in values] + [fill] * (n - len(values))))


def run_masked(lib, img, ops, params, mask_of, planes, src_pad=1, out_pad=3, mask_pad=2, noise=0xA5, steps=None):
    """The masked tile program over the whole picture; source, destination and mask planes at the given byte offsets
    inside larger buffers (the bytes around the planes are `noise`); checks that no byte outside the destination picture
    changes."""
    h, w = img.shape[:2]
    src = np.full(src_pad + img.size + 5, 0xC3, np.uint8)
    src[src_pad:src_pad + img.size] = img.reshape(-1)
    out = np.full(out_pad + img.size + 7, SENTINEL, np.uint8)
    buf, offsets = MC.pack_masks(planes, mask_pad)
    buf[~_inside(buf.size, offsets, h * w)] = noise
    offs = (ctypes.c_longlong * 4)(*(offsets + [0] * (4 - len(offsets))))
    params = np.ascontiguousarray(params, np.float32)
    rc = lib.emul_replay_u8_masked(src.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(src_pad), out.ctypes.data_as(ctypes.c_void_p),
                                   ctypes.c_longlong(out_pad), h, w, len(ops) if steps is None else steps, _c_ints(ops),
                                   _c_ints(mask_of, fill=-1), params.ctypes.data_as(ctypes.c_void_p),
                                   buf.ctypes.data_as(ctypes.c_void_p), offs, len(planes))
    assert rc == 0
    assert (out[:out_pad] == SENTINEL).all() and (out[out_pad + img.size:] == SENTINEL).all()
    return out[out_pad:out_pad + img.size].reshape(h, w, 3)


def _inside(n, offsets, size):
    keep = np.zeros(n, bool)
    for off in offsets:
        keep[off:off + size] = True
    return keep


def run_plain(lib, img, ops, params, steps=None):
    h, w = img.shape[:2]
    src = np.ascontiguousarray(img.reshape(-1))
    out = np.zeros(img.size, np.uint8)
    params = np.ascontiguousarray(params, np.float32)
    rc = lib.emul_replay_u8(src.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(0), out.ctypes.data_as(ctypes.c_void_p),
                            ctypes.c_longlong(0), h, w, len(ops) if steps is None else steps, _c_ints(ops),
                            params.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out.reshape(h, w, 3)


@pytest.mark.parametrize('name', MC.NAMES)
def test_tile_program_within_the_oracle_interval(emul, name):
    """Every list x pattern x size; sources, masks and outputs walk through all four byte alignments."""
    ops, mask_of = MC.LISTS[name]
    seen = set()
    i = MC.NAMES.index(name)
    for p, pattern in enumerate(MC.PATTERNS):
        for s, (h, w) in enumerate(RC.SIZES):
            img = RC.picture(h, w, 100 + s)
            params = RC.params_for(ops, 7 + s)
            planes = MC.masks_for(name, pattern, h, w, seed=s)
            pads = (i % 4, (i + 1) % 4, (i + 2 + i // 4) % 4)
            seen.add(pads)
            got = run_masked(emul, img, ops, params, mask_of, planes, *pads)
            RC.assert_in_interval(got, MC.oracle(img, ops, params, mask_of, planes), '%s %s %dx%d' % (name, pattern, h, w))
            i += 1
    assert {a for a, _, _ in seen} == {b for _, b, _ in seen} == {c for _, _, c in seen} == {0, 1, 2, 3}


@pytest.mark.parametrize('name', MC.NAMES)
def test_full_and_zero_masks_are_the_unmasked_program(emul, emul_plain, name):
    """255 everywhere: blend(o, x, 1) = o, the bytes of the unmasked emulation of the same list.  0 everywhere:
    blend(o, x, 0) = x for the steps that name a mask -- the bytes of steps = 0 where every step names one, and in any
    case those of the unmasked program with the masked steps made the identity (-1)."""
    ops, mask_of = MC.LISTS[name]
    for s, (h, w) in enumerate(RC.SIZES):
        img = RC.picture(h, w, 100 + s)
        params = RC.params_for(ops, 7 + s)
        full = [MC.mask('full', h, w)] * (max(mask_of) + 1)
        zeros = [MC.mask('zeros', h, w)] * (max(mask_of) + 1)
        assert np.array_equal(run_masked(emul, img, ops, params, mask_of, full), run_plain(emul_plain, img, ops, params))
        got = run_masked(emul, img, ops, params, mask_of, zeros)
        kept = [-1 if m >= 0 else op for op, m in zip(ops, mask_of)]
        assert np.array_equal(got, run_plain(emul_plain, img, kept, params))
        if all(m >= 0 or op < 0 for op, m in zip(ops, mask_of)):
            assert np.array_equal(got, run_plain(emul_plain, img, ops, params, steps=0))
    assert name != 'steps8_masked' or all(m >= 0 for m in mask_of)       # the all-masked list exists


def test_bytes_around_a_mask_plane_are_never_used(emul):
    """The host replay_load_dword reads only inside the plane: other bytes around the planes, same output."""
    for name in ('two_masks', 'sharp_middle_front', 'm_white'):
        ops, mask_of = MC.LISTS[name]
        h, w = RC.SIZES[5]
        img = RC.picture(h, w, 105)
        params = RC.params_for(ops, 3)
        planes = MC.masks_for(name, 'soft', h, w)
        for pad in range(4):
            a = run_masked(emul, img, ops, params, mask_of, planes, mask_pad=pad, noise=0x00)
            b = run_masked(emul, img, ops, params, mask_of, planes, mask_pad=pad, noise=0xFF)
            assert np.array_equal(a, b)


def test_every_byte_alignment_gives_the_same_bytes(emul):
    ops, mask_of = MC.LISTS['two_masks']
    h, w = RC.TILE + 1, 2 * RC.TILE + 1
    img = RC.picture(h, w, 5)
    params = RC.params_for(ops, 9)
    planes = MC.masks_for('two_masks', 'soft', h, w)
    want = run_masked(emul, img, ops, params, mask_of, planes, 0, 0, 0)
    for pads in [(1, 2, 3), (2, 3, 1), (3, 1, 2), (0, 0, 1)]:
        assert np.array_equal(run_masked(emul, img, ops, params, mask_of, planes, *pads), want)


def test_masked_step_in_front_of_a_sharpness_is_blended_on_the_ring(emul):
    """White under a mask that is 255 on one tile's ring column only (x = 32, just right of tile 0): the sharpness in
    tile 0 must see the whitened neighbour, so column 31 changes although its own mask bytes are 0."""
    h, w = 8, 2 * RC.TILE
    img = np.full((h, w, 3), 100, np.uint8)
    m = np.zeros((h, w), np.uint8)
    m[:, RC.TILE] = 255
    params = np.zeros((8, 24), np.float32)
    params[1, 0] = 0.5
    got = run_masked(emul, img, [7, 6], params, [0, -1], [m])
    none = run_masked(emul, img, [7, 6], params, [0, -1], [np.zeros((h, w), np.uint8)])
    assert (got[1:-1, RC.TILE - 1] < none[1:-1, RC.TILE - 1]).all()         # a brighter neighbour darkens the sharpened pixel
    assert np.array_equal(got[:, :RC.TILE - 1], none[:, :RC.TILE - 1])
    RC.assert_in_interval(got, MC.oracle(img, [7, 6], params, [0, -1], [m]), 'ring')


def _library():
    from t2onet_amd import build, _lib
    if os.path.exists(build.hipcc_path()):
        build.build()
    elif not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libt2onet_hip.so is absent and there is no hipcc to build it')
    return _lib.load()


def test_status_codes_before_any_launch():
    import t2onet_amd.functional as T
    lib = _library()
    p = torch.zeros(64).data_ptr()
    offs4 = (ctypes.c_longlong * 5)(0, 0, 0, 0, 0)

    def status(jobs, src=p, out=p, params=p, masks=p, offs=offs4, n_masks=1, table=True):
        return lib.t2o_replay_u8_masked(src, out, T.replay_jobs([j[:5] for j in jobs]), T.replay_mask_table(jobs) if table else None,
                                        len(jobs), params, masks, offs, n_masks, None)
    one = (0, 0, 4, 4, [0], [0])
    assert status([one], src=None) == 1 and b'null' in lib.t2o_last_error()
    assert status([one], out=None) == 1 and status([one], table=False) == 1
    assert status([one], masks=None) == 1 and b'mask' in lib.t2o_last_error()
    assert status([one], offs=None) == 1
    assert status([one], params=None) == 1 and b'parameter' in lib.t2o_last_error()
    assert lib.t2o_replay_u8_masked(p, p, None, T.replay_mask_table([one]), 1, p, p, offs4, 1, None) == 1
    assert lib.t2o_replay_u8_masked(p, p, T.replay_jobs([one[:5]]), T.replay_mask_table([one]), 0, p, p, offs4, 1, None) == 1
    assert status([one] * 65) == 1 and b'64' in lib.t2o_last_error()
    assert status([one], n_masks=5) == 1 and b'4 masks' in lib.t2o_last_error()
    assert status([one], n_masks=-1) == 1
    assert status([(0, 0, 4, 4, [0], [1])]) == 1 and b'mask index' in lib.t2o_last_error()      # one mask in the table
    assert status([(0, 0, 4, 4, [0], [0])], n_masks=0, masks=None, offs=None) == 1 and b'mask index' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [0, 1], [-1, -2])]) == 1 and b'mask index' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [4], [0])]) == 2 and b'inpaint' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [0], [0]), (0, 48, 4, 4, [6, 0, 6], [0, -1, 0])]) == 2 and b'sharpness' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [0] * 9, [0] * 8)]) == 1 and b'steps' in lib.t2o_last_error()
    assert status([(0, 0, 0, 4, [0], [0])]) == 1 and status([(-1, 0, 4, 4, [0], [0])]) == 1
    assert status([one], offs=(ctypes.c_longlong * 1)(-4)) == 1 and b'offset' in lib.t2o_last_error()
    # the Python surface turns them into exceptions that carry the library's text
    with pytest.raises(ValueError, match='mask index'):
        T.replay_status(status([(0, 0, 4, 4, [0], [3])]), 't2o_replay_u8_masked')
    with pytest.raises(NotImplementedError, match='inpaint'):
        T.replay_status(status([(0, 0, 4, 4, [4], [0])]), 't2o_replay_u8_masked')
    with pytest.raises(ValueError, match='GPU'):
        T.replay_u8_masked(torch.zeros(48, dtype=torch.uint8), [one], None, torch.zeros(16, dtype=torch.uint8), [0])


@pytest.mark.parametrize('src,dst', [(80, 53), (48, 32), (7, 7), (5, 9)])
def test_nearest_index_is_the_published_rule(src, dst):
    from t2onet_amd.edit import nearest_index
    got = nearest_index(src, dst)
    assert got.dtype == np.int64 and got.shape == (dst,)
    assert got.tolist() == [min((x * src) // dst, src - 1) for x in range(dst)]           # integers: floor(x * src / dst) exactly
    assert got[0] == 0 and got[-1] <= src - 1 and (np.diff(got) >= 0).all()


def test_mask_option_parsing(tmp_path):
    from PIL import Image
    from t2onet_amd import edit_cli
    assert edit_cli.parse_mask_args(None) == {} and edit_cli.parse_mask_args([]) == {}
    assert edit_cli.parse_mask_args(['sky.png']) == {'all': 'sky.png'}
    assert edit_cli.parse_mask_args(['brightness=sky.png', 'tone=b.png', 'rest.png']) == {'brightness': 'sky.png', 'tone': 'b.png', 'all': 'rest.png'}
    assert edit_cli.parse_mask_args(['out/a=b.png']) == {'all': 'out/a=b.png'}            # a path, not a name
    with pytest.raises(ValueError, match='glow.*not an operator name'):
        edit_cli.parse_mask_args(['glow=sky.png'])
    with pytest.raises(ValueError, match='no file'):
        edit_cli.parse_mask_args(['tone='])
    names = ['brightness', 'contrast', 'saturation', 'color', 'tone']
    with pytest.raises(ValueError, match='5 distinct mask files, at most 4'):
        edit_cli.parse_mask_args(['%s=m%d.png' % (n, i) for i, n in enumerate(names)])
    assert len(edit_cli.parse_mask_args(['%s=m%d.png' % (n, i % 4) for i, n in enumerate(names)])) == 5     # 4 files, 5 names
    # decoding: 8-bit grey, one array per file, the photo's size or an error that names both sizes
    m = MC.mask('blocks', 48, 80)
    Image.fromarray(m).save(str(tmp_path / 'm.png'))
    Image.fromarray(np.stack([m, m, m], -1)).save(str(tmp_path / 'rgb.png'))
    masks = edit_cli.load_masks({'all': str(tmp_path / 'm.png'), 'tone': str(tmp_path / 'm.png'), 'color': str(tmp_path / 'rgb.png')}, 48, 80)
    assert set(masks) == {'all', 5, 3} and masks['all'] is masks[5]
    assert all(v.dtype == np.uint8 and np.array_equal(v, m) for v in masks.values())
    with pytest.raises(ValueError, match=r'80 x 48.*the photo is 81 x 48'):
        edit_cli.load_masks({'all': str(tmp_path / 'm.png')}, 48, 81)
    # the command refuses a wrong mask before it needs a model or a GPU
    Image.fromarray(RC.picture(20, 30, 1)).save(str(tmp_path / 'photo.png'))
    common = ['--img', str(tmp_path / 'photo.png'), '--request', 'x', '--checkpoint', 'none.pth']
    with pytest.raises(ValueError, match=r'80 x 48.*the photo is 30 x 20'):
        edit_cli.main(common + ['--mask', str(tmp_path / 'm.png')])
    with pytest.raises(ValueError, match='not an operator name'):
        edit_cli.main(common + ['--mask', 'glow=' + str(tmp_path / 'm.png')])
    # the record gains 'masks' only when masks were given
    steps = np.stack([RC.picture(20, 30, 2)])
    par = torch.zeros(1, 24)
    rec = edit_cli.write_outputs(str(tmp_path / 'a'), str(tmp_path / 'photo.png'), 'x', RC.picture(20, 30, 1), steps, [0], par,
                                 masks={'all': 'm.png'})
    assert rec['masks'] == {'all': 'm.png'}
    assert 'masks' not in edit_cli.write_outputs(str(tmp_path / 'b'), str(tmp_path / 'photo.png'), 'x', RC.picture(20, 30, 1), steps, [0], par)
