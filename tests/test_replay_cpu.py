"""No-GPU checks of the 8-bit replay (t2o_replay.hip): the kernel's tile program, compiled for the host from the shared
header (tests/host_emul/emul_replay.cpp) and run for whole pictures, against the fp32 oracle byte by byte; zero padding of
the INTERMEDIATE image at the picture's border; the C entry point's status codes; the request tokeniser and the JSON
record of the edit command."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import replay_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A


@pytest.fixture(scope='module')
def emul():
    out = os.path.join(ROOT, 'tests', '_build')
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, 'libt2o_emul_replay.so')
    src = os.path.join(ROOT, 'tests', 'host_emul', 'emul_replay.cpp')
    deps = [src] + [os.path.join(ROOT, 't2onet_amd', 'csrc', h) for h in ('t2o_replay_math.h', 't2o_pixel_math.h', 't2o_image_math.h')]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = '%s.tmp.%d' % (so, os.getpid())
        subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-fPIC', '-shared', '-o', tmp, src])
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    assert lib.emul_replay_tile() == RC.TILE
    return lib


def run_emul(lib, img, ops, params, src_pad=1, out_pad=3):
    """The tile program over the whole picture, source and destination at odd byte offsets inside larger buffers; checks
    that no byte outside the destination picture changes."""
    h, w = img.shape[:2]
    src = np.full(src_pad + img.size + 5, 0xC3, np.uint8)
    src[src_pad:src_pad + img.size] = img.reshape(-1)
    out = np.full(out_pad + img.size + 7, SENTINEL, np.uint8)
    c_ops = (ctypes.c_int * 8)(*([int(o) for o in ops] + [0] * (8 - len(ops))))
    params = np.ascontiguousarray(params, np.float32)
    rc = lib.emul_replay_u8(src.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(src_pad), out.ctypes.data_as(ctypes.c_void_p),
                            ctypes.c_longlong(out_pad), h, w, len(ops), c_ops, params.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    assert (out[:out_pad] == SENTINEL).all() and (out[out_pad + img.size:] == SENTINEL).all()
    return out[out_pad:out_pad + img.size].reshape(h, w, 3)


@pytest.mark.parametrize('name', sorted(RC.LISTS))
def test_tile_program_within_the_oracle_interval(emul, name):
    ops, forced = RC.LISTS[name]
    for i, (h, w) in enumerate(RC.SIZES):
        img = RC.picture(h, w, 100 + i)
        params = RC.params_for(ops, 7 + i, forced)
        got = run_emul(emul, img, ops, params, src_pad=i % 4, out_pad=(i + 1) % 4)
        RC.assert_in_interval(got, RC.oracle(img, ops, params), '%s %dx%d' % (name, h, w))


def test_zero_steps_is_the_two_conversions(emul):
    """steps = 0 over every byte value: (b / 255 in fp32) * 255 truncated, whatever that is -- not assumed to be b."""
    img = (np.arange(16 * 16 * 3) % 256).astype(np.uint8).reshape(16, 16, 3)
    got = run_emul(emul, img, [], np.zeros((8, 24), np.float32))
    want = ((img.astype(np.float32) / np.float32(255.0)) * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(got, want)


@pytest.mark.parametrize('alignment', [(0, 0), (1, 2), (2, 3), (3, 1)])
def test_every_byte_alignment_gives_the_same_bytes(emul, alignment):
    img = RC.picture(RC.TILE + 1, 2 * RC.TILE + 1, 5)
    ops, _ = RC.LISTS['sharp_middle']
    params = RC.params_for(ops, 9)
    assert np.array_equal(run_emul(emul, img, ops, params, *alignment), run_emul(emul, img, ops, params, 0, 0))


def test_sharpness_pads_the_intermediate_image_with_zeros(emul):
    """A constant picture: after a per-pixel step it is still constant (value v), and a sharpness with zero padding then
    gives v inside, v + p v on the edges and v + 2 p v in the corners.  White first makes v = 1 while the source's ring
    would be 0 -> 1 had the halo been filled BEFORE the per-pixel steps: with p < 0 the border must darken."""
    h, w = RC.TILE + 8, 2 * RC.TILE + 6
    img = np.full((h, w, 3), 100, np.uint8)
    params = np.zeros((8, 24), np.float32)
    params[1, 0] = -0.25
    got = run_emul(emul, img, [7, 6], params)
    want = np.full((h, w, 3), 255, np.uint8)
    want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = int(0.75 * 255)
    want[0, 0] = want[0, -1] = want[-1, 0] = want[-1, -1] = int(0.5 * 255)
    assert np.array_equal(got, want)
    # a brightening step, then a sharpening one: the border ring brightens by p v (edges) and 2 p v (corners)
    params = np.zeros((8, 24), np.float32)
    params[0, 0], params[1, 0] = 0.5, 0.5
    got = run_emul(emul, img, [0, 6], params)
    v = RC.oracle(img[:1, :1], [0], params)[0, 0, 0]
    assert abs(v - 1.5 * 100 / 255) < 1e-5
    ring = np.zeros((h, w))
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = 1
    ring[0, 0] = ring[0, -1] = ring[-1, 0] = ring[-1, -1] = 2
    predicted = np.clip(v + 0.5 * ring * v, 0, 1)[None].repeat(3, 0).astype(np.float32)
    assert np.trunc(255 * predicted[0, 0, 0]) > np.trunc(255 * predicted[0, 1, 1])          # the ring is visible in bytes
    RC.assert_in_interval(got, predicted, 'brighten + sharpen')
    RC.assert_in_interval(got, RC.oracle(img, [0, 6], params), 'brighten + sharpen (oracle)')


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
    assert lib.t2o_abi_version() == 4
    assert ctypes.sizeof(T.ReplayJob) == 64
    p = torch.zeros(64).data_ptr()

    def status(jobs, src=p, out=p, params=p):
        return lib.t2o_replay_u8(src, out, T.replay_jobs(jobs), len(jobs), params, None)
    assert status([(0, 0, 4, 4, [4])]) == 2 and b'inpaint' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [0]), (0, 48, 4, 4, [6, 0, 6])]) == 2 and b'sharpness' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [0])] * 65) == 1 and b'64' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [0] * 9)]) == 1 and b'steps' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [8])]) == 1 and status([(0, 0, 4, 4, [-2])]) == 1
    assert status([(0, 0, 0, 4, [0])]) == 1 and status([(0, 0, 4, -1, [0])]) == 1 and status([(-1, 0, 4, 4, [0])]) == 1
    assert status([(0, 0, 4, 4, [0])], src=None) == 1 and status([(0, 0, 4, 4, [0])], out=None) == 1
    assert status([(0, 0, 4, 4, [0])], params=None) == 1 and b'parameter' in lib.t2o_last_error()
    assert lib.t2o_replay_u8(p, p, None, 1, p, None) == 1
    # the Python surface turns them into exceptions that carry the library's text
    with pytest.raises(NotImplementedError, match='inpaint'):
        T.replay_status(status([(0, 0, 4, 4, [4])]))
    with pytest.raises(ValueError, match='steps'):
        T.replay_status(status([(0, 0, 4, 4, [0] * 9)]))
    with pytest.raises(ValueError, match='GPU'):
        T.replay_u8(torch.zeros(48, dtype=torch.uint8), [(0, 0, 4, 4, [0])], None)


def test_request_to_idx_rows():
    from t2onet_amd import data, default_options
    from t2onet_amd.edit import request_to_idx
    opt = default_options()
    words = ['<NULL>', '<START>', '<END>', '<UNK>', 'make', 'the', 'photo', 'brighter', 'and', 'more', 'colorful', 'please',
             'sky', 'bluer', 'remove', 'shadows', 'from', 'faces', 'sharpen', 'details', 'warm', 'tones', 'it']
    vocab2id = {t: i for i, t in enumerate(words)}
    long_one = 'Please make the sky bluer and the photo more colorful and warm and sharpen the details and remove the shadows from the faces'
    assert len(data.parse_sent(long_one)) > 15
    for text in ('Make it brighter!', 'make the photo xylophonic, please', long_one):
        row = request_to_idx(text, vocab2id, opt)
        assert row.dtype == torch.long and tuple(row.shape) == (1, opt.encoder_max_len)
        assert torch.equal(row, data.txt2idx(text, vocab2id, opt.encoder_max_len))
    assert request_to_idx('make the photo xylophonic, please', vocab2id, opt)[0].tolist()[:7] == [1, 4, 5, 6, 3, 11, 2]
    row = request_to_idx(long_one, vocab2id, opt)[0].tolist()
    assert row[0] == 1 and row[-1] == 2 and 0 not in row                       # cut to 15 words, END behind them


def test_edit_record_names_and_parameter_counts(tmp_path):
    from PIL import Image
    from t2onet_amd import edit_cli
    from t2onet_amd.edit import first_end
    assert edit_cli.ACTIONS == ['brightness', 'contrast', 'saturation', 'color', 'inpaint', 'tone', 'sharpness', 'white']
    ops = [0, 1, 2, 3, 5, 6, 7]
    params = torch.arange(7 * 24, dtype=torch.float32).view(7, 24)
    rec = edit_cli.operations_record(ops, params)
    assert [n for n, _ in rec] == ['brightness', 'contrast', 'saturation', 'color', 'tone', 'sharpness', 'white']
    assert [len(p) for _, p in rec] == [1, 1, 1, 24, 8, 1, 0]
    assert rec[3][1] == [float(v) for v in range(72, 96)] and rec[4][1] == [float(v) for v in range(96, 104)]
    assert first_end([5, 3, 2, 4, 2], 2) == 2 and first_end([2, 3, 4, 5, 6], 2) == 0 and first_end([3, 4, 5, 6, 8], 2) == 5
    img = RC.picture(6, 9, 1)
    steps = np.stack([RC.picture(6, 9, 2 + k) for k in range(2)])
    src = tmp_path / 'photo.png'
    Image.fromarray(img).save(str(src))
    info = edit_cli.write_outputs(str(tmp_path / 'out'), str(src), 'make it pop', img, steps, [0, 5], params[:2], multi_img=True)
    d = tmp_path / 'out' / 'photo'
    assert sorted(os.listdir(str(d))) == ['1_inference_photo.png', '2_inference_photo.png', 'photo.json', 'photo.png', 'photo_in.png']
    with open(str(d / 'photo.json')) as f:
        saved = json.load(f)
    assert saved == [{'input': 'photo_in.png', 'request': 'make it pop', 'output': 'photo.png',
                      'operations': [['brightness', [0.0]], ['tone', [float(v) for v in range(24, 32)]]]}]
    assert info['output'] == 'photo.png'
    assert np.array_equal(np.asarray(Image.open(str(d / 'photo.png'))), steps[1])
    assert np.array_equal(np.asarray(Image.open(str(d / '1_inference_photo.png'))), steps[0])
    assert np.array_equal(np.asarray(Image.open(str(d / 'photo_in.png'))), img)
