"""No-GPU checks of the stencils replay (t2o_replay_stencils.hip): the kernel's tile program, compiled for the host from the
shared header (tests/host_emul/emul_replay_stencils.cpp) and run for whole pictures, byte for byte against a whole-image
chain of the same device functions (the test of the ring, the padding and the shrinking region); against the fp32 oracle
for the lists whose error the oracle's bound covers; the zero padding of every intermediate image against a numpy
restatement; against the two existing tile programs; the C entry point's status codes; a stand-alone sanitizer program;
the record parsing, job lists and wrapper choice of apply_cli."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import replay_cases as RC
from tests import replay_mask_cases as MC
from tests import replay_stencils_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A
HEADERS = ('t2o_replay_stencils_math.h', 't2o_replay_mask_math.h', 't2o_replay_math.h', 't2o_pixel_math.h', 't2o_image_math.h')


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
    lib = _compile('emul_replay_stencils')
    assert lib.emul_replay_stencils_tile() == RC.TILE
    assert lib.emul_replay_stencils_lds_bytes() < 52 * 1024           # three workgroups in a CU's 160 KB; a static allocation may have 64 KB
    assert lib.emul_replay_stencils_small_lds_bytes() < 32 * 1024     # the instance for R <= 2: five
    assert lib.emul_replay_stencils_small_ring() == 2
    assert lib.emul_replay_stencils_args_bytes() < 4096                # the job table travels in the kernel arguments
    return lib


@pytest.fixture(scope='module')
def emul_plain():
    return _compile('emul_replay')


@pytest.fixture(scope='module')
def emul_masked():
    return _compile('emul_replay_mask')


def _c_ints(values, n=8, fill=0):
    return (ctypes.c_int * n)(*([int(v) for v in values] + [fill] * (n - len(values))))


def _inside(n, offsets, size):
    keep = np.zeros(n, bool)
    for off in offsets:
        keep[off:off + size] = True
    return keep


def run(fn, img, ops, params, mask_of=None, planes=(), src_pad=1, out_pad=3, mask_pad=2):
    """One job through `fn` (the tile program or the whole-image chain); source, destination and mask planes at the given
    byte offsets inside larger buffers; checks that no byte outside the destination picture changes."""
    h, w = img.shape[:2]
    src = np.full(src_pad + img.size + 5, 0xC3, np.uint8)
    src[src_pad:src_pad + img.size] = img.reshape(-1)
    out = np.full(out_pad + img.size + 7, SENTINEL, np.uint8)
    params = np.ascontiguousarray(params, np.float32)
    if planes:
        buf, offsets = MC.pack_masks(list(planes), mask_pad)
        offs = (ctypes.c_longlong * 4)(*(offsets + [0] * (4 - len(offsets))))
        mask_args = (_c_ints(mask_of, fill=-1), params.ctypes.data_as(ctypes.c_void_p), buf.ctypes.data_as(ctypes.c_void_p), offs, len(planes))
    else:
        mask_args = (None, params.ctypes.data_as(ctypes.c_void_p), None, None, 0)
    rc = fn(src.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(src_pad), out.ctypes.data_as(ctypes.c_void_p),
            ctypes.c_longlong(out_pad), h, w, len(ops), _c_ints(ops), *mask_args)
    assert rc == 0
    assert (out[:out_pad] == SENTINEL).all() and (out[out_pad + img.size:] == SENTINEL).all()
    return out[out_pad:out_pad + img.size].reshape(h, w, 3)


@pytest.mark.parametrize('name', SC.NAMES)
def test_tile_program_equals_the_whole_image_chain(emul, name):
    """Every list x size, unmasked and under every mask case: the tile program's bytes EQUAL those of one full-image pass
    per step.  Sources, masks and outputs walk through all four byte alignments."""
    ops = SC.LISTS[name]
    i, seen = SC.NAMES.index(name), set()
    for s, (h, w) in enumerate(SC.SIZES):
        img = RC.picture(h, w, 200 + s)
        params = SC.params_for(name, 11 + s)
        for case in [None] + SC.MASK_NAMES:
            mask_of, planes = SC.mask_case(name, case, h, w, seed=s) if case else (None, ())
            pads = (i % 4, (i + 1 + i // 4) % 4, (i + 2 + i // 16) % 4)
            seen.add(pads)
            got = run(emul.emul_replay_u8_stencils, img, ops, params, mask_of, planes, *pads)
            want = run(emul.chain_replay_u8_stencils, img, ops, params, mask_of, planes, *pads)
            assert np.array_equal(got, want), '%s %s %dx%d: %d bytes differ, first at %s' % (
                name, case, h, w, int((got != want).sum()), tuple(np.argwhere(got != want)[0]))
            if sum(op == 6 for op in ops) <= 2:                  # beside a job with R > 2 the launch takes the large instance
                assert np.array_equal(run(emul.emul_replay_u8_stencils_large, img, ops, params, mask_of, planes, *pads), want)
            i += 1
    assert {a for a, _, _ in seen} == {b for _, b, _ in seen} == {c for _, _, c in seen} == {0, 1, 2, 3}


@pytest.mark.parametrize('name', SC.ORACLE_NAMES)
def test_tile_program_within_the_oracle_interval(emul, name):
    """The lists with at most two sharpness steps at p = 0.3, unmasked and masked, inside RC.BOUND of the fp32 oracle: no
    exception allowed.  (Longer or stronger lists amplify the oracle's own fp32 error past the bound -- up to 1 + 8 p per
    sharpness -- and are held by the byte equality above.)"""
    ops = SC.LISTS[name]
    assert sum(op == 6 for op in ops) == 2
    for s, (h, w) in enumerate(SC.SIZES):
        img = RC.picture(h, w, 300 + s)
        params = SC.params_for(name, 21 + s, sharp=SC.ORACLE_SHARP)
        got = run(emul.emul_replay_u8_stencils, img, ops, params)
        RC.assert_in_interval(got, RC.oracle(img, ops, params), '%s %dx%d' % (name, h, w))
        for case in ('soft_all', 'blocks_sharp', 'soft_front'):
            mask_of, planes = SC.mask_case(name, case, h, w, seed=s)
            got = run(emul.emul_replay_u8_stencils, img, ops, params, mask_of, planes)
            RC.assert_in_interval(got, MC.oracle(img, ops, params, mask_of, planes), '%s %s %dx%d' % (name, case, h, w))


def test_every_intermediate_image_is_zero_padded(emul):
    """A constant picture larger than a tile through white, sharpness, sharpness with negative parameters: white makes the
    image 1 everywhere, so only the padding can change a pixel -- the outermost ring after the first sharpness (zeros, not
    white's ones, outside the picture), the two outermost rings after the second.  Expected: an independent numpy fp32
    restatement with np.pad."""
    h, w = RC.TILE + 9, 2 * RC.TILE + 5
    img = np.full((h, w, 3), 90, np.uint8)
    ops = SC.LISTS['white_ss']
    params = np.zeros((8, 24), np.float32)
    params[1, 0], params[2, 0] = -0.11, -0.07
    got = run(emul.emul_replay_u8_stencils, img, ops, params)
    RC.assert_in_interval(got, SC.numpy_chain(img, ops, params), 'white, sharpness, sharpness')
    inner = got[2:-2, 2:-2]
    assert (inner == 255).all()
    ring0 = np.concatenate([got[0].ravel(), got[-1].ravel(), got[:, 0].ravel(), got[:, -1].ravel()])
    ring1 = np.concatenate([got[1, 1:-1].ravel(), got[-2, 1:-1].ravel(), got[1:-1, 1].ravel(), got[1:-1, -2].ravel()])
    assert (ring0 < 255).all() and (ring1 < 255).all()
    assert (ring0.max() < ring1.min())                               # the outer ring lost to the padding twice


@pytest.mark.parametrize('name', sorted(RC.LISTS))
def test_lists_of_the_plain_tile_program_give_its_bytes(emul, emul_plain, name):
    ops, forced = RC.LISTS[name]
    fn = emul_plain.emul_replay_u8
    for s, (h, w) in enumerate(RC.SIZES):
        img = RC.picture(h, w, 100 + s)
        params = np.ascontiguousarray(RC.params_for(ops, 7 + s, forced))
        src, out = np.ascontiguousarray(img.reshape(-1)), np.zeros(img.size, np.uint8)
        assert fn(src.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(0), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(0),
                  h, w, len(ops), _c_ints(ops), params.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.array_equal(run(emul.emul_replay_u8_stencils, img, ops, params), out.reshape(h, w, 3)), (name, h, w)


@pytest.mark.parametrize('name', MC.NAMES)
def test_lists_of_the_masked_tile_program_give_its_bytes(emul, emul_masked, name):
    ops, mask_of = MC.LISTS[name]
    for p, pattern in enumerate(MC.PATTERNS):
        s = p % len(RC.SIZES)
        for h, w in (RC.SIZES[s], RC.SIZES[5]):
            img = RC.picture(h, w, 100 + s)
            params = RC.params_for(ops, 7 + s)
            planes = MC.masks_for(name, pattern, h, w, seed=s)
            want = run(emul_masked.emul_replay_u8_masked, img, ops, params, mask_of, planes)
            assert np.array_equal(run(emul.emul_replay_u8_stencils, img, ops, params, mask_of, planes), want), (name, pattern, h, w)


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
    assert lib.t2o_abi_version() == 4                                # an added entry point does not bump it
    p = torch.zeros(64).data_ptr()
    offs4 = (ctypes.c_longlong * 5)(0, 0, 0, 0, 0)

    def status(jobs, src=p, out=p, params=p, masks=p, offs=offs4, n_masks=1, table=True):
        return lib.t2o_replay_u8_stencils(src, out, T.replay_jobs([j[:5] for j in jobs]), T.replay_mask_table(jobs) if table else None,
                                          len(jobs), params, masks, offs, n_masks, None)
    one = (0, 0, 4, 4, [6, 6], [0, 0])
    assert status([one], src=None) == 1 and b'null' in lib.t2o_last_error()
    assert status([one], out=None) == 1
    assert status([one], table=False) == 1 and status([one], masks=None) == 1 and status([one], offs=None) == 1      # n_masks = 1
    assert status([one], params=None) == 1 and b'parameter' in lib.t2o_last_error()
    assert lib.t2o_replay_u8_stencils(p, p, None, None, 1, p, None, None, 0, None) == 1
    assert lib.t2o_replay_u8_stencils(p, p, T.replay_jobs([one[:5]]), None, 0, p, None, None, 0, None) == 1
    assert status([one] * 65) == 1 and b'64' in lib.t2o_last_error()
    assert status([one], n_masks=5) == 1 and b'4 masks' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [6, 6], [0, 1])]) == 1 and b'mask index' in lib.t2o_last_error()       # one mask in the table
    assert status([(0, 0, 4, 4, [6, 6], [0, 0])], n_masks=0, masks=None, offs=None) == 1 and b'mask index' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [6, 6], [-1, -2])]) == 1 and b'mask index' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [6, 4, 6], [0, 0, 0])]) == 2 and b'inpaint' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [6] * 9, [0] * 8)]) == 1 and b'steps' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, [8], [0])]) == 1 and status([(0, 0, 0, 4, [6], [0])]) == 1 and status([(-1, 0, 4, 4, [6], [0])]) == 1
    assert status([one], offs=(ctypes.c_longlong * 1)(-4)) == 1 and b'offset' in lib.t2o_last_error()
    with pytest.raises(NotImplementedError, match='inpaint'):
        T.replay_status(status([(0, 0, 4, 4, [4], [0])]), 't2o_replay_u8_stencils')
    with pytest.raises(ValueError, match='GPU'):
        T.replay_u8_stencils(torch.zeros(48, dtype=torch.uint8), [one[:5]], None)


def test_tile_program_is_clean_under_the_sanitizers(tmp_path):
    """Host code only: a stand-alone program over the tile program with the LDS struct as a heap object of its own, built
    with -fsanitize=address,undefined and run as its own process, the runtimes linked in statically; nothing of it is
    loaded into this one."""
    exe = str(tmp_path / 'sanitize_replay_stencils')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan',
                           '-o', exe, os.path.join(ROOT, 'tests', 'host_emul', 'sanitize_replay_stencils.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'replay stencils tile program: clean', r.stdout + r.stderr


# ---------------------------------------------------------------- apply_cli without a GPU
RECORD = [{'input': 'a_in.png', 'request': 'crisper', 'output': 'a.png',
           'operations': [['sharpness', [0.4]], ['tone', [1.0, 1.1, 0.9, 1.2, 0.8, 1.0, 1.3, 0.7]], ['sharpness', [0.3]]]}]


def test_apply_cli_parses_a_record_and_names_what_is_wrong():
    from t2onet_amd import apply_cli
    request, ops, params = apply_cli.parse_record(json.loads(json.dumps(RECORD)))
    assert request == 'crisper' and ops == [6, 5, 6]
    assert params.shape == (3, 24) and params.dtype == np.float32
    assert params[0, 0] == np.float32(0.4) and params[2, 0] == np.float32(0.3) and not params[0, 1:].any()
    assert params[1, :8].tolist() == [np.float32(v) for v in RECORD[0]['operations'][1][1]] and not params[1, 8:].any()
    assert apply_cli.parse_record([{'operations': []}]) [1] == []

    def bad(operations, match):
        with pytest.raises(ValueError, match=match):
            apply_cli.parse_record([{'request': 'x', 'operations': operations}])
    bad([['sharpness', [0.4]], ['glow', [1.0]]], r'operation 1.*glow.*not an operator name')
    bad([['tone', [1.0] * 7]], r'operation 0: tone takes 8 values, got 7')
    bad([['white', [1.0]]], r'operation 0: white takes 0 values, got 1')
    bad([['brightness', [0.1]], ['contrast', [0.1]], ['inpaint', []]], r'operation 2: inpaint')
    bad([['sharpness', [0.1]]] * 9, r'9 operations.*8')
    bad([['sharpness', ['much']]], r'operation 0.*not a number')
    bad(['sharpness'], r'operation 0')
    with pytest.raises(ValueError, match='operations'):
        apply_cli.parse_record({'request': 'x'})
    # what edit_cli writes is what parse_record reads
    from t2onet_amd import edit_cli
    rows = torch.zeros(3, 24)
    rows[0, 0], rows[1, :8], rows[2, 0] = 0.4, torch.tensor(RECORD[0]['operations'][1][1]), 0.3
    written = json.loads(json.dumps([{'request': 'r', 'operations': edit_cli.operations_record([6, 5, 6], rows)}]))
    assert apply_cli.parse_record(written)[1] == [6, 5, 6]
    assert np.array_equal(apply_cli.parse_record(written)[2], rows.numpy())


def test_apply_cli_job_lists():
    from t2onet_amd import apply_cli
    ops = [6, 5, 6]
    one = apply_cli.job_lists([(5, 7)], [16], ops)
    assert one == [[(0, (16, 0, 5, 7, ops))]]
    shapes = [(3 + i % 4, 5 + i % 3) for i in range(70)]
    offsets = list(np.cumsum([16 * 70] + [3 * h * w for h, w in shapes[:-1]]))
    launches = apply_cli.job_lists(shapes, offsets, ops)
    assert [len(l) for l in launches] == [64, 6]                       # two launches
    assert [i for l in launches for i, _ in l] == list(range(70))
    for launch in launches:
        pos = 0
        for i, (so, oo, h, w, o) in launch:
            assert (so, oo, (h, w), o) == (offsets[i], pos, shapes[i], ops)
            pos += 3 * h * w
    multi = apply_cli.job_lists(shapes[:2], offsets[:2], ops, multi_img=True)
    assert [(i, job[4]) for i, job in multi[0]] == [(0, [6]), (0, [6, 5]), (0, [6, 5, 6]), (1, [6]), (1, [6, 5]), (1, [6, 5, 6])]
    assert [len(l) for l in apply_cli.job_lists(shapes[:30], offsets[:30], ops, multi_img=True)] == [64, 26]
    assert apply_cli.job_lists([(5, 7)], [16], [], multi_img=True) == [[(0, (16, 0, 5, 7, []))]]      # an empty list: one job


def test_apply_cli_picks_the_wrapper_by_the_list(monkeypatch):
    """The wrappers and the upload replaced by host recorders: a list with at most one sharpness goes through replay_u8, any
    other through replay_u8_stencils; 70 photos are two calls of 64 and 6 jobs on ONE uploaded buffer."""
    import t2onet_amd.functional as T
    from t2onet_amd import apply_cli
    calls = []

    def recorder(name):
        def fn(src, jobs, params, *rest):
            calls.append((name, src, [tuple(j) for j in jobs], params))
            return torch.zeros(sum(3 * j[2] * j[3] for j in jobs), dtype=torch.uint8)
        return fn
    uploads = []

    def upload(buffer, descs, device=None):
        uploads.append(buffer)
        return buffer, 0, T.image_descs(descs, buffer.numel()), None
    monkeypatch.setattr(T, 'replay_u8', recorder('replay_u8'))
    monkeypatch.setattr(T, 'replay_u8_stencils', recorder('replay_u8_stencils'))
    monkeypatch.setattr(T, 'upload_packed', upload)
    images = [RC.picture(3 + i % 4, 5 + i % 3, i) for i in range(70)]
    for ops, want in (([6, 5, 6], 'replay_u8_stencils'), ([0, 6, 5], 'replay_u8'), ([0, 5], 'replay_u8'), ([], 'replay_u8'),
                      ([6] * 8, 'replay_u8_stencils')):
        del calls[:], uploads[:]
        assert apply_cli.pick_wrapper(ops) == want
        params = RC.params_for(ops, 3)[:len(ops)]
        steps = apply_cli.apply_record(images, ops, params, device=torch.device('cpu'))
        assert len(uploads) == 1
        assert [(name, len(jobs)) for name, _, jobs, _ in calls] == [(want, 64), (want, 6)]
        assert all(src is uploads[0] for _, src, _, _ in calls)
        assert all(job[4] == ops for _, _, jobs, _ in calls for job in jobs)
        table = calls[0][3]
        assert tuple(table.shape) == (64, 8, 24) and np.array_equal(table[5, :len(ops)].numpy(), params) and not table[:, len(ops):].any()
        assert [s.shape for s in steps] == [(1,) + im.shape for im in images]
