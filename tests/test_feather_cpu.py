"""No-GPU checks of the mask feathering (t2o_feather.hip): the weight rule against numpy's fp64 Gaussian; the kernels' tile
programs, compiled for the host from the shared header (tests/host_emul/emul_feather.cpp) and run for every workgroup of
both launches, against the int64 oracle byte for byte, guard bytes included; the properties of the definition on those
outputs; the status codes of the three entry points; the --feather option of the edit command and edit_image's checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import feather_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('t2o_feather_math.h', 't2o_replay_math.h', 't2o_pixel_math.h', 't2o_image_math.h')


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
    lib = _compile('emul_feather')
    assert {'kFeatherRowW': lib.emul_feather_row_tile_w(), 'kFeatherRowH': lib.emul_feather_row_tile_h(),
            'kFeatherColW': lib.emul_feather_col_tile_w(), 'kFeatherColH': lib.emul_feather_col_tile_h()} == FC.TILES
    assert lib.emul_feather_max_radius() == 192
    assert lib.emul_feather_args_bytes() <= 2048                     # the job table and the weights travel in the kernel arguments
    assert lib.emul_feather_row_lds_bytes() <= 8 * 1024
    assert lib.emul_feather_col_lds_bytes(192) <= 64 * 1024          # two workgroups on a CU's 160 KB at the largest radius
    return lib


def run_emul(lib, src, out, jobs):
    """The two tile programs over every job; src / out: numpy byte buffers (the same object for a call in one buffer)."""
    J = len(jobs)
    rc = lib.emul_feather_u8(src.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                             (ctypes.c_longlong * J)(*[j[0] for j in jobs]), (ctypes.c_longlong * J)(*[j[1] for j in jobs]),
                             (ctypes.c_int * J)(*[j[2] for j in jobs]), (ctypes.c_int * J)(*[j[3] for j in jobs]),
                             (ctypes.c_double * J)(*[float(j[4]) for j in jobs]), J)
    assert rc == 0
    return out


def run_call(lib, call):
    src = call.src.copy()
    out = src if call.out is call.src else call.out.copy()
    return run_emul(lib, src, out, call.jobs)


def feather_one(lib, m, sigma):
    h, w = m.shape
    return run_emul(lib, np.ascontiguousarray(m.reshape(-1)), np.zeros(h * w, np.uint8), [(0, 0, h, w, sigma)]).reshape(h, w)


def _library():
    from t2onet_amd import build, _lib
    if os.path.exists(build.hipcc_path()):
        build.build()
    elif not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libt2onet_hip.so is absent and there is no hipcc to build it')
    return _lib.load()


# ---------------------------------------------------------------- weights
EXPECTED_RADIUS = {0: 0, 0.1: 0, 0.5: 2, 2.5: 8, 7: 21, 20: 60, 64: 192}


@pytest.mark.parametrize('sigma', FC.SIGMAS)
def test_weights_follow_the_tail_sum_rule(sigma):
    import t2onet_amd.functional as T
    _library()
    got = T.feather_weights(sigma)
    assert got.dtype == np.uint16 and got.ndim == 1
    R = len(got) - 1
    if sigma in (0, 0.1):                                            # the copy rule: one tap of 65536, held modulo 2^16
        assert got.tolist() == [0]
        return
    w = got.astype(np.int64)
    assert w[0] + 2 * w[1:].sum() == 65536
    r0 = min(int(np.ceil(3.0 * sigma)), 192)
    i = np.arange(r0 + 1, dtype=np.float64)
    g = np.exp(-i * i / (2.0 * np.float64(sigma) ** 2))
    e = 65536.0 * g / (g[0] + 2.0 * g[1:].sum())
    full = np.zeros(r0 + 1, np.int64)
    full[:R + 1] = w
    assert np.abs(full - e).max() <= 1 + 1e-9
    # R as specified: min(ceil(3 sigma), 192) with the trailing zero weights trimmed -- the last weight kept is not zero,
    # and what was trimmed rounds to nothing: e_i <= 1 there
    assert R <= r0 and w[R] > 0 and (e[R + 1:] <= 1 + 1e-9).all()
    assert R == EXPECTED_RADIUS[sigma]
    assert w[0] <= 65534                                             # fits uint16


def test_the_emulation_has_the_librarys_weights(emul):
    import t2onet_amd.functional as T
    _library()
    for sigma in FC.SIGMAS + [1.0, 3.3, 63.9]:
        w = np.zeros(193, np.uint16)
        r = ctypes.c_int(-1)
        assert emul.emul_feather_weights(ctypes.c_double(sigma), w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(r)) == 0
        assert np.array_equal(w[:r.value + 1], T.feather_weights(sigma)) and not w[r.value + 1:].any()


# ---------------------------------------------------------------- tile programs
CALLS = None


def _calls():
    global CALLS
    if CALLS is None:
        _library()                                                   # the oracle takes its weights from the library
        CALLS = FC.calls()
    return CALLS


def test_cases_cover_what_they_should():
    calls = _calls()
    jobs = [j for _, c in calls for j in c.jobs]
    assert {j[0] % 4 for j in jobs} == {j[1] % 4 for j in jobs} == {0, 1, 2, 3}
    assert {(j[2], j[3]) for j in jobs} >= set(FC.SIZES) and {j[4] for j in jobs} >= set(FC.SIGMAS)
    assert len(FC.specs()) == len(FC.SIZES) * len(FC.SIGMAS)
    for h, w in FC.SIZES:
        assert {p for hh, ww, _, p, _ in FC.specs() if (hh, ww) == (h, w)} == set(FC.PATTERNS)
    assert any(len(c.jobs) == 4 and len({j[2:4] for j in c.jobs}) > 1 and len({j[4] for j in c.jobs}) > 1 for _, c in calls)
    assert any(c.out is c.src and all(j[0] == j[1] for j in c.jobs) for _, c in calls)              # in place
    assert any(n == 'overlap_call' for n, _ in calls)
    radius = {s: len(FC.weights_int(s)) - 1 for s in FC.SIGMAS}
    assert radius[0] == radius[0.1] == 0                             # R = 0
    assert radius[64] > max(FC.TILES['kFeatherColH'], FC.TILES['kFeatherRowH']) and radius[64] > FC.BIG[0]      # R above a tile, above the plane
    assert FC.BIG == (2 * 64 + 1, 2 * 256 + 1)


@pytest.mark.parametrize('n', range(12))
def test_tile_programs_equal_the_oracle(emul, n):
    calls = _calls()
    assert len(calls) == 12
    name, call = calls[n]
    got = run_call(emul, call)
    np.testing.assert_array_equal(got, call.want, err_msg='%s %s' % (name, call.jobs))     # planes AND the bytes around them


def test_other_bytes_around_a_source_plane_give_the_same_output(emul):
    """The host load reads only inside the plane; whatever surrounds it, same bytes."""
    _library()
    m = FC.plane('random', 33, 65, 5)
    want = FC.oracle(m, 2.5)
    for pad in range(4):
        for noise in (0x00, 0xFF):
            src = np.full(pad + m.size + 5, noise, np.uint8)
            src[pad:pad + m.size] = m.reshape(-1)
            out = np.full(m.size + 9, FC.GUARD, np.uint8)
            run_emul(emul, src, out, [(pad, 3, 33, 65, 2.5)])
            assert np.array_equal(out[3:3 + m.size].reshape(33, 65), want)
            assert (out[:3] == FC.GUARD).all() and (out[3 + m.size:] == FC.GUARD).all()


def test_tile_programs_are_clean_under_the_sanitizers(tmp_path):
    """Host code only: a stand-alone program over the tile programs, built with -fsanitize=address,undefined, every buffer
    of exactly the size the library asks for.  It runs as its own process with the sanitizers' runtimes linked in
    statically (no library order to satisfy); nothing of it is loaded into this one."""
    exe = str(tmp_path / 'sanitize_feather')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan',
                           '-o', exe, os.path.join(ROOT, 'tests', 'host_emul', 'sanitize_feather.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'feather tile programs: clean', r.stdout + r.stderr


# ---------------------------------------------------------------- properties of the definition, on the programs' outputs
PROPERTY_SIGMAS = [0.5, 2.5, 20, 64]


def test_constant_planes_come_out_unchanged(emul):
    for sigma in PROPERTY_SIGMAS:
        for v0 in range(0, 256, 4):
            src = np.repeat(np.arange(v0, v0 + 4, dtype=np.uint8), 45)          # four 5 x 9 planes, one value each
            out = run_emul(emul, src, np.zeros_like(src), [(45 * k, 45 * k, 5, 9, sigma) for k in range(4)])
            assert np.array_equal(out, src), (sigma, v0)
    for h, w in FC.SIZES:
        for v in (0, 1, 127, 128, 254, 255):
            assert (feather_one(emul, np.full((h, w), v, np.uint8), 7) == v).all()


def test_output_lies_within_the_inputs_range(emul):
    for s, (h, w) in enumerate(FC.SIZES):
        for sigma in PROPERTY_SIGMAS:
            m = np.random.default_rng(300 + s).integers(37, 203, (h, w), dtype=np.uint8)
            got = feather_one(emul, m, sigma)
            assert m.min() <= got.min() and got.max() <= m.max(), (h, w, sigma)


def test_flipping_both_axes_flips_the_output(emul):
    for s, (h, w) in enumerate(FC.SIZES):
        for sigma in PROPERTY_SIGMAS:
            m = FC.plane('random', h, w, 400 + s)
            a = feather_one(emul, m, sigma)
            b = feather_one(emul, np.ascontiguousarray(m[::-1, ::-1]), sigma)
            assert np.array_equal(b[::-1, ::-1], a), (h, w, sigma)


# ---------------------------------------------------------------- status codes, no device
def test_status_codes_before_any_launch():
    import t2onet_amd.functional as T
    lib = _library()
    p = torch.zeros(64).data_ptr()

    def status(jobs, src=p, out=p, ws=p, ws_bytes=1 << 20, J=None, table=True):
        return lib.t2o_feather_u8(src, out, T.feather_jobs(jobs) if table else None, len(jobs) if J is None else J, ws, ws_bytes, None)
    one = (0, 0, 4, 4, 2.0)
    assert status([one], src=None) == 1 and b'null' in lib.t2o_last_error()
    assert status([one], out=None) == 1 and status([one], table=False) == 1
    assert status([one], J=0) == 1 and b'1 <= J <= 4' in lib.t2o_last_error()
    assert status([one] * 5) == 1 and status([one], J=-1) == 1
    assert status([(0, 0, 4, 4, -0.5)]) == 1 and b'sigma' in lib.t2o_last_error()
    assert status([(0, 0, 4, 4, float('nan'))]) == 1 and status([(0, 0, 4, 4, 64.5)]) == 1
    assert status([(0, 0, 0, 4, 2.0)]) == 1 and b'positive' in lib.t2o_last_error()
    assert status([(0, 0, 4, -1, 2.0)]) == 1
    assert status([(0, 0, 1 << 16, 1 << 15, 2.0)]) == 1 and b'2^31' in lib.t2o_last_error()
    assert status([(-1, 0, 4, 4, 2.0)]) == 1 and b'offset' in lib.t2o_last_error()
    assert status([(0, -1, 4, 4, 2.0)]) == 1
    assert status([one, (32, 15, 4, 4, 2.0)]) == 1 and b'overlap' in lib.t2o_last_error()
    assert status([(0, 20, 4, 4, 2.0), one, (0, 35, 2, 2, 1.0)]) == 1 and b'overlap' in lib.t2o_last_error()
    # the workspace: 2 bytes per pixel, rows padded to 4 pixels; too small or absent is status 3, as elsewhere
    assert lib.t2o_feather_workspace_bytes(T.feather_jobs([one]), 1) == 4 * 4 * 2
    assert lib.t2o_feather_workspace_bytes(T.feather_jobs([(0, 0, 3, 5, 1.0), (0, 16, 2, 9, 0)]), 2) == (3 * 8 + 2 * 12) * 2
    assert lib.t2o_feather_workspace_bytes(T.feather_jobs([(0, 0, 0, 5, 1.0)]), 1) == 0
    assert lib.t2o_feather_workspace_bytes(None, 1) == 0 and lib.t2o_feather_workspace_bytes(T.feather_jobs([one]), 5) == 0
    assert status([one], ws_bytes=31) == 3 and b'workspace' in lib.t2o_last_error()
    assert status([one], ws=None) == 3
    # the weights
    w = np.zeros(193, np.uint16)
    r = ctypes.c_int(0)
    assert lib.t2o_feather_weights(2.0, None, ctypes.addressof(r)) == 1 and lib.t2o_feather_weights(2.0, w.ctypes.data, None) == 1
    for bad in (-1.0, float('nan'), 64.0001, float('inf')):
        assert lib.t2o_feather_weights(bad, w.ctypes.data, ctypes.addressof(r)) == 1 and b'sigma' in lib.t2o_last_error()
    assert lib.t2o_feather_weights(64.0, w.ctypes.data, ctypes.addressof(r)) == 0 and r.value == 192
    # the Python surface turns them into exceptions that carry the library's text
    with pytest.raises(ValueError, match='sigma'):
        T.feather_weights(65)
    with pytest.raises(ValueError, match='GPU'):
        T.feather_u8(torch.zeros(48, dtype=torch.uint8), [one])


# ---------------------------------------------------------------- the Python surface
def test_feather_option_parsing(tmp_path):
    from PIL import Image
    from t2onet_amd import edit_cli
    named = {'all': 'a.png', 'tone': 'b.png'}
    assert edit_cli.parse_feather_args(None, named) == {} and edit_cli.parse_feather_args([], {}) == {}
    assert edit_cli.parse_feather_args(['3'], named) == {'all': 3.0}
    assert edit_cli.parse_feather_args(['tone=2.5', '8'], named) == {'tone': 2.5, 'all': 8.0}
    assert edit_cli.parse_feather_args(['0', 'tone=64'], named) == {'all': 0.0, 'tone': 64.0}
    with pytest.raises(ValueError, match='no --mask to feather'):
        edit_cli.parse_feather_args(['3'], {})
    with pytest.raises(ValueError, match="no --mask was given under 'color'"):
        edit_cli.parse_feather_args(['color=3'], named)
    with pytest.raises(ValueError, match="no --mask was given under 'all'"):
        edit_cli.parse_feather_args(['all=3'], {'tone': 'b.png'})
    for bad in ('soft', 'tone=', 'tone=x'):
        with pytest.raises(ValueError, match='not a number'):
            edit_cli.parse_feather_args([bad], named)
    for bad in ('-1', '64.5', 'nan', 'tone=inf'):
        with pytest.raises(ValueError, match=r'\[0, 64\]'):
            edit_cli.parse_feather_args([bad], named)
    # keyed like the masks: an unnamed sigma stands for every mask, a named one wins
    m1 = FC.plane('vedge', 20, 30)
    assert edit_cli.ACTIONS.index('tone') == 5
    assert edit_cli.feather_argument({}, named) is None
    assert edit_cli.feather_argument({'all': 3.0}, named) == {'all': 3.0, 5: 3.0}
    assert edit_cli.feather_argument({'tone': 2.0}, named) == {5: 2.0}
    assert edit_cli.feather_argument({'tone': 2.0, 'all': 8.0}, named) == {'all': 8.0, 5: 2.0}
    # the command refuses before it needs a model or a GPU
    Image.fromarray(np.zeros((20, 30, 3), np.uint8)).save(str(tmp_path / 'photo.png'))
    Image.fromarray(m1).save(str(tmp_path / 'm.png'))
    common = ['--img', str(tmp_path / 'photo.png'), '--request', 'x', '--checkpoint', 'none.pth']
    with pytest.raises(ValueError, match='no --mask to feather'):
        edit_cli.main(common + ['--feather', '3'])
    with pytest.raises(ValueError, match="no --mask was given under 'tone'"):
        edit_cli.main(common + ['--mask', str(tmp_path / 'm.png'), '--feather', 'tone=3'])
    with pytest.raises(ValueError, match=r'\[0, 64\]'):
        edit_cli.main(common + ['--mask', str(tmp_path / 'm.png'), '--feather', '65'])
    with pytest.raises(ValueError, match='another key feathers the same plane'):          # two names, one file, two sigmas
        edit_cli.main(common + ['--mask', str(tmp_path / 'm.png'), '--mask', 'tone=' + str(tmp_path / 'm.png'),
                                '--feather', '3', '--feather', 'tone=4'])
    # the record gains 'feather' only when the flag was given
    steps = np.zeros((1, 20, 30, 3), np.uint8)
    par = torch.zeros(1, 24)
    rec = edit_cli.write_outputs(str(tmp_path / 'a'), str(tmp_path / 'photo.png'), 'x', steps[0], steps, [0], par,
                                 masks={'all': 'm.png'}, feather={'all': 3.0})
    assert rec['feather'] == {'all': 3.0} and rec['masks'] == {'all': 'm.png'}
    rec = edit_cli.write_outputs(str(tmp_path / 'b'), str(tmp_path / 'photo.png'), 'x', steps[0], steps, [0], par, masks={'all': 'm.png'})
    assert 'feather' not in rec and rec['masks'] == {'all': 'm.png'}


def test_edit_image_checks_feather_before_any_device_use():
    from t2onet_amd.edit import checked_feather, edit_image
    img = np.zeros((6, 8, 3), np.uint8)
    m1, m2 = FC.plane('vedge', 6, 8), FC.plane('hedge', 6, 8)
    x = torch.zeros(1, 4, dtype=torch.long)
    # model = None: any use of the model or a device would raise something else than ValueError
    with pytest.raises(ValueError, match='feather without masks'):
        edit_image(None, img, x, feather=3)
    with pytest.raises(ValueError, match='feather without masks'):
        edit_image(None, img, x, feather={'all': 3})
    with pytest.raises(ValueError, match='names no mask'):
        edit_image(None, img, x, masks={'all': m1}, feather={0: 3})
    with pytest.raises(ValueError, match='another key feathers the same plane'):
        edit_image(None, img, x, masks={'all': m1, 0: m1}, feather={'all': 3, 0: 4})
    for bad in (-1, 64.5, float('nan')):
        with pytest.raises(ValueError, match='sigma must lie'):
            edit_image(None, img, x, masks={'all': m1}, feather=bad)
    # what the call is made from: one sigma per distinct plane, 0 left out
    assert checked_feather(None, None) == {} and checked_feather(None, {'all': m1}) == {}
    assert checked_feather(3, {'all': m1, 0: m1, 1: m2}) == {id(m1): 3.0, id(m2): 3.0}
    assert checked_feather({'all': 2, 0: 2.0, 1: 0}, {'all': m1, 0: m1, 1: m2}) == {id(m1): 2.0}
