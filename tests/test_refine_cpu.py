"""No-GPU checks of the mask refine kernels (t2o_refine.hip): the kernels' phase functions, compiled for the host from the
shared header (tests/host_emul/emul_refine.cpp) and run for every workgroup of the four grids, against the int64 oracle
byte for byte, guard bytes included; the exact properties of the definition; the status codes of the entry point;
--refine, the E rounding, edit_image's checks, the record keys and apply_cli's reading of them."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import refine_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('t2o_refine_math.h', 't2o_select_math.h', 't2o_replay_math.h', 't2o_pixel_math.h', 't2o_image_math.h')


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
    lib = _compile('emul_refine')
    assert {'kRefineRowW': lib.emul_refine_row_tile_w(), 'kRefineRowH': lib.emul_refine_row_tile_h(),
            'kRefineColW': lib.emul_refine_col_tile_w(), 'kRefineColH': lib.emul_refine_col_tile_h()} == RC.TILES
    assert lib.emul_refine_max_radius() == 64 == max(RC.RADII)
    assert lib.emul_refine_args_bytes() <= 2048                      # the job table travels in the kernel arguments
    assert max(lib.emul_refine_lds_bytes(p) for p in (1, 3, 4)) <= 32 * 1024 and lib.emul_refine_lds_bytes(2) == 0
    return lib


def run_emul(lib, photo, src, out, jobs):
    """The phase functions over every workgroup of the call's four grids; photo / src / out: numpy byte buffers."""
    J = len(jobs)
    cols = list(zip(*jobs))
    LL, II = ctypes.c_longlong * J, ctypes.c_int * J
    rc = lib.emul_refine_u8(photo.ctypes.data_as(ctypes.c_void_p), src.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                            LL(*cols[0]), LL(*cols[1]), LL(*cols[2]), II(*cols[3]), II(*cols[4]), II(*cols[5]), II(*cols[6]), J)
    assert rc == 0
    return out


def refine_one(lib, photo, plane, r, E):
    h, w = plane.shape
    return run_emul(lib, np.ascontiguousarray(photo).reshape(-1), np.ascontiguousarray(plane).reshape(-1), np.zeros(h * w, np.uint8),
                    [(0, 0, 0, h, w, r, E)]).reshape(h, w)


def _library():
    from t2onet_amd import build, _lib
    if os.path.exists(build.hipcc_path()):
        build.build()
    elif not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libt2onet_hip.so is absent and there is no hipcc to build it')
    return _lib.load()


# ---------------------------------------------------------------- the phase functions against the oracle
N_CALLS = 24


def test_cases_cover_what_they_should():
    calls = RC.calls()
    assert len(calls) == N_CALLS
    jobs = [j for _, c in calls for j in c.jobs]
    assert RC.SIZES == [(1, 1), (1, 5), (3, 1), (5, 7), (37, 53), (64, 64), (9, 257), (257, 65)]
    sp = RC.specs()
    assert {(s[0], s[1], s[2]) for s in sp} == {(h, w, r) for h, w in RC.SIZES for r in RC.RADII}      # every size at every radius
    assert {s[3] for s in sp} == set(RC.EPS2) and {s[4] for s in sp} == set(RC.PATTERNS)
    assert {(s[2], s[4]) for s in sp} >= {(r, p) for r in RC.RADII for p in ('contrast1', 'anti')}
    assert all(s[3] == 1 for s in sp if s[4] == 'contrast1')
    assert {(j[3], j[4], j[5], j[6]) for j in jobs} >= {s[:4] for s in sp}
    for k in range(3):                                               # all 4 residues of each offset on the two smallest sizes
        for size in RC.SIZES[:2]:
            assert {j[k] % 4 for j in jobs if (j[3], j[4]) == size} == {0, 1, 2, 3}
        assert {j[k] % 4 for j in jobs if (j[3], j[4]) not in RC.SIZES[:2]} == {0, 1, 2, 3}
    mixed = dict(calls)['mixed_call']
    assert len(mixed.jobs) == 4 and mixed.src is mixed.out
    assert sum(j[1] == j[2] for j in mixed.jobs) == 1                # one job in place
    (_, _, b, h, w, _, _), (_, s1, _, _, _, _, _) = mixed.jobs[:2]
    assert b < s1 < b + h * w                                        # job 1 reads what job 0 overwrites
    assert any(c.src is c.out and len(c.jobs) == 4 for n, c in calls if n.startswith('in_place'))
    # the guards exist: every plane of a destination buffer has an untouched byte on either side
    for _, c in calls:
        for j in c.jobs:
            assert j[2] >= 1 and j[2] + j[3] * j[4] < len(c.out)


def test_the_adversarial_patterns_reach_the_corners_of_the_arithmetic():
    """Conditions on the INPUTS, by the oracle's own intermediates: the anti-correlated plane gives negative cov, A and
    numerators (the floor-division case); the 1-byte guide step under a 0/255 plane at E = 1 gives |A| > 2^15."""
    photo, plane = RC.case('anti', 37, 53, 1)
    I, p = RC.lum(photo), plane.astype(np.int64)
    n = 25
    cov = n * RC.box(I * p, 2) - RC.box(I, 2) * RC.box(p, 2)
    den = n * RC.box(I * I, 2) - RC.box(I, 2) ** 2 + 26 * n * n
    A = (2 * cov * 1024 + den) // (2 * den)
    assert (cov < 0).mean() > 0.9 and A.min() < -500 and ((2 * cov * 1024 + den) % (2 * den) != 0).any()
    RC.PEAK['A'] = 0
    photo, plane = RC.case('contrast1', 37, 53, 1)
    RC.refine(RC.lum(photo), plane.astype(np.int64), 7, 1)
    assert 1 << 15 < RC.PEAK['A'] <= 65281


@pytest.mark.parametrize('n', range(N_CALLS))
def test_phase_functions_equal_the_oracle(emul, n):
    name, call = RC.calls()[n]
    out = call.out.copy()
    src = out if call.src is call.out else call.src.copy()
    got = run_emul(emul, call.photo.copy(), src, out, call.jobs)
    np.testing.assert_array_equal(got, call.want, err_msg='%s %s' % (name, call.jobs))        # planes AND the bytes around them
    if call.src is not call.out:
        np.testing.assert_array_equal(src, call.src)


# ---------------------------------------------------------------- the exact properties
def test_a_constant_plane_comes_out_unchanged(emul):
    photo = np.random.default_rng(1).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for c in (0, 1, 127, 254, 255):
        for r, E in [(1, 1), (7, 26), (64, 65025), (2, 65025)]:
            assert (refine_one(emul, photo, np.full((37, 53), c, np.uint8), r, E) == c).all(), (c, r, E)


def test_radius_zero_is_a_copy(emul):
    rng = np.random.default_rng(2)
    photo, plane = rng.integers(0, 256, (9, 257, 3), dtype=np.uint8), rng.integers(0, 256, (9, 257), dtype=np.uint8)
    for E in RC.EPS2:
        assert np.array_equal(refine_one(emul, photo, plane, 0, E), plane)


def test_a_constant_photo_leaves_a_function_of_the_plane_alone(emul):
    """A = 0 everywhere: the result is the plane's rounded box mean, box-meaned and rounded again -- whatever the photo's
    constant and whatever E."""
    plane = np.random.default_rng(3).integers(0, 256, (37, 53), dtype=np.uint8)
    for r in (1, 7):
        n = (2 * r + 1) ** 2
        B = (2 * (RC.box(plane.astype(np.int64), r) << 10) + n) // (2 * n)
        want = np.clip((2 * RC.box(B, r) + (n << 10)) // (2 * (n << 10)), 0, 255)
        for colour, E in [((0, 0, 0), 1), ((255, 255, 255), 26), ((10, 200, 30), 65025)]:
            photo = np.empty((37, 53, 3), np.uint8)
            photo[:] = colour
            assert np.array_equal(refine_one(emul, photo, plane, r, E), want), (r, colour, E)


def test_a_flip_of_both_axes_commutes(emul):
    rng = np.random.default_rng(4)
    photo, plane = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), rng.integers(0, 256, (37, 53), dtype=np.uint8)
    for r, E in [(1, 1), (2, 26), (7, 26), (64, 1)]:
        a = refine_one(emul, photo, plane, r, E)
        b = refine_one(emul, photo[::-1, ::-1].copy(), plane[::-1, ::-1].copy(), r, E)
        assert np.array_equal(a[::-1, ::-1], b), (r, E)


def test_the_jump_moves_onto_the_guide_edge(emul):
    """What the flag promises: a guide edge 4 pixels beside the plane's edge takes the plane's jump along."""
    h, w = 32, 64
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    photo = RC.grey(np.where(x >= 32, 230, 20))
    plane = np.where(x >= 36, 255, 0).astype(np.uint8)
    out = refine_one(emul, photo, plane, 8, 26).astype(np.int64)
    assert np.array_equal(out, RC.oracle(photo, plane, 8, 26))
    jump = np.abs(np.diff(out[h // 2]))
    assert jump.argmax() == 31                                       # between columns 31 and 32: the guide's edge
    assert jump[31] >= 2 * np.delete(jump, 31).max()                 # and no other step comes near it,
    assert jump[35] < 255 // 4                                       # least of all the 255 where the plane was painted


def test_programs_are_clean_under_the_sanitizers(tmp_path):
    """Host code only: a stand-alone program over the phase functions, built with -fsanitize=address,undefined, every buffer
    of exactly the needed size.  It runs as its own process with the sanitizers' runtimes linked in statically; nothing of
    it is loaded into this one."""
    exe = str(tmp_path / 'sanitize_refine')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan',
                           '-o', exe, os.path.join(ROOT, 'tests', 'host_emul', 'sanitize_refine.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'refine programs: clean', r.stdout + r.stderr


# ---------------------------------------------------------------- status codes, no device
def test_status_codes_before_any_launch():
    import t2onet_amd.functional as T
    lib = _library()
    buf = torch.zeros(4096, dtype=torch.uint8)
    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    p, o, wp = buf.data_ptr(), torch.zeros(4096, dtype=torch.uint8).data_ptr(), ws.data_ptr()
    assert wp % 16 == 0

    def status(jobs, photo=p, src=p, out=o, J=None, table=True, work=wp, work_bytes=1 << 16):
        return lib.t2o_refine_u8(photo, src, out, T.refine_jobs(jobs) if table else None, len(jobs) if J is None else J, work, work_bytes, None)

    def one(po=0, so=100, oo=0, h=4, w=4, r=2, E=26):
        return [(po, so, oo, h, w, r, E)]
    assert status(one(), photo=None) == 1 and b'null' in lib.t2o_last_error()
    assert status(one(), src=None) == 1 and status(one(), out=None) == 1 and status(one(), table=False) == 1
    assert status(one(), J=0) == 1 and b'1 <= J <= 4' in lib.t2o_last_error()
    assert status(one() * 5) == 1 and status(one(), J=-1) == 1
    for bad in (-1, 65, 1 << 20):
        assert status(one(r=bad)) == 1 and b'radius' in lib.t2o_last_error(), bad
    for bad in (0, -1, 65026):
        assert status(one(E=bad)) == 1 and b'eps2' in lib.t2o_last_error(), bad
    assert status(one(h=0)) == 1 and b'positive' in lib.t2o_last_error()
    assert status(one(w=-1)) == 1 and b'positive' in lib.t2o_last_error()
    assert status(one(h=1 << 16, w=1 << 15)) == 1 and b'2^31' in lib.t2o_last_error()
    for k in ('po', 'so', 'oo'):
        assert status(one(**{k: -1})) == 1 and b'offset' in lib.t2o_last_error(), k
    # one writer per byte
    assert status(one() + one(oo=15)) == 1 and b'destinations overlap' in lib.t2o_last_error()
    assert status(one(oo=20) + one() + one(h=2, w=2, oo=35)) == 1 and b'destinations overlap' in lib.t2o_last_error()
    # photo and out address the same memory: no destination on a photo of the call, its own or another job's
    assert status(one(oo=47), out=p) == 1 and b'overlaps a photo' in lib.t2o_last_error()
    assert status(one(po=100, oo=0) + one(po=0, oo=300), out=p) == 1 and b'overlaps a photo' in lib.t2o_last_error()
    assert status(one(po=1, oo=47), out=p + 1) == 1 and b'overlaps a photo' in lib.t2o_last_error()        # two views of one buffer
    # the workspace
    need = lib.t2o_refine_workspace_bytes(T.refine_jobs(one()), 1)
    assert need == 20 * 4 * 4
    assert status(one(), work=None) == 3 and b'workspace' in lib.t2o_last_error()
    assert status(one(), work_bytes=need - 1) == 3 and b'workspace' in lib.t2o_last_error()
    assert status(one(), work=wp + 8) == 3 and b'16-byte aligned' in lib.t2o_last_error()
    assert status(one(r=65), work=None) == 1                         # the values are judged first
    # the Python surface turns them into exceptions before anything else
    with pytest.raises(ValueError, match='GPU'):
        T.refine_u8(buf, buf, one())
    with pytest.raises(ValueError, match='is \\(photo_offset'):
        T.refine_jobs([(0, 0, 0, 4, 4, 2)])
    with pytest.raises(ValueError, match='not an integer'):
        T.refine_jobs([(0, 0, 0, 4, 4, 2.5, 26)])
    with pytest.raises(ValueError, match='does not fit'):
        T.refine_jobs([(0, 0, 0, 4, 1 << 31, 2, 26)])
    assert (T.REFINE_MAX_JOBS, T.REFINE_MAX_RADIUS, T.REFINE_MAX_EPS2, T.REFINE_LAUNCHES) == (4, 64, 65025, 4)
    assert lib.t2o_abi_version() == 4


def test_workspace_bytes():
    import t2onet_amd.functional as T
    lib = _library()

    def need(jobs, J=None):
        return lib.t2o_refine_workspace_bytes(T.refine_jobs(jobs), len(jobs) if J is None else J)
    assert ctypes.sizeof(T.RefineJob) == 40
    assert need([(0, 0, 0, 1, 1, 0, 1)]) == 20 * 4                   # rows padded to 4 pixels
    assert need([(0, 0, 0, 37, 53, 64, 26)]) == 20 * 37 * 56
    assert need([(0, 0, 0, 4000, 6000, 8, 26)]) == 20 * 4000 * 6000  # the radius does not enter
    assert need([(0, 0, 0, 5, 7, 1, 1), (9, 9, 99, 3, 8, 2, 2)]) == 20 * (5 * 8 + 3 * 8)
    assert need([(0, 0, 0, 46340, 46340, 1, 1)]) == 20 * 46340 * 46340
    assert need([(0, 0, 0, 5, 7, 1, 1)] * 4) % 16 == 0
    # 0 for a table that would be refused
    for bad in ([(0, 0, 0, 5, 7, 65, 1)], [(0, 0, 0, 5, 7, 1, 0)], [(0, 0, 0, 0, 7, 1, 1)], [(0, 0, -1, 5, 7, 1, 1)],
                [(0, 0, 0, 1 << 16, 1 << 15, 1, 1)], [(0, 0, 0, 5, 7, 1, 1)] * 5):
        assert need(bad) == 0, bad
    assert need([(0, 0, 0, 5, 7, 1, 1)], J=0) == 0 and lib.t2o_refine_workspace_bytes(None, 1) == 0


# ---------------------------------------------------------------- the Python surface
def test_eps_rounds_as_specified():
    from t2onet_amd.edit import REFINE_EPS, checked_refine, refine_eps2
    assert REFINE_EPS == 0.02 and refine_eps2(0.02) == 26            # 5.1^2 = 26.01
    assert refine_eps2(1.0) == 65025 and refine_eps2(1e-6) == 1 and refine_eps2(1 / 255.0) == 1
    assert refine_eps2(0.1) == 650 and refine_eps2(0.5) == 16256     # 25.5^2 = 650.25, 127.5^2 = 16256.25
    for eps in (0.003, 0.0048, 0.0049, 0.01, 0.25, 0.9999):
        assert refine_eps2(eps) == max(1, int(np.floor((np.float64(255.0) * np.float64(eps)) ** 2 + 0.5))), eps
    for bad in (0, -0.1, 1.0001, float('nan')):
        with pytest.raises(ValueError, match=r'\(0, 1\]'):
            refine_eps2(bad)
    m1, m2 = np.zeros((6, 8), np.uint8), np.zeros((6, 8), np.uint8)
    assert checked_refine(None, {'all': m1}) == {}
    assert checked_refine(4, {'all': m1, 0: m2}) == {id(m1): (4, 26), id(m2): (4, 26)}
    assert checked_refine((8, 0.1), {'all': m1}) == {id(m1): (8, 650)}
    assert checked_refine({'all': 4, 0: (0, 0.5)}, {'all': m1, 0: m2}) == {id(m1): (4, 26)}       # radius 0 leaves its plane
    assert checked_refine({0: 4.0, 1: (4, 0.02)}, {0: m1, 1: m1}) == {id(m1): (4, 26)}            # two keys, one plane, one value


def test_refine_option_parsing(tmp_path):
    from PIL import Image
    from t2onet_amd import edit_cli
    planes = {'all': 'm.png', 'tone': 'lum:0.5:1'}
    P = edit_cli.parse_refine_args
    assert P(None, planes) == {} and P([], {}) == {}
    assert P(['4'], planes) == {'all': (4, 0.02)} and P(['tone=8:0.1', '2'], planes) == {'tone': (8, 0.1), 'all': (2, 0.02)}
    assert P(['0:1'], planes) == {'all': (0, 1.0)} and P(['64:1e-3'], planes) == {'all': (64, 0.001)}
    assert edit_cli.refine_argument(P(['4', 'tone=8:0.1'], planes), planes) == {'all': (4, 0.02), 5: (8, 0.1)}
    assert edit_cli.refine_argument(P(['4'], planes), planes) == {'all': (4, 0.02), 5: (4, 0.02)}  # unnamed: every plane
    assert edit_cli.refine_argument(P(['tone=3'], planes), planes) == {5: (3, 0.02)}
    assert edit_cli.refine_argument({}, planes) is None
    for bad, why in [('65', '0..64'), ('-1', '0..64'), ('2.5', 'not a whole number'), ('a', 'not a whole number'), ('', 'RADIUS'),
                     ('4:0', r'\(0, 1\]'), ('4:1.5', r'\(0, 1\]'), ('4:nan', r'\(0, 1\]'), ('4:x', 'not a number'), ('4:0.1:2', 'RADIUS'),
                     ('color=4', "under 'color'"), ('glow=4', "under 'glow'")]:
        with pytest.raises(ValueError, match=why) as e:
            P([bad], planes)
        assert bad in str(e.value)                                   # errors name the spec
    with pytest.raises(ValueError, match='no --mask or --select to refine'):
        P(['4'], {})
    # the command refuses before it needs a model or a GPU
    Image.fromarray(np.zeros((20, 30, 3), np.uint8)).save(str(tmp_path / 'photo.png'))
    Image.fromarray(np.zeros((20, 30), np.uint8)).save(str(tmp_path / 'mask.png'))
    common = ['--request', 'x', '--checkpoint', 'none.pth', '--img', str(tmp_path / 'photo.png')]
    with pytest.raises(ValueError, match='no --mask or --select to refine'):
        edit_cli.main(common + ['--refine', '4'])
    with pytest.raises(ValueError, match='0..64'):
        edit_cli.main(common + ['--select', 'lum:0:1', '--refine', '65'])
    with pytest.raises(ValueError, match="under 'color'"):
        edit_cli.main(common + ['--mask', str(tmp_path / 'mask.png'), '--refine', 'color=4'])
    with pytest.raises(ValueError, match='another key refines the same plane'):
        edit_cli.main(common + ['--mask', str(tmp_path / 'mask.png'), '--mask', 'tone=' + str(tmp_path / 'mask.png'), '--refine', '4', '--refine', 'tone=5'])
    with pytest.raises(ValueError, match='another key refines the same plane'):
        edit_cli.main(common + ['--select', 'lum:0:1', '--select', 'tone=lum:0:1', '--refine', 'tone=5', '--refine', '4:0.5'])
    # the record gains 'refine' only when it was given
    steps, par = np.zeros((1, 20, 30, 3), np.uint8), torch.zeros(1, 24)
    rec = edit_cli.write_outputs(str(tmp_path / 'a'), str(tmp_path / 'photo.png'), 'x', steps[0], steps, [0], par,
                                 select={'all': 'lum:0.5:1'}, refine={'all': (4, 0.02)})
    assert rec['refine'] == {'all': [4, 0.02]} and rec['select'] == {'all': 'lum:0.5:1'} and 'feather' not in rec
    with open(str(tmp_path / 'a' / 'photo' / 'photo.json')) as f:
        assert json.load(f) == [json.loads(json.dumps(rec))]
    rec = edit_cli.write_outputs(str(tmp_path / 'b'), str(tmp_path / 'photo.png'), 'x', steps[0], steps, [0], par, select={'all': 'lum:0.5:1'})
    assert 'refine' not in rec


def test_edit_image_checks_refine_before_any_device_use():
    from t2onet_amd.edit import edit_image, select_plan
    img = np.zeros((6, 8, 3), np.uint8)
    m1, m2 = np.zeros((6, 8), np.uint8), np.full((6, 8), 255, np.uint8)
    x = torch.zeros(1, 4, dtype=torch.long)
    lum, sat = [('lum', 0.5, 1.0)], [('!sat', 0.0, 0.5, 0.1)]
    # model = None: any use of the model or a device would raise something else than ValueError
    with pytest.raises(ValueError, match='refine without masks'):
        edit_image(None, img, x, refine=4)
    for bad, why in [(65, '0..64'), (-1, '0..64'), (2.5, 'whole number'), ((4, 0), r'\(0, 1\]'), ((4, 1.5), r'\(0, 1\]'), ((4, 0.1, 2), 'neither a radius'),
                     ('a', 'not a number'), ((), 'neither a radius'), ({0: 4}, 'names no mask'), ({'all': 65}, '0..64')]:
        with pytest.raises(ValueError, match=why):
            edit_image(None, img, x, masks={'all': m1}, refine=bad)
        with pytest.raises(ValueError, match=why):
            edit_image(None, img, x, select={'all': lum}, refine=bad)
    with pytest.raises(ValueError, match='another key refines the same plane'):
        edit_image(None, img, x, masks={'all': m1, 0: m1}, refine={'all': 4, 0: 5})
    with pytest.raises(ValueError, match='another key refines the same plane'):
        edit_image(None, img, x, select={'all': lum, 0: lum}, refine={'all': (4, 0.02), 0: (4, 0.03)})
    with pytest.raises(ValueError, match='sigma must lie'):          # the older checks still run
        edit_image(None, img, x, select={'all': lum}, refine=4, feather=65)
    # what the launches are made from: a fifth value, only when refine is given
    plan = select_plan({'all': lum, 0: sat, 1: lum}, {0: m1, 2: m2, 3: m2}, {'all': 2}, 6, 8)
    assert len(plan) == 4
    plan = select_plan({'all': lum, 0: sat, 1: lum}, {0: m1, 2: m2, 3: m2}, {'all': 2}, 6, 8, {'all': 4, 2: (8, 0.1), 3: (8, 0.1), 0: 0})
    assert len(plan) == 5 and plan[:4] == select_plan({'all': lum, 0: sat, 1: lum}, {0: m1, 2: m2, 3: m2}, {'all': 2}, 6, 8)
    assert plan[4] == {0: (4, 26), 2: (8, 650)}                      # 'all' and 1 share plane 0; plane 1 (key 0) has radius 0
    assert select_plan({'all': lum}, None, None, 6, 8, {})[4] == {}


def test_apply_cli_reads_the_refine_of_a_record():
    from t2onet_amd import apply_cli
    ops = [['brightness', [0.5]], ['tone', [0.5] * 8]]
    rec = {'operations': ops, 'select': {'all': 'lum:0.5:1:0.1', 'tone': '!hue:200:260'}, 'feather': {'tone': 2.5}}
    assert apply_cli.parse_refine([rec]) == {}
    assert apply_cli.parse_refine([dict(rec, refine={'all': [4, 0.02], 'tone': [8, 0.1]})]) == {'all': (4, 0.02), 'tone': (8, 0.1)}
    assert apply_cli.parse_refine([{'operations': ops, 'masks': {'all': 'm.png'}, 'refine': {'all': [4, 0.02]}}]) == {}     # replayed globally
    select, feather = apply_cli.parse_local([rec])
    lum, hue = (('lum', 0.5, 1.0, 0.1),), (('!hue', 200.0, 260.0),)
    assert apply_cli.local_planes([0, 5, 0], select, feather) == ([(lum, 0.0), (hue, 2.5)], [0, 1, 0])                     # as before
    assert apply_cli.local_planes([0, 5, 0], select, feather, {'all': (4, 0.02)}) == ([(lum, 0.0, (4, 0.02)), (hue, 2.5, (4, 0.02))], [0, 1, 0])
    assert apply_cli.local_planes([0, 5], select, feather, {'tone': (8, 0.1)}) == ([(lum, 0.0, None), (hue, 2.5, (8, 0.1))], [0, 1])
    assert apply_cli.local_planes([0, 5], select, feather, {'all': (4, 0.02), 'tone': (0, 0.1)}) == ([(lum, 0.0, (4, 0.02)), (hue, 2.5, None)], [0, 1])
    for bad, why in [({'all': [65, 0.02]}, '0..64'), ({'all': [4, 2]}, r'\(0, 1\]'), ({'color': [4, 0.02]}, "under 'color'"),
                     ({'all': 4}, 'radius, eps'), (['4'], 'radius, eps')]:
        with pytest.raises(ValueError, match=why):
            apply_cli.parse_refine([dict(rec, refine=bad)])
