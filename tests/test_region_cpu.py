"""No-GPU checks of the region kernels (t2o_region.hip): the kernels' programs, compiled for the host from the shared header
(tests/host_emul/emul_region.cpp) and run for every workgroup of the three grids with the border lanes in three orders,
against the flood-fill oracle byte for byte, guard bytes included; the cases themselves; the status codes of the entry
point; the wand terms of edit.py, --select's reading of them and apply_cli's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import region_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('t2o_region_math.h', 't2o_select_math.h', 't2o_replay_math.h', 't2o_pixel_math.h', 't2o_image_math.h')


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
    lib = _compile('emul_region')
    import t2onet_amd.functional as T
    assert lib.emul_region_tile() == RC.TILE and lib.emul_region_launches() == T.REGION_LAUNCHES
    assert lib.emul_region_args_bytes() <= 2048                      # the job table travels in the kernel arguments
    assert lib.emul_region_lds_bytes() <= 16 * 1024 and lib.emul_region_ws_align() == 16
    return lib


def run_emul(lib, photo, out, jobs, order=0, roots=None):
    """The programs over every workgroup of the call's three grids; photo / out: numpy byte buffers."""
    J = len(jobs)
    cols = list(zip(*jobs))
    LL, II = ctypes.c_longlong * J, ctypes.c_int * J
    rc = lib.emul_region_u8(photo.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), LL(*cols[0]), LL(*cols[1]),
                            *([II(*cols[k]) for k in range(2, 8)] + [J, order, roots.ctypes.data_as(ctypes.c_void_p) if roots is not None else None]))
    assert rc == 0
    return out


def _library():
    from t2onet_amd import build, _lib
    if os.path.exists(build.hipcc_path()):
        build.build()
    elif not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libt2onet_hip.so is absent and there is no hipcc to build it')
    return _lib.load()


# ---------------------------------------------------------------- the cases and the oracle
N_CALLS = 16


def _blocks_touched(plane):
    ys, xs = np.nonzero(plane)
    return len(set(zip((ys // 64).tolist(), (xs // 64).tolist())))


def test_cases_cover_what_they_should():
    cs = {c[0]: c for c in RC.cases()}
    calls = RC.calls()
    assert len(calls) == N_CALLS and len(cs) == 56
    shapes = {c[1].shape[:2] for c in cs.values()}
    assert shapes >= {(1, 1), (1, 7), (7, 1), (5, 6), (65, 67), (67, 131), (130, 197), (129, 129), (96, 160), (257, 263), (300, 301), (513, 1027)}
    assert {c[5] for c in cs.values()} == {4, 8} and {c[4] for c in cs.values()} >= {0, 7, RC.TOL, 255}
    for c in cs.values():                                            # the seed is always selected
        assert RC.want(c[0])[c[3], c[2]] == 255, c[0]
    # checkerboards: the seed alone with 4 steps, every square of its colour with 8
    for name, (h, w) in (('checker_5x6', (5, 6)), ('checker_65x67', (65, 67))):
        assert RC.want(name + '_c4').sum() == 255
        assert np.array_equal(RC.want(name + '_c8') == 255, RC.checkerboard(h, w))
    for name in ('blobs_small', 'blobs_corner', 'blobs_anticorner'):  # two blobs that touch at one diagonal corner
        a, b = RC.want(name + '_c4') == 255, RC.want(name + '_c8') == 255
        assert a.sum() > 10 and b.sum() > a.sum() + 10 and (b | ~a).all()
    for conn in (4, 8):
        assert np.array_equal(RC.want('u_shape_c%d' % conn) == 255, RC.u_shape())           # both arms, through the bottom row
        assert np.array_equal(RC.want('comb_c%d' % conn) == 255, RC.comb())                 # all 17 teeth from the last one
        assert np.array_equal(RC.want('serpentine_far_end_c%d' % conn) == 255, RC.serpentine(130, 197))
        wall = RC.want('serpentine_wall_c%d' % conn) == 255
        assert wall.sum() == 196 and wall[1, :196].all()                                     # one wall between two turns
        assert np.array_equal(RC.want('spiral_c%d' % conn) == 255, RC.spiral(129)[0])
        assert np.array_equal(RC.want('rings_c%d' % conn) == 255, RC.ring_depth(96, 160) // 2 == 4)      # the third ring only
        assert (RC.want('all_passing_c%d' % conn) == 255).all()
        patch = np.zeros((45, 59), bool)
        patch[10:31, 12:41] = True
        assert np.array_equal(RC.want('tol0_patch_c%d' % conn) == 255, patch)
        assert np.array_equal(RC.want('tolerance_edges_c%d' % conn), RC.tolerance_edges()[1])
    assert RC.want('serpentine_far_end_c4')[0, 0] == 255 and cs['serpentine_far_end_c4'][2:4] == (196, 128)   # the smallest index is farthest
    assert RC.spiral(129)[0].sum() > 129 * 129 // 3 and RC.spiral(129)[1] == cs['spiral_c4'][3:1:-1]
    # the noise cases have not degenerated: large ragged regions and single pixels are both among them
    noisy = [n for n in cs if n.startswith('noise')]
    assert len(noisy) == 2 * 5 * 2
    assert sum(_blocks_touched(RC.want(n)) >= 3 for n in noisy) >= 1
    assert sum(int(RC.want(n).sum()) == 255 for n in noisy) >= 1
    print('noise regions (pixels, 64 x 64 blocks):', [(n, int(RC.want(n).sum()) // 255, _blocks_touched(RC.want(n))) for n in noisy])
    # the larger frame: from the noise below through the one joint up the whole serpentine, and back
    for n in ('big_from_noise_c8', 'big_from_path_c4'):
        sel = RC.want(n) == 255
        assert sel[0, 0] and sel[255, 700] and sel[256, 700] and sel[256:].sum() > 1000 and _blocks_touched(sel) > 50, n
    # offsets: every residue of both, the misaligned call with none at 0, guards around every destination
    jobs = [j for _, c in calls for j in c.jobs]
    assert {j[0] % 4 for j in jobs} == {0, 1, 2, 3} == {j[1] % 4 for j in jobs}
    mis = dict(calls)['misaligned']
    assert sorted(j[0] % 4 for j in mis.jobs) == [1, 2, 3] == sorted(j[1] % 4 for j in mis.jobs) and all(j[3] % 2 == 1 for j in mis.jobs)
    for _, c in calls:
        for j in c.jobs:
            assert j[1] >= 1 and j[1] + j[2] * j[3] < len(c.out)
    multi = dict(calls)['multi_job']
    assert len(multi.jobs) == 4 and len({j[0] for j in multi.jobs}) == 3               # two jobs share a photo
    for k in (2, 3, 6, 7):
        assert len({j[k] for j in multi.jobs}) >= 2                                   # sizes, tol and conn differ
    assert len({j[4:6] for j in multi.jobs}) == 4


def test_oracle_agrees_with_scipy_label():
    ndimage = pytest.importorskip('scipy.ndimage')
    for name in ('noise50_seed0', 'noise59_seed1', 'blobs_anticorner', 'spiral', 'checker_65x67'):
        for conn, structure in ((4, [[0, 1, 0], [1, 1, 1], [0, 1, 0]]), (8, np.ones((3, 3), int))):
            _, photo, sx, sy, tol, _ = next(c for c in RC.cases() if c[0] == '%s_c%d' % (name, conn))
            labels, _ = ndimage.label(RC.passing(photo, sx, sy, tol), structure=structure)
            assert np.array_equal(RC.want('%s_c%d' % (name, conn)) == 255, labels == labels[sy, sx]), (name, conn)


@pytest.mark.parametrize('n', range(N_CALLS))
def test_programs_equal_the_oracle_in_every_lane_order(emul, n):
    name, call = RC.calls()[n]
    total = sum(j[2] * j[3] for j in call.jobs)
    first = None
    for order in range(3):
        roots = np.full(total, -2, np.int32)
        got = run_emul(emul, call.photo.copy(), call.out.copy(), call.jobs, order, roots)
        np.testing.assert_array_equal(got, call.want, err_msg='%s order %d %s' % (name, order, call.names))      # planes AND the bytes around them
        if first is None:
            first = roots
            at = 0
            for j, nm in zip(call.jobs, call.names):                  # a root is the smallest index of its component
                r = roots[at:at + j[2] * j[3]]
                sel = np.flatnonzero(RC.want(nm).reshape(-1) == 255)
                assert (r[sel] == sel.min()).all() and (r[np.setdiff1d(np.flatnonzero(r >= 0), sel)] != sel.min()).all(), nm
                at += j[2] * j[3]
        np.testing.assert_array_equal(roots, first, err_msg='%s: the final roots depend on the order' % name)


def test_multi_job_call_equals_separate_calls(emul):
    call = dict(RC.calls())['multi_job']
    whole = run_emul(emul, call.photo.copy(), call.out.copy(), call.jobs)
    single = call.out.copy()
    for job in call.jobs:
        run_emul(emul, call.photo.copy(), single, [job])
    assert np.array_equal(whole, single) and np.array_equal(whole, call.want)


def test_programs_are_clean_under_the_sanitizers(tmp_path):
    """Host code only: a stand-alone program over the programs, built with -fsanitize=address,undefined, every buffer of
    exactly the needed size.  It runs as its own process with the sanitizers' runtimes linked in statically; nothing of it
    is loaded into this one."""
    exe = str(tmp_path / 'sanitize_region')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan',
                           '-o', exe, os.path.join(ROOT, 'tests', 'host_emul', 'sanitize_region.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'region programs: clean', r.stdout + r.stderr


# ---------------------------------------------------------------- status codes, no device
def test_status_codes_before_any_launch():
    import t2onet_amd.functional as T
    lib = _library()
    buf = torch.zeros(4096, dtype=torch.uint8)
    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    p, o, wp = buf.data_ptr(), torch.zeros(4096, dtype=torch.uint8).data_ptr(), ws.data_ptr()
    assert wp % 16 == 0

    def status(jobs, photo=p, out=o, J=None, table=True, work=wp, work_bytes=1 << 16):
        return lib.t2o_region_u8(photo, out, T.region_jobs(jobs) if table else None, len(jobs) if J is None else J, work, work_bytes, None)

    def one(po=0, oo=0, h=4, w=4, sx=1, sy=2, tol=32, conn=4):
        return [(po, oo, h, w, sx, sy, tol, conn)]
    assert status(one(), photo=None) == 1 and b'null' in lib.t2o_last_error()
    assert status(one(), out=None) == 1 and status(one(), table=False) == 1
    assert status(one(), J=0) == 1 and b'1 <= J <= 4' in lib.t2o_last_error()
    assert status(one() * 5) == 1 and status(one(), J=-1) == 1
    assert status(one(h=0)) == 1 and b'positive' in lib.t2o_last_error()
    assert status(one(w=-1)) == 1 and b'positive' in lib.t2o_last_error()
    assert status(one(h=1 << 16, w=1 << 15)) == 1 and b'2^31' in lib.t2o_last_error()
    for k in ('po', 'oo'):
        assert status(one(**{k: -1})) == 1 and b'offset' in lib.t2o_last_error(), k
    for bad in (dict(sx=-1), dict(sx=4), dict(sy=-1), dict(sy=4), dict(sx=1 << 20)):
        assert status(one(**bad)) == 1 and b'seed' in lib.t2o_last_error(), bad
    for bad in (-1, 256, 1 << 20):
        assert status(one(tol=bad)) == 1 and b'tol' in lib.t2o_last_error(), bad
    for bad in (0, 6, -4, 5, 16):
        assert status(one(conn=bad)) == 1 and b'conn' in lib.t2o_last_error(), bad
    # one writer per byte
    assert status(one() + one(oo=15)) == 1 and b'destinations overlap' in lib.t2o_last_error()
    assert status(one(oo=20) + one() + one(h=2, w=2, sx=0, sy=0, oo=35)) == 1 and b'destinations overlap' in lib.t2o_last_error()
    # photo and out address the same memory: no destination on a photo of the call, its own or another job's
    assert status(one(oo=47), out=p) == 1 and b'overlaps a photo' in lib.t2o_last_error()
    assert status(one(po=100, oo=0) + one(po=0, oo=300), out=p) == 1 and b'overlaps a photo' in lib.t2o_last_error()
    assert status(one(po=1, oo=47), out=p + 1) == 1 and b'overlaps a photo' in lib.t2o_last_error()        # two views of one buffer
    # the workspace
    need = lib.t2o_region_workspace_bytes(T.region_jobs(one()), 1)
    assert need == 4 * 4 * 4
    assert status(one(), work=None) == 3 and b'workspace' in lib.t2o_last_error()
    assert status(one(), work_bytes=need - 1) == 3 and b'workspace' in lib.t2o_last_error()
    assert status(one(), work=wp + 8) == 3 and b'16-byte aligned' in lib.t2o_last_error()
    assert status(one(tol=256), work=None) == 1                      # the values are judged first
    # the Python surface turns them into exceptions before anything else
    with pytest.raises(ValueError, match='GPU'):
        T.region_u8(buf, one())
    with pytest.raises(ValueError, match='is \\(photo_offset'):
        T.region_jobs([(0, 0, 4, 4, 1, 2, 32)])
    with pytest.raises(ValueError, match='not an integer'):
        T.region_jobs([(0, 0, 4, 4, 1.5, 2, 32, 4)])
    with pytest.raises(ValueError, match='does not fit'):
        T.region_jobs([(0, 0, 4, 1 << 31, 1, 2, 32, 4)])
    assert (T.REGION_MAX_JOBS, T.REGION_LAUNCHES) == (4, 3) and T.REGION_LAUNCHES <= 4
    assert T.SELECT_KINDS == ('lum', 'sat', 'hue', 'linear', 'radial', 'plane')               # the wand is no kind of select_u8
    assert lib.t2o_abi_version() == 4


def test_workspace_bytes_and_the_struct():
    import t2onet_amd.functional as T
    lib = _library()

    def need(jobs, J=None):
        return lib.t2o_region_workspace_bytes(T.region_jobs(jobs), len(jobs) if J is None else J)
    assert need([(0, 0, 1, 1, 0, 0, 0, 4)]) == 16                    # 4 bytes per pixel, a job's rounded up to 16
    assert need([(0, 0, 37, 53, 5, 5, 32, 8)]) == 7856 == (4 * 37 * 53 + 15) // 16 * 16
    assert need([(0, 0, 4000, 6000, 0, 0, 255, 4)]) == 4 * 4000 * 6000
    assert need([(0, 0, 5, 7, 1, 1, 1, 4), (9, 99, 3, 9, 2, 2, 2, 8)]) == 144 + 112
    assert need([(0, 0, 46340, 46340, 1, 1, 1, 4)]) == 4 * 46340 * 46340
    assert need([(0, 0, 5, 7, 1, 1, 1, 4)] * 4) == 4 * 144
    # 0 for a table that would be refused
    for bad in ([(0, 0, 5, 7, 7, 1, 1, 4)], [(0, 0, 5, 7, 1, 5, 1, 4)], [(0, 0, 5, 7, 1, 1, 256, 4)], [(0, 0, 5, 7, 1, 1, 1, 6)], [(0, 0, 0, 7, 0, 0, 1, 4)],
                [(0, -1, 5, 7, 1, 1, 1, 4)], [(-1, 0, 5, 7, 1, 1, 1, 4)], [(0, 0, 1 << 16, 1 << 15, 1, 1, 1, 4)], [(0, 0, 5, 7, 1, 1, 1, 4)] * 5):
        assert need(bad) == 0, bad
    assert need([(0, 0, 5, 7, 1, 1, 1, 4)], J=0) == 0 and lib.t2o_region_workspace_bytes(None, 1) == 0
    # the ctypes struct against the header, field for field
    with open(os.path.join(ROOT, 'include', 't2onet_hip.h')) as f:
        body = re.search(r'typedef struct \{([^}]*)\} t2o_region_job_t;', f.read()).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [(t.strip(), n.strip()) for t, names in re.findall(r'(long long|int)\s+([^;]+);', body) for n in names.split(',')]
    kinds = {'long long': ctypes.c_longlong, 'int': ctypes.c_int}
    assert [(n, kinds[t]) for t, n in fields] == list(T.RegionJob._fields_)
    assert ctypes.sizeof(T.RegionJob) == 40 and T.RegionJob.h.offset == 16 and T.RegionJob.conn.offset == 36
    assert '#define T2O_REGION_MAX_JOBS 4' in open(os.path.join(ROOT, 'include', 't2onet_hip.h')).read()


# ---------------------------------------------------------------- the Python surface
def test_wand_terms_in_user_units():
    from t2onet_amd.edit import WAND_TOL, check_select_terms, select_terms, wand_keys, wand_resolved
    assert WAND_TOL == 0.125
    assert select_terms([('wand', 0.5, 0.1)], 101, 201) == [('wand', 0, 100, 10, 32)]              # the default tolerance is the byte 32
    assert select_terms([('!wand8', 1.0, 1.0, 0.08)], 101, 201) == [('wand8', 1, 200, 100, 20)]    # 20.4 -> 20
    assert select_terms([('wand', 0, 0, 0), ('wand8', 1, 0, 1)], 7, 9) == [('wand', 0, 0, 0, 0), ('wand8', 0, 8, 0, 255)]
    # rounding at w - 1 and h - 1: floor(v (w - 1) + 0.5), never outside the frame
    assert select_terms([('wand', 0.9999, 0.9999)], 6, 8)[0][2:4] == (7, 5)
    assert select_terms([('wand', 0.5, 0.5)], 6, 8)[0][2:4] == (4, 3)                              # 3.5 -> 4, 2.5 -> 3
    assert select_terms([('wand', 0.07, 0.93)], 1, 1)[0][2:4] == (0, 0)
    assert select_terms([('wand', 0.4999, 0.1, 0.002)], 3, 3)[0][2:] == (1, 0, 1)                  # 0.51 -> 1
    for bad, why in [(('wand', -0.01, 0.5), r'the seed lies in \[0, 1\]'), (('wand', 0.5, 1.01), r'the seed lies in \[0, 1\]'),
                     (('wand8', 2, 0), r'the seed lies in \[0, 1\]'), (('wand', 0.5, 0.5, -0.1), r'tolerance lies in \[0, 1\]'),
                     (('wand', 0.5, 0.5, 1.5), r'tolerance lies in \[0, 1\]'), (('wand', 0.5), 'takes a seed x, y'),
                     (('wand8', 0.5, 0.5, 0.1, 0.2), 'takes a seed x, y'), (('wand',), 'takes a seed x, y'), (('wand', 'a', 0), 'not a number'),
                     (('wand', float('nan'), 0), 'not finite'), (('wand4', 0, 0), 'the kind is one of')]:
        with pytest.raises(ValueError, match=why):
            check_select_terms([bad])
    with pytest.raises(ValueError, match='the kind is one of lum, sat, hue, linear, radial'):       # the list only grew
        check_select_terms([('plane', 0)])
    with pytest.raises(ValueError, match='1 to 4 terms'):
        check_select_terms([('wand', 0, 0)] * 5)
    a = select_terms([('wand', 0.5, 0.5), ('hue', 200, 260), ('!wand', 0.5, 0.5)], 6, 8)
    b = select_terms([('wand8', 0.5, 0.5), ('wand', 0.5, 0.5, 0.2), ('wand', 0.5, 0.5)], 6, 8)
    assert wand_keys([a, b]) == [(4, 3, 32, 4), (4, 3, 32, 8), (4, 3, 51, 4)]                      # equal ones are shared
    at = {(4, 3, 32, 4): 1000, (4, 3, 32, 8): 2000, (4, 3, 51, 4): 3000}
    assert wand_resolved(a, at) == [('plane', 0, 1000), a[1], ('plane', 1, 1000)]                  # the invert flag stays with the term
    assert wand_resolved(b, at) == [('plane', 0, 2000), ('plane', 0, 3000), ('plane', 0, 1000)]


def test_select_plan_counts_a_painted_mask_beside_wand_terms():
    import t2onet_amd.functional as T
    from t2onet_amd.edit import edit_image, select_plan
    m = np.zeros((6, 8), np.uint8)
    wand = ('wand', 0.5, 0.5)
    painted, specs, by_op, sigma = select_plan({'all': [wand, ('hue', 200, 260), ('!wand8', 0, 0, 0.5)]}, {'all': m}, {'all': 2}, 6, 8)
    assert len(painted) == 1 and specs == [((('wand', 0, 4, 3, 32), ('hue', 0, 853, 1109, 0), ('wand8', 1, 0, 0, 128)), 0)] and sigma == {0: 2.0}
    with pytest.raises(ValueError, match='4 terms and a painted mask'):
        select_plan({'all': [wand] * 4}, {'all': m}, None, 6, 8)
    assert len(select_plan({'all': [wand] * 4}, None, None, 6, 8)[1]) == 1
    with pytest.raises(ValueError, match='5 distinct planes'):
        select_plan({k: [('wand', 0.25 * k, 0.5)] for k in range(5)}, None, None, 6, 8)
    # edit_image checks everything before any device use: model = None would raise something else than ValueError
    img, x = np.zeros((6, 8, 3), np.uint8), torch.zeros(1, 4, dtype=torch.long)
    for bad, why in [([('wand', 1.5, 0)], 'the seed lies'), ([('wand', 0, 0, 2)], 'tolerance lies'), ([('wand', 0)], 'takes a seed')]:
        with pytest.raises(ValueError, match=why):
            edit_image(None, img, x, select={'all': bad})
    with pytest.raises(ValueError, match='sigma must lie'):
        edit_image(None, img, x, select={'all': [wand]}, feather=65)
    assert T.SELECT_KINDS == ('lum', 'sat', 'hue', 'linear', 'radial', 'plane')
    with pytest.raises(ValueError, match='not a term kind'):         # an unresolved wand term never reaches the select kernel
        T.select_jobs([(0, 0, 6, 8, [('wand', 0, 4, 3, 32)])])


def test_select_option_parsing_and_the_record():
    from t2onet_amd import apply_cli, edit_cli
    P = edit_cli.parse_select_terms
    assert P('wand:0.5,0.1:0.08+hue:200:260:20') == [('wand', 0.5, 0.1, 0.08), ('hue', 200.0, 260.0, 20.0)]
    assert P('!wand8:0,1') == [('!wand8', 0.0, 1.0)] and P('wand8:1e-1,.5:1') == [('wand8', 0.1, 0.5, 1.0)]
    for bad, why in [('wand9:0,0', 'not a term'), ('!!wand:0,0', 'not a term'), ('wand', r'X,Y\[:TOL\]'), ('wand:0,0:0.1:3', r'X,Y\[:TOL\]'),
                     ('wand:0.5', 'does not have the numbers'), ('wand:0.5:0.1', 'does not have the numbers'), ('wand:0,0,0', 'does not have the numbers'),
                     ('wand:0,0:1,2', 'does not have the numbers'), ('wand:a,b', 'not a number')]:
        with pytest.raises(ValueError, match=why) as e:
            P(bad)
        assert bad in str(e.value)                                   # errors name the spec
    A = edit_cli.parse_select_args
    assert A(['tone=wand:0.5,0.1:0.08+hue:200:260:20', '!wand8:0,0']) == {'tone': 'wand:0.5,0.1:0.08+hue:200:260:20', 'all': '!wand8:0,0'}
    for bad, why in [('wand:1.5,0', 'the seed lies'), ('tone=wand:0,0:1.5', 'tolerance lies'), ('wand:0,-0.1', 'the seed lies')]:
        with pytest.raises(ValueError, match=why) as e:
            A([bad])
        assert bad in str(e.value)
    assert edit_cli.select_argument(A(['tone=!wand:0.5,0.1'])) == {5: [('!wand', 0.5, 0.1)]}
    # the record keeps the rule text; apply_cli reads it back and gives every photo its own seed pixel
    ops = [['brightness', [0.5]], ['tone', [0.5] * 8]]
    rec = {'operations': ops, 'select': {'all': 'wand:0.5,0.1:0.08+hue:200:260:20', 'tone': '!wand8:1,1'}, 'feather': {'tone': 2.5}}
    select, feather = apply_cli.parse_local([rec])
    assert select == rec['select'] and feather == {'tone': 2.5}
    planes, mask_of = apply_cli.local_planes([0, 5, 0], select, feather)
    assert planes == [((('wand', 0.5, 0.1, 0.08), ('hue', 200.0, 260.0, 20.0)), 0.0), ((('!wand8', 1.0, 1.0),), 2.5)] and mask_of == [0, 1, 0]
    from t2onet_amd.edit import select_terms
    assert select_terms(planes[0][0], 40, 60, 'record')[0] == ('wand', 0, 30, 4, 20)               # 29.5 -> 30, 3.9 -> 4
    assert select_terms(planes[0][0], 33, 90, 'record')[0] == ('wand', 0, 45, 3, 20)               # 44.5 -> 45, 3.2 -> 3
    with pytest.raises(ValueError, match='the seed lies'):
        apply_cli.parse_local([dict(rec, select={'all': 'wand:2,0'})])
