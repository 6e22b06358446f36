"""No-GPU checks of the mask morphology (t2o_morph.hip): the cases and the exact consequences of the definition on the
oracle; the kernels' tile programs, compiled for the host from the shared header (tests/host_emul/emul_morph.cpp) and run
for every workgroup of both launches in two thread orders, against the brute-force int64 oracle byte for byte, guard bytes
included; the same programs under the sanitizers as a program of their own; the status codes of the entry points; the
`grow` of edit.py, --grow / --shrink / --border and apply_cli's reading of a record's 'grow'."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import morph_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('t2o_morph_math.h', 't2o_feather_math.h', 't2o_replay_math.h', 't2o_pixel_math.h', 't2o_image_math.h')


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
    lib = _compile('emul_morph')
    assert (lib.emul_morph_col_tile_h(), lib.emul_morph_col_tile_w()) == MC.COL_TILE
    assert (lib.emul_morph_row_tile_h(), lib.emul_morph_row_tile_w()) == MC.ROW_TILE
    assert lib.emul_morph_max_radius() == 64
    return lib


@pytest.fixture(scope='module')
def calls():
    return MC.calls()                                                # the oracle runs once per plane, here


def run_emul(lib, src, out, jobs, reverse=0):
    """The two tile programs over every job; src / out: numpy byte buffers (the same object for a call in one buffer)."""
    J = len(jobs)
    rc = lib.emul_morph_u8(src.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                           (ctypes.c_longlong * J)(*[j[0] for j in jobs]), (ctypes.c_longlong * J)(*[j[1] for j in jobs]),
                           (ctypes.c_int * J)(*[j[2] for j in jobs]), (ctypes.c_int * J)(*[j[3] for j in jobs]),
                           (ctypes.c_int * J)(*[j[4] for j in jobs]), (ctypes.c_int * J)(*[MC.MODES.index(j[5]) for j in jobs]), J, reverse)
    assert rc == 0
    return out


def run_call(lib, call, reverse=0):
    src = call.src.copy()
    out = src if call.out is call.src else call.out.copy()
    return run_emul(lib, src, out, call.jobs, reverse)


def _library():
    from t2onet_amd import build, _lib
    if os.path.exists(build.hipcc_path()):
        build.build()
    elif not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libt2onet_hip.so is absent and there is no hipcc to build it')
    return _lib.load()


# ---------------------------------------------------------------- the cases and the definition
def test_cases_cover_what_they_should(calls):
    cases = MC.cases()
    shapes = {c[1].shape for c in cases}
    assert {c[1].shape for c in cases if c[2] == 64} >= {(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (130, 200)}      # the radius exceeds the frame
    assert shapes >= {(63, 65), (64, 64), (65, 63), (129, 67), (200, 136), (130, 200)}
    for h, w in ((63, 65), (64, 64), (65, 63), (129, 67)):              # features on the tile corners, in every mode
        m = MC.corners(h, w)
        assert any(m[y, x] >= 128 for y in (62, 63, 64) for x in (62, 63, 64) if y < h and x < w)     # the 64 x 64 tiles' corner
        assert any(m[y, x] >= 128 for y in (7, 8) for x in (62, 63, 64) if x < w) or w < 64            # the 8-row tiles'
        assert m[0, 0] >= 128 and m[h - 1, w - 1] >= 128
        assert {c[3] for c in cases if c[1].shape == (h, w) and c[0].startswith('corner')} == set(MC.MODES)
    assert {c[2] for c in cases} >= set(MC.RADII) and {c[3] for c in cases} == set(MC.MODES)
    assert {(c[2], c[3]) for c in cases} >= {(r, 'grow') for r in MC.RADII}
    by_name = {c[0]: c for c in cases}
    wide = by_name['wide_130x200_grow'][1]
    (y,), (x,) = np.nonzero(wide)
    assert len({(y + d) // 64 for d in (-64, 0, 64)}) == 3 and len({(x + d) // 64 for d in (-64, 0, 49)}) == 3 and x + 64 > 199
    assert by_name['last_pixel_grow'][1][-1, -1] == 255 and by_name['last_pixel_grow'][1].sum() == 255
    first = by_name['first_unset_shrink'][1]
    assert first[0, 0] == 0 and (first.reshape(-1)[1:] == 255).all()
    assert not by_name['all_0_grow'][1].any() and (by_name['all_255_grow'][1] == 255).all()
    assert set(np.unique(by_name['threshold_grow'][1])) == {127, 128}
    assert by_name['soft_grow'][1].min() >= 1 and by_name['soft_grow'][1].max() <= 254 and len(np.unique(by_name['soft_grow'][1])) > 200
    sky = by_name['frame_shrink_5'][1]
    assert sky[0].all() and sky[:, 0].all() and not sky[-1, -1]
    jobs = [j for _, c in calls for j in c.jobs]
    assert all(j[0] % 2 == 1 for n, c in calls for j in c.jobs if c.out is not c.src)                    # sources at odd offsets
    assert {j[1] % 4 for j in jobs} == {0, 1, 2, 3}
    assert all((c.out == MC.GUARD).all() for _, c in calls if c.out is not c.src)                        # guard bytes around every destination
    by_call = dict(calls)
    assert by_call['in_place'].out is by_call['in_place'].src and all(j[0] == j[1] for j in by_call['in_place'].jobs)
    four = by_call['four_jobs'].jobs
    assert len(four) == 4 and len({j[2:4] for j in four}) >= 3 and {j[5] for j in four} == set(MC.MODES)
    shared = by_call['shared_source'].jobs
    assert shared[0][0] == shared[1][0] and shared[0][1] != shared[1][1]


def test_exact_consequences_of_the_definition():
    for name, m, radius, mode in MC.cases():
        if m.size > 9000:
            continue                                                 # (the complement of a large sparse plane: brute force would take long)
        inv = 255 - m                                                # S of the inverse is the complement of S: 255 - b >= 128 <=> b < 128
        np.testing.assert_array_equal(MC.oracle(m, radius, 'shrink'), 255 - MC.oracle(inv, radius, 'grow'), err_msg=name)
        np.testing.assert_array_equal(MC.oracle(m, 0, 'grow'), np.where(m >= 128, 255, 0))
        assert not MC.oracle(m, 0, 'border').any()
        g, s, b = (MC.oracle(m, radius, k) for k in MC.MODES)
        assert np.array_equal(b, g & ~s) and (s <= np.where(m >= 128, 255, 0)).all() and (g >= np.where(m >= 128, 255, 0)).all()
    for r in MC.RADII:
        zero, full = np.zeros((9, 11), np.uint8), np.full((9, 11), 255, np.uint8)
        assert not any(MC.oracle(zero, r, k).any() for k in MC.MODES)
        assert (MC.oracle(full, r, 'grow') == 255).all() and (MC.oracle(full, r, 'shrink') == 255).all() and not MC.oracle(full, r, 'border').any()
    assert len(MC.disc_offsets(25)) == 1961 and len(MC.disc_offsets(5)) == 81
    for r in (25, 5):
        m = np.zeros((57, 59), np.uint8)
        m[28, 29] = 255
        got = MC.oracle(m, r, 'grow')
        ys, xs = np.nonzero(got)
        assert {(int(y) - 28, int(x) - 29) for y, x in zip(ys, xs)} == MC.disc_offsets(r)
    disc = MC.disc_offsets(25)
    assert (7, 24) in disc and (15, 20) in disc and (18, 18) not in disc and (25, 1) not in disc
    # the frame rule: a sky that touches the top of the photo still touches it after a shrink
    sky = np.zeros((40, 70), np.uint8)
    sky[:20] = 255
    want = np.zeros((40, 70), np.uint8)
    want[:15] = 255
    assert np.array_equal(MC.oracle(sky, 5, 'shrink'), want)


# ---------------------------------------------------------------- tile programs
def test_threshold_tables(emul):
    for r in range(65):
        c = np.full(68, 9, np.uint8)
        assert emul.emul_morph_thresholds(r, c.ctypes.data_as(ctypes.c_void_p)) == 0
        want = [int(np.floor(np.sqrt(np.float64(r * r - k * k)))) for k in range(r + 1)]
        assert all(v * v + k * k <= r * r < (v + 1) ** 2 + k * k for k, v in enumerate(want))
        assert c[:r + 1].tolist() == want and not c[r + 1:].any()
    c = np.zeros(68, np.uint8)
    assert emul.emul_morph_thresholds(65, c.ctypes.data_as(ctypes.c_void_p)) == 1 and emul.emul_morph_thresholds(-1, c.ctypes.data_as(ctypes.c_void_p)) == 1


@pytest.mark.parametrize('reverse', [0, 1], ids=['threads_up', 'threads_down'])
def test_tile_programs_equal_the_oracle(emul, calls, reverse):
    for name, call in calls:
        got = run_call(emul, call, reverse)
        np.testing.assert_array_equal(got, call.want, err_msg='%s %s' % (name, call.jobs))     # planes AND the bytes around them


def test_other_bytes_around_a_source_plane_give_the_same_output(emul):
    m = MC.corners(65, 63)
    want = MC.oracle(m, 5, 'border')
    for pad in range(4):
        for noise in (0x00, 0xFF):
            src = np.full(pad + m.size + 5, noise, np.uint8)
            src[pad:pad + m.size] = m.reshape(-1)
            out = np.full(m.size + 9, MC.GUARD, np.uint8)
            run_emul(emul, src, out, [(pad, 3, 65, 63, 5, 'border')])
            assert np.array_equal(out[3:3 + m.size].reshape(65, 63), want)
            assert (out[:3] == MC.GUARD).all() and (out[3 + m.size:] == MC.GUARD).all()


def test_tile_programs_are_clean_under_the_sanitizers(tmp_path):
    """Host code only: a stand-alone program over the tile programs, built with -fsanitize=address,undefined, every buffer
    of exactly the size the library asks for.  It runs as its own process with the sanitizers' runtimes linked in
    statically (no library order to satisfy); nothing of it is loaded into this one."""
    exe = str(tmp_path / 'sanitize_morph')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan',
                           '-o', exe, os.path.join(ROOT, 'tests', 'host_emul', 'sanitize_morph.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'morph tile programs: clean', r.stdout + r.stderr


def test_kernel_argument_and_lds_budgets(emul):
    assert emul.emul_morph_args_bytes() <= 1024                      # the job table and the thresholds travel in the kernel arguments
    assert emul.emul_morph_col_lds_bytes() == (64 + 2 * 64) * 64 <= 12 * 1024
    assert emul.emul_morph_row_lds_bytes() <= 9 * 1024               # several workgroups of either pass on a CU's 160 KB


# ---------------------------------------------------------------- status codes, no device
def test_status_codes_before_any_launch():
    import t2onet_amd.functional as T
    lib = _library()
    p = torch.zeros(64).data_ptr()
    assert (T.MORPH_MAX_JOBS, T.MORPH_MAX_RADIUS, T.MORPH_MODES) == (4, 64, MC.MODES)

    def status(jobs, src=p, out=p, ws=p, ws_bytes=1 << 20, J=None, table=True):
        return lib.t2o_morph_u8(src, out, T.morph_jobs(jobs) if table else None, len(jobs) if J is None else J, ws, ws_bytes, None)

    def need(jobs, J=None):
        return lib.t2o_morph_workspace_bytes(T.morph_jobs(jobs), len(jobs) if J is None else J)
    one = (0, 0, 4, 4, 2, 'grow')
    assert status([one], src=None) == 1 and b'null' in lib.t2o_last_error()
    assert status([one], out=None) == 1 and status([one], table=False) == 1
    assert status([one], J=0) == 1 and b'1 <= J <= 4' in lib.t2o_last_error()
    assert status([one] * 5) == 1 and status([one], J=-1) == 1
    refused = [([(0, 0, 0, 4, 2, 'grow')], b'positive'), ([(0, 0, 4, -1, 2, 'grow')], b'positive'),
               ([(0, 0, 1 << 16, 1 << 15, 2, 'grow')], b'2^31'),
               ([(-1, 0, 4, 4, 2, 'grow')], b'offset'), ([(0, -1, 4, 4, 2, 'grow')], b'offset'),
               ([(0, 0, 4, 4, -1, 'grow')], b'radius'), ([(0, 0, 4, 4, 65, 'shrink')], b'radius'),
               ([(0, 0, 4, 4, 2, 3)], b'mode'), ([(0, 0, 4, 4, 2, -1)], b'mode'),
               ([one, (32, 15, 4, 4, 2, 'border')], b'overlap'), ([(0, 20, 4, 4, 2, 'grow'), one, (0, 35, 2, 2, 1, 'shrink')], b'overlap')]
    for jobs, word in refused:
        assert status(jobs) == 1 and word in lib.t2o_last_error(), (jobs, lib.t2o_last_error())
        assert need(jobs) == 0, jobs
    assert lib.t2o_morph_workspace_bytes(None, 1) == 0 and need([one], 5) == 0 and need([one], 0) == 0
    # the workspace: 1 byte per pixel and field, rows padded to 4 pixels; too small or absent is status 3, misaligned status 1
    assert need([one]) == 4 * 4 and need([(0, 0, 4, 4, 2, 'border')]) == 2 * 4 * 4
    assert need([(0, 0, 3, 5, 1, 'shrink'), (0, 16, 2, 9, 0, 'border')]) == 3 * 8 + 2 * 2 * 12
    assert status([one], ws_bytes=15) == 3 and b'workspace' in lib.t2o_last_error()
    assert status([one], ws=None) == 3
    assert status([one], ws=p + 4) == 1 and b'aligned' in lib.t2o_last_error()
    # the Python surface turns them into exceptions before it needs a device
    with pytest.raises(ValueError, match='GPU'):
        T.morph_u8(torch.zeros(48, dtype=torch.uint8), [one])
    with pytest.raises(ValueError, match='mode'):
        T.morph_jobs([(0, 0, 4, 4, 2, 'melt')])


# ---------------------------------------------------------------- the Python surface
def test_checked_grow_and_select_plan():
    from t2onet_amd.edit import checked_grow, edit_image, select_plan
    img = np.zeros((6, 8, 3), np.uint8)
    m1, m2 = np.zeros((6, 8), np.uint8), np.full((6, 8), 255, np.uint8)
    x = torch.zeros(1, 4, dtype=torch.long)
    # model = None: any use of the model or a device would raise something else than ValueError
    with pytest.raises(ValueError, match='grow without masks'):
        edit_image(None, img, x, grow=3)
    with pytest.raises(ValueError, match='grow without masks'):
        edit_image(None, img, x, grow={'all': 3})
    with pytest.raises(ValueError, match='names no mask'):
        edit_image(None, img, x, masks={'all': m1}, grow={0: 3})
    with pytest.raises(ValueError, match='names no mask'):
        edit_image(None, img, x, select={4: [('lum', 0, 1)]}, grow={5: 3})
    with pytest.raises(ValueError, match='another key moves the same plane'):
        edit_image(None, img, x, masks={'all': m1, 0: m1}, grow={'all': 3, 0: 4})
    with pytest.raises(ValueError, match='another key moves the same plane'):
        edit_image(None, img, x, masks={'all': m1, 0: m1}, grow={'all': 3, 0: -3})
    for bad in (65, -65, 2.5, float('nan'), 'x', True, ('border', 65), ('border', -1), ('melt', 2), ('border',), ('grow', 1.5)):
        with pytest.raises(ValueError, match='grow'):
            edit_image(None, img, x, masks={'all': m1}, grow=bad)
    # what the call is made from: one (mode, radius) per distinct plane; growing or shrinking by 0 left out, a border of 0 kept
    assert checked_grow(None, None) == {} and checked_grow(None, {'all': m1}) == {}
    assert checked_grow(3, {'all': m1, 0: m1, 1: m2}) == {id(m1): ('grow', 3), id(m2): ('grow', 3)}
    assert checked_grow(-64, {'all': m1}) == {id(m1): ('shrink', 64)}
    assert checked_grow({'all': 2, 0: 2.0, 1: 0}, {'all': m1, 0: m1, 1: m2}) == {id(m1): ('grow', 2)}
    assert checked_grow({'all': ('border', 5), 1: ('shrink', 2)}, {'all': m1, 1: m2}) == {id(m1): ('border', 5), id(m2): ('shrink', 2)}
    assert checked_grow({'all': 0, 0: ('shrink', 0), 1: ('border', 0)}, {'all': m1, 0: m1, 1: m2}) == {id(m2): ('border', 0)}
    # select_plan: today's 4 and 5 values stay; with grow one more follows
    sel = {4: [('lum', 0, 1)], 'all': [('sat', 0, 0.5)]}
    four = select_plan(sel, None, None, 6, 8)
    five = select_plan(sel, None, None, 6, 8, {})
    assert len(four) == 4 and len(five) == 5 and five[:4] == four and five[4] == {}
    keys = {}
    plus = select_plan(sel, None, None, 6, 8, keys=keys, grow={4: 4, 'all': ('border', 2)})
    assert len(plus) == 5 and plus[:4] == four and plus[4] == {keys[4]: ('grow', 4), keys['all']: ('border', 2)}
    six = select_plan(sel, None, {4: 2}, 6, 8, {4: 3}, None, -2)
    assert len(six) == 6 and six[5] == {0: ('shrink', 2), 1: ('shrink', 2)} and list(six[4]) == [keys[4]] and six[3] == {keys[4]: 2.0}
    assert select_plan(sel, None, None, 6, 8, grow={})[4] == {} and select_plan(sel, None, None, 6, 8, grow=0)[4] == {}
    with pytest.raises(ValueError, match='names no mask'):
        select_plan(sel, None, None, 6, 8, grow={5: 3})


def test_grow_option_parsing(tmp_path):
    from PIL import Image
    from t2onet_amd import edit_cli
    named = {'all': 'a.png', 'tone': 'b.png'}
    assert edit_cli.parse_grow_args(None, None, None, named) == {} and edit_cli.parse_grow_args([], [], [], {}) == {}
    assert edit_cli.parse_grow_args(['3'], None, None, named) == {'all': ('grow', 3)}
    assert edit_cli.parse_grow_args(['tone=4'], ['0'], None, named) == {'tone': ('grow', 4), 'all': ('shrink', 0)}
    assert edit_cli.parse_grow_args(None, None, ['tone=64'], named) == {'tone': ('border', 64)}
    for flag in range(3):
        with pytest.raises(ValueError, match='no --mask or --select to'):
            edit_cli.parse_grow_args(*[['3'] if k == flag else None for k in range(3)], {})
        with pytest.raises(ValueError, match="no --mask or --select was given under 'color'"):
            edit_cli.parse_grow_args(*[['color=3'] if k == flag else None for k in range(3)], named)
        for bad in ('soft', 'tone=', 'tone=x', '2.5', 'nan'):
            with pytest.raises(ValueError, match='not a whole number'):
                edit_cli.parse_grow_args(*[[bad] if k == flag else None for k in range(3)], named)
        for bad in ('-1', '65', 'tone=100'):
            with pytest.raises(ValueError, match=r'0\.\.64'):
                edit_cli.parse_grow_args(*[[bad] if k == flag else None for k in range(3)], named)
    for a in ((['3', '4'], None, None), (['3'], ['3'], None), (None, ['tone=1'], ['tone=2']), (['tone=1', '2', 'tone=1'], None, None)):
        with pytest.raises(ValueError, match='one of --grow, --shrink and --border to a plane'):
            edit_cli.parse_grow_args(*a, named)
    # keyed like the planes: an unnamed value stands for every plane, a named one wins
    assert edit_cli.ACTIONS.index('tone') == 5
    assert edit_cli.grow_argument({}, named) is None
    assert edit_cli.grow_argument({'all': ('grow', 3)}, named) == {'all': ('grow', 3), 5: ('grow', 3)}
    assert edit_cli.grow_argument({'tone': ('border', 2)}, named) == {5: ('border', 2)}
    assert edit_cli.grow_argument({'tone': ('shrink', 2), 'all': ('grow', 8)}, named) == {'all': ('grow', 8), 5: ('shrink', 2)}
    # the command refuses before it needs a model or a GPU
    Image.fromarray(np.zeros((20, 30, 3), np.uint8)).save(str(tmp_path / 'photo.png'))
    Image.fromarray(np.zeros((20, 30), np.uint8)).save(str(tmp_path / 'm.png'))
    common = ['--img', str(tmp_path / 'photo.png'), '--request', 'x', '--checkpoint', 'none.pth']
    with pytest.raises(ValueError, match='no --mask or --select to grow'):
        edit_cli.main(common + ['--grow', '3'])
    with pytest.raises(ValueError, match="no --mask or --select was given under 'tone'"):
        edit_cli.main(common + ['--mask', str(tmp_path / 'm.png'), '--shrink', 'tone=3'])
    with pytest.raises(ValueError, match=r'0\.\.64'):
        edit_cli.main(common + ['--select', 'inpaint=wand:0.5,0.5', '--border', 'inpaint=65'])
    with pytest.raises(ValueError, match='one of --grow, --shrink and --border'):
        edit_cli.main(common + ['--select', 'inpaint=wand:0.5,0.5', '--grow', 'inpaint=4', '--shrink', 'inpaint=4'])
    with pytest.raises(ValueError, match='another key moves the same plane'):             # two names, one file, two moves
        edit_cli.main(common + ['--mask', str(tmp_path / 'm.png'), '--mask', 'tone=' + str(tmp_path / 'm.png'), '--grow', '3', '--grow', 'tone=4'])
    # the record gains 'grow' only when a flag was given
    steps = np.zeros((1, 20, 30, 3), np.uint8)
    par = torch.zeros(1, 24)
    rec = edit_cli.write_outputs(str(tmp_path / 'a'), str(tmp_path / 'photo.png'), 'x', steps[0], steps, [0], par,
                                 select={'inpaint': 'wand:0.5,0.5'}, grow={'inpaint': ('grow', 4), 'all': ('border', 2)})
    assert rec['grow'] == {'inpaint': ['grow', 4], 'all': ['border', 2]}
    rec = edit_cli.write_outputs(str(tmp_path / 'b'), str(tmp_path / 'photo.png'), 'x', steps[0], steps, [0], par, select={'inpaint': 'wand:0.5,0.5'})
    assert 'grow' not in rec


def test_apply_cli_reads_grow_from_a_record():
    from t2onet_amd import apply_cli
    select = {'inpaint': 'wand:0.5,0.4:0.1', 'all': 'lum:0:1'}

    def rec(grow, **more):
        return [dict({'operations': [['tone', [0.0] * 8]], 'select': select, 'grow': grow}, **more)]
    assert apply_cli.parse_grow([{'operations': [], 'select': select}]) == {}
    assert apply_cli.parse_grow([{'operations': [], 'grow': {'all': ['grow', 4]}}]) == {}            # no 'select': a global replay
    assert apply_cli.parse_grow(rec({})) == {} and apply_cli.parse_grow(rec(None)) == {}
    assert apply_cli.parse_grow(rec({'inpaint': ['grow', 4], 'all': ['border', 2]})) == {'inpaint': ('grow', 4), 'all': ('border', 2)}
    assert apply_cli.parse_grow(rec({'all': ['shrink', 0]})) == {'all': ('shrink', 0)}
    for bad, word in (({'x': ['grow', 4]}, "entry 'x'"), ({'all': ['grow', 65]}, "entry 'all'"), ({'all': ['grow', -1]}, "entry 'all'"),
                      ({'inpaint': ['melt', 2]}, "entry 'inpaint'"), ({'all': ['grow', 2.5]}, "entry 'all'"), ({'all': ['grow', True]}, "entry 'all'"),
                      ({'all': 4}, "entry 'all'"), ({'all': ['grow']}, "entry 'all'"), ({'all': ['grow', '4']}, "entry 'all'"),
                      (['grow', 4], 'is {name'), ('4', 'is {name')):
        with pytest.raises(ValueError, match='record: \'grow\'.*' + word):
            apply_cli.parse_grow(rec(bad))
    # the planes of a list: a named entry wins over 'all'; growing or shrinking by 0 is no move
    grow = {'inpaint': ('grow', 4), 'all': ('border', 2)}
    planes, mask_of, fill_no = apply_cli.local_planes([5], select, {}, {}, 'inpaint', grow)
    assert [p[3] for p in planes] == [('border', 2), ('grow', 4)] and mask_of == [0] and fill_no == 1
    planes, mask_of = apply_cli.local_planes([5], select, {}, {}, None, {'all': ('shrink', 0)})
    assert planes[0][3] is None
    # today's shapes stay
    assert len(apply_cli.local_planes([5], select, {})[0][0]) == 2 and len(apply_cli.local_planes([5], select, {}, {})[0][0]) == 3
