"""No-GPU checks of the fill kernels (t2o_fill.hip): the exact consequences of the definition on the oracle; the kernels'
programs, compiled for the host from the shared header (tests/host_emul/emul_fill.cpp) and run for every workgroup of the
three grids in two thread orders, against the oracle byte for byte, guard bytes included; the same programs under the
sanitizers as a program of their own; the status codes of the entry point; the `fill` of edit.py, --fill and apply_cli's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import fill_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('t2o_fill_math.h', 't2o_select_math.h', 't2o_replay_math.h', 't2o_pixel_math.h', 't2o_image_math.h')


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
    lib = _compile('emul_fill')
    import t2onet_amd.functional as T
    lib.emul_fill_ws_bytes.restype = ctypes.c_longlong
    assert lib.emul_fill_tile() == LC.TILE and lib.emul_fill_launches() == T.FILL_LAUNCHES
    assert lib.emul_fill_args_bytes() <= 2048                        # the job table travels in the kernel arguments
    assert lib.emul_fill_lds_bytes() <= 32 * 1024
    return lib


def run_emul(lib, call, jobs=None, order=0, buf=None):
    """The programs over every workgroup of the call's three grids -> the destination buffer."""
    jobs = call.jobs if jobs is None else jobs
    J = len(jobs)
    cols = list(zip(*jobs))
    LL, II = ctypes.c_longlong * J, ctypes.c_int * J
    photo = call.photo.copy() if buf is None else buf
    out = photo if call.same else call.out.copy()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.emul_fill_u8(P(photo), P(call.planes), P(out), LL(*cols[0]), LL(*cols[1]), LL(*cols[2]), II(*cols[3]), II(*cols[4]), J, order) == 0
    if not call.same:
        assert np.array_equal(photo, call.photo)
    return out


def _library():
    from t2onet_amd import build, _lib
    if os.path.exists(build.hipcc_path()):
        build.build()
    elif not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libt2onet_hip.so is absent and there is no hipcc to build it')
    return _lib.load()


def hard(plane):
    return np.where(plane > 0, 255, 0).astype(np.uint8)


# ---------------------------------------------------------------- the cases and the exact consequences of the definition
def test_cases_cover_what_they_should():
    cs = {c[0]: c for c in LC.cases()}
    assert len(cs) == 18 and len(LC.calls()) == 19
    assert {c[2].shape for c in cs.values()} >= {(1, 1), (1, 7), (7, 1), (2, 2), (63, 65), (64, 64), (65, 63), (129, 67), (200, 136), (300, 521), (130, 70)}
    assert sorted(tuple(np.argwhere(cs['two_by_two_known_%d%d' % (y, x)][2] == 0)[0]) for y in (0, 1) for x in (0, 1)) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for name in ('corner_63x65', 'corner_64x64', 'corner_65x63', 'corner_129x67'):
        m = cs[name][2]
        assert 0.02 < np.isin(m, LC.SOFT).mean() < 0.08 and set(np.unique(m)) == {0, 255} | set(LC.SOFT) and m[60, 60] == 255
        assert m[min(64, m.shape[0] - 1), min(64, m.shape[1] - 1)] == 255              # the hole reaches across the tile corner
    C, known = LC.pyramid(cs['tile_200x136'][1], cs['tile_200x136'][2])
    assert known[6].shape == (4, 3) and not known[6][1, 1] and known[6].sum() == 11     # one cell of level 6 is unknown
    C, known = LC.pyramid(cs['big_300x521'][1], cs['big_300x521'][2])
    assert len(known) == 11 and not known[7][0, 0] and not known[7][1, 1] and not known[8][0, 0] and known[9].all()
    assert (cs['big_300x521'][2][256:, 448:] == 255).mean() > 0.5                       # the ragged border tiles hold a hole
    m = cs['last_pixel_130x70'][2]
    assert (m == 0).sum() == 1 and m[129, 69] == 0
    assert (cs['all_255_70x66'][2] == 255).all() and not (cs['none_known_70x66'][2] == 0).any() and not cs['all_0_70x66'][2].any()
    # offsets: photos and planes at odd ones, every residue of the destination, guards around every destination
    jobs = [j for _, c in LC.calls() for j in c.jobs]
    assert all(j[0] % 2 == 1 and j[1] % 2 == 1 for j in jobs) and {j[2] % 4 for j in jobs} == {0, 1, 2, 3}
    for _, c in LC.calls():
        buf = c.photo if c.same else c.out
        for j in c.jobs:
            assert j[2] >= 1 and j[2] + 3 * j[3] * j[4] < len(buf)
    multi = dict(LC.calls())['multi_job']
    assert len(multi.jobs) == 4 and len({j[3:] for j in multi.jobs}) == 3 and len({j[0] for j in multi.jobs}) == 3     # sizes differ, two share a photo
    assert [j[0] == j[2] for j in multi.jobs] == [False, True, False, False]             # one runs in place, on a photo of its own
    assert multi.jobs[0][0] == multi.jobs[2][0] and multi.jobs[0][1] != multi.jobs[2][1]


def test_exact_consequences_on_every_case():
    for name, photo, plane in LC.cases():
        got = LC.want(name)
        kept = plane == 0
        assert np.array_equal(got[kept], photo[kept]), name           # kept pixels come out byte for byte
        if not kept.any():
            assert np.array_equal(got, photo), name                   # no source: the picture as it is
            continue
        fill = LC.oracle(photo, hard(plane))                          # the same sources: the fill itself where M > 0
        lo, hi = photo[kept].min(axis=0), photo[kept].max(axis=0)
        assert ((fill[~kept] >= lo) & (fill[~kept] <= hi)).all(), name
        P, M, F = photo.astype(np.int64), plane.astype(np.int64)[:, :, None], fill.astype(np.int64)
        assert np.array_equal(got, np.where(M == 0, P, (P * (255 - M) + F * M + 127) // 255)), name
        # transposing the photo and the plane transposes the output
        assert np.array_equal(LC.oracle(np.ascontiguousarray(photo.transpose(1, 0, 2)), np.ascontiguousarray(plane.T)), got.transpose(1, 0, 2)), name
    assert np.array_equal(LC.want('all_0_70x66'), next(c for c in LC.cases() if c[0] == 'all_0_70x66')[1])            # M == 0 is a copy


def test_one_colour_around_a_hole_and_one_known_pixel():
    rng = np.random.default_rng(5)
    for h, w, hole in ((70, 130, (slice(30, 70), slice(40, 129))), (5, 9, (slice(1, 4), slice(0, 8))), (129, 65, (slice(0, 128), slice(0, 64)))):
        photo = np.empty((h, w, 3), np.uint8)
        photo[:] = (201, 17, 94)
        plane = np.zeros((h, w), np.uint8)
        plane[hole] = 255
        photo[hole] = rng.integers(0, 256, photo[hole].shape, dtype=np.uint8)     # whatever lies under the hole
        got = LC.oracle(photo, plane)
        assert (got == np.array([201, 17, 94], np.uint8)).all(), (h, w)
    _, photo, plane = next(c for c in LC.cases() if c[0] == 'last_pixel_130x70')
    got = LC.want('last_pixel_130x70')
    assert (got[plane == 255] == photo[129, 69]).all()
    for y in (0, 1):
        for x in (0, 1):
            _, photo, plane = next(c for c in LC.cases() if c[0] == 'two_by_two_known_%d%d' % (y, x))
            assert (LC.want('two_by_two_known_%d%d' % (y, x))[plane == 255] == photo[y, x]).all()
    # flips are NO symmetry of the definition (the pyramid is anchored at the top-left): nothing here may rest on one
    _, photo, plane = next(c for c in LC.cases() if c[0] == 'corner_65x63')
    assert not np.array_equal(LC.oracle(photo[::-1].copy(), plane[::-1].copy())[::-1], LC.want('corner_65x63'))


def test_a_ramp_is_refilled_smoothly():
    """Not a bound of the definition, a sanity figure: a hole in a linear colour ramp comes back within a few bytes."""
    y, x = np.mgrid[:200, :320]
    photo = np.stack([x * 255 // 319, y * 255 // 199, (x + y) * 255 // 518], axis=2).astype(np.uint8)
    plane = np.zeros((200, 320), np.uint8)
    plane[60:140, 100:220] = 255
    err = np.abs(LC.oracle(photo, plane).astype(np.int64) - photo)[plane == 255]
    print('ramp, 80 x 120 hole: max error %d, mean %.2f bytes' % (err.max(), err.mean()))
    assert err.max() <= 16 and err.mean() <= 4.0


# ---------------------------------------------------------------- the kernels' programs on the host
N_CALLS = 19


@pytest.mark.parametrize('n', range(N_CALLS))
def test_programs_equal_the_oracle_in_both_thread_orders(emul, n):
    name, call = LC.calls()[n]
    for order in (0, 1):
        np.testing.assert_array_equal(run_emul(emul, call, order=order), call.want, err_msg='%s order %d %s' % (name, order, call.jobs))


def test_multi_job_call_equals_separate_calls(emul):
    call = dict(LC.calls())['multi_job']
    whole = run_emul(emul, call)
    buf = call.photo.copy()
    for k in (0, 2, 3, 1):                                           # the job in place last: it overwrites a photo
        run_emul(emul, call, [call.jobs[k]], buf=buf)
    assert np.array_equal(whole, buf) and np.array_equal(whole, call.want)


def test_workspace_layout(emul):
    """Levels 1..K at 8 bytes per cell, F from level min(6, K) up, every array rounded up to a 128-byte line."""
    def want(h, w):
        dims = [(h, w)]
        while dims[-1] != (1, 1):
            dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
        K = len(dims) - 1
        line = lambda n: (8 * n + 127) // 128 * 128
        return sum(line(a * b) for a, b in dims[1:]) + sum(line(a * b) for a, b in dims[min(6, K):])
    for h, w in ((1, 1), (1, 7), (2, 2), (64, 64), (65, 63), (300, 521), (4000, 6000)):
        assert emul.emul_fill_ws_bytes(h, w) == want(h, w), (h, w)
    assert emul.emul_fill_ws_bytes(4000, 6000) < 4000 * 6000 * 8 // 3 * 1.01           # about 8/3 bytes per pixel
    assert emul.emul_fill_ws_bytes(0, 5) == 0 and emul.emul_fill_ws_bytes(1 << 15, 1 << 15) == 0


def test_programs_are_clean_under_the_sanitizers(tmp_path):
    """Host code only: a stand-alone program over the programs, built with -fsanitize=address,undefined, every buffer of
    exactly the needed size.  It runs as its own process with the sanitizers' runtimes linked in statically; nothing of it
    is loaded into this one."""
    exe = str(tmp_path / 'sanitize_fill')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan',
                           '-o', exe, os.path.join(ROOT, 'tests', 'host_emul', 'sanitize_fill.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'fill programs: clean', r.stdout + r.stderr


# ---------------------------------------------------------------- status codes, no device
def test_status_codes_before_any_launch():
    import t2onet_amd.functional as T
    lib = _library()
    buf = torch.zeros(4096, dtype=torch.uint8)
    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    planes, dest = torch.zeros(4096, dtype=torch.uint8), torch.zeros(4096, dtype=torch.uint8)        # three buffers, alive to the end
    p, m, o, wp = buf.data_ptr(), planes.data_ptr(), dest.data_ptr(), ws.data_ptr()
    assert wp % 16 == 0 and len({p, m, o}) == 3

    def status(jobs, photo=p, plane=m, out=o, J=None, table=True, work=wp, work_bytes=1 << 16):
        return lib.t2o_fill_u8(photo, plane, out, T.fill_jobs(jobs) if table else None, len(jobs) if J is None else J, work, work_bytes, None)

    def one(po=0, mo=0, oo=0, h=4, w=4):
        return [(po, mo, oo, h, w)]
    assert status(one(), photo=None) == 1 and b'null' in lib.t2o_last_error()
    assert status(one(), plane=None) == 1 and status(one(), out=None) == 1 and status(one(), table=False) == 1
    assert status(one(), J=0) == 1 and b'1 <= J <= 4' in lib.t2o_last_error()
    assert status(one() * 5) == 1 and status(one(), J=-1) == 1
    assert status(one(h=0)) == 1 and b'positive' in lib.t2o_last_error()
    assert status(one(w=-1)) == 1 and b'positive' in lib.t2o_last_error()
    assert status(one(h=1 << 15, w=21846)) == 1 and b'2^31' in lib.t2o_last_error()      # 3 h w = 2^31 + 2^16
    for k in ('po', 'mo', 'oo'):
        assert status(one(**{k: -1})) == 1 and b'offset' in lib.t2o_last_error(), k
    # one writer per byte
    assert status(one() + one(oo=47)) == 1 and b'destinations overlap' in lib.t2o_last_error()
    assert status(one(oo=60) + one() + one(h=2, w=2, oo=107)) == 1 and b'destinations overlap' in lib.t2o_last_error()
    # no destination on a plane of the call, its own or another job's
    assert status(one(mo=40), plane=o) == 1 and b'overlaps a plane' in lib.t2o_last_error()
    assert status(one(mo=100) + one(oo=60, mo=200), plane=o) == 1 and b'overlaps a plane' in lib.t2o_last_error()
    # photo and out address the same memory: only a job's own photo at exactly its own address
    assert status(one(oo=47), out=p) == 1 and b'overlaps a photo' in lib.t2o_last_error()
    assert status(one(po=1, oo=0), out=p) == 1 and b'overlaps a photo' in lib.t2o_last_error()
    assert status(one(po=100, oo=200) + one(po=0, oo=120), out=p) == 1 and b'overlaps a photo' in lib.t2o_last_error()
    assert status(one(po=1, oo=47), out=p + 1) == 1 and b'overlaps a photo' in lib.t2o_last_error()         # two views of one buffer
    assert status(one() + one(po=0, mo=16, oo=100), out=p) == 1 and b'overlaps a photo' in lib.t2o_last_error()   # in place on a photo another job reads
    # the workspace
    need = lib.t2o_fill_workspace_bytes(T.fill_jobs(one()), 1)
    assert need == 3 * 128 + 112                                      # C_1 (2 x 2), C_2 and F_2 (1 x 1), and room to round the base up
    assert status(one(), work=None) == 3 and b'workspace' in lib.t2o_last_error()
    assert status(one(), work_bytes=need - 1) == 3 and b'workspace' in lib.t2o_last_error()
    assert status(one(), work=wp + 8) == 3 and b'16-byte aligned' in lib.t2o_last_error()
    assert status(one(h=0), work=None) == 1                          # the values are judged first
    assert status(one(oo=47), out=p, work=None) == 1                 # and so are the overlaps
    # the Python surface turns them into exceptions before anything else
    with pytest.raises(ValueError, match='GPU'):
        T.fill_u8(buf, buf, one())
    with pytest.raises(ValueError, match='is \\(photo_offset'):
        T.fill_jobs([(0, 0, 0, 4)])
    with pytest.raises(ValueError, match='not an integer'):
        T.fill_jobs([(0, 0, 0, 4.5, 4)])
    with pytest.raises(ValueError, match='does not fit'):
        T.fill_jobs([(0, 0, 0, 4, 1 << 31)])
    assert (T.FILL_MAX_JOBS, T.FILL_LAUNCHES) == (4, 3) and T.FILL_LAUNCHES <= 4
    assert lib.t2o_abi_version() == 4


def test_workspace_bytes_and_the_struct(emul):
    import t2onet_amd.functional as T
    lib = _library()

    def need(jobs, J=None):
        return lib.t2o_fill_workspace_bytes(T.fill_jobs(jobs), len(jobs) if J is None else J)
    for h, w in ((1, 1), (37, 53), (300, 521), (4000, 6000)):
        assert need([(0, 0, 0, h, w)]) == emul.emul_fill_ws_bytes(h, w) + 112
    assert need([(0, 0, 0, 5, 7), (9, 99, 999, 3, 9)]) == emul.emul_fill_ws_bytes(5, 7) + emul.emul_fill_ws_bytes(3, 9) + 112
    assert need([(0, 0, 0, 1, (1 << 31) // 3)]) == 0 and need([(0, 0, 0, 1, (1 << 31) // 3 - 300000000)]) == 0   # 3 h w, a side above 65535 tiles
    assert need([(0, 0, 0, 4194240, 170)]) > 0 and need([(0, 0, 0, 4194241, 170)]) == 0
    for bad in ([(0, 0, 0, 0, 7)], [(0, 0, 0, 5, -7)], [(-1, 0, 0, 5, 7)], [(0, -1, 0, 5, 7)], [(0, 0, -1, 5, 7)], [(0, 0, 0, 1 << 15, 1 << 15)],
                [(0, 0, 0, 5, 7)] * 5):
        assert need(bad) == 0, bad
    assert need([(0, 0, 0, 5, 7)], J=0) == 0 and lib.t2o_fill_workspace_bytes(None, 1) == 0
    # the ctypes struct and the constants against the header
    with open(os.path.join(ROOT, 'include', 't2onet_hip.h')) as f:
        header = f.read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} t2o_fill_job_t;', header).group(1), flags=re.S)
    fields = [(t.strip(), n.strip()) for t, names in re.findall(r'(long long|int)\s+([^;]+);', body) for n in names.split(',')]
    kinds = {'long long': ctypes.c_longlong, 'int': ctypes.c_int}
    assert [(n, kinds[t]) for t, n in fields] == list(T.FillJob._fields_)
    assert ctypes.sizeof(T.FillJob) == 32 and T.FillJob.h.offset == 24 and T.FillJob.w.offset == 28
    assert '#define T2O_FILL_MAX_JOBS %d\n' % T.FILL_MAX_JOBS in header and '#define T2O_FILL_LAUNCHES %d\n' % T.FILL_LAUNCHES in header
    table = T.fill_jobs([(5, 6, 7, 8, 9), (1 << 40, 2, 3, 4, 5)])
    assert [(c.photo_offset, c.plane_offset, c.out_offset, c.h, c.w) for c in table] == [(5, 6, 7, 8, 9), (1 << 40, 2, 3, 4, 5)]


# ---------------------------------------------------------------- the Python surface, no device
def test_edit_image_refuses_a_fill_without_a_plane_before_any_device_use():
    from t2onet_amd.edit import checked_fill, edit_image, select_plan
    img, x = np.zeros((6, 8, 3), np.uint8), torch.zeros(1, 4, dtype=torch.long)
    m = np.zeros((6, 8), np.uint8)
    wand = [('wand', 0.5, 0.5)]
    # model = None would raise something else than ValueError
    for kw, why in [(dict(fill=4), 'names no plane'), (dict(fill=4, masks={'all': m}), 'names no plane'), (dict(fill='all', select={4: wand}), 'names no plane'),
                    (dict(fill=4, select={5: wand}, masks={0: m}), r"names no plane \(masks: 0; select: 5\)"),
                    (dict(fill=8, select={4: wand}), 'neither'), (dict(fill='inpaint', select={4: wand}), 'neither'), (dict(fill=True, masks={4: m}), 'neither'),
                    (dict(fill=4, select={4: [('wand', 2, 0)]}), 'the seed lies'), (dict(fill=4, select={4: wand}, feather={4: 65}), 'sigma must lie')]:
        with pytest.raises(ValueError, match=why):
            edit_image(None, img, x, **kw)
    with pytest.raises(AttributeError):                               # everything was in order: the model is asked for its device
        edit_image(None, img, x, fill=4, select={4: wand})
    assert checked_fill(None, None, None) is None and checked_fill(4, {4: m}, None) == 4 and checked_fill('all', None, {'all': wand}) == 'all'
    # the fill plane counts towards the four planes of a call; select_plan tells which plane a key got
    keys = {}
    plan = select_plan({4: wand, 0: [('lum', 0, 0.5)]}, {5: m}, None, 6, 8, keys=keys)
    assert len(plan[1]) == 3 and sorted(keys) == [0, 4, 5] and plan[2][4] == keys[4] and len(set(keys.values())) == 3
    with pytest.raises(ValueError, match='5 distinct planes'):
        edit_image(None, img, x, fill=4, select={k: [('wand', 0.25 * k, 0.5)] for k in range(5)})


def test_fill_option_and_the_record(tmp_path):
    from t2onet_amd import apply_cli, edit_cli
    assert edit_cli.parse_fill_arg(None, {}) is None and edit_cli.parse_fill_arg('inpaint', {'inpaint': 'wand:0,0'}) == 'inpaint'
    assert edit_cli.parse_fill_arg('all', {'all': 'm.png'}) == 'all'
    for name, named in (('inpaint', {}), ('inpaint', {'tone': 'wand:0,0'}), ('sky', {'inpaint': 'm.png'})):
        with pytest.raises(ValueError, match='--fill %s: no --mask or --select was given under' % name):
            edit_cli.parse_fill_arg(name, named)
    # main refuses before the photo is decoded or a model made: the files do not exist
    with pytest.raises(ValueError, match='--fill inpaint: no --mask or --select'):
        edit_cli.main(['--img', 'none.jpg', '--request', 'r', '--checkpoint', 'none.pth', '--select', 'tone=wand:0.5,0.5', '--fill'])
    with pytest.raises(ValueError, match='--fill tone: no --mask or --select'):
        edit_cli.main(['--img', 'none.jpg', '--request', 'r', '--checkpoint', 'none.pth', '--fill', 'tone'])
    # the record
    img = np.zeros((4, 5, 3), np.uint8)
    info = edit_cli.write_outputs(str(tmp_path), 'a.png', 'remove it', img, img[None], [], torch.zeros(0, 24), select={'inpaint': 'wand:0.5,0.5'}, fill='inpaint')
    assert info['fill'] == 'inpaint' and info['operations'] == []
    assert 'fill' not in edit_cli.write_outputs(str(tmp_path), 'b.png', 'r', img, img[None], [], torch.zeros(0, 24))
    # apply_cli: the fill travels with a selection, never with a painted mask, and an inpaint OPERATION stays refused
    ops = [['brightness', [0.5]], ['tone', [0.5] * 8]]
    rec = {'operations': ops, 'select': {'inpaint': 'wand:0.5,0.4:0.1', 'tone': 'lum:0:0.5'}, 'feather': {'inpaint': 2.0}, 'refine': {'inpaint': [6, 0.02]},
           'fill': 'inpaint'}
    assert apply_cli.parse_fill([rec]) == 'inpaint' and apply_cli.parse_fill([dict(rec, fill=None)]) is None
    assert apply_cli.parse_fill([{'operations': ops}]) is None
    select, feather = apply_cli.parse_local([rec])
    planes, mask_of, no = apply_cli.local_planes([0, 5], select, feather, apply_cli.parse_refine([rec]), 'inpaint')
    assert mask_of == [-1, 0] and no == 1 and planes[1] == ((('wand', 0.5, 0.4, 0.1),), 2.0, (6, 0.02)) and planes[0][1:] == (0.0, None)
    assert apply_cli.local_planes([0, 5], select, feather, apply_cli.parse_refine([rec])) == (planes[:1], [-1, 0])      # without fill: what it was
    assert apply_cli.local_planes([0], select, feather, None, 'inpaint') == ([((('wand', 0.5, 0.4, 0.1),), 2.0)], [-1], 0)
    with pytest.raises(ValueError, match=r"'fill': 'inpaint' names the painted mask 'obj.png'"):
        apply_cli.parse_fill([{'operations': ops, 'masks': {'inpaint': 'obj.png'}, 'fill': 'inpaint'}])
    with pytest.raises(ValueError, match=r"'fill': 'inpaint' names the painted mask 'obj.png'"):
        apply_cli.parse_fill([{'operations': ops, 'masks': {'inpaint': 'obj.png'}, 'select': {'tone': 'lum:0:1'}, 'fill': 'inpaint'}])
    with pytest.raises(ValueError, match=r"'fill': 'inpaint' names no entry of 'select' \(given: tone\)"):
        apply_cli.parse_fill([{'operations': ops, 'select': {'tone': 'lum:0:1'}, 'fill': 'inpaint'}])
    with pytest.raises(ValueError, match="names no entry of 'select' \\(given: none\\)"):
        apply_cli.parse_fill([{'operations': ops, 'fill': 'inpaint'}])
    with pytest.raises(ValueError, match='is the name a selection goes by'):
        apply_cli.parse_fill([dict(rec, fill=4)])
    with pytest.raises(ValueError, match='5 distinct selections'):
        apply_cli.local_planes([0, 1, 2, 3], {n: 'lum:0:0.%d' % (k + 1) for k, n in enumerate(['brightness', 'contrast', 'saturation', 'color', 'inpaint'])},
                               {}, None, 'inpaint')
    with pytest.raises(ValueError, match='inpaint is not supported by the replay'):
        apply_cli.parse_record([dict(rec, operations=[['inpaint', []]])])
    # main refuses a painted fill before any photo is decoded
    path = str(tmp_path / 'painted.json')
    with open(path, 'w') as f:
        import json
        json.dump([{'operations': ops, 'masks': {'inpaint': 'obj.png'}, 'fill': 'inpaint'}], f)
    with pytest.raises(ValueError, match='names the painted mask'):
        apply_cli.main(['--record', path, '--img', 'none.jpg'])


def test_the_documents_say_what_the_stage_is():
    with open(os.path.join(ROOT, 'README.md')) as f:
        readme = f.read()
    with open(os.path.join(ROOT, 'DESIGN.md')) as f:
        design = f.read()
    assert '--fill' in readme and 'fill_u8' in design
    for text in (readme, design):
        assert 'smooth fill' in text and 'no texture' in text and 'not the reference' in text
