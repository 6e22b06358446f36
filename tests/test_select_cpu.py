"""No-GPU checks of the selection kernel (t2o_select.hip): the kernel's lane program, compiled for the host from the shared
header (tests/host_emul/emul_select.cpp) and run for every workgroup, against the int64 oracle byte for byte, guard bytes
included; the three colour measures over all 2^24 colours; the properties of the definition; the status codes of the
entry point; --select, the record keys, edit_image's checks and apply_cli's refusal."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import select_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('t2o_select_math.h', 't2o_replay_math.h', 't2o_pixel_math.h', 't2o_image_math.h')


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
    import t2onet_amd.functional as T
    lib = _compile('emul_select')
    assert lib.emul_select_tile_px() == SC.TILE == 4096
    assert lib.emul_select_args_bytes() <= 2048                      # the job table travels in the kernel arguments
    assert lib.emul_select_job_bytes() == ctypes.sizeof(T.SelectJob)
    return lib


def run_emul(lib, src, out, jobs):
    """The lane program over every workgroup of the call's grid; src / out: numpy byte buffers."""
    import t2onet_amd.functional as T
    rc = lib.emul_select_u8(src.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), T.select_jobs(jobs), len(jobs))
    assert rc == 0
    return out


def select_one(lib, img, terms, plane=None):
    """One selection of one picture; plane: the bytes a ('plane', invert, 0) term reads -- its offset is moved behind the photo."""
    h, w = img.shape[:2]
    src = np.concatenate([img.reshape(-1), np.zeros(0, np.uint8) if plane is None else plane.reshape(-1)])
    terms = [(t[0], t[1], 3 * h * w) if t[0] == 'plane' else t for t in terms]
    return run_emul(lib, src, np.zeros(h * w, np.uint8), [(0, 0, h, w, terms)]).reshape(h, w)


def _library():
    from t2onet_amd import build, _lib
    if os.path.exists(build.hipcc_path()):
        build.build()
    elif not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libt2onet_hip.so is absent and there is no hipcc to build it')
    return _lib.load()


# ---------------------------------------------------------------- the lane program against the oracle
N_CALLS = 41


def test_cases_cover_what_they_should():
    calls = SC.calls()
    assert len(calls) == N_CALLS
    jobs = [(j, n) for _, c in calls for j, n in zip(c.jobs, c.names)]
    assert {j[0] % 4 for j, _ in jobs} == {j[1] % 4 for j, _ in jobs} == {0, 1, 2, 3}
    assert {(j[0] % 4, j[1] % 4) for j, _ in jobs if j[2:4] in ((5, 7), (37, 53))} == {(a, b) for a in range(4) for b in range(4)}
    assert SC.SIZES == [(1, 1), (1, 5), (3, 1), (5, 7), (37, 53), (64, 64), (1, 4097), (4097, 1)]
    assert {(j[2], j[3], n) for j, n in jobs} >= set(SC.specs()) and len(SC.specs()) == len(SC.SIZES) * len(SC.NAMES)
    terms = [t for j, _ in jobs for t in j[4]]
    assert {(t[0], t[1]) for t in terms} == {(k, i) for k in SC.KINDS for i in (0, 1)}            # every kind, plain and inverted
    assert any(t[0] == 'hue' and t[3] < t[2] for t in terms)                                        # an arc that wraps
    assert any(t[0] in ('lum', 'sat', 'hue') and t[4] == 0 for t in terms)                          # soft = 0
    assert any(len(j[4]) == 4 for j, _ in jobs)                                                     # a four-term product
    assert any(t[0] == 'linear' and (t[4] - t[2]) ** 2 + (t[5] - t[3]) ** 2 >= 1 << 24 for t in terms)      # the 64-bit division
    shared = dict(calls)['shared_photo']
    assert len(shared.jobs) == 4 and len({j[0] for j in shared.jobs}) == 1 and len({j[2:4] for j in shared.jobs}) == 4
    for h, w in [(37, 53), (64, 64)]:
        rgb = SC.picture(h, w, 3).reshape(-1, 3).astype(np.int64)
        assert (rgb.max(1) == 0).any() and ((rgb.max(1) == rgb.min(1)) & (rgb.max(1) > 0)).any()   # black pixels, grey pixels


def test_colour_and_position_planes_hold_zero_full_and_between():
    """A condition on the INPUTS: on sizes from 37 x 53 on every one-term colour or position plane of the case list holds 0,
    255 and a value between -- a hard step (soft = 0) holds 0 and 255 and, by its definition, nothing between."""
    seen = 0
    for name, call in SC.calls():
        for (so, oo, h, w, terms), sel in zip(call.jobs, call.names):
            if h * w < 37 * 53 or min(h, w) < 37 or len(terms) != 1 or terms[0][0] == 'plane':
                continue
            plane = call.want[oo:oo + h * w]
            step = terms[0][0] in ('lum', 'sat', 'hue') and terms[0][4] == 0
            assert (plane == 0).any() and (plane == 255).any(), (name, sel, h, w)
            assert ((plane > 0) & (plane < 255)).any() != step, (name, sel, h, w)
            seen += 1
    assert seen >= 2 * (len(SC.NAMES) - 5)                           # both sizes, every selection but the multi-term and plane ones


@pytest.mark.parametrize('n', range(N_CALLS))
def test_lane_program_equals_the_oracle(emul, n):
    name, call = SC.calls()[n]
    got = run_emul(emul, call.src.copy(), call.out.copy(), call.jobs)
    np.testing.assert_array_equal(got, call.want, err_msg='%s %s' % (name, call.names))       # planes AND the bytes around them


def test_the_ramp_divides_exactly_for_every_softness(emul):
    """The kernel's ramp multiplies by a reciprocal instead of dividing: every softness a term may carry (0..768) at every
    distance a colour measure can have (0..1536) against the definition's floor division."""
    dist = np.arange(1537, dtype=np.int64)
    got = np.zeros(1537, np.int32)
    for soft in range(769):
        emul.emul_select_ramp(soft, 1537, got.ctypes.data_as(ctypes.c_void_p))
        assert np.array_equal(got, SC.ramp(dist, soft)), soft


def test_all_colours(emul):
    """L, S and H over all 2^24 colours as one 4096 x 4096 picture through the emulation: an inverted range [0, 0] of
    softness 255 gives the measure itself (255 - ramp(v, 255) = v for v < 255, and 255 at 255); six hue arcs [c, c] of
    softness 255 around the sector borders c give 255 - distance within 254 steps; with three hard arcs that tell c - 1
    from c + 1 they determine H."""
    v = np.arange(256, dtype=np.uint8)
    img = np.empty((4096, 4096, 3), np.uint8)
    img.reshape(256, 256, 256, 3)[..., 0] = v[:, None, None]
    img.reshape(256, 256, 256, 3)[..., 1] = v[None, :, None]
    img.reshape(256, 256, 256, 3)[..., 2] = v[None, None, :]
    hue_terms = [('hue', 0, c, c, 255) for c in range(0, 1536, 256)] + [('hue', 0, c + 1, c + 256, 0) for c in range(0, 1536, 512)]
    terms = [('lum', 1, 0, 0, 255), ('sat', 1, 0, 0, 255)] + hue_terms
    n = 4096 * 4096
    got = np.zeros(len(terms) * n, np.uint8)
    src = img.reshape(-1)
    for a in range(0, len(terms), 4):
        run_emul(emul, src, got, [(0, (a + k) * n, 4096, 4096, [t]) for k, t in enumerate(terms[a:a + 4])])
    got = got.reshape(len(terms), n)
    rows = 256                                                       # the oracle in slabs: int64 temporaries stay small
    for y in range(0, 4096, rows):
        part = img[y:y + rows].reshape(-1, 3)
        L, S, H = SC.measures(part)
        assert L.min() >= 0 and L.max() <= 255 and S.min() >= 0 and S.max() <= 255 and H.min() >= -1 and H.max() <= 1535
        sl = slice(y * 4096, (y + rows) * 4096)
        assert np.array_equal(got[0, sl], L) and np.array_equal(got[1, sl], S)
        for k, term in enumerate(hue_terms):
            want = SC.term_weight(term, part.reshape(-1, 1, 3)).reshape(-1)
            assert np.array_equal(got[2 + k, sl], want), term
    # the hue planes determine H: every hue has its own weights, none of them the zeros of an undefined hue
    hues = np.arange(1536, dtype=np.int64)
    rows = np.stack([SC.hue_weight(term, hues) for term in hue_terms], 1)
    assert len({tuple(r) for r in rows.tolist()}) == 1536 and rows.max(1).min() > 0
    primaries = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255], [255, 0, 1]])
    assert SC.measures(primaries)[2].tolist() == [0, 256, 512, 768, 1024, 1280, 1535]


def test_inverting_a_one_term_selection_gives_the_complement(emul):
    img = SC.picture(37, 53, 5)
    plane = np.random.default_rng(6).integers(0, 256, (37, 53), dtype=np.uint8)
    for name, terms in SC.selections(37, 53, 0):
        if len(terms) == 1:
            flipped = [(terms[0][0], 1 - terms[0][1]) + tuple(terms[0][2:])]
            a, b = select_one(emul, img, terms, plane), select_one(emul, img, flipped, plane)
            assert np.array_equal(a.astype(np.int64) + b, np.full((37, 53), 255)), name


def test_a_full_plane_term_changes_nothing_and_an_empty_one_clears(emul):
    img = SC.picture(37, 53, 7)
    full, empty = np.full((37, 53), 255, np.uint8), np.zeros((37, 53), np.uint8)
    for name, terms in SC.selections(37, 53, 0):
        if len(terms) <= 3 and all(t[0] != 'plane' for t in terms):
            alone = select_one(emul, img, terms)
            assert np.array_equal(select_one(emul, img, terms + [('plane', 0, 0)], full), alone), name
            assert np.array_equal(select_one(emul, img, [('plane', 0, 0)] + terms, full), alone), name
            assert not select_one(emul, img, terms + [('plane', 0, 0)], empty).any(), name


def test_other_bytes_around_the_sources_give_the_same_output(emul):
    """The host loads read only inside the photo and the plane term; whatever surrounds them, same bytes."""
    h, w = 37, 53
    img, plane = SC.picture(h, w, 8), np.random.default_rng(9).integers(0, 256, h * w, dtype=np.uint8)
    outs = []
    for noise in (0x00, 0xFF):
        for pad in range(4):
            src = np.full(pad + 3 * h * w + 3 + h * w + 5, noise, np.uint8)
            src[pad:pad + 3 * h * w] = img.reshape(-1)
            po = pad + 3 * h * w + 3
            src[po:po + h * w] = plane
            terms = dict(SC.selections(h, w, po))['four'][:3] + [('plane', 1, po)]
            out = np.full(h * w + 9, SC.GUARD, np.uint8)
            run_emul(emul, src, out, [(pad, 3, h, w, terms)])
            assert (out[:3] == SC.GUARD).all() and (out[3 + h * w:] == SC.GUARD).all()
            assert np.array_equal(out[3:3 + h * w].reshape(h, w), SC.selection(terms, img, src))
            outs.append(out)
    assert all(np.array_equal(o, outs[0]) for o in outs)


def test_programs_are_clean_under_the_sanitizers(tmp_path):
    """Host code only: a stand-alone program over the lane program, built with -fsanitize=address,undefined, every buffer of
    exactly the needed size.  It runs as its own process with the sanitizers' runtimes linked in statically; nothing of
    it is loaded into this one."""
    exe = str(tmp_path / 'sanitize_select')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan',
                           '-o', exe, os.path.join(ROOT, 'tests', 'host_emul', 'sanitize_select.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'select programs: clean', r.stdout + r.stderr


# ---------------------------------------------------------------- user units
def test_user_units_round_as_specified():
    from t2onet_amd.edit import select_terms
    user = [('lum', 0.5, 1.0, 0.125), ('!sat', 0.0, 96 / 255.0, 48 / 255.0), ('hue', 320, 40, 30), ('!linear', 0, 0, 1, 1)]
    assert select_terms(user, 37, 53) == SC.round_units(user, 37, 53) == [
        ('lum', 0, 128, 255, 32), ('sat', 1, 0, 96, 48), ('hue', 0, 1365, 171, 128), ('linear', 1, 0, 0, 52, 36)]
    user = [('radial', 0.5, 0.5, 0.1, 0.6), ('hue', 359.95, 0, 180), ('lum', 0.25, 0.75), ('linear', -1, 2, 2, -1)]
    for h, w in [(37, 53), (48, 80), (3000, 4001), (65535, 65535)]:
        assert select_terms(user, h, w) == SC.round_units(user, h, w)
    assert select_terms(user, 48, 80) == [('radial', 0, 40, 24, 5, 29), ('hue', 0, 0, 0, 768), ('lum', 0, 64, 191, 0), ('linear', 0, -79, 94, 158, -47)]
    assert select_terms([('lum', 0.5 / 255, 1.5 / 255)], 4, 4) == [('lum', 0, 1, 2, 0)]              # halves round up


# ---------------------------------------------------------------- status codes, no device
def test_status_codes_before_any_launch():
    import t2onet_amd.functional as T
    lib = _library()
    buf = torch.zeros(4096, dtype=torch.uint8)
    p, o = buf.data_ptr(), torch.zeros(4096, dtype=torch.uint8).data_ptr()
    lum = ('lum', 0, 10, 20, 5)

    def status(jobs, src=p, out=o, J=None, table=True):
        return lib.t2o_select_u8(src, out, T.select_jobs(jobs) if table else None, len(jobs) if J is None else J, None)

    def one(*terms, h=4, w=4, so=0, oo=0):
        return [(so, oo, h, w, list(terms))]
    assert status(one(lum), src=None) == 1 and b'null' in lib.t2o_last_error()
    assert status(one(lum), out=None) == 1 and status(one(lum), table=False) == 1
    assert status(one(lum), J=0) == 1 and b'1 <= J <= 4' in lib.t2o_last_error()
    assert status(one(lum) * 5) == 1 and status(one(lum), J=-1) == 1
    assert status(one()) == 1 and b'n_terms' in lib.t2o_last_error()
    assert status(one(*[lum] * 5)) == 1 and b'n_terms' in lib.t2o_last_error()
    assert status(one(lum, h=0)) == 1 and b'positive' in lib.t2o_last_error()
    assert status(one(lum, w=-1)) == 1
    assert status(one(lum, h=1 << 16, w=1 << 15)) == 1 and b'2^31' in lib.t2o_last_error()
    for pos in (('linear', 0, 0, 0, 5, 5), ('radial', 0, 2, 2, 0, 5)):
        assert status(one(pos, h=1, w=65536)) == 1 and b'65535' in lib.t2o_last_error()
        assert status(one(pos, h=65536, w=1)) == 1 and b'65535' in lib.t2o_last_error()
    assert status(one(lum, so=-1)) == 1 and b'offset' in lib.t2o_last_error()
    assert status(one(lum, oo=-1)) == 1 and b'offset' in lib.t2o_last_error()
    assert status(one(('plane', 0, -1))) == 1 and b'offset' in lib.t2o_last_error()
    assert status(one((6, 0, 0, 0, 0))) == 1 and b'kind' in lib.t2o_last_error()
    assert status(one((-1, 0, 0, 0, 0))) == 1 and b'kind' in lib.t2o_last_error()
    assert status(one(('lum', 2, 10, 20, 5))) == 1 and b'invert' in lib.t2o_last_error()
    for kind in ('lum', 'sat'):
        for bad in ((20, 10, 5), (-1, 10, 5), (0, 256, 5), (0, 10, 256), (0, 10, -1)):
            assert status(one((kind, 0) + bad)) == 1 and b'lum / sat' in lib.t2o_last_error(), bad
    for bad in ((1536, 0, 5), (0, 1536, 5), (-1, 0, 5), (0, 0, 769), (0, 0, -1)):
        assert status(one(('hue', 0) + bad)) == 1 and b'hue' in lib.t2o_last_error(), bad
    assert status(one(('linear', 0, 3, 4, 3, 4))) == 1 and b'equal' in lib.t2o_last_error()
    assert status(one(('linear', 0, 131071, 0, 0, 0))) == 1 and b'131070' in lib.t2o_last_error()
    assert status(one(('radial', 0, 0, -131071, 0, 1))) == 1 and b'131070' in lib.t2o_last_error()
    for bad in ((5, 5), (6, 5), (-1, 5)):
        assert status(one(('radial', 0, 2, 2) + bad)) == 1 and b'RI < RO' in lib.t2o_last_error(), bad
    assert status(one(('radial', 0, 2, 2, 0, 131071))) == 1
    # one writer per byte
    assert status(one(lum) + one(lum, oo=15)) == 1 and b'destinations overlap' in lib.t2o_last_error()
    assert status(one(lum, oo=20) + one(lum) + one(lum, h=2, w=2, oo=35)) == 1 and b'destinations overlap' in lib.t2o_last_error()
    # src and out address the same memory: no destination on anything the call reads
    assert status(one(lum, oo=47), out=p) == 1 and b'overlaps a photo' in lib.t2o_last_error()
    assert status(one(lum, so=100, oo=0) + one(lum, so=0, oo=300), out=p) == 1 and b'overlaps a photo' in lib.t2o_last_error()
    assert status(one(lum, ('plane', 0, 100), oo=115), out=p) == 1 and b'overlaps a plane term' in lib.t2o_last_error()
    assert status(one(lum, ('plane', 0, 100), oo=84), out=p + 1) == 1 and b'overlaps a plane term' in lib.t2o_last_error()    # two views of one buffer
    # the Python surface turns them into exceptions before anything else
    with pytest.raises(ValueError, match='GPU'):
        T.select_u8(buf, one(lum))
    with pytest.raises(ValueError, match='not a term kind'):
        T.select_jobs(one(('luma', 0, 1, 2, 3)))
    with pytest.raises(ValueError, match='wrong number of values'):
        T.select_jobs(one(('linear', 0, 1, 2, 3)))
    assert (T.SELECT_MAX_JOBS, T.SELECT_MAX_TERMS) == (4, 4) and T.SELECT_KINDS == SC.KINDS
    assert lib.t2o_abi_version() == 4


# ---------------------------------------------------------------- the Python surface
def test_select_option_parsing(tmp_path):
    from PIL import Image
    from t2onet_amd import edit_cli
    P = edit_cli.parse_select_terms
    assert P('lum:0.5:1') == [('lum', 0.5, 1.0)] and P('!sat:0:0.4:0.2') == [('!sat', 0.0, 0.4, 0.2)]
    assert P('hue:320:40:30+!linear:0,0:1,1+radial:0.5,0.5:0.1:0.6') == [
        ('hue', 320.0, 40.0, 30.0), ('!linear', 0.0, 0.0, 1.0, 1.0), ('radial', 0.5, 0.5, 0.1, 0.6)]
    A = edit_cli.parse_select_args
    assert A(None) == {} and A([]) == {}
    assert A(['lum:0.5:1', 'tone=hue:200:260:20+!sat:0:0.2']) == {'all': 'lum:0.5:1', 'tone': 'hue:200:260:20+!sat:0:0.2'}
    assert edit_cli.select_argument(A(['lum:0.5:1', 'tone=hue:200:260'])) == {'all': [('lum', 0.5, 1.0)], 5: [('hue', 200.0, 260.0)]}
    assert edit_cli.select_argument({}) is None
    for bad, why in [('luma:0:1', 'not a term'), ('!!lum:0:1', 'not a term'), ('lum:0', 'LO:HI'), ('lum:0:1:0:0', 'LO:HI'),
                     ('lum:a:1', 'not a number'), ('linear:0,0:1', 'does not have the numbers'), ('linear:0,0', 'X0,Y0:X1,Y1'),
                     ('radial:0.5,0.5:0.1', 'CX,CY:RIN:ROUT'), ('radial:0.5:0.1:0.2', 'does not have the numbers'),
                     ('lum:0.6:0.5', 'lo <= hi'), ('sat:0:1.5', 'lo <= hi'), ('lum:0:1:2', 'softness'), ('hue:0:360', r'\[0, 360\)'),
                     ('hue:0:90:181', r'\[0, 180\]'), ('linear:0,0:0,0', 'end points are equal'), ('linear:0,0:3,0', r'\[-1, 2\]'),
                     ('radial:0.5,0.5:0.3:0.3', 'rin < rout'), ('radial:0.5,0.5:0:2.5', 'rin < rout'),
                     ('lum:0:1+lum:0:1+lum:0:1+lum:0:1+lum:0:1', '1 to 4 terms'), ('tone=', 'no term'), ('glow=lum:0:1', 'not an operator name')]:
        with pytest.raises(ValueError, match=why) as e:
            A([bad])
        assert bad in str(e.value)                                   # errors name the spec
    # --feather may name a --select as well as a --mask
    planes = dict({'color': 'm.png'}, **A(['tone=lum:0.5:1']))
    assert edit_cli.parse_feather_args(['tone=3', 'color=2'], planes) == {'tone': 3.0, 'color': 2.0}
    assert edit_cli.feather_argument({'tone': 3.0}, planes) == {5: 3.0}
    # the command refuses before it needs a model or a GPU
    Image.fromarray(np.zeros((20, 30, 3), np.uint8)).save(str(tmp_path / 'photo.png'))
    Image.fromarray(np.zeros((1, 30, 3), np.uint8)).save(str(tmp_path / 'line.png'))
    common = ['--request', 'x', '--checkpoint', 'none.pth', '--img']
    with pytest.raises(ValueError, match='not a term'):
        edit_cli.main(common + [str(tmp_path / 'photo.png'), '--select', 'value:0:1'])
    with pytest.raises(ValueError, match="no --mask was given under 'color'"):
        edit_cli.main(common + [str(tmp_path / 'photo.png'), '--select', 'tone=lum:0:1', '--feather', 'color=3'])
    with pytest.raises(ValueError, match='fall on one pixel'):
        edit_cli.main(common + [str(tmp_path / 'line.png'), '--select', 'linear:0,0:0,1'])
    with pytest.raises(ValueError, match='5 distinct planes'):
        edit_cli.main(common + [str(tmp_path / 'photo.png')] + [a for k, n in enumerate(['all', 'tone', 'color', 'white', 'contrast'])
                                                                  for a in ('--select', ('' if n == 'all' else n + '=') + 'lum:0:0.%d' % (k + 1))])
    # the record gains 'select' only when it was given; the positional arguments and the older keywords are unchanged
    steps, par = np.zeros((1, 20, 30, 3), np.uint8), torch.zeros(1, 24)
    rec = edit_cli.write_outputs(str(tmp_path / 'a'), str(tmp_path / 'photo.png'), 'x', steps[0], steps, [0], par,
                                 feather={'all': 3.0}, select={'all': 'lum:0.5:1'})
    assert rec['select'] == {'all': 'lum:0.5:1'} and rec['feather'] == {'all': 3.0} and 'masks' not in rec
    with open(str(tmp_path / 'a' / 'photo' / 'photo.json')) as f:
        assert json.load(f) == [json.loads(json.dumps(rec))]
    rec = edit_cli.write_outputs(str(tmp_path / 'b'), str(tmp_path / 'photo.png'), 'x', steps[0], steps, [0], par, False, {'all': 'm.png'})
    assert 'select' not in rec and rec['masks'] == {'all': 'm.png'}


def test_edit_image_checks_select_before_any_device_use():
    from t2onet_amd.edit import edit_image, select_plan
    img = np.zeros((6, 8, 3), np.uint8)
    m1, m2 = np.zeros((6, 8), np.uint8), np.full((6, 8), 255, np.uint8)
    x = torch.zeros(1, 4, dtype=torch.long)
    lum, sat = [('lum', 0.5, 1.0)], [('!sat', 0.0, 0.5, 0.1)]
    # model = None: any use of the model or a device would raise something else than ValueError
    for bad, why in [({}, 'select is'), ([lum], 'select is'), ({'all': []}, '1 to 4 terms'), ({'all': lum * 5}, '1 to 4 terms'),
                     ({9: lum}, 'neither'), ({'tone': lum}, 'neither'), ({'all': [('value', 0, 1)]}, 'the kind is one of'),
                     ({'all': [('lum', 0.5)]}, 'takes lo, hi'), ({'all': [('lum', 'a', 1)]}, 'not a number'),
                     ({'all': [('lum', float('nan'), 1)]}, 'not finite'), ({'all': [('lum', 0.6, 0.5)]}, 'lo <= hi'),
                     ({'all': [('hue', 0, 400)]}, r'\[0, 360\)'), ({'all': [('linear', 0, 0, 0.01, 0.01)]}, 'fall on one pixel'),
                     ({'all': [('radial', 0.5, 0.5, 0.01, 0.02)]}, 'radii fall together'), ({'all': ['lum']}, 'is not'),
                     ({k: [('lum', 0.0, 0.1 * (k + 1))] for k in range(5)}, '5 distinct planes')]:
        with pytest.raises(ValueError, match=why):
            edit_image(None, img, x, select=bad)
    with pytest.raises(ValueError, match='painted mask, which counts as one'):
        edit_image(None, img, x, select={'all': lum * 4}, masks={'all': m1})
    with pytest.raises(ValueError, match=r'must be uint8 \(6, 8\)'):
        edit_image(None, img, x, select={'all': lum}, masks={0: np.zeros((6, 9), np.uint8)})
    with pytest.raises(ValueError, match='names no mask'):
        edit_image(None, img, x, select={'all': lum}, feather={0: 3})
    with pytest.raises(ValueError, match='another key feathers the same plane'):
        edit_image(None, img, x, select={'all': lum, 0: lum}, feather={'all': 3, 0: 4})
    with pytest.raises(ValueError, match='sigma must lie'):
        edit_image(None, img, x, select={'all': lum}, feather=65)
    with pytest.raises(ValueError, match='5 distinct planes'):
        edit_image(None, img, x, select={'all': lum}, masks={k: np.zeros((6, 8), np.uint8) for k in range(4)})
    # what the one launch is made from
    painted, specs, by_op, sigma_of = select_plan({'all': lum, 0: sat, 1: lum}, {0: m1, 2: m2, 3: m2}, {'all': 2, 2: 3, 1: 2.0}, 6, 8)
    assert [id(p) for p in painted] == [id(m1), id(m2)] or [p.tolist() for p in painted] == [m1.tolist(), m2.tolist()]
    assert specs == [((('lum', 0, 128, 255, 0),), None), ((('sat', 1, 0, 128, 26),), 0), ((), 1)]
    assert by_op[0] == 1 and by_op[1] == 0 and by_op[2] == by_op[3] == 2 and by_op[5] == 0
    assert sigma_of == {0: 2.0, 2: 3.0}


def test_apply_cli_reads_the_local_part_of_a_record(tmp_path):
    from t2onet_amd import apply_cli
    ops = [['brightness', [0.5]], ['tone', [0.5] * 8]]
    assert apply_cli.parse_local([{'operations': ops}]) is None
    assert apply_cli.parse_local([{'operations': ops, 'masks': {'all': 'm.png'}}]) is None           # as before: replayed globally
    rec = {'operations': ops, 'select': {'all': 'lum:0.5:1:0.1', 'tone': '!hue:200:260+linear:0,0:0,1'}, 'feather': {'tone': 2.5}}
    assert apply_cli.parse_local([rec]) == (rec['select'], {'tone': 2.5})
    assert apply_cli.parse_record([rec])[1] == [0, 5]                                                  # the global part is read as before
    planes, mask_of = apply_cli.local_planes([0, 5, 0], *apply_cli.parse_local([rec]))
    assert mask_of == [0, 1, 0] and planes == [((('lum', 0.5, 1.0, 0.1),), 0.0), ((('!hue', 200.0, 260.0), ('linear', 0.0, 0.0, 0.0, 1.0)), 2.5)]
    assert apply_cli.local_planes([0], {'tone': 'lum:0:1'}, {}) == ([], [-1])
    # an unnamed sigma is recorded as 'all' and stands for EVERY plane, a named one wins over it: what edit_cli feathered
    from t2onet_amd import edit_cli
    lum, hue = (('lum', 0.5, 1.0, 0.1),), (('!hue', 200.0, 260.0), ('linear', 0.0, 0.0, 0.0, 1.0))
    for given, want in [(['4'], {'all': 4.0, 'tone': 4.0}), (['4', 'tone=2.5'], {'all': 4.0, 'tone': 2.5}),
                        (['4', 'tone=0'], {'all': 4.0, 'tone': 0.0}), (['tone=2.5'], {'all': 0.0, 'tone': 2.5})]:
        sigmas = edit_cli.parse_feather_args(given, rec['select'])
        assert edit_cli.feather_argument(sigmas, rec['select']) == {('all' if n == 'all' else 5): s for n, s in want.items() if n in sigmas or 'all' in sigmas}
        select, feather = apply_cli.parse_local([dict(rec, feather=sigmas)])
        assert feather == sigmas
        assert apply_cli.local_planes([0, 5, 0], select, feather) == ([(lum, want['all']), (hue, want['tone'])], [0, 1, 0]), given
    select, feather = apply_cli.parse_local([{'operations': ops, 'select': {'tone': rec['select']['tone']}, 'feather': {'all': 4}}])
    assert apply_cli.local_planes([0, 5], select, feather) == ([(hue, 4.0)], [-1, 0])                 # no 'all' selection: 'all' still feathers tone
    with pytest.raises(ValueError, match="'select' and 'masks'"):
        apply_cli.parse_local([dict(rec, masks={'all': 'm.png'})])
    with pytest.raises(ValueError, match='not a term'):
        apply_cli.parse_local([dict(rec, select={'all': 'value:0:1'})])
    with pytest.raises(ValueError, match='not an operator name'):
        apply_cli.parse_local([dict(rec, select={'glow': 'lum:0:1'})])
    with pytest.raises(ValueError, match="no --mask was given under 'color'"):
        apply_cli.parse_local([dict(rec, feather={'color': 2})])
    with pytest.raises(ValueError, match='TERM'):
        apply_cli.parse_local([dict(rec, select=['lum:0:1'])])
    # the command refuses before any decode or device use
    path = str(tmp_path / 'both.json')
    with open(path, 'w') as f:
        json.dump([dict(rec, masks={'all': 'm.png'})], f)
    with pytest.raises(ValueError, match="'select' and 'masks'"):
        apply_cli.main(['--record', path, '--img', str(tmp_path / 'absent.png')])
