"""The region kernels (t2o_region.hip), the wand terms of edit_image's `select`, the edit command's --select wand: and the
local apply command on the GPU.  The kernels' bytes must EQUAL the flood-fill oracle's (tests/region_cases.py, shared
with tests/test_region_cpu.py), guard bytes around every destination plane included; everything downstream must equal
what the oracle's planes give when they are handed over as painted masks."""
import json
import re

import numpy as np
import pytest
import torch

from tests import feather_cases as FC
from tests import refine_cases as FR
from tests import region_cases as RC
from tests import select_cases as SC
from tests.test_gpu_select import REQUEST, StubActor, _png, _same, _setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def run_call(dev, call, jobs=None, out=None):
    import t2onet_amd.functional as T
    photo = torch.from_numpy(call.photo).to(dev)
    out = torch.from_numpy(call.out).to(dev) if out is None else out
    assert T.region_u8(photo, call.jobs if jobs is None else jobs, out=out) is out
    assert np.array_equal(photo.cpu().numpy(), call.photo)          # the photo is only read
    return out.cpu().numpy()


def test_bytes_equal_the_oracle(dev):
    """Every case of the list, four jobs of mixed size to a call, every residue of both offsets, the misaligned call and
    the one whose jobs share a photo."""
    for name, call in RC.calls():
        np.testing.assert_array_equal(run_call(dev, call), call.want, err_msg='%s %s %s' % (name, call.names, call.jobs))


def test_two_runs_are_equal_and_out_is_allocated_to_fit(dev):
    import t2onet_amd.functional as T
    for name in ('call_11', 'multi_job'):
        call = dict(RC.calls())[name]
        a, b = run_call(dev, call), run_call(dev, call)
        assert np.array_equal(a, b) and np.array_equal(a, call.want)
    photo = torch.from_numpy(call.photo).to(dev)
    a = T.region_u8(photo, call.jobs)
    assert a.numel() == max(j[1] + j[2] * j[3] for j in call.jobs) and a.dtype == torch.uint8 and a.device == photo.device
    for _, oo, h, w, *_ in call.jobs:                                # (the bytes between the planes of a fresh tensor are nobody's)
        assert np.array_equal(a[oo:oo + h * w].cpu().numpy(), call.want[oo:oo + h * w])


def test_multi_job_call_equals_separate_calls(dev):
    call = dict(RC.calls())['multi_job']
    whole = run_call(dev, call)
    out = torch.from_numpy(call.out).to(dev)
    for job in call.jobs:
        single = run_call(dev, call, [job], out)
    assert np.array_equal(whole, single) and np.array_equal(whole, call.want)


def test_photo_and_out_may_be_one_buffer(dev):
    import t2onet_amd.functional as T
    _, photo, sx, sy, tol, conn = next(c for c in RC.cases() if c[0] == 'comb_c4')
    h, w = photo.shape[:2]
    buf = torch.full((5 + 3 * h * w + 3 + h * w + 2,), RC.GUARD, dtype=torch.uint8, device=dev)
    buf[5:5 + 3 * h * w] = torch.from_numpy(photo.reshape(-1)).to(dev)
    at = 5 + 3 * h * w + 3
    want = buf.cpu().numpy()
    want[at:at + h * w] = RC.want('comb_c4').reshape(-1)
    assert T.region_u8(buf, [(5, at, h, w, sx, sy, tol, conn)], out=buf) is buf
    np.testing.assert_array_equal(buf.cpu().numpy(), want)


def test_call_is_graph_capturable(dev):
    import t2onet_amd.functional as T
    call = dict(RC.calls())['call_5']
    photo, out = torch.from_numpy(call.photo).to(dev), torch.from_numpy(call.out).to(dev)

    def run():
        return T.region_u8(photo, call.jobs, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    out.copy_(torch.from_numpy(call.out).to(dev))
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), call.want)


def _kernels(prof):
    from torch.autograd import DeviceType
    return [(e.key, e.count) for e in prof.key_averages() if e.device_type == DeviceType.CUDA]


def test_three_launches_for_one_job_and_for_four(dev):
    import t2onet_amd.functional as T
    from torch.profiler import profile, ProfilerActivity
    call = dict(RC.calls())['call_5']
    photo, out = torch.from_numpy(call.photo).to(dev), torch.from_numpy(call.out).to(dev)
    for jobs in (call.jobs, call.jobs[:1]):
        T.region_u8(photo, jobs, out=out)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            T.region_u8(photo, jobs, out=out)
            torch.cuda.synchronize()
        ks = _kernels(prof)
        print('region_u8, %d jobs: %s' % (len(jobs), ks))
        assert sorted(re.findall(r'k_region_\w+', k)[0] for k, _ in ks if 'k_region_' in k) == ['k_region_border', 'k_region_resolve', 'k_region_tile'], ks
        assert sum(c for _, c in ks) == T.REGION_LAUNCHES == 3, ks


def test_wrapper_refuses_before_any_launch(dev):
    import t2onet_amd.functional as T
    photo = torch.full((128,), 9, dtype=torch.uint8, device=dev)
    out = torch.zeros(64, dtype=torch.uint8, device=dev)

    def one(po=0, oo=0, h=4, w=4, sx=1, sy=2, tol=32, conn=4):
        return [(po, oo, h, w, sx, sy, tol, conn)]
    for bad in (81, -1):
        with pytest.raises(ValueError, match='reads outside the 128-byte photo buffer'):
            T.region_u8(photo, one(po=bad), out=out)
    with pytest.raises(ValueError, match='writes outside the 64-byte output'):
        T.region_u8(photo, one(oo=49), out=out)
    with pytest.raises(ValueError, match='writes outside the 8-byte output'):
        T.region_u8(photo, one(), out=torch.zeros(8, dtype=torch.uint8, device=dev))
    for oo in (-1, -16, -100):
        with pytest.raises(ValueError, match='writes before the output'):
            T.region_u8(photo, one(oo=oo), out=out)
        with pytest.raises(ValueError, match='writes before the output'):
            T.region_u8(photo, one(oo=oo))                           # before `out` is allocated to fit
    for bad in (dict(sx=-1), dict(sx=4), dict(sy=4), dict(sy=-1)):
        with pytest.raises(ValueError, match='seed'):
            T.region_u8(photo, one(**bad), out=out)
    with pytest.raises(ValueError, match='photo must be'):
        T.region_u8(photo.cpu(), one(), out=out)
    with pytest.raises(ValueError, match='photo must be'):
        T.region_u8(photo.to(torch.int8), one(), out=out)
    with pytest.raises(ValueError, match='out must be'):
        T.region_u8(photo, one(), out=out.cpu())
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.region_u8(photo, [], out=out)
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.region_u8(photo, [(0, 4 * k, 2, 2, 0, 0, 1, 4) for k in range(5)], out=out)
    # what only the library can tell: its text arrives in the exception
    for bad in (-1, 256):
        with pytest.raises(ValueError, match='tol'):
            T.region_u8(photo, one(tol=bad), out=out)
    for bad in (0, 6):
        with pytest.raises(ValueError, match='conn'):
            T.region_u8(photo, one(conn=bad), out=out)
    with pytest.raises(ValueError, match='positive'):
        T.region_u8(photo, one(h=0), out=out)
    with pytest.raises(ValueError, match='destinations overlap'):
        T.region_u8(photo, one() + one(oo=15), out=out)
    with pytest.raises(ValueError, match='overlaps a photo'):
        T.region_u8(photo, one(oo=40), out=photo)
    assert not out.any().item() and (photo == 9).all().item()       # nothing was launched on the way


# ---------------------------------------------------------------- edit_image(select={... wand ...}) against the oracle's planes handed over as masks
def scene(h, w, seed):
    """Random bytes with a sky (the top third) and a lake (a block at the bottom) of the same jittered blue."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    blue = np.zeros((h, w), bool)
    blue[:h // 3] = True
    blue[2 * h // 3:, w // 4:3 * w // 4] = True
    img[blue] = (np.array([40, 90, 200]) + rng.integers(-5, 6, (h, w, 3)))[blue].astype(np.uint8)
    return img


def expected_plane(user_terms, img, painted=None):
    """The plane of a selection in user units on `img` by the oracles: every wand term a flood fill from its own seed pixel
    (the rounding of the issue, by tests/select_cases.py's rnd), handed to the selection oracle as a plane term."""
    h, w = img.shape[:2]
    terms, planes = [], []
    for term in user_terms:
        kind = term[0].lstrip('!')
        if kind in ('wand', 'wand8'):
            sx, sy, tol = SC.rnd(term[1], w - 1), SC.rnd(term[2], h - 1), SC.rnd(term[3] if len(term) == 4 else 0.125, 255.0)
            terms.append(('plane', int(term[0].startswith('!')), len(planes) * h * w))
            planes.append(RC.oracle(img, sx, sy, tol, 4 if kind == 'wand' else 8).reshape(-1))
        else:
            terms.extend(SC.round_units([term], h, w))
    if painted is not None:
        terms.append(('plane', 0, len(planes) * h * w))
        planes.append(painted.reshape(-1))
    return SC.selection(terms, img, np.concatenate(planes) if planes else None)


WAND = [('wand', 0.5, 0.1, 0.08)]
NOT_WAND = [('!wand', 0.5, 0.1, 0.08)]
MIXED = [('wand8', 0.5, 0.1, 0.08), ('hue', 200, 260, 20)]


def count_launches(monkeypatch):
    import t2onet_amd.functional as T
    taken = []
    for name in ('region_u8', 'select_u8', 'refine_u8', 'feather_u8', 'replay_u8', 'replay_u8_masked', 'replay_u8_stencils'):
        monkeypatch.setattr(T, name, (lambda f, n: lambda *a, **k: (taken.append(n), f(*a, **k))[1])(getattr(T, name), name))
    return taken


@pytest.fixture(scope='module')
def stub(dev):
    from tests import replay_cases as PC
    ops = [0, 5, 6]
    return StubActor(ops + [None], PC.params_for(ops + [-1], 4)[:4]).to(dev), torch.ones(1, 4, dtype=torch.long), ops


def test_the_scene_separates_sky_and_lake():
    img = scene(48, 80, 7)
    sky = expected_plane(WAND, img)
    assert sky[:16].all() and not sky[32:].any() and (expected_plane([('hue', 200, 260, 20)], img)[32:, 20:60] == 255).all()
    assert np.array_equal(expected_plane(NOT_WAND, img), 255 - sky)


def test_edit_image_wand_equals_the_oracle_planes_as_masks(dev, stub, monkeypatch):
    from t2onet_amd.edit import edit_image
    model, x, ops = stub
    img = scene(48, 80, 7)
    painted = FC.oracle(FC.plane('vedge', 48, 80), 4)
    taken = count_launches(monkeypatch)
    # a wand alone: region, select, replay
    got = _same(edit_image(model, img, x, select={'all': WAND}), edit_image(model, img, x, masks={'all': expected_plane(WAND, img)}))
    assert got[1] == ops and taken == ['region_u8', 'select_u8', 'replay_u8_masked', 'replay_u8_masked']
    assert not torch.equal(got[0], edit_image(model, img, x)[0])                               # the selection shows
    _same(edit_image(model, img, x, select={'all': NOT_WAND}), edit_image(model, img, x, masks={'all': expected_plane(NOT_WAND, img)}))
    # a wand times a hue term times a painted mask; a second key with the same seed under the other sign shares the region job
    del taken[:]
    _same(edit_image(model, img, x, select={'all': MIXED, 5: [('!wand8', 0.5, 0.1, 0.08)]}, masks={'all': painted}),
          edit_image(model, img, x, masks={'all': expected_plane(MIXED, img, painted), 5: expected_plane([('!wand8', 0.5, 0.1, 0.08)], img)}))
    assert taken[:2] == ['region_u8', 'select_u8'] and taken.count('region_u8') == 1
    # five distinct regions: region_u8 once per 4 jobs
    del taken[:]
    five = [('wand', 0.5, 0.1, 0.08), ('wand8', 0.5, 0.1, 0.08), ('wand', 0.5, 0.9, 0.08), ('!wand', 0.1, 0.5, 0.5)]
    _same(edit_image(model, img, x, select={'all': five, 0: [('wand8', 0.9, 0.9)]}),
          edit_image(model, img, x, masks={'all': expected_plane(five, img), 0: expected_plane([('wand8', 0.9, 0.9)], img)}))
    assert taken[:3] == ['region_u8', 'region_u8', 'select_u8']
    # refine and feather on top: region, select, refine, feather
    del taken[:]
    _same(edit_image(model, img, x, select={'all': WAND, 5: MIXED}, refine={'all': 4, 5: (2, 0.1)}, feather={'all': 1.5, 5: 2.5}),
          edit_image(model, img, x, masks={'all': FR.oracle(img, expected_plane(WAND, img), 4, 26), 5: FR.oracle(img, expected_plane(MIXED, img), 2, 650)},
                     feather={'all': 1.5, 5: 2.5}))
    assert taken[:4] == ['region_u8', 'select_u8', 'refine_u8', 'feather_u8'] and taken.count('region_u8') == 1
    # on a proxy smaller than the photo
    _same(edit_image(model, img, x, proxy_short=32, select={'all': WAND}), edit_image(model, img, x, proxy_short=32, masks={'all': expected_plane(WAND, img)}))


def test_a_call_without_wand_launches_what_it_launched_before(dev, stub, monkeypatch):
    from torch.profiler import profile, ProfilerActivity
    from t2onet_amd.edit import edit_image
    model, x, ops = stub
    img = scene(48, 80, 7)
    rule = [('lum', 0.3, 1.0, 0.2), ('!linear', 0.0, 0.0, 1.0, 1.0)]

    def names(**kw):
        edit_image(model, img, x, **kw)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            edit_image(model, img, x, **kw)
            torch.cuda.synchronize()
        return sorted((re.findall(r'k_\w+', k) or [k])[0] for k, c in _kernels(prof) for _ in range(c) if 'Memcpy' not in k and 'Memset' not in k)
    plain, ruled, wand = names(), names(select={'all': rule}), names(select={'all': rule + WAND})
    print('kernels without a selection: %s\nwith a rule: %s\nwith a wand term: %s' % (plain, ruled, wand))
    assert not [k for k in plain + ruled if 'region' in k]
    assert ruled.count('k_select_u8') == 1 and 'k_select_u8' not in plain
    assert sorted(wand) == sorted(ruled + ['k_region_tile', 'k_region_border', 'k_region_resolve'])       # the wand adds its three and nothing else
    taken = count_launches(monkeypatch)
    edit_image(model, img, x)
    edit_image(model, img, x, select={'all': rule})
    edit_image(model, img, x, masks={'all': FC.plane('vedge', 48, 80)}, refine=2, feather=2)
    assert taken == ['replay_u8', 'select_u8', 'replay_u8_masked', 'refine_u8', 'feather_u8', 'replay_u8_masked']


# ---------------------------------------------------------------- edit_cli --select wand: writes the rule, apply_cli gives every photo its own seed pixel
def test_edit_cli_wand_and_apply_cli_on_other_photos(dev, tmp_path, monkeypatch):
    from PIL import Image
    import t2onet_amd.functional as T
    from t2onet_amd import apply_cli, edit_cli
    from t2onet_amd.data import ACTIONS
    opt, model, ckpt, vocab_dir, _ = _setup(tmp_path, dev)
    common = ['--request', REQUEST, '--checkpoint', ckpt, '--vocab_dir', vocab_dir, '--multi_img']
    Image.fromarray(scene(48, 80, 7)).save(str(tmp_path / 'scene.png'))
    rules = {'all': 'wand:0.5,0.1:0.08', 'tone': '!wand8:0.5,0.9:0.1+hue:200:260:20'}
    flags = [a for name, text in rules.items() for a in ('--select', text if name == 'all' else '%s=%s' % (name, text))]
    info = edit_cli.main(['--img', str(tmp_path / 'scene.png'), '--save_dir', str(tmp_path / 'edited')] + common + flags + ['--feather', 'tone=2'])
    record = str(tmp_path / 'edited' / 'scene' / 'scene.json')
    with open(record) as f:
        saved = json.load(f)
    assert saved == [json.loads(json.dumps(info))]
    assert saved[0]['select'] == rules and saved[0]['feather'] == {'tone': 2.0}                    # the record keeps the rule text
    names = [n for n, _ in info['operations']]
    print('operators chosen:', names)
    assert names, 'the seeded actor chose END first: the test would show nothing'
    request, ops, params = apply_cli.parse_record(saved)
    sigma = {'all': 0.0, 'tone': 2.0}
    photos = {'p.png': scene(40, 60, 11), 'q.png': scene(33, 90, 12)}
    for name, a in photos.items():
        Image.fromarray(a).save(str(tmp_path / name))
    taken = count_launches(monkeypatch)
    infos = apply_cli.main(['--record', record, '--img'] + [str(tmp_path / n) for n in photos] + ['--save_dir', str(tmp_path / 'applied'), '--multi_img'])
    used = {('tone' if ACTIONS[op] == 'tone' else 'all') for op in ops}
    assert taken.count('region_u8') == taken.count('select_u8') == 1 and taken[:2] == ['region_u8', 'select_u8']      # 2 photos x <= 2 seeds: one call
    par = np.zeros((8, 24), np.float32)
    par[:len(ops)] = params
    for new, (name, a) in zip(infos, photos.items()):
        stem, (h, w) = name[:-4], a.shape[:2]
        planes, slot = [], {}
        for key in sorted(used):
            slot[key] = len(planes)
            planes.append(FC.oracle(expected_plane(edit_cli.parse_select_terms(rules[key]), a), sigma[key]))        # THIS photo's own seed pixel
        mask_of = [slot['tone' if ACTIONS[op] == 'tone' else 'all'] for op in ops]
        jobs = [(0, k * a.size, h, w, ops[:k + 1], mask_of[:k + 1]) for k in range(len(ops))]
        want = T.replay_u8_any(torch.from_numpy(a.reshape(-1).copy()).to(dev), jobs, torch.from_numpy(par).to(dev)[None].repeat(len(ops), 1, 1),
                               torch.from_numpy(np.concatenate([p.reshape(-1) for p in planes])).to(dev),
                               [k * h * w for k in range(len(planes))]).cpu().numpy().reshape(len(ops), h, w, 3)
        d = tmp_path / 'applied' / stem
        assert np.array_equal(_png(str(d / name)), want[-1])
        for k in range(len(ops)):
            assert np.array_equal(_png(str(d / ('%d_inference_%s' % (k + 1, name)))), want[k]), (name, k)
        with open(str(d / (stem + '.json'))) as f:
            again = json.load(f)
        assert again == [json.loads(json.dumps(new))] and again[0]['select'] == rules and again[0]['record'] == record
