"""The fill kernels (t2o_fill.hip), edit_image's `fill`, the edit command's --fill and the local apply command on the GPU.
The kernels' bytes must EQUAL the int64 oracle's (tests/fill_cases.py, shared with tests/test_fill_cpu.py), guard bytes
around every destination included; everything downstream must equal what the oracle-filled photo gives without a fill."""
import json
import re

import numpy as np
import pytest
import torch

from tests import feather_cases as FC
from tests import fill_cases as LC
from tests import refine_cases as FR
from tests.test_gpu_region import expected_plane, scene
from tests.test_gpu_select import REQUEST, StubActor, _png, _same, _setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def run_call(dev, call, jobs=None, out=None):
    """The call on the device -> the destination buffer (the photo buffer itself for a call whose destinations lie in it)."""
    import t2onet_amd.functional as T
    photo, planes = torch.from_numpy(call.photo).to(dev), torch.from_numpy(call.planes).to(dev)
    if out is None:
        out = photo if call.same else torch.from_numpy(call.out).to(dev)
    assert T.fill_u8(photo, planes, call.jobs if jobs is None else jobs, out=out) is out
    assert np.array_equal(planes.cpu().numpy(), call.planes)        # the planes are only read
    if out is not photo:
        assert np.array_equal(photo.cpu().numpy(), call.photo)      # and so is the photo
    return out.cpu().numpy()


def test_bytes_equal_the_oracle(dev):
    """Every case of the list at every residue of the destination offset, photos and planes at odd offsets, and the call of
    four jobs in one buffer, one of them in place."""
    for name, call in LC.calls():
        np.testing.assert_array_equal(run_call(dev, call), call.want, err_msg='%s %s %s' % (name, call.names, call.jobs))


def test_two_runs_are_equal_and_out_is_allocated_to_fit(dev):
    import t2onet_amd.functional as T
    for name in ('big_300x521', 'multi_job'):
        call = dict(LC.calls())[name]
        a, b = run_call(dev, call), run_call(dev, call)
        assert np.array_equal(a, b) and np.array_equal(a, call.want)
    call = dict(LC.calls())['tile_200x136']
    photo, planes = torch.from_numpy(call.photo).to(dev), torch.from_numpy(call.planes).to(dev)
    a = T.fill_u8(photo, planes, call.jobs)
    (_, _, oo, h, w), = call.jobs
    assert a.numel() == oo + 3 * h * w and a.dtype == torch.uint8 and a.device == photo.device
    assert np.array_equal(a[oo:].cpu().numpy(), call.want[oo:oo + 3 * h * w])


def test_multi_job_call_equals_separate_calls(dev):
    call = dict(LC.calls())['multi_job']
    whole = run_call(dev, call)
    buf = torch.from_numpy(call.photo).to(dev)
    planes = torch.from_numpy(call.planes).to(dev)
    import t2onet_amd.functional as T
    order = [k for k, j in enumerate(call.jobs) if j[0] != j[2]] + [k for k, j in enumerate(call.jobs) if j[0] == j[2]]     # the job in place last
    for k in order:
        T.fill_u8(buf, planes, [call.jobs[k]], out=buf)
    assert np.array_equal(whole, buf.cpu().numpy()) and np.array_equal(whole, call.want)


def test_in_place_equals_out_of_place(dev):
    import t2onet_amd.functional as T
    for name in ('corner_129x67', 'big_300x521', 'last_pixel_130x70', 'all_255_70x66', 'all_0_70x66', 'row_1x7'):
        _, photo, plane = next(c for c in LC.cases() if c[0] == name)
        h, w = plane.shape
        buf = torch.full((7 + 3 * h * w + 5,), LC.GUARD, dtype=torch.uint8, device=dev)
        buf[7:7 + 3 * h * w] = torch.from_numpy(photo.reshape(-1)).to(dev)
        planes = torch.from_numpy(plane.reshape(-1).copy()).to(dev)
        apart = T.fill_u8(buf, planes, [(7, 0, 0, h, w)])
        want = buf.cpu().numpy()
        want[7:7 + 3 * h * w] = LC.want(name).reshape(-1)
        assert T.fill_u8(buf, planes, [(7, 0, 7, h, w)], out=buf) is buf
        np.testing.assert_array_equal(buf.cpu().numpy(), want, err_msg=name)
        assert np.array_equal(apart.cpu().numpy(), LC.want(name).reshape(-1)), name


def test_call_is_graph_capturable(dev):
    import t2onet_amd.functional as T
    call = dict(LC.calls())['big_300x521']
    photo, planes, out = (torch.from_numpy(a).to(dev) for a in (call.photo, call.planes, call.out))

    def run():
        return T.fill_u8(photo, planes, call.jobs, out=out)
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


def test_three_launches_whatever_the_pictures_hold(dev):
    """One job and four; a picture without a hole and one that is all hole."""
    import t2onet_amd.functional as T
    from torch.profiler import profile, ProfilerActivity
    runs = []
    multi = dict(LC.calls())['multi_job']
    buf, planes = torch.from_numpy(multi.photo).to(dev), torch.from_numpy(multi.planes).to(dev)
    runs.append(('four jobs', buf, planes, multi.jobs, buf))
    for name in ('big_300x521', 'all_0_70x66', 'all_255_70x66'):
        call = dict(LC.calls())[name]
        runs.append((name, torch.from_numpy(call.photo).to(dev), torch.from_numpy(call.planes).to(dev), call.jobs, torch.from_numpy(call.out).to(dev)))
    for name, photo, planes, jobs, out in runs:
        T.fill_u8(photo, planes, jobs, out=out)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            T.fill_u8(photo, planes, jobs, out=out)
            torch.cuda.synchronize()
        ks = _kernels(prof)
        print('fill_u8, %s: %s' % (name, ks))
        assert sorted(re.findall(r'k_fill_\w+', k)[0] for k, _ in ks if 'k_fill_' in k) == ['k_fill_pull', 'k_fill_push', 'k_fill_top'], ks
        assert sum(c for _, c in ks) == T.FILL_LAUNCHES == 3, ks


def test_wrapper_refuses_before_any_launch(dev):
    import t2onet_amd.functional as T
    photo = torch.full((128,), 9, dtype=torch.uint8, device=dev)
    planes = torch.full((32,), 255, dtype=torch.uint8, device=dev)
    out = torch.full((64,), 7, dtype=torch.uint8, device=dev)

    def one(po=0, mo=0, oo=0, h=4, w=4):
        return [(po, mo, oo, h, w)]
    for bad in (81, -1):
        with pytest.raises(ValueError, match='reads outside the 128-byte photo buffer'):
            T.fill_u8(photo, planes, one(po=bad), out=out)
    for bad in (17, -1):
        with pytest.raises(ValueError, match='reads outside the 32-byte plane buffer'):
            T.fill_u8(photo, planes, one(mo=bad), out=out)
    with pytest.raises(ValueError, match='writes outside the 64-byte output'):
        T.fill_u8(photo, planes, one(oo=17), out=out)
    with pytest.raises(ValueError, match='writes outside the 8-byte output'):
        T.fill_u8(photo, planes, one(), out=torch.zeros(8, dtype=torch.uint8, device=dev))
    for oo in (-1, -16, -100):
        with pytest.raises(ValueError, match='writes before the output'):
            T.fill_u8(photo, planes, one(oo=oo), out=out)
        with pytest.raises(ValueError, match='writes before the output'):
            T.fill_u8(photo, planes, one(oo=oo))                     # before `out` is allocated to fit
    with pytest.raises(ValueError, match='photo and planes must be'):
        T.fill_u8(photo.cpu(), planes, one(), out=out)
    with pytest.raises(ValueError, match='photo and planes must be'):
        T.fill_u8(photo, planes.to(torch.int8), one(), out=out)
    with pytest.raises(ValueError, match='out must be'):
        T.fill_u8(photo, planes, one(), out=out.cpu())
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.fill_u8(photo, planes, [], out=out)
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.fill_u8(photo, planes, [(0, 0, 12 * k, 2, 2) for k in range(5)], out=out)
    # what only the library can tell: its text arrives in the exception
    with pytest.raises(ValueError, match='positive'):
        T.fill_u8(photo, planes, one(h=0), out=out)
    with pytest.raises(ValueError, match='destinations overlap'):
        T.fill_u8(photo, planes, [(0, 0, 0, 2, 2), (12, 4, 11, 2, 2)], out=out)
    with pytest.raises(ValueError, match='overlaps a photo'):
        T.fill_u8(photo, planes, one(oo=40), out=photo)              # on its own photo, but not at its own address
    with pytest.raises(ValueError, match='overlaps a photo'):
        T.fill_u8(photo, planes, [(0, 0, 0, 4, 4), (0, 16, 60, 4, 4)], out=photo)      # in place on a photo another job reads
    with pytest.raises(ValueError, match='overlaps a plane'):
        T.fill_u8(photo, photo, one(mo=100, oo=60), out=photo)
    assert (out == 7).all().item() and (photo == 9).all().item() and (planes == 255).all().item()       # nothing was launched on the way


# ---------------------------------------------------------------- edit_image(fill=...) against the oracle-filled photo handed over without fill
WAND = [('wand', 0.5, 0.1, 0.08)]


def count_launches(monkeypatch):
    import t2onet_amd.functional as T
    taken = []
    for name in ('region_u8', 'select_u8', 'refine_u8', 'feather_u8', 'fill_u8', 'replay_u8', 'replay_u8_masked', 'replay_u8_stencils'):
        monkeypatch.setattr(T, name, (lambda f, n: lambda *a, **k: (taken.append(n), f(*a, **k))[1])(getattr(T, name), name))
    return taken


@pytest.fixture(scope='module')
def stub(dev):
    from tests import replay_cases as PC
    ops = [0, 5, 6]
    return StubActor(ops + [None], PC.params_for(ops + [-1], 4)[:4]).to(dev), torch.ones(1, 4, dtype=torch.long), ops


def test_edit_image_fill_equals_the_oracle_filled_photo(dev, stub, monkeypatch):
    from t2onet_amd.edit import edit_image
    model, x, ops = stub
    img = scene(48, 80, 7)
    sky = expected_plane(WAND, img)                                   # from the ORIGINAL bytes
    assert sky[:16].all() and not sky[32:].any()
    taken = count_launches(monkeypatch)
    # the wand's plane under the inpaint slot: region, select, fill, replay -- and the same without fill on the filled photo
    filled = LC.oracle(img, sky)
    assert not np.array_equal(filled, img) and np.array_equal(filled[sky == 0], img[sky == 0])
    got = _same(edit_image(model, img, x, select={4: WAND}, fill=4), edit_image(model, filled, x, masks={4: sky}))
    assert got[1] == ops and taken == ['region_u8', 'select_u8', 'fill_u8', 'replay_u8_masked', 'replay_u8_masked']
    assert not torch.equal(got[0], edit_image(model, img, x, select={4: WAND})[0])               # the fill shows
    # refined and feathered first: region, select, refine, feather, fill
    del taken[:]
    soft = FC.oracle(FR.oracle(img, sky, 4, 26), 1.5)
    _same(edit_image(model, img, x, select={4: WAND}, refine={4: 4}, feather={4: 1.5}, fill=4),
          edit_image(model, LC.oracle(img, soft), x, masks={4: soft}))
    assert taken[:5] == ['region_u8', 'select_u8', 'refine_u8', 'feather_u8', 'fill_u8'] and taken.count('fill_u8') == 1
    # under 'all' the plane also localises the operators, as it does without fill
    _same(edit_image(model, img, x, select={'all': WAND}, feather=1.5, fill='all'),
          edit_image(model, LC.oracle(img, FC.oracle(sky, 1.5)), x, masks={'all': FC.oracle(sky, 1.5)}))
    # a painted plane, beside a rule for another operator and alone
    painted = FC.oracle(FC.plane('vedge', 48, 80), 2)
    _same(edit_image(model, img, x, select={5: WAND}, masks={4: painted}, fill=4),
          edit_image(model, LC.oracle(img, painted), x, masks={4: painted, 5: sky}))
    del taken[:]
    _same(edit_image(model, img, x, masks={4: painted}, fill=4), edit_image(model, LC.oracle(img, painted), x, masks={4: painted}))
    assert taken == ['fill_u8', 'replay_u8_masked', 'replay_u8_masked']
    # on a proxy smaller than the photo: the actor decides on the filled picture
    _same(edit_image(model, img, x, proxy_short=32, select={4: WAND}, fill=4), edit_image(model, filled, x, proxy_short=32, masks={4: sky}))


def test_a_call_without_fill_launches_what_it_launched_before(dev, stub, monkeypatch):
    from torch.profiler import profile, ProfilerActivity
    from t2onet_amd.edit import edit_image
    model, x, ops = stub
    img = scene(48, 80, 7)

    def names(**kw):
        edit_image(model, img, x, **kw)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            edit_image(model, img, x, **kw)
            torch.cuda.synchronize()
        ks = _kernels(prof)
        return (sorted((re.findall(r'k_\w+', k) or [k])[0] for k, c in ks for _ in range(c) if 'Memcpy' not in k and 'Memset' not in k),
                sum(c for k, c in ks if 'Memcpy HtoD' in k))
    plain, wand, filled = names(), names(select={4: WAND}), names(select={4: WAND}, fill=4)
    print('kernels without a selection: %s\nwith a wand: %s\nwith the fill: %s' % (plain[0], wand[0], filled[0]))
    assert not [k for k in plain[0] + wand[0] if 'fill' in k]
    assert filled[0] == sorted(wand[0] + ['k_fill_pull', 'k_fill_top', 'k_fill_push'])             # the fill adds its three and nothing else
    assert filled[1] == wand[1]                                                                    # and no upload
    taken = count_launches(monkeypatch)
    edit_image(model, img, x)
    edit_image(model, img, x, select={'all': WAND})
    edit_image(model, img, x, masks={'all': FC.plane('vedge', 48, 80)}, refine=2, feather=2)
    edit_image(model, img, x, masks={'all': FC.plane('vedge', 48, 80)}, fill=None)
    assert taken == ['replay_u8', 'region_u8', 'select_u8', 'replay_u8_masked', 'refine_u8', 'feather_u8', 'replay_u8_masked', 'replay_u8_masked']


# ---------------------------------------------------------------- edit_cli --fill writes the record, apply_cli fills every photo under its own plane
def test_edit_cli_fill_and_apply_cli_on_other_photos(dev, tmp_path, monkeypatch):
    from PIL import Image
    import t2onet_amd.functional as T
    from t2onet_amd import apply_cli, edit_cli
    from t2onet_amd.data import ACTIONS
    opt, model, ckpt, vocab_dir, _ = _setup(tmp_path, dev)
    common = ['--request', REQUEST, '--checkpoint', ckpt, '--vocab_dir', vocab_dir, '--multi_img']
    first = scene(48, 80, 7)
    Image.fromarray(first).save(str(tmp_path / 'scene.png'))
    rules = {'inpaint': 'wand:0.5,0.1:0.08', 'tone': '!wand8:0.5,0.9:0.1+hue:200:260:20'}
    flags = [a for name, text in rules.items() for a in ('--select', '%s=%s' % (name, text))] + ['--feather', 'inpaint=2']
    plain = edit_cli.main(['--img', str(tmp_path / 'scene.png'), '--save_dir', str(tmp_path / 'plain')] + common + flags)
    assert 'fill' not in plain
    info = edit_cli.main(['--img', str(tmp_path / 'scene.png'), '--save_dir', str(tmp_path / 'edited')] + common + flags + ['--fill'])
    record = str(tmp_path / 'edited' / 'scene' / 'scene.json')
    with open(record) as f:
        saved = json.load(f)
    assert saved == [json.loads(json.dumps(info))]
    assert saved[0]['fill'] == 'inpaint' and saved[0]['select'] == rules and saved[0]['feather'] == {'inpaint': 2.0}
    assert not np.array_equal(_png(str(tmp_path / 'edited' / 'scene' / 'scene.png')), _png(str(tmp_path / 'plain' / 'scene' / 'scene.png')))
    names = [n for n, _ in info['operations']]
    print('operators chosen:', names)
    assert names, 'the seeded actor chose END first: the test would show nothing'
    request, ops, params = apply_cli.parse_record(saved)
    photos = {'p.png': scene(40, 60, 11), 'q.png': scene(33, 90, 12)}
    for name, a in photos.items():
        Image.fromarray(a).save(str(tmp_path / name))
    taken = count_launches(monkeypatch)
    infos = apply_cli.main(['--record', record, '--img'] + [str(tmp_path / n) for n in photos] + ['--save_dir', str(tmp_path / 'applied'), '--multi_img'])
    assert taken.count('fill_u8') == 1 and taken.index('fill_u8') == taken.index('feather_u8') + 1       # two photos: one call, behind feather
    assert taken.index('fill_u8') < min(i for i, n in enumerate(taken) if n.startswith('replay'))
    par = np.zeros((8, 24), np.float32)
    par[:len(ops)] = params
    for new, (name, a) in zip(infos, photos.items()):
        stem, (h, w) = name[:-4], a.shape[:2]
        hole = FC.oracle(expected_plane(edit_cli.parse_select_terms(rules['inpaint']), a), 2.0)     # THIS photo's own seed pixel and size
        filled = LC.oracle(a, hole)
        assert not np.array_equal(filled, a)
        tone = expected_plane(edit_cli.parse_select_terms(rules['tone']), a)                         # from the ORIGINAL bytes
        mask_of = [0 if ACTIONS[op] == 'tone' else -1 for op in ops]
        jobs = [(0, k * a.size, h, w, ops[:k + 1], mask_of[:k + 1]) for k in range(len(ops))]
        want = T.replay_u8_any(torch.from_numpy(filled.reshape(-1).copy()).to(dev), jobs, torch.from_numpy(par).to(dev)[None].repeat(len(ops), 1, 1),
                               torch.from_numpy(tone.reshape(-1).copy()).to(dev), [0]).cpu().numpy().reshape(len(ops), h, w, 3)
        d = tmp_path / 'applied' / stem
        assert np.array_equal(_png(str(d / name)), want[-1])
        for k in range(len(ops)):
            assert np.array_equal(_png(str(d / ('%d_inference_%s' % (k + 1, name)))), want[k]), (name, k)
        with open(str(d / (stem + '.json'))) as f:
            again = json.load(f)
        assert again == [json.loads(json.dumps(new))] and again[0]['fill'] == 'inpaint' and again[0]['select'] == rules and again[0]['record'] == record
