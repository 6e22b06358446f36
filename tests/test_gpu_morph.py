"""The mask morph kernels (t2o_morph.hip), edit_image's `grow`, the edit command's --grow and the local apply command on the
GPU.  Integers throughout: the kernels' bytes must EQUAL the brute-force int64 oracle's (tests/morph_cases.py, shared with
tests/test_morph_cpu.py), guard bytes around every destination plane included; everything downstream must equal what the
oracle-grown plane gives when it is handed over as a painted mask."""
import json
import re

import numpy as np
import pytest
import torch

from tests import fill_cases as LC
from tests import morph_cases as MC
from tests.test_gpu_region import expected_plane, scene
from tests.test_gpu_select import REQUEST, StubActor, _png, _same, _setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def calls(dev):
    return MC.calls()                                                # the oracle runs once per plane, here


def run_call(dev, call):
    """One morph_u8 call on device copies of the call's buffers -> the destination buffer afterwards."""
    import t2onet_amd.functional as T
    src = torch.from_numpy(call.src).to(dev)
    if call.out is call.src:
        assert T.morph_u8(src, call.jobs) is src                    # out = None: inside the buffer
        return src.cpu().numpy()
    out = torch.from_numpy(call.out).to(dev)
    assert T.morph_u8(src, call.jobs, out=out) is out
    assert np.array_equal(src.cpu().numpy(), call.src)              # the source is only read
    return out.cpu().numpy()


def test_bytes_equal_the_oracle(dev, calls):
    """Every case at its own destination residue with the source at an odd offset, the call of four jobs of three sizes and
    three modes, the call in place and the call whose jobs share a source."""
    assert {j[1] % 4 for _, c in calls for j in c.jobs} == {0, 1, 2, 3}
    assert {j[5] for _, c in calls for j in c.jobs} == set(MC.MODES) and {j[4] for _, c in calls for j in c.jobs} >= set(MC.RADII)
    for name, call in calls:
        np.testing.assert_array_equal(run_call(dev, call), call.want, err_msg='%s %s' % (name, call.jobs))


def test_two_runs_are_equal(dev, calls):
    by_name = dict(calls)
    for name in ('big_200x136_grow_25', 'wide_130x200_grow', 'four_jobs', 'shared_source'):
        a, b = run_call(dev, by_name[name]), run_call(dev, by_name[name])
        assert np.array_equal(a, b) and np.array_equal(a, by_name[name].want), name


def test_in_place_equals_out_of_place(dev):
    import t2onet_amd.functional as T
    by_name = {c[0]: c for c in MC.cases()}
    for name in ('corner_129x67_border', 'big_200x136_inverse_shrink', 'wide_130x200_grow', 'tiny_1x7_grow', 'first_unset_border'):
        _, m, radius, mode = by_name[name]
        h, w = m.shape
        buf = torch.full((7 + h * w + 5,), MC.GUARD, dtype=torch.uint8, device=dev)
        buf[7:7 + h * w] = torch.from_numpy(m.reshape(-1).copy()).to(dev)
        apart = T.morph_u8(buf, [(7, 1, h, w, radius, mode)], out=torch.full((h * w + 2,), MC.GUARD, dtype=torch.uint8, device=dev))
        want = MC.oracle(m, radius, mode).reshape(-1)
        assert T.morph_u8(buf, [(7, 7, h, w, radius, mode)]) is buf
        got = buf.cpu().numpy()
        np.testing.assert_array_equal(got[7:7 + h * w], want, err_msg=name)
        assert (got[:7] == MC.GUARD).all() and (got[7 + h * w:] == MC.GUARD).all()
        assert np.array_equal(apart.cpu().numpy()[1:1 + h * w], want), name


def test_call_is_graph_capturable(dev, calls):
    import t2onet_amd.functional as T
    call = dict(calls)['four_jobs']
    src = torch.from_numpy(call.src).to(dev)
    out = torch.from_numpy(call.out).to(dev)

    def run():
        return T.morph_u8(src, call.jobs, out=out)
    eager = run().clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                        # one stream, two kernels in a row: no parallel branches
        run()
    out.copy_(torch.from_numpy(call.out).to(dev))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    np.testing.assert_array_equal(out.cpu().numpy(), call.want)


def test_wrapper_refuses_what_the_library_refuses(dev):
    import t2onet_amd.functional as T
    buf = torch.zeros(64, dtype=torch.uint8, device=dev)
    one = (0, 16, 4, 4, 2, 'grow')
    for bad in (-1, 65):
        with pytest.raises(ValueError, match='radius'):
            T.morph_u8(buf, [(0, 16, 4, 4, bad, 'grow')])
    with pytest.raises(ValueError, match='not a whole number'):
        T.morph_u8(buf, [(0, 16, 4, 4, 2.5, 'grow')])
    with pytest.raises(ValueError, match='mode'):
        T.morph_u8(buf, [(0, 16, 4, 4, 2, 3)])
    with pytest.raises(ValueError, match='mode'):
        T.morph_u8(buf, [(0, 16, 4, 4, 2, 'melt')])
    with pytest.raises(ValueError, match='positive'):
        T.morph_u8(buf, [(0, 16, 0, 4, 2, 'grow')])
    with pytest.raises(ValueError, match='overlap'):
        T.morph_u8(buf, [one, (32, 20, 4, 4, 2, 'shrink')])
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.morph_u8(buf, [])
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.morph_u8(buf, [(0, 8 * k, 2, 2, 1, 'grow') for k in range(5)])
    with pytest.raises(ValueError, match='reads outside the 64-byte buffer'):
        T.morph_u8(buf, [(49, 0, 4, 4, 2, 'grow')])
    with pytest.raises(ValueError, match='reads outside the 64-byte buffer'):
        T.morph_u8(buf, [(-1, 0, 4, 4, 2, 'grow')])
    with pytest.raises(ValueError, match='writes outside the 64-byte output'):
        T.morph_u8(buf, [(0, 49, 4, 4, 2, 'grow')])
    with pytest.raises(ValueError, match='writes outside the 8-byte output'):
        T.morph_u8(buf, [one], out=torch.zeros(8, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='out must be'):
        T.morph_u8(buf, [one], out=torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(ValueError, match='buffer must be'):
        T.morph_u8(buf.to(torch.int8), [one])
    assert not buf.any().item()                                      # nothing was launched on the way


# ---------------------------------------------------------------- edit_image(grow=...) against the oracle-grown plane handed over as a mask
WAND = [('wand', 0.5, 0.1, 0.08)]
LAUNCHERS = ('region_u8', 'select_u8', 'morph_u8', 'refine_u8', 'feather_u8', 'fill_u8', 'replay_u8', 'replay_u8_masked', 'replay_u8_stencils')


def count_launches(monkeypatch):
    import t2onet_amd.functional as T
    taken = []
    for name in LAUNCHERS:
        monkeypatch.setattr(T, name, (lambda f, n: lambda *a, **k: (taken.append(n), f(*a, **k))[1])(getattr(T, name), name))
    return taken


@pytest.fixture(scope='module')
def stub(dev):
    from tests import replay_cases as PC
    ops = [0, 5, 6]
    return StubActor(ops + [None], PC.params_for(ops + [-1], 4)[:4]).to(dev), torch.ones(1, 4, dtype=torch.long), ops


def test_edit_image_grow_equals_the_oracle_grown_plane(dev, stub, monkeypatch):
    from tests import feather_cases as FC
    from t2onet_amd.edit import edit_image
    model, x, ops = stub
    img = scene(48, 80, 7)
    taken = count_launches(monkeypatch)
    # a painted plane (soft: it is binarised at 128), grown by 3 in place behind the photo
    painted = FC.oracle(FC.plane('vedge', 48, 80), 2)
    grown = MC.oracle(painted, 3, 'grow')
    assert not np.array_equal(grown, np.where(painted >= 128, 255, 0)) and 0 < grown.mean() < 255
    got = _same(edit_image(model, img, x, masks={4: painted, 5: painted}, grow={4: 3}), edit_image(model, img, x, masks={4: grown, 5: grown}))
    assert got[1] == ops and taken == ['morph_u8', 'replay_u8_masked', 'replay_u8_masked']
    assert not torch.equal(got[0], edit_image(model, img, x, masks={4: painted, 5: painted})[0])      # the move shows
    # shrunk and bordered, one call for two planes; 0 leaves a plane exactly as it is, soft bytes included
    other = FC.oracle(FC.plane('hedge', 48, 80), 2)
    del taken[:]
    _same(edit_image(model, img, x, masks={5: painted, 0: other}, grow={5: -4, 0: ('border', 2)}),
          edit_image(model, img, x, masks={5: MC.oracle(painted, 4, 'shrink'), 0: MC.oracle(other, 2, 'border')}))
    assert taken.count('morph_u8') == 1
    del taken[:]
    _same(edit_image(model, img, x, masks={5: painted}, grow=0), edit_image(model, img, x, masks={5: painted}))
    assert 'morph_u8' not in taken
    # a wand's plane: region, select, grow, then refine and feather on the grown plane
    sky = expected_plane(WAND, img)
    assert sky[:16].all() and not sky[32:].any()
    wide = MC.oracle(sky, 3, 'grow')
    assert wide[:19].all() and not wide[40:].any() and not np.array_equal(wide, sky)
    del taken[:]
    _same(edit_image(model, img, x, select={5: WAND}, grow={5: 3}), edit_image(model, img, x, masks={5: wide}))
    assert taken[:3] == ['region_u8', 'select_u8', 'morph_u8'] and taken.count('morph_u8') == 1
    del taken[:]
    _same(edit_image(model, img, x, select={5: WAND}, grow=3, feather=1.5), edit_image(model, img, x, masks={5: FC.oracle(wide, 1.5)}))
    assert taken[:4] == ['region_u8', 'select_u8', 'morph_u8', 'feather_u8']
    # the fill under the grown plane: the rim of the region is no source of the fill any more
    del taken[:]
    filled = _same(edit_image(model, img, x, select={4: WAND}, grow={4: 3}, fill=4), edit_image(model, LC.oracle(img, wide), x, masks={4: wide}))
    assert taken[:4] == ['region_u8', 'select_u8', 'morph_u8', 'fill_u8']
    assert not torch.equal(filled[0], edit_image(model, img, x, select={4: WAND}, fill=4)[0])
    # on a proxy smaller than the photo
    _same(edit_image(model, img, x, proxy_short=32, select={5: WAND}, grow={5: ('border', 2)}),
          edit_image(model, img, x, proxy_short=32, masks={5: MC.oracle(sky, 2, 'border')}))


def _kernels(prof):
    from torch.autograd import DeviceType
    return [(e.key, e.count) for e in prof.key_averages() if e.device_type == DeviceType.CUDA]


def test_a_call_without_grow_launches_what_it_launched_before(dev, stub, monkeypatch):
    from torch.profiler import profile, ProfilerActivity
    from tests import feather_cases as FC
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
    wand, none, grown = names(select={4: WAND}, fill=4), names(select={4: WAND}, fill=4, grow=None), names(select={4: WAND}, fill=4, grow={4: 3})
    print('kernels with a wand and the fill: %s\nwith grow on top: %s' % (wand[0], grown[0]))
    assert none == wand and not [k for k in wand[0] if 'morph' in k]
    assert grown[0] == sorted(wand[0] + ['k_morph_cols', 'k_morph_rows'])                          # grow adds its two and nothing else
    assert grown[1] == wand[1]                                                                     # and no upload
    a = edit_image(model, img, x, select={4: WAND}, masks={5: FC.plane('vedge', 48, 80)}, feather=2)
    b = edit_image(model, img, x, select={4: WAND}, masks={5: FC.plane('vedge', 48, 80)}, feather=2, grow=None)
    _same(a, b)
    taken = count_launches(monkeypatch)
    edit_image(model, img, x)
    edit_image(model, img, x, select={'all': WAND}, grow=None)
    edit_image(model, img, x, masks={'all': FC.plane('vedge', 48, 80)}, refine=2, feather=2, grow=None)
    assert taken == ['replay_u8', 'region_u8', 'select_u8', 'replay_u8_masked', 'refine_u8', 'feather_u8', 'replay_u8_masked']


# ---------------------------------------------------------------- edit_cli --grow writes the record, apply_cli grows every photo's plane at its own size
def test_edit_cli_grow_and_apply_cli_on_another_photo(dev, tmp_path, monkeypatch):
    from PIL import Image
    import t2onet_amd.functional as T
    from t2onet_amd import apply_cli, edit_cli
    opt, model, ckpt, vocab_dir, _ = _setup(tmp_path, dev)
    common = ['--request', REQUEST, '--checkpoint', ckpt, '--vocab_dir', vocab_dir, '--multi_img']
    first = scene(48, 80, 7)
    Image.fromarray(first).save(str(tmp_path / 'scene.png'))
    rule = 'wand:0.5,0.1:0.08'
    flags = ['--select', rule]
    plain = edit_cli.main(['--img', str(tmp_path / 'scene.png'), '--save_dir', str(tmp_path / 'plain')] + common + flags)
    assert 'grow' not in plain
    info = edit_cli.main(['--img', str(tmp_path / 'scene.png'), '--save_dir', str(tmp_path / 'edited')] + common + flags + ['--grow', '5'])
    record = str(tmp_path / 'edited' / 'scene' / 'scene.json')
    with open(record) as f:
        saved = json.load(f)
    assert saved == [json.loads(json.dumps(info))]
    assert saved[0]['grow'] == {'all': ['grow', 5]} and saved[0]['select'] == {'all': rule}
    names = [n for n, _ in info['operations']]
    print('operators chosen:', names)
    assert names, 'the seeded actor chose END first: the test would show nothing'
    assert not np.array_equal(_png(str(tmp_path / 'edited' / 'scene' / 'scene.png')), _png(str(tmp_path / 'plain' / 'scene' / 'scene.png')))
    request, ops, params = apply_cli.parse_record(saved)
    par = np.zeros((8, 24), np.float32)
    par[:len(ops)] = params

    def replayed(a, plane):
        h, w = a.shape[:2]
        jobs = [(0, k * a.size, h, w, ops[:k + 1], [0] * (k + 1)) for k in range(len(ops))]
        return T.replay_u8_any(torch.from_numpy(a.reshape(-1).copy()).to(dev), jobs, torch.from_numpy(par).to(dev)[None].repeat(len(ops), 1, 1),
                               torch.from_numpy(plane.reshape(-1).copy()).to(dev), [0]).cpu().numpy().reshape(len(ops), h, w, 3)
    # the first photo itself: what --grow 5 wrote is the replay under the oracle-grown plane
    terms = edit_cli.parse_select_terms(rule)
    want = replayed(first, MC.oracle(expected_plane(terms, first), 5, 'grow'))
    assert np.array_equal(_png(str(tmp_path / 'edited' / 'scene' / 'scene.png')), want[-1])
    # a second photo of another size: its own seed pixel, its own size, the same number of pixels
    other = scene(33, 90, 12)
    Image.fromarray(other).save(str(tmp_path / 'q.png'))
    taken = count_launches(monkeypatch)
    new, = apply_cli.main(['--record', record, '--img', str(tmp_path / 'q.png'), '--save_dir', str(tmp_path / 'applied'), '--multi_img'])
    assert taken.count('morph_u8') == 1 and taken.index('morph_u8') == taken.index('select_u8') + 1
    assert taken.index('morph_u8') < min(i for i, n in enumerate(taken) if n.startswith('replay'))
    own = expected_plane(terms, other)
    grown = MC.oracle(own, 5, 'grow')
    assert not np.array_equal(grown, own)
    want = replayed(other, grown)
    d = tmp_path / 'applied' / 'q'
    assert np.array_equal(_png(str(d / 'q.png')), want[-1])
    for k in range(len(ops)):
        assert np.array_equal(_png(str(d / ('%d_inference_q.png' % (k + 1)))), want[k]), k
    assert not np.array_equal(want[-1], replayed(other, own)[-1])                                   # the move shows on this photo too
    with open(str(d / 'q.json')) as f:
        again = json.load(f)
    assert again == [json.loads(json.dumps(new))] and again[0]['grow'] == {'all': ['grow', 5]} and again[0]['select'] == {'all': rule} and again[0]['record'] == record
