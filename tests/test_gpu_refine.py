"""The mask refine kernels (t2o_refine.hip), edit_image's `refine`, the edit command's --refine and the local apply command on
the GPU.  Integers throughout: the kernels' bytes must EQUAL the int64 oracle's (tests/refine_cases.py, shared with
tests/test_refine_cpu.py), guard bytes around every destination plane included; everything downstream must equal what
the oracle-refined planes give when they are handed over as painted masks."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import feather_cases as FC
from tests import refine_cases as RC
from tests import select_cases as SC
from tests.test_gpu_select import OTHER, REQUEST, RULE, _png, _same, _setup, oracle_plane

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def run_call(dev, call):
    import t2onet_amd.functional as T
    photo = torch.from_numpy(call.photo).to(dev)
    out = torch.from_numpy(call.out).to(dev)
    src = out if call.src is call.out else torch.from_numpy(call.src).to(dev)
    assert T.refine_u8(photo, src, call.jobs, out=None if src is out else out) is out
    assert np.array_equal(photo.cpu().numpy(), call.photo)          # the photo is only read
    if src is not out:
        assert np.array_equal(src.cpu().numpy(), call.src)
    return out.cpu().numpy()


def test_bytes_equal_the_oracle(dev):
    """Every size x radius of the case list, four jobs of mixed size to a call, separate and in place, every residue of the
    three offsets, the call whose jobs overlap."""
    for name, call in RC.calls():
        np.testing.assert_array_equal(run_call(dev, call), call.want, err_msg='%s %s' % (name, call.jobs))


def test_two_runs_are_equal(dev):
    for name in ('separate_call_0', 'mixed_call'):
        call = dict(RC.calls())[name]
        a, b = run_call(dev, call), run_call(dev, call)
        assert np.array_equal(a, b) and np.array_equal(a, call.want)


def test_call_is_graph_capturable(dev):
    import t2onet_amd.functional as T
    call = dict(RC.calls())['separate_call_1']
    photo, src = torch.from_numpy(call.photo).to(dev), torch.from_numpy(call.src).to(dev)
    out = torch.from_numpy(call.out).to(dev)

    def run():
        return T.refine_u8(photo, src, call.jobs, out=out)
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


@pytest.mark.parametrize('name', ['separate_call_0', 'mixed_call'])
def test_four_launches_whatever_the_number_of_jobs(dev, name):
    import t2onet_amd.functional as T
    from torch.profiler import profile, ProfilerActivity
    call = dict(RC.calls())[name]
    photo, buf = torch.from_numpy(call.photo).to(dev), torch.from_numpy(call.src).to(dev)
    out = buf if call.src is call.out else torch.from_numpy(call.out).to(dev)
    for jobs in (call.jobs, call.jobs[:1]):
        T.refine_u8(photo, buf.clone(), jobs, out=None if out is buf else out)
        torch.cuda.synchronize()
        work = buf.clone()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            T.refine_u8(photo, work, jobs, out=None if out is buf else out)
            torch.cuda.synchronize()
        ks = _kernels(prof)
        print('refine_u8, %d jobs: %s' % (len(jobs), ks))
        assert sorted(re.findall(r'k_refine_\w+', k)[0] for k, _ in ks if 'k_refine_' in k) == ['k_refine_cols2', 'k_refine_cols4', 'k_refine_rows1', 'k_refine_rows3'], ks
        assert sum(c for _, c in ks) == T.REFINE_LAUNCHES == 4, ks


def test_wrapper_refuses_before_any_launch(dev):
    import t2onet_amd.functional as T
    photo = torch.zeros(128, dtype=torch.uint8, device=dev)
    buf = torch.full((64,), 7, dtype=torch.uint8, device=dev)
    out = torch.zeros(64, dtype=torch.uint8, device=dev)

    def one(po=0, so=0, oo=0, h=4, w=4, r=2, E=26):
        return [(po, so, oo, h, w, r, E)]
    for bad in (81, -1):
        with pytest.raises(ValueError, match='reads outside the 128-byte photo buffer'):
            T.refine_u8(photo, buf, one(po=bad), out=out)
    for bad in (49, -1):
        with pytest.raises(ValueError, match='reads outside the 64-byte buffer'):
            T.refine_u8(photo, buf, one(so=bad), out=out)
    with pytest.raises(ValueError, match='writes outside the 64-byte output'):
        T.refine_u8(photo, buf, one(oo=49), out=out)
    with pytest.raises(ValueError, match='writes outside the 8-byte output'):
        T.refine_u8(photo, buf, one(), out=torch.zeros(8, dtype=torch.uint8, device=dev))
    for oo in (-1, -16, -100):
        with pytest.raises(ValueError, match='writes before the output'):
            T.refine_u8(photo, buf, one(oo=oo), out=out)
        with pytest.raises(ValueError, match='writes before the output'):
            T.refine_u8(photo, buf, one(oo=oo))
    with pytest.raises(ValueError, match='photo and buffer must be'):
        T.refine_u8(photo.cpu(), buf, one(), out=out)
    with pytest.raises(ValueError, match='photo and buffer must be'):
        T.refine_u8(photo, buf.to(torch.int8), one(), out=out)
    with pytest.raises(ValueError, match='out must be'):
        T.refine_u8(photo, buf, one(), out=out.cpu())
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.refine_u8(photo, buf, [], out=out)
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.refine_u8(photo, buf, [(0, 0, 4 * k, 2, 2, 1, 1) for k in range(5)], out=out)
    # what only the library can tell: its text arrives in the exception
    with pytest.raises(ValueError, match='radius'):
        T.refine_u8(photo, buf, one(r=65), out=out)
    with pytest.raises(ValueError, match='eps2'):
        T.refine_u8(photo, buf, one(E=0), out=out)
    with pytest.raises(ValueError, match='positive'):
        T.refine_u8(photo, buf, one(h=0), out=out)
    with pytest.raises(ValueError, match='destinations overlap'):
        T.refine_u8(photo, buf, one() + one(oo=15), out=out)
    with pytest.raises(ValueError, match='overlaps a photo'):
        T.refine_u8(photo, photo, one(so=100, oo=40))
    assert not out.any().item() and not photo.any().item() and (buf == 7).all().item()       # nothing was launched on the way


# ---------------------------------------------------------------- edit_image(refine=...) against the oracle-refined planes handed over as masks
@pytest.fixture(scope='module')
def cli(dev, tmp_path_factory):
    from t2onet_amd.edit import request_to_idx
    from t2onet_amd.edit_cli import load_vocab
    tmp_path = tmp_path_factory.mktemp('edit_refine')
    opt, model, ckpt, vocab_dir, imgs = _setup(tmp_path, dev)
    x = request_to_idx(REQUEST, load_vocab(vocab_dir, 1, opt.dataset), opt)
    return {'tmp': tmp_path, 'opt': opt, 'model': model, 'imgs': imgs, 'x': x,
            'common': ['--request', REQUEST, '--checkpoint', ckpt, '--vocab_dir', vocab_dir, '--multi_img']}


def count_launches(monkeypatch):
    import t2onet_amd.functional as T
    taken = []
    for name in ('select_u8', 'refine_u8', 'feather_u8', 'replay_u8', 'replay_u8_masked', 'replay_u8_stencils'):
        monkeypatch.setattr(T, name, (lambda f, n: lambda *a, **k: (taken.append(n), f(*a, **k))[1])(getattr(T, name), name))
    return taken


def test_edit_image_refine_equals_the_oracle_planes_as_masks(cli, monkeypatch):
    from t2onet_amd.edit import edit_image
    model, img, x = cli['model'], cli['imgs'][0], cli['x']
    rule, other = oracle_plane(RULE, img), oracle_plane(OTHER, img)
    taken = count_launches(monkeypatch)
    # plain: select, then refine, then the replay
    plain = _same(edit_image(model, img, x, select={'all': RULE}, refine=4), edit_image(model, img, x, masks={'all': RC.oracle(img, rule, 4, 26)}))
    print('operators chosen:', plain[1])
    assert len(plain[1]) >= 1, 'the seeded actor chose END first: the test would show nothing'
    assert taken[:2] == ['select_u8', 'refine_u8'] and taken.count('refine_u8') == 1 and 'feather_u8' not in taken and len(taken) == 4
    assert not torch.equal(plain[0], edit_image(model, img, x, select={'all': RULE})[0])        # the refinement shows
    # with feather, two planes with their own radius and eps: select, refine, feather
    del taken[:]
    _same(edit_image(model, img, x, select={'all': RULE, 5: OTHER}, refine={'all': (2, 0.1), 5: 7}, feather={5: 2.5, 'all': 1.5}),
          edit_image(model, img, x, masks={'all': RC.oracle(img, rule, 2, 650), 5: RC.oracle(img, other, 7, 26)}, feather={5: 2.5, 'all': 1.5}))
    assert taken[:3] == ['select_u8', 'refine_u8', 'feather_u8'] and taken.count('refine_u8') == 1 and len(taken) == 6
    # on a proxy smaller than the photo
    _same(edit_image(model, img, x, proxy_short=32, select={'all': RULE}, refine=(4, 0.02)),
          edit_image(model, img, x, proxy_short=32, masks={'all': RC.oracle(img, rule, 4, 26)}))
    # painted planes are refined where they were uploaded, behind the photo
    painted = FC.plane('vedge', 48, 80)
    del taken[:]
    _same(edit_image(model, img, x, masks={'all': painted}, refine=4, feather=2),
          edit_image(model, img, x, masks={'all': RC.oracle(img, painted, 4, 26)}, feather=2))
    assert taken[:2] == ['refine_u8', 'feather_u8'] and taken[3] == 'feather_u8' and len(taken) == 5
    # refine=None launches what it launched before
    del taken[:]
    edit_image(model, img, x, select={'all': RULE})
    assert taken[0] == 'select_u8' and 'refine_u8' not in taken and len(taken) == 2


def _blocks(h, w):
    m = np.zeros((h, w), np.uint8)
    m[h // 4:3 * h // 4, w // 8:w // 2] = 255
    m[h // 8:h // 2, 5 * w // 8:7 * w // 8] = 255
    return m


def test_edit_cli_refine_and_apply_cli_on_other_photos(cli, dev, monkeypatch):
    from PIL import Image
    import t2onet_amd.functional as T
    from t2onet_amd import apply_cli, edit_cli
    from t2onet_amd.data import ACTIONS
    tmp, img = cli['tmp'], cli['imgs'][0]
    # --mask blocks.png --refine 4 equals --mask with the oracle's plane
    blocks = _blocks(48, 80)
    Image.fromarray(blocks).save(str(tmp / 'blocks.png'))
    Image.fromarray(RC.oracle(img, blocks, 4, 26)).save(str(tmp / 'snapped.png'))
    info = edit_cli.main(['--img', str(tmp / 'noise0.png'), '--save_dir', str(tmp / 'refined'), '--mask', str(tmp / 'blocks.png'), '--refine', '4'] + cli['common'])
    want = edit_cli.main(['--img', str(tmp / 'noise0.png'), '--save_dir', str(tmp / 'snapped'), '--mask', str(tmp / 'snapped.png')] + cli['common'])
    assert info['operations'] == want['operations'] and info['refine'] == {'all': [4, 0.02]} and 'refine' not in want
    names = [n for n, _ in info['operations']]
    print('operators chosen:', names)
    assert names, 'the seeded actor chose END first: the test would show nothing'
    files = sorted(f for f in os.listdir(str(tmp / 'refined' / 'noise0')) if f.endswith('.png'))
    assert files == sorted(f for f in os.listdir(str(tmp / 'snapped' / 'noise0')) if f.endswith('.png')) and len(files) == 2 + len(names)
    for f in files:
        np.testing.assert_array_equal(_png(str(tmp / 'refined' / 'noise0' / f)), _png(str(tmp / 'snapped' / 'noise0' / f)), err_msg=f)
    # a record with 'select' and 'refine', applied to two other photos of two other sizes
    rules = {'all': 'lum:0.3:1:0.2+!linear:0,0:1,1', 'tone': 'hue:320:40:60+radial:0.5,0.5:0.1:0.7'}
    flags = [a for name, text in rules.items() for a in ('--select', text if name == 'all' else '%s=%s' % (name, text))]
    info = edit_cli.main(['--img', str(tmp / 'noise0.png'), '--save_dir', str(tmp / 'edited')] + cli['common'] + flags
                         + ['--refine', '3', '--refine', 'tone=6:0.1', '--feather', 'tone=2'])
    record = str(tmp / 'edited' / 'noise0' / 'noise0.json')
    with open(record) as f:
        saved = json.load(f)
    assert saved == [json.loads(json.dumps(info))]
    assert saved[0]['select'] == rules and saved[0]['refine'] == {'all': [3, 0.02], 'tone': [6, 0.1]} and saved[0]['feather'] == {'tone': 2.0}
    request, ops, params = apply_cli.parse_record(saved)
    snap, sigma = {'all': (3, 26), 'tone': (6, 650)}, {'all': 0.0, 'tone': 2.0}
    photos = {'p.png': SC.picture(40, 60, 11), 'q.png': SC.picture(33, 90, 12)}
    for name, a in photos.items():
        Image.fromarray(a).save(str(tmp / name))
    taken = count_launches(monkeypatch)
    infos = apply_cli.main(['--record', record, '--img'] + [str(tmp / n) for n in photos] + ['--save_dir', str(tmp / 'applied'), '--multi_img'])
    used = {('tone' if ACTIONS[op] == 'tone' else 'all') for op in ops}
    groups = 1 if 2 * len(used) <= 4 else 2
    assert taken.count('select_u8') == taken.count('refine_u8') == groups and len([t for t in taken if t.startswith('replay')]) == groups
    order = [t for t in taken if not t.startswith('replay')][:3]
    assert order[:2] == ['select_u8', 'refine_u8'] and ('tone' not in used or order[2] == 'feather_u8')
    par = np.zeros((8, 24), np.float32)
    par[:len(ops)] = params
    for new, (name, a) in zip(infos, photos.items()):
        stem, (h, w) = name[:-4], a.shape[:2]
        planes, slot = [], {}
        for key in sorted(used):
            m = RC.oracle(a, oracle_plane(edit_cli.parse_select_terms(rules[key]), a), *snap[key])      # under THIS photo's luminance
            slot[key] = len(planes)
            planes.append(FC.oracle(m, sigma[key]))
        mask_of = [slot['tone' if ACTIONS[op] == 'tone' else 'all'] for op in ops]
        jobs = [(0, k * a.size, h, w, ops[:k + 1], mask_of[:k + 1]) for k in range(len(ops))]
        want = T.replay_u8_any(torch.from_numpy(a.reshape(-1).copy()).to(dev), jobs, torch.from_numpy(par).to(dev)[None].repeat(len(ops), 1, 1),
                               torch.from_numpy(np.concatenate([p.reshape(-1) for p in planes])).to(dev),
                               [k * h * w for k in range(len(planes))]).cpu().numpy().reshape(len(ops), h, w, 3)
        d = tmp / 'applied' / stem
        assert np.array_equal(_png(str(d / name)), want[-1])
        for k in range(len(ops)):
            assert np.array_equal(_png(str(d / ('%d_inference_%s' % (k + 1, name)))), want[k]), (name, k)
        with open(str(d / (stem + '.json'))) as f:
            again = json.load(f)
        assert again == [json.loads(json.dumps(new))]
        assert again[0]['select'] == rules and again[0]['refine'] == {'all': [3, 0.02], 'tone': [6, 0.1]} and again[0]['record'] == record
        assert apply_cli.parse_refine(again) == {'all': (3, 0.02), 'tone': (6, 0.1)}                   # a written record can be applied again
