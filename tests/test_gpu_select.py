"""The selection kernel (t2o_select.hip), edit_image's `select`, the edit command's --select and the local apply command on
the GPU.  Integers throughout: the kernel's bytes must EQUAL the int64 oracle's (tests/select_cases.py, shared with
tests/test_select_cpu.py), guard bytes around every destination plane included; everything downstream must equal what
the same planes give when they are handed over as painted masks."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import feather_cases as FC
from tests import select_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def run_call(dev, call):
    import t2onet_amd.functional as T
    src = torch.from_numpy(call.src).to(dev)
    out = torch.from_numpy(call.out).to(dev)
    assert T.select_u8(src, call.jobs, out=out) is out
    assert np.array_equal(src.cpu().numpy(), call.src)              # the source is only read
    return out.cpu().numpy()


def test_bytes_equal_the_oracle(dev):
    """Every size x selection of the case list, four jobs of mixed size to a call, every residue of both offsets, the
    call whose jobs share a photo."""
    for name, call in SC.calls():
        np.testing.assert_array_equal(run_call(dev, call), call.want, err_msg='%s %s %s' % (name, call.names, call.jobs))


def test_out_is_allocated_to_fit_and_two_runs_are_equal(dev):
    import t2onet_amd.functional as T
    name, call = SC.calls()[0]
    src = torch.from_numpy(call.src).to(dev)
    a, b = T.select_u8(src, call.jobs), T.select_u8(src, call.jobs)
    assert a.numel() == b.numel() == max(j[1] + j[2] * j[3] for j in call.jobs) and a.dtype == torch.uint8 and a.device == src.device
    for so, oo, h, w, terms in call.jobs:                            # (the bytes between the planes of a fresh tensor are nobody's)
        assert np.array_equal(a[oo:oo + h * w].cpu().numpy(), call.want[oo:oo + h * w])
        assert torch.equal(a[oo:oo + h * w], b[oo:oo + h * w])


def test_call_is_graph_capturable(dev):
    import t2onet_amd.functional as T
    call = dict(SC.calls())['shared_photo']
    src = torch.from_numpy(call.src).to(dev)
    out = torch.from_numpy(call.out).to(dev)

    def run():
        return T.select_u8(src, call.jobs, out=out)
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


def test_wrapper_refuses_before_any_launch(dev):
    import t2onet_amd.functional as T
    buf = torch.zeros(128, dtype=torch.uint8, device=dev)
    out = torch.zeros(64, dtype=torch.uint8, device=dev)
    lum = ('lum', 0, 0, 255, 0)                                      # would write 255 everywhere

    def one(*terms, h=4, w=4, so=0, oo=0):
        return [(so, oo, h, w, list(terms))]
    with pytest.raises(ValueError, match='reads outside the 128-byte source'):
        T.select_u8(buf, one(lum, so=81), out=out)
    with pytest.raises(ValueError, match='reads outside the 128-byte source'):
        T.select_u8(buf, one(lum, so=-1), out=out)
    with pytest.raises(ValueError, match='plane term outside the 128-byte source'):
        T.select_u8(buf, one(lum, ('plane', 0, 113)), out=out)
    with pytest.raises(ValueError, match='plane term outside the 128-byte source'):
        T.select_u8(buf, one(('plane', 0, -1)), out=out)
    with pytest.raises(ValueError, match='writes outside the 64-byte output'):
        T.select_u8(buf, one(lum, oo=49), out=out)
    with pytest.raises(ValueError, match='writes before the output'):
        T.select_u8(buf, one(lum, oo=-1), out=out)
    for oo in (-1, -16, -100):                                       # out=None: refused before a tensor of 15, 0 or -84 bytes is asked for
        with pytest.raises(ValueError, match='writes before the output'):
            T.select_u8(buf, one(lum, oo=oo))
    with pytest.raises(ValueError, match='writes outside the 8-byte output'):
        T.select_u8(buf, one(lum), out=torch.zeros(8, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='src must be'):
        T.select_u8(buf.cpu(), one(lum), out=out)
    with pytest.raises(ValueError, match='src must be'):
        T.select_u8(buf.to(torch.int8), one(lum), out=out)
    with pytest.raises(ValueError, match='out must be'):
        T.select_u8(buf, one(lum), out=out.cpu())
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.select_u8(buf, [], out=out)
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.select_u8(buf, [(0, 4 * k, 2, 2, [lum]) for k in range(5)], out=out)
    # what only the library can tell: its text arrives in the exception
    with pytest.raises(ValueError, match='n_terms'):
        T.select_u8(buf, one(), out=out)
    with pytest.raises(ValueError, match='positive'):
        T.select_u8(buf, one(lum, h=0), out=out)
    with pytest.raises(ValueError, match='lum / sat'):
        T.select_u8(buf, one(('lum', 0, 9, 8, 0)), out=out)
    with pytest.raises(ValueError, match='destinations overlap'):
        T.select_u8(buf, one(lum) + one(lum, oo=15), out=out)
    with pytest.raises(ValueError, match='overlaps a photo'):
        T.select_u8(buf, one(lum, oo=40), out=buf)
    with pytest.raises(ValueError, match='overlaps a plane term'):
        T.select_u8(buf, one(lum, ('plane', 0, 100), oo=90), out=buf)
    assert not out.any().item() and not buf.any().item()            # nothing was launched on the way


# ---------------------------------------------------------------- edit_image(select=...) against the same planes handed over as masks
# the seeded 48 x 80 set-up of tests/test_gpu_replay_mask.py
WORDS = ['<NULL>', '<START>', '<END>', '<UNK>', 'make', 'the', 'photo', 'brighter', 'and', 'more', 'colorful', 'please']
MODEL_SEED = 13            # as tests/test_gpu_replay.py: END is the seeded actor's least likely first token
REQUEST = 'Please make the photo brighter and more colorful'
RULE = [('lum', 0.3, 1.0, 0.2), ('!linear', 0.0, 0.0, 1.0, 1.0)]
OTHER = [('hue', 320, 40, 60), ('radial', 0.5, 0.5, 0.1, 0.7)]


def _setup(tmp_path, dev):
    import t2onet_amd
    from PIL import Image
    from t2onet_amd.actor import Actor
    vocab_dir = tmp_path / 'language'
    vocab_dir.mkdir()
    with open(str(vocab_dir / 'FiveK_vocabs_sess_1.json'), 'w') as f:
        json.dump(WORDS + ['word%d' % i for i in range(918 - len(WORDS))], f)
    with open(str(vocab_dir / 'FiveK_operator_vocabs_sess_1.json'), 'w') as f:
        json.dump(['<NULL>', '<START>', '<END>'] + ['op%d' % i for i in range(8)], f)
    opt = t2onet_amd.default_options(vocab_dir=str(vocab_dir))
    torch.manual_seed(MODEL_SEED)
    model = Actor(opt)
    ckpt = tmp_path / 'model.pth'
    torch.save(model.state_dict(), str(ckpt))
    imgs = []
    for k in range(2):
        img = np.random.default_rng(40 + k).integers(0, 256, (48, 80, 3), dtype=np.uint8)
        Image.fromarray(img).save(str(tmp_path / ('noise%d.png' % k)))
        imgs.append(img)
    return opt, model.to(dev).eval(), str(ckpt), str(vocab_dir), imgs


@pytest.fixture(scope='module')
def cli(dev, tmp_path_factory):
    from t2onet_amd.edit import request_to_idx
    from t2onet_amd.edit_cli import load_vocab
    tmp_path = tmp_path_factory.mktemp('edit_select')
    opt, model, ckpt, vocab_dir, imgs = _setup(tmp_path, dev)
    x = request_to_idx(REQUEST, load_vocab(vocab_dir, 1, opt.dataset), opt)
    return {'tmp': tmp_path, 'opt': opt, 'model': model, 'imgs': imgs, 'x': x,
            'common': ['--request', REQUEST, '--checkpoint', ckpt, '--vocab_dir', vocab_dir, '--multi_img']}


def oracle_plane(user_terms, img, painted=None):
    """The plane of a selection in user units on `img` by the oracle, multiplied by a painted plane when one is given."""
    h, w = img.shape[:2]
    terms = SC.round_units(user_terms, h, w)
    if painted is None:
        return SC.selection(terms, img)
    return SC.selection(terms + [('plane', 0, 0)], img, painted.reshape(-1))


def _same(a, b):
    assert a[1] == b[1] and torch.equal(a[2], b[2]) and torch.equal(a[0], b[0])
    return a


def count_launches(monkeypatch):
    """Every wrapper that launches for a local edit, counted the way tests/test_gpu_replay_stencils.py counts the replays."""
    import t2onet_amd.functional as T
    taken = []
    for name in ('select_u8', 'feather_u8', 'replay_u8', 'replay_u8_masked', 'replay_u8_stencils'):
        monkeypatch.setattr(T, name, (lambda f, n: lambda *a, **k: (taken.append(n), f(*a, **k))[1])(getattr(T, name), name))
    return taken


def test_edit_image_select_equals_the_oracle_planes_as_masks(cli, monkeypatch):
    from t2onet_amd.edit import edit_image
    model, img, x = cli['model'], cli['imgs'][0], cli['x']
    taken = count_launches(monkeypatch)
    plain = _same(edit_image(model, img, x, select={'all': RULE}), edit_image(model, img, x, masks={'all': oracle_plane(RULE, img)}))
    print('operators chosen:', plain[1])
    assert len(plain[1]) >= 1, 'the seeded actor chose END first: the test would show nothing'
    assert taken[0] == 'select_u8' and taken.count('select_u8') == 1 and 'feather_u8' not in taken and len(taken) == 3
    assert not torch.equal(plain[0], edit_image(model, img, x)[0])                             # the selection shows
    # two planes, one of them feathered: still one select_u8 launch
    del taken[:]
    two = {'all': RULE, 5: OTHER}
    _same(edit_image(model, img, x, select=two, feather={5: 2.5, 'all': 0}),
          edit_image(model, img, x, masks={'all': oracle_plane(RULE, img), 5: oracle_plane(OTHER, img)}, feather={5: 2.5}))
    assert taken[:3] == ['select_u8', 'feather_u8', taken[2]] and taken.count('select_u8') == 1 and len(taken) == 5
    _same(edit_image(model, img, x, select={'all': RULE}, feather=3), edit_image(model, img, x, masks={'all': oracle_plane(RULE, img)}, feather=3))
    # a painted mask under the same key is intersected; a key with only a painted mask keeps it
    painted = FC.oracle(FC.plane('vedge', 48, 80), 4)
    other = FC.plane('hedge', 48, 80)
    del taken[:]
    _same(edit_image(model, img, x, select={'all': RULE}, masks={'all': painted, 0: other}),
          edit_image(model, img, x, masks={'all': oracle_plane(RULE, img, painted), 0: other}))
    assert taken.count('select_u8') == 1
    # on a proxy smaller than the photo
    _same(edit_image(model, img, x, proxy_short=32, select={'all': RULE}),
          edit_image(model, img, x, proxy_short=32, masks={'all': oracle_plane(RULE, img)}))


class StubActor(torch.nn.Module):
    """What edit_image needs of the actor (tests/test_gpu_replay_stencils.py): a parameter, `opt`, a fixed decision."""

    def __init__(self, ops, params):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.opt = types.SimpleNamespace(null_id=0, end_id=2)
        self.ops, self.params = ops, params

    def episode_forward(self, x, img, mask_dict, reinforce_sample=False, lengths=None):
        dev = self.anchor.device
        vocab = [self.opt.end_id if op is None else op + 3 for op in self.ops]
        return None, None, torch.tensor([vocab], device=dev), [torch.from_numpy(p[None]).to(dev) for p in self.params]


def test_edit_image_select_with_a_list_that_repeats_the_sharpness(dev, monkeypatch):
    from tests import replay_cases as RC
    from t2onet_amd.edit import edit_image
    img = np.random.default_rng(40).integers(0, 256, (48, 80, 3), dtype=np.uint8)
    ops = [6, 0, 6]
    params = RC.params_for(ops + [-1], 4)
    model = StubActor(ops + [None], params[:4]).to(dev)
    x = torch.ones(1, 4, dtype=torch.long)
    taken = count_launches(monkeypatch)
    got = edit_image(model, img, x, select={'all': RULE, 6: OTHER})
    assert taken == ['select_u8', 'replay_u8_stencils'] and got[1] == ops and tuple(got[0].shape) == (3, 48, 80, 3)
    _same(got, edit_image(model, img, x, masks={'all': oracle_plane(RULE, img), 6: oracle_plane(OTHER, img)}))


def test_a_call_without_select_launches_what_it_launched_before(dev, monkeypatch):
    from tests import replay_cases as RC
    from t2onet_amd.edit import edit_image
    img = np.random.default_rng(41).integers(0, 256, (48, 80, 3), dtype=np.uint8)
    ops = [0, 6]
    model = StubActor(ops + [None], RC.params_for(ops + [-1], 4)[:3]).to(dev)
    x = torch.ones(1, 4, dtype=torch.long)
    plane = FC.plane('vedge', 48, 80)
    taken = count_launches(monkeypatch)
    edit_image(model, img, x)
    assert taken == ['replay_u8']
    del taken[:]
    edit_image(model, img, x, masks={'all': plane})
    assert taken == ['replay_u8_masked']
    del taken[:]
    edit_image(model, img, x, masks={'all': plane}, feather=2)
    assert taken == ['feather_u8', 'replay_u8_masked']


# ---------------------------------------------------------------- edit_cli --select writes the rule, apply_cli carries it to other photos
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def test_edit_cli_select_and_apply_cli_on_other_photos(cli, dev, monkeypatch):
    from PIL import Image
    import t2onet_amd.functional as T
    from t2onet_amd import apply_cli, edit_cli
    from t2onet_amd.data import ACTIONS
    tmp = cli['tmp']
    rules = {'all': 'lum:0.3:1:0.2+!linear:0,0:1,1', 'tone': 'hue:320:40:60+radial:0.5,0.5:0.1:0.7', 'color': '!sat:0:0.3:0.2'}
    # an unnamed sigma stands for every plane, a named one wins over it -- in edit_cli and, from the record, in apply_cli
    FEATHER, sigma = ['--feather', '1.5', '--feather', 'tone=2'], {'all': 1.5, 'tone': 2.0, 'color': 1.5}
    flags = [a for name, text in rules.items() for a in ('--select', text if name == 'all' else '%s=%s' % (name, text))]
    info = edit_cli.main(['--img', str(tmp / 'noise0.png'), '--save_dir', str(tmp / 'edited')] + cli['common'] + flags + FEATHER)
    record = str(tmp / 'edited' / 'noise0' / 'noise0.json')
    with open(record) as f:
        saved = json.load(f)
    assert saved == [json.loads(json.dumps(info))]
    assert saved[0]['select'] == rules and saved[0]['feather'] == {'all': 1.5, 'tone': 2.0} and 'masks' not in saved[0]
    names = [n for n, _ in saved[0]['operations']]
    print('operators chosen:', names)
    assert names, 'the seeded actor chose END first: the test would show nothing'
    request, ops, params = apply_cli.parse_record(saved)
    # the edited photo is the one that the oracle's planes give as --mask files
    masks = []
    for name, text in rules.items():
        Image.fromarray(oracle_plane(edit_cli.parse_select_terms(text), cli['imgs'][0])).save(str(tmp / (name + '_plane.png')))
        masks += ['--mask', ('' if name == 'all' else name + '=') + str(tmp / (name + '_plane.png'))]
    painted = edit_cli.main(['--img', str(tmp / 'noise0.png'), '--save_dir', str(tmp / 'painted')] + cli['common'] + masks + FEATHER)
    assert painted['operations'] == info['operations'] and 'select' not in painted
    files = sorted(f for f in os.listdir(str(tmp / 'painted' / 'noise0')) if f.endswith('.png'))
    assert files == sorted(f for f in os.listdir(str(tmp / 'edited' / 'noise0')) if f.endswith('.png')) and len(files) == 2 + len(names)
    for f in files:
        np.testing.assert_array_equal(_png(str(tmp / 'edited' / 'noise0' / f)), _png(str(tmp / 'painted' / 'noise0' / f)), err_msg=f)
    # two other photos, two other sizes
    photos = {'p.png': SC.picture(40, 60, 11), 'q.png': SC.picture(33, 90, 12)}
    for name, a in photos.items():
        Image.fromarray(a).save(str(tmp / name))
    taken = count_launches(monkeypatch)
    infos = apply_cli.main(['--record', record, '--img'] + [str(tmp / n) for n in photos] + ['--save_dir', str(tmp / 'applied'), '--multi_img'])
    used = {('tone' if ACTIONS[op] == 'tone' else 'color' if ACTIONS[op] == 'color' else 'all') for op in ops}
    groups = 1 if 2 * len(used) <= 4 else 2
    assert taken.count('select_u8') == groups and len([t for t in taken if t.startswith('replay')]) == groups
    assert taken.count('feather_u8') == groups                                          # every plane is feathered: 'all' reaches the named ones
    par = np.zeros((8, 24), np.float32)
    par[:len(ops)] = params
    for new, (name, a) in zip(infos, photos.items()):
        stem, (h, w) = name[:-4], a.shape[:2]
        planes, slot = [], {}
        for key in sorted(used):
            m = oracle_plane(edit_cli.parse_select_terms(rules[key]), a)
            slot[key] = len(planes)
            planes.append(FC.oracle(m, sigma[key]))
        mask_of = [slot['tone' if ACTIONS[op] == 'tone' else 'color' if ACTIONS[op] == 'color' else 'all'] for op in ops]
        jobs = [(0, k * a.size, h, w, ops[:k + 1], mask_of[:k + 1]) for k in range(len(ops))]
        assert T.replay_u8_pick(jobs) in ('replay_u8_masked', 'replay_u8_stencils')
        want = T.replay_u8_any(torch.from_numpy(a.reshape(-1).copy()).to(dev), jobs, torch.from_numpy(par).to(dev)[None].repeat(len(ops), 1, 1),
                               torch.from_numpy(np.concatenate([p.reshape(-1) for p in planes])).to(dev),
                               [k * h * w for k in range(len(planes))]).cpu().numpy().reshape(len(ops), h, w, 3)
        d = tmp / 'applied' / stem
        assert np.array_equal(_png(str(d / name)), want[-1])
        for k in range(len(ops)):
            assert np.array_equal(_png(str(d / ('%d_inference_%s' % (k + 1, name)))), want[k]), (name, k)
        assert not np.array_equal(want[-1], T.replay_u8_any(torch.from_numpy(a.reshape(-1).copy()).to(dev), [(0, 0, h, w, ops)],
                                                            torch.from_numpy(par).to(dev)[None]).cpu().numpy().reshape(h, w, 3))      # local, not global
        with open(str(d / (stem + '.json'))) as f:
            again = json.load(f)
        assert again == [json.loads(json.dumps(new))]
        assert again[0]['select'] == rules and again[0]['feather'] == {'all': 1.5, 'tone': 2.0} and again[0]['record'] == record
        assert apply_cli.parse_local(again) == (rules, {'all': 1.5, 'tone': 2.0})                       # a written record can be applied again
