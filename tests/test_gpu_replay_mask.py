"""The masked 8-bit replay kernel (t2o_replay_mask.hip) and the edit command's --mask on the GPU.  The kernel's bytes must
EQUAL those of the materialised path -- resize_u8 at the picture's own size, operator_apply per step with the mask as
(1,1,h,w) fp32 = byte / 255 and every image materialised, to_u8_hwc -- with no tolerance: both sides run the same device
functions.  Lists, patterns and the oracle are shared with tests/test_replay_mask_cpu.py (tests/replay_mask_cases.py).

A call takes at most 4 mask planes, shared by its jobs, and a plane is bytes at an offset read with the JOB's own (h, w).
So every call here carries the same table -- soft, blocks, one_pixel and border at the largest size of RC.SIZES -- and a
job of that size sees those four patterns, while a smaller job reads a prefix of the plane it names: all 0 in front of
one_pixel's pixel (`zeros`), all 255 inside border's first row (`full`), other 0/255 or random bytes elsewhere.  The
pattern a job really sees is worked out from its bytes (seen_pattern)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import replay_cases as RC
from tests import replay_mask_cases as MC

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A
BIG = RC.SIZES[5]
TABLE = ['soft', 'blocks', 'one_pixel', 'border']
PLANES = [MC.mask(p, BIG[0], BIG[1]) for p in TABLE]
MASK_BUF, MASK_OFFSETS = MC.pack_masks(PLANES)
_reference = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def plane_of(slot, h, w):
    """What a job of size (h, w) reads when it names table entry `slot`."""
    assert h * w <= BIG[0] * BIG[1]
    return MASK_BUF[MASK_OFFSETS[slot]:MASK_OFFSETS[slot] + h * w].reshape(h, w)


def seen_pattern(m):
    h, w = m.shape
    for p in ('zeros', 'full', 'blocks', 'one_pixel', 'border'):
        if np.array_equal(m, MC.mask(p, h, w)):
            return p
    return 'soft' if len(np.unique(m)) > 2 else 'other'


def case(i):
    """Job i of a call: list i mod 17 on a size and with table entries that walk along ->
    (key, img, ops, params, mask_of, slots)."""
    name, s = MC.NAMES[i % len(MC.NAMES)], (i + i // len(MC.NAMES)) % len(RC.SIZES)
    ops, mask_of = MC.LISTS[name]
    slots = [(i + i // 4) % 4, (i + i // 4 + 1) % 4][:max(mask_of) + 1]
    h, w = RC.SIZES[s]
    return (name, s, tuple(slots)), RC.picture(h, w, 100 + s), ops, RC.params_for(ops, 7 + i % len(MC.NAMES)), mask_of, slots


def materialised(dev, img, ops, params, mask_of, slots):
    """The path the kernel replaces: / 255 on the device, one t2o_op_fwd per step WITH its mask, * 255 truncated."""
    import t2onet_amd.functional as T
    h, w = img.shape[:2]
    x = T.resize_u8([img], (h, w), device=dev)
    for k, op in enumerate(ops):
        if op >= 0:
            m = None if mask_of[k] < 0 else MC.mask_f32(plane_of(slots[mask_of[k]], h, w)).to(dev)
            x = T.operator_apply(op, x, torch.from_numpy(params[k:k + 1]).to(dev), m)
    return T.to_u8_hwc(x)[0].cpu().numpy()


def reference(dev, i):
    key, img, ops, params, mask_of, slots = case(i)
    if key not in _reference:
        _reference[key] = materialised(dev, img, ops, params, mask_of, slots)
    return _reference[key]


def run_jobs(dev, cases, share_first_source=False, graph=False, mask_buf=MASK_BUF):
    """One replay_u8_masked call over `cases` = [(img, ops, params, mask_of, slots)], sources and destinations packed at
    odd byte offsets with gaps; returns the per-job pictures after checking that every byte outside them still holds the
    sentinel."""
    import t2onet_amd.functional as T
    src_parts, jobs, pos_s, pos_o = [], [], 1, 3
    for i, (img, ops, params, mask_of, slots) in enumerate(cases):
        h, w = img.shape[:2]
        if share_first_source and i == 1:
            assert img.shape == cases[0][0].shape and np.array_equal(img, cases[0][0])
            so = jobs[0][0]
        else:
            so = pos_s
            src_parts.append((so, img))
            pos_s += img.size + 1 + 2 * (i % 2)                # the next source starts at another residue modulo 4
        jobs.append((so, pos_o, h, w, list(ops), [-1 if m < 0 else slots[m] for m in mask_of]))
        pos_o += img.size + 1 + 2 * ((i + 1) % 2)
    src = np.full(pos_s + 4, 0xC3, np.uint8)
    for so, img in src_parts:
        src[so:so + img.size] = img.reshape(-1)
    src_d = torch.from_numpy(src).to(dev)
    msk_d = torch.from_numpy(mask_buf).to(dev)
    out_d = torch.full((pos_o + 4,), SENTINEL, dtype=torch.uint8, device=dev)
    par_d = torch.from_numpy(np.stack([c[2] for c in cases])).to(dev)

    def call():
        return T.replay_u8_masked(src_d, jobs, par_d, msk_d, MASK_OFFSETS, out=out_d)
    if graph:
        eager = call().clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()                                               # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        out_d.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_d, eager)
    else:
        assert call() is out_d
    out = out_d.cpu().numpy()
    untouched = np.ones(out.size, bool)
    pictures = []
    for so, oo, h, w, _, _ in jobs:
        untouched[oo:oo + 3 * h * w] = False
        pictures.append(out[oo:oo + 3 * h * w].reshape(h, w, 3))
    assert (out[untouched] == SENTINEL).all(), 'a byte outside every job was written'
    return pictures


@pytest.mark.parametrize('J', [1, 7, 64])
def test_bytes_equal_the_materialised_path(dev, J):
    idx = [3 + i for i in range(J)]
    cases = [case(i)[1:] for i in idx]
    if J == 1:                                                   # a masked step in front of the sharpness on the largest size, under `blocks`
        ops, mask_of = MC.LISTS['sharp_middle_front']
        cases = [(RC.picture(*BIG, 105), ops, RC.params_for(ops, 11), mask_of, [TABLE.index('blocks')])]
        refs = [materialised(dev, *cases[0])]
    else:
        refs = [reference(dev, i) for i in idx]
    if J > 1:                                                    # job 1 reads job 0's source under job 0's mask with its own list
        img0, slots0 = cases[0][0], cases[0][4]
        _, ops, params, mask_of, slots = cases[1]
        slots = [slots0[0], (slots0[0] + 1) % 4][:len(slots)]
        cases[1] = (img0, ops, params, mask_of, slots)
        refs[1] = materialised(dev, img0, ops, params, mask_of, slots)
    got = run_jobs(dev, cases, share_first_source=J > 1)
    for i, g, r in zip(idx, got, refs):
        np.testing.assert_array_equal(g, r, err_msg='job %d: %s' % (i, (case(i)[0],)))
    seen = set()
    for img, ops, _, mask_of, slots in cases:
        seen |= {seen_pattern(plane_of(slots[m], *img.shape[:2])) for m in mask_of if m >= 0}
    if J == 1:
        assert seen == {'blocks'}
    if J == 64:
        assert {case(i)[0][0] for i in idx} == set(MC.NAMES) and {case(i)[0][1] for i in idx} == set(range(len(RC.SIZES)))
        assert seen >= set(MC.PATTERNS), seen
        # tiles whose mask window is all zero (the tile skip) are among the jobs: one_pixel on the largest size
        assert any(s == 5 and TABLE[slots[0]] == 'one_pixel' for (_, s, slots) in (case(i)[0] for i in idx))


@pytest.mark.parametrize('name,size,patterns', [('sharp_middle_front', 3, ['soft']), ('sharp_middle_self', 3, ['soft']),
                                                ('sharp_middle_behind', 3, ['soft']), ('two_masks', 5, ['blocks', 'border'])])
def test_bytes_within_the_oracle_interval(dev, name, size, patterns):
    """A soft-masked sharp_middle on 37 x 50 and the two-mask list on 33 x 65 against the fp32 oracle."""
    ops, mask_of = MC.LISTS[name]
    h, w = RC.SIZES[size]
    img = RC.picture(h, w, 100 + size)
    params = RC.params_for(ops, 31)
    slots = [TABLE.index(p) for p in patterns]
    planes = [plane_of(s, h, w) for s in slots]
    assert size != 5 or [seen_pattern(p) for p in planes] == patterns
    assert size != 3 or seen_pattern(planes[0]) == 'soft'
    got, = run_jobs(dev, [(img, ops, params, mask_of, slots)])
    RC.assert_in_interval(got, MC.oracle(img, ops, params, mask_of, planes), name)


@pytest.mark.parametrize('value', [255, 0])
def test_degenerate_masks_are_the_unmasked_kernel(dev, value):
    """255 on every masked step: the bytes of replay_u8 of the same list.  0: those of replay_u8 with the masked steps
    made the identity -- steps = 0 where every step names a mask."""
    import t2onet_amd.functional as T
    buf = np.full_like(MASK_BUF, value)
    cases, plain, zero_steps = [], [], []
    for n, name in enumerate(MC.NAMES):
        ops, mask_of = MC.LISTS[name]
        for s in (3, 5):
            img = RC.picture(*RC.SIZES[s], 100 + s)
            cases.append((img, ops, RC.params_for(ops, 40 + n), mask_of, [n % 4, (n + 1) % 4][:max(mask_of) + 1]))
            plain.append(list(ops) if value else [-1 if m >= 0 else op for op, m in zip(ops, mask_of)])
            zero_steps.append(not value and all(m >= 0 or op < 0 for op, m in zip(ops, mask_of)))
    got = run_jobs(dev, cases, mask_buf=buf)
    assert any(zero_steps) == (value == 0)
    src = torch.from_numpy(np.concatenate([c[0].reshape(-1) for c in cases])).to(dev)
    jobs, pos = [], 0
    for (img, _, _, _, _), ops, z in zip(cases, plain, zero_steps):
        jobs.append((pos, pos, img.shape[0], img.shape[1], [] if z else ops))
        pos += img.size
    par = torch.from_numpy(np.stack([c[2] for c in cases])).to(dev)
    want = T.replay_u8(src, jobs, par).cpu().numpy()
    for g, (so, _, h, w, _), name in zip(got, jobs, [n for n in MC.NAMES for _ in (3, 5)]):
        np.testing.assert_array_equal(g, want[so:so + 3 * h * w].reshape(h, w, 3), err_msg=name)


def test_call_is_graph_capturable(dev):
    cases = [case(i)[1:] for i in (5, 16, 33, 9)]                   # masks of one_pixel (tile skip), soft, blocks, border
    got = run_jobs(dev, cases, graph=True)
    for i, g in zip((5, 16, 33, 9), got):
        np.testing.assert_array_equal(g, reference(dev, i))


def test_wrapper_refuses_what_the_library_refuses(dev):
    import t2onet_amd.functional as T
    src = torch.zeros(64, dtype=torch.uint8, device=dev)
    msk = torch.zeros(32, dtype=torch.uint8, device=dev)
    par = torch.zeros(1, 8, 24, device=dev)
    with pytest.raises(NotImplementedError, match='inpaint'):
        T.replay_u8_masked(src, [(0, 0, 4, 4, [4], [0])], par, msk, [0])
    with pytest.raises(NotImplementedError, match='sharpness'):
        T.replay_u8_masked(src, [(0, 0, 4, 4, [6, 6], [0, -1])], par, msk, [0])
    with pytest.raises(ValueError, match='steps'):
        T.replay_u8_masked(src, [(0, 0, 4, 4, [0] * 9, [0] * 9)], par, msk, [0])
    with pytest.raises(ValueError, match='64'):
        T.replay_u8_masked(src, [(0, 0, 4, 4, [0], [0])] * 65, torch.zeros(65, 8, 24, device=dev), msk, [0])
    with pytest.raises(ValueError, match='mask index'):
        T.replay_u8_masked(src, [(0, 0, 4, 4, [0], [1])], par, msk, [0])
    with pytest.raises(ValueError, match='mask index'):
        T.replay_u8_masked(src, [(0, 0, 4, 4, [0], [0])], par, None, [])
    with pytest.raises(ValueError, match='4 masks'):
        T.replay_u8_masked(src, [(0, 0, 4, 4, [0], [0])], par, msk, [0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match='outside the 64-byte source'):
        T.replay_u8_masked(src, [(20, 0, 4, 4, [0], [0])], par, msk, [0])
    with pytest.raises(ValueError, match='outside the 32-byte mask buffer'):
        T.replay_u8_masked(src, [(0, 0, 4, 4, [0], [0])], par, msk, [17])
    with pytest.raises(ValueError, match='masks must be'):
        T.replay_u8_masked(src, [(0, 0, 4, 4, [0], [0])], par, msk.cpu(), [0])
    # a call without any mask is the unmasked kernel's
    img = torch.from_numpy(RC.picture(4, 4, 1).reshape(-1)).to(dev)
    assert torch.equal(T.replay_u8_masked(img, [(0, 0, 4, 4, [0], [-1])], par + 0.25, None, []),
                       T.replay_u8(img, [(0, 0, 4, 4, [0])], par + 0.25))


# ---------------------------------------------------------------- the edit command with --mask, end to end
WORDS = ['<NULL>', '<START>', '<END>', '<UNK>', 'make', 'the', 'photo', 'brighter', 'and', 'more', 'colorful', 'please']
MODEL_SEED = 13            # as tests/test_gpu_replay.py: END is the seeded actor's least likely first token
REQUEST = 'Please make the photo brighter and more colorful'


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
    from PIL import Image
    tmp_path = tmp_path_factory.mktemp('edit_mask')
    opt, model, ckpt, vocab_dir, imgs = _setup(tmp_path, dev)
    for p in ('blocks', 'zeros'):
        Image.fromarray(MC.mask(p, 48, 80)).save(str(tmp_path / (p + '.png')))
    return {'tmp': tmp_path, 'opt': opt, 'model': model, 'imgs': imgs, 'vocab_dir': vocab_dir,
            'common': ['--request', REQUEST, '--checkpoint', ckpt, '--vocab_dir', vocab_dir, '--multi_img']}


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def _run(cli, name, save, extra):
    from t2onet_amd import edit_cli
    save_dir = str(cli['tmp'] / save)
    info = edit_cli.main(['--img', str(cli['tmp'] / (name + '.png')), '--save_dir', save_dir] + cli['common'] + extra)
    d = os.path.join(save_dir, name)
    with open(os.path.join(d, name + '.json')) as f:
        saved = json.load(f)
    assert saved == [json.loads(json.dumps(info))]
    return d, saved[0]


def _episode(cli, dev, img, mask_dict):
    import t2onet_amd.functional as T
    from t2onet_amd import edit_cli
    from t2onet_amd.edit import request_to_idx
    opt = cli['opt']
    x = request_to_idx(REQUEST, edit_cli.load_vocab(cli['vocab_dir'], 1), opt)
    img_t = T.resize_u8([img], img.shape[:2], device=dev)
    with torch.no_grad():
        _, pred_imgs, pred_ops, _ = cli['model'].episode_forward(x.to(dev), img_t, mask_dict, reinforce_sample=False,
                                                                 lengths=(x != opt.null_id).sum(1))
    return pred_imgs, pred_ops


def test_edit_cli_mask_equals_the_masked_episode(cli, dev):
    """(1) the picture is its own proxy: the files are the pixels of a direct episode with the same mask_dict."""
    import t2onet_amd.functional as T
    from t2onet_amd.actor import OP_MASK
    from t2onet_amd.train import select_end_images
    mask_file = str(cli['tmp'] / 'blocks.png')
    d, rec = _run(cli, 'noise0', 'out1', ['--mask', mask_file])
    assert rec['masks'] == {'all': mask_file}
    n = len(rec['operations'])
    print('operators chosen:', [name for name, _ in rec['operations']])
    assert n >= 1, 'the seeded actor chose END first: the test would show nothing'
    m = torch.from_numpy(MC.mask('blocks', 48, 80).astype(np.float32) / np.float32(255.0)).unsqueeze(0).to(dev)
    mask_dict = [{str(i): [m] for i, allowed in enumerate(OP_MASK) if allowed and i >= 3}]
    pred_imgs, pred_ops = _episode(cli, dev, cli['imgs'][0], mask_dict)
    want = T.to_u8_hwc(select_end_images(pred_imgs, pred_ops, cli['opt'].end_id))[0].cpu().numpy()
    np.testing.assert_array_equal(_png(os.path.join(d, 'noise0.png')), want)
    for k in range(1, n + 1):
        np.testing.assert_array_equal(_png(os.path.join(d, '%d_inference_noise0.png' % k)),
                                      T.to_u8_hwc(pred_imgs[:, k - 1])[0].cpu().numpy(), err_msg='step %d' % k)
    # the mask did something: outside it the photo only went through the two conversions
    keep = MC.mask('blocks', 48, 80) == 0
    unedited = T.to_u8_hwc(T.resize_u8([cli['imgs'][0]], (48, 80), device=dev))[0].cpu().numpy()
    assert keep.any() and np.array_equal(want[keep], unedited[keep])
    assert not np.array_equal(want[~keep], unedited[~keep])


def _replay_of_record(dev, rec, img, mask):
    import t2onet_amd.functional as T
    from t2onet_amd import edit_cli
    ops = [edit_cli.ACTIONS.index(name) for name, _ in rec['operations']]
    table = torch.zeros(1, 8, 24)
    for k, (_, values) in enumerate(rec['operations']):
        table[0, k, :len(values)] = torch.tensor(values)
    src = torch.from_numpy(img.reshape(-1)).to(dev)
    if mask is None:
        return T.replay_u8(src, [(0, 0, 48, 80, ops)], table.to(dev)).view(48, 80, 3).cpu().numpy(), ops
    got = T.replay_u8_masked(src, [(0, 0, 48, 80, ops, [0] * len(ops))], table.to(dev), torch.from_numpy(mask.reshape(-1)).to(dev), [0])
    return got.view(48, 80, 3).cpu().numpy(), ops


def test_edit_cli_mask_with_a_resized_proxy(cli, dev):
    """(2) a 32-row proxy decides under the nearest-neighbour mask, the native bytes are edited under the native mask."""
    d, rec = _run(cli, 'noise1', 'out2', ['--proxy_short', '32', '--mask', str(cli['tmp'] / 'blocks.png')])
    want, ops = _replay_of_record(dev, rec, cli['imgs'][1], MC.mask('blocks', 48, 80))
    np.testing.assert_array_equal(_png(os.path.join(d, 'noise1.png')), want)
    assert len([f for f in os.listdir(d) if '_inference_' in f]) == len(ops) and 'masks' in rec


def test_edit_cli_zero_mask_leaves_the_photo(cli, dev):
    """(3) a mask of zeros: the photo through the two conversions, whatever the record lists."""
    import t2onet_amd.functional as T
    d, rec = _run(cli, 'noise0', 'out3', ['--mask', 'brightness=' + str(cli['tmp'] / 'zeros.png'), '--mask', str(cli['tmp'] / 'zeros.png')])
    assert rec['masks'] == {'brightness': str(cli['tmp'] / 'zeros.png'), 'all': str(cli['tmp'] / 'zeros.png')}
    want = T.to_u8_hwc(T.resize_u8([cli['imgs'][0]], (48, 80), device=dev))[0].cpu().numpy()
    np.testing.assert_array_equal(_png(os.path.join(d, 'noise0.png')), want)
    for f in os.listdir(d):
        if '_inference_' in f:
            np.testing.assert_array_equal(_png(os.path.join(d, f)), want)


def test_edit_cli_without_mask_is_unchanged(cli, dev):
    """(4) no --mask: the unmasked episode's pixels, replay_u8's bytes, and a record without a 'masks' key."""
    import t2onet_amd.functional as T
    from t2onet_amd.train import select_end_images
    d, rec = _run(cli, 'noise0', 'out4', [])
    assert sorted(rec) == ['input', 'operations', 'output', 'request']
    n = len(rec['operations'])
    assert sorted(os.listdir(d)) == sorted(['noise0.json', 'noise0.png', 'noise0_in.png'] + ['%d_inference_noise0.png' % (k + 1) for k in range(n)])
    pred_imgs, pred_ops = _episode(cli, dev, cli['imgs'][0], None)
    want = T.to_u8_hwc(select_end_images(pred_imgs, pred_ops, cli['opt'].end_id))[0].cpu().numpy()
    np.testing.assert_array_equal(_png(os.path.join(d, 'noise0.png')), want)
    np.testing.assert_array_equal(_replay_of_record(dev, rec, cli['imgs'][0], None)[0], want)
    for k in range(1, n + 1):
        np.testing.assert_array_equal(_png(os.path.join(d, '%d_inference_noise0.png' % k)),
                                      T.to_u8_hwc(pred_imgs[:, k - 1])[0].cpu().numpy(), err_msg='step %d' % k)
