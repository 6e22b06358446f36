"""The 8-bit replay kernel (t2o_replay.hip) and the edit command on the GPU.  The kernel's bytes must EQUAL those of the
path that existed before it -- resize_u8 at the picture's own size, t2o_op_fwd per step with every image materialised,
to_u8_hwc -- with no tolerance: both sides run the same device functions.  Cases and the oracle condition are shared with
tests/test_replay_cpu.py (tests/replay_cases.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import replay_cases as RC

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A
NAMES = sorted(RC.LISTS)
_reference = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def case(i):
    """Job i of a call: list i mod 20 on a size that walks through RC.SIZES -> (key, img, ops, params)."""
    name, s = NAMES[i % len(NAMES)], (i + i // len(NAMES)) % len(RC.SIZES)
    ops, forced = RC.LISTS[name]
    h, w = RC.SIZES[s]
    return (name, s), RC.picture(h, w, 100 + s), ops, RC.params_for(ops, 7 + i % len(NAMES), forced)


def materialised(dev, img, ops, params):
    """What existed before the kernel: / 255 on the device, one t2o_op_fwd per step, * 255 truncated."""
    import t2onet_amd.functional as T
    x = T.resize_u8([img], img.shape[:2], device=dev)
    for k, op in enumerate(ops):
        if op >= 0:
            x = T.operator_apply(op, x, torch.from_numpy(params[k:k + 1]).to(dev))
    return T.to_u8_hwc(x)[0].cpu().numpy()


def reference(dev, i):
    key, img, ops, params = case(i)
    if key not in _reference:
        _reference[key] = materialised(dev, img, ops, params)
    return _reference[key]


def run_jobs(dev, cases, share_first_source=False, graph=False):
    """One replay_u8 call over `cases` = [(img, ops, params)], sources and destinations packed at odd byte offsets with
    gaps; returns the per-job pictures after checking that every byte outside them still holds the sentinel."""
    import t2onet_amd.functional as T
    src_parts, jobs, pos_s, pos_o = [], [], 1, 3
    for i, (img, ops, params) in enumerate(cases):
        h, w = img.shape[:2]
        if share_first_source and i == 1:
            assert img.shape == cases[0][0].shape and np.array_equal(img, cases[0][0])
            so = jobs[0][0]
        else:
            so = pos_s
            src_parts.append((so, img))
            pos_s += img.size + 1 + 2 * (i % 2)                # the next source starts at another residue modulo 4
        jobs.append((so, pos_o, h, w, list(ops)))
        pos_o += img.size + 1 + 2 * ((i + 1) % 2)
    src = np.full(pos_s + 4, 0xC3, np.uint8)
    for so, img in src_parts:
        src[so:so + img.size] = img.reshape(-1)
    src_d = torch.from_numpy(src).to(dev)
    out_d = torch.full((pos_o + 4,), SENTINEL, dtype=torch.uint8, device=dev)
    par_d = torch.from_numpy(np.stack([p for _, _, p in cases])).to(dev)
    if graph:
        eager = T.replay_u8(src_d, jobs, par_d, out=out_d).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            T.replay_u8(src_d, jobs, par_d, out=out_d)           # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            T.replay_u8(src_d, jobs, par_d, out=out_d)
        out_d.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_d, eager)
    else:
        assert T.replay_u8(src_d, jobs, par_d, out=out_d) is out_d
    out = out_d.cpu().numpy()
    untouched = np.ones(out.size, bool)
    pictures = []
    for so, oo, h, w, _ in jobs:
        untouched[oo:oo + 3 * h * w] = False
        pictures.append(out[oo:oo + 3 * h * w].reshape(h, w, 3))
    assert (out[untouched] == SENTINEL).all(), 'a byte outside every job was written'
    return pictures


@pytest.mark.parametrize('J', [1, 7, 64])
def test_bytes_equal_the_materialised_path(dev, J):
    first = {1: 33, 7: 3, 64: 3}[J]                              # job 33: sharp_middle on 31 x 33; job 3: clamp_chain on 37 x 50
    idx = [first + i for i in range(J)]
    cases = [case(i)[1:] for i in idx]
    refs = [reference(dev, i) for i in idx]
    if J > 1:                                                    # job 1 reads job 0's source with its own list
        img0 = cases[0][0]
        ops, params = cases[1][1], cases[1][2]
        cases[1] = (img0, ops, params)
        refs[1] = materialised(dev, img0, ops, params)
    got = run_jobs(dev, cases, share_first_source=J > 1)
    for i, g, r in zip(idx, got, refs):
        np.testing.assert_array_equal(g, r, err_msg='job %d: %s' % (i, (case(i)[0],)))
    if J == 64:
        assert {case(i)[0][0] for i in idx} == set(NAMES) and {case(i)[0][1] for i in idx} == set(range(len(RC.SIZES)))


@pytest.mark.parametrize('name,size', [('sharp_middle', 3), ('steps8', 5)])
def test_bytes_within_the_oracle_interval(dev, name, size):
    ops, forced = RC.LISTS[name]
    img = RC.picture(*RC.SIZES[size], 100 + size)
    params = RC.params_for(ops, 31, forced)
    got, = run_jobs(dev, [(img, ops, params)])
    RC.assert_in_interval(got, RC.oracle(img, ops, params), name)


def test_call_is_graph_capturable(dev):
    cases = [case(i)[1:] for i in (11, 16, 33, 9)]
    got = run_jobs(dev, cases, graph=True)
    for i, g in zip((11, 16, 33, 9), got):
        np.testing.assert_array_equal(g, reference(dev, i))


def test_wrapper_refuses_what_the_library_refuses(dev):
    import t2onet_amd.functional as T
    src = torch.zeros(64, dtype=torch.uint8, device=dev)
    par = torch.zeros(1, 8, 24, device=dev)
    with pytest.raises(NotImplementedError, match='inpaint'):
        T.replay_u8(src, [(0, 0, 4, 4, [4])], par)
    with pytest.raises(NotImplementedError, match='sharpness'):
        T.replay_u8(src, [(0, 0, 4, 4, [6, 6])], par)
    with pytest.raises(ValueError, match='steps'):
        T.replay_u8(src, [(0, 0, 4, 4, [0] * 9)], par)
    with pytest.raises(ValueError, match='64'):
        T.replay_u8(src, [(0, 0, 4, 4, [0])] * 65, torch.zeros(65, 8, 24, device=dev))
    with pytest.raises(ValueError, match='outside'):
        T.replay_u8(src, [(20, 0, 4, 4, [0])], par)


# ---------------------------------------------------------------- the edit command, end to end
WORDS = ['<NULL>', '<START>', '<END>', '<UNK>', 'make', 'the', 'photo', 'brighter', 'and', 'more', 'colorful', 'please']
MODEL_SEED = 13            # a random-weight actor's choices are near-uniform; with this seed END is its LEAST likely first token
                           # (0.086 against 0.094 in the fp32 oracle), so at least one operator is chosen


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


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def test_edit_cli_end_to_end(dev, tmp_path):
    import t2onet_amd.functional as T
    from t2onet_amd import edit_cli
    from t2onet_amd.edit import request_to_idx
    from t2onet_amd.train import select_end_images
    opt, model, ckpt, vocab_dir, imgs = _setup(tmp_path, dev)
    request = 'Please make the photo brighter and more colorful'
    save_dir = str(tmp_path / 'out')
    common = ['--request', request, '--checkpoint', ckpt, '--vocab_dir', vocab_dir, '--save_dir', save_dir, '--multi_img']
    # (1) the picture is its own proxy: files, record, and pixels of a direct episode on the same tensor
    info = edit_cli.main(['--img', str(tmp_path / 'noise0.png')] + common)
    d = os.path.join(save_dir, 'noise0')
    with open(os.path.join(d, 'noise0.json')) as f:
        saved = json.load(f)
    assert saved == [json.loads(json.dumps(info))] and saved[0]['request'] == request
    n = len(saved[0]['operations'])
    print('operators chosen:', [name for name, _ in saved[0]['operations']])
    assert n >= 1, 'the seeded actor chose END first: the test would show nothing'
    files = sorted(os.listdir(d))
    assert files == sorted(['noise0.json', 'noise0.png', 'noise0_in.png'] + ['%d_inference_noise0.png' % (k + 1) for k in range(n)])
    assert np.array_equal(_png(os.path.join(d, 'noise0_in.png')), imgs[0])
    x = request_to_idx(request, edit_cli.load_vocab(vocab_dir, 1), opt)
    img_t = T.resize_u8([imgs[0]], (48, 80), device=dev)
    with torch.no_grad():
        _, pred_imgs, pred_ops, pred_params = model.episode_forward(x.to(dev), img_t, None, reinforce_sample=False,
                                                                    lengths=(x != opt.null_id).sum(1))
    want = T.to_u8_hwc(select_end_images(pred_imgs, pred_ops, opt.end_id))[0].cpu().numpy()
    np.testing.assert_array_equal(_png(os.path.join(d, 'noise0.png')), want)
    for k in range(1, n + 1):
        np.testing.assert_array_equal(_png(os.path.join(d, '%d_inference_noise0.png' % k)),
                                      T.to_u8_hwc(pred_imgs[:, k - 1])[0].cpu().numpy(), err_msg='step %d' % k)
    ops = [edit_cli.ACTIONS.index(name) for name, _ in saved[0]['operations']]
    assert ops == [int(o) - 3 for o in pred_ops[0, :n].tolist()]
    for (name, values), par in zip(saved[0]['operations'], pred_params):
        assert values == par[0, :len(values)].tolist() and len(values) == edit_cli.ACT2PN[name]
    # (2) a resized proxy decides, the native bytes are edited: the result is replay_u8 of the record's own list
    edit_cli.main(['--img', str(tmp_path / 'noise1.png'), '--proxy_short', '32'] + common)
    d = os.path.join(save_dir, 'noise1')
    with open(os.path.join(d, 'noise1.json')) as f:
        rec = json.load(f)[0]
    ops = [edit_cli.ACTIONS.index(name) for name, _ in rec['operations']]
    table = torch.zeros(1, 8, 24)
    for k, (_, values) in enumerate(rec['operations']):
        table[0, k, :len(values)] = torch.tensor(values)
    got = T.replay_u8(torch.from_numpy(imgs[1].reshape(-1)).to(dev), [(0, 0, 48, 80, ops)], table.to(dev))
    np.testing.assert_array_equal(_png(os.path.join(d, 'noise1.png')), got.view(48, 80, 3).cpu().numpy())
    assert len([f for f in os.listdir(d) if '_inference_' in f]) == len(ops)
