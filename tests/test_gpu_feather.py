"""The mask feather kernels (t2o_feather.hip) and the edit command's --feather on the GPU.  Integers throughout: the
kernels' bytes must EQUAL the int64 oracle's (tests/feather_cases.py, shared with tests/test_feather_cpu.py), guard bytes
around every destination plane included."""
import json
import os

import numpy as np
import pytest
import torch

from tests import feather_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def calls(dev):
    return FC.calls()                                                # the oracle runs once per plane, here


def run_call(dev, call):
    """One feather_u8 call on device copies of the call's buffers -> the destination buffer afterwards."""
    import t2onet_amd.functional as T
    src = torch.from_numpy(call.src).to(dev)
    if call.out is call.src:
        assert T.feather_u8(src, call.jobs) is src                  # out = None: inside the buffer
        return src.cpu().numpy()
    out = torch.from_numpy(call.out).to(dev)
    assert T.feather_u8(src, call.jobs, out=out) is out
    assert np.array_equal(src.cpu().numpy(), call.src)              # the source is only read
    return out.cpu().numpy()


def test_bytes_equal_the_oracle(dev, calls):
    """Every size x sigma, four jobs of mixed size and sigma to a call, into a separate output and in place, and the call
    whose source overlaps another job's destination."""
    assert any(c.out is c.src for _, c in calls) and any(c.out is not c.src for _, c in calls)
    assert {j[0] % 4 for _, c in calls for j in c.jobs} == {j[1] % 4 for _, c in calls for j in c.jobs} == {0, 1, 2, 3}
    assert {(j[2], j[3]) for _, c in calls for j in c.jobs} >= set(FC.SIZES)
    assert {j[4] for _, c in calls for j in c.jobs} >= set(FC.SIGMAS)
    for name, call in calls:
        np.testing.assert_array_equal(run_call(dev, call), call.want, err_msg='%s %s' % (name, call.jobs))


def test_two_runs_are_equal(dev, calls):
    for name, call in calls[:3] + calls[-1:]:
        assert np.array_equal(run_call(dev, call), run_call(dev, call)), name


def test_call_is_graph_capturable(dev, calls):
    import t2onet_amd.functional as T
    name, call = next((n, c) for n, c in calls if c.out is not c.src and len(c.jobs) == 4)
    src = torch.from_numpy(call.src).to(dev)
    out = torch.from_numpy(call.out).to(dev)

    def run():
        return T.feather_u8(src, call.jobs, out=out)
    eager = run().clone()
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
    assert torch.equal(out, eager)
    np.testing.assert_array_equal(out.cpu().numpy(), call.want, err_msg=name)


def test_wrapper_refuses_what_the_library_refuses(dev):
    import t2onet_amd.functional as T
    buf = torch.zeros(64, dtype=torch.uint8, device=dev)
    one = (0, 16, 4, 4, 2.0)
    with pytest.raises(ValueError, match='sigma'):
        T.feather_u8(buf, [(0, 16, 4, 4, -1.0)])
    with pytest.raises(ValueError, match='sigma'):
        T.feather_u8(buf, [(0, 16, 4, 4, 64.5)])
    with pytest.raises(ValueError, match='sigma'):
        T.feather_u8(buf, [(0, 16, 4, 4, float('nan'))])
    with pytest.raises(ValueError, match='positive'):
        T.feather_u8(buf, [(0, 16, 0, 4, 2.0)])
    with pytest.raises(ValueError, match='overlap'):
        T.feather_u8(buf, [one, (32, 20, 4, 4, 2.0)])
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.feather_u8(buf, [])
    with pytest.raises(ValueError, match='1 to 4 jobs'):
        T.feather_u8(buf, [(0, 8 * k, 2, 2, 1.0) for k in range(5)])
    with pytest.raises(ValueError, match='reads outside the 64-byte buffer'):
        T.feather_u8(buf, [(49, 0, 4, 4, 2.0)])
    with pytest.raises(ValueError, match='reads outside the 64-byte buffer'):
        T.feather_u8(buf, [(-1, 0, 4, 4, 2.0)])
    with pytest.raises(ValueError, match='writes outside the 64-byte output'):
        T.feather_u8(buf, [(0, 49, 4, 4, 2.0)])
    with pytest.raises(ValueError, match='writes outside the 8-byte output'):
        T.feather_u8(buf, [one], out=torch.zeros(8, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='out must be'):
        T.feather_u8(buf, [one], out=torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(ValueError, match='buffer must be'):
        T.feather_u8(buf.to(torch.int8), [one])
    assert not buf.any().item()                                      # nothing was launched on the way


# ---------------------------------------------------------------- the edit command with --feather, end to end
# the seeded 48 x 80 set-up of tests/test_gpu_replay_mask.py
WORDS = ['<NULL>', '<START>', '<END>', '<UNK>', 'make', 'the', 'photo', 'brighter', 'and', 'more', 'colorful', 'please']
MODEL_SEED = 13            # as tests/test_gpu_replay.py: END is the seeded actor's least likely first token
REQUEST = 'Please make the photo brighter and more colorful'
SIGMA = 3


def blocks_mask(h, w, T=32):
    """0/255 rectangles with edges at 31, 32 and 33 in both directions (tests/replay_mask_cases.py's `blocks`)."""
    m = np.zeros((h, w), np.uint8)
    m[:T - 1, :T + 1] = 255
    m[T:, T - 1:] = 255
    m[T + 1:, :T] = 255
    return m


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
    tmp_path = tmp_path_factory.mktemp('edit_feather')
    opt, model, ckpt, vocab_dir, imgs = _setup(tmp_path, dev)
    blocks = blocks_mask(48, 80)
    Image.fromarray(blocks).save(str(tmp_path / 'blocks.png'))
    Image.fromarray(FC.oracle(blocks, SIGMA)).save(str(tmp_path / 'soft.png'))          # the oracle's feathering of blocks.png
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


@pytest.mark.parametrize('proxy', [[], ['--proxy_short', '32']], ids=['own_proxy', 'proxy_short_32'])
def test_edit_cli_feather_equals_the_feathered_mask_file(cli, proxy):
    """--mask blocks.png --feather 3 writes the bytes of --mask soft.png, soft.png being the oracle's feathering of
    blocks.png: the planes are feathered on the device before the proxy's decision and before the native replay."""
    tag = 'p' if proxy else 'n'
    hard_file, soft_file = str(cli['tmp'] / 'blocks.png'), str(cli['tmp'] / 'soft.png')
    d_f, rec_f = _run(cli, 'noise0', 'feathered_' + tag, proxy + ['--mask', hard_file, '--feather', str(SIGMA)])
    d_s, rec_s = _run(cli, 'noise0', 'soft_' + tag, proxy + ['--mask', soft_file])
    d_h, rec_h = _run(cli, 'noise0', 'hard_' + tag, proxy + ['--mask', hard_file])
    print('operators chosen:', [name for name, _ in rec_f['operations']])
    assert len(rec_f['operations']) >= 1, 'the seeded actor chose END first: the test would show nothing'
    assert rec_f['feather'] == {'all': 3.0} and rec_f['masks'] == {'all': hard_file}
    assert 'feather' not in rec_s and 'feather' not in rec_h
    assert rec_f['operations'] == rec_s['operations']
    files = sorted(f for f in os.listdir(d_f) if f.endswith('.png'))
    assert files == sorted(f for f in os.listdir(d_s) if f.endswith('.png')) and 'noise0.png' in files
    assert len([f for f in files if '_inference_' in f]) == len(rec_f['operations'])
    for f in files:
        np.testing.assert_array_equal(_png(os.path.join(d_f, f)), _png(os.path.join(d_s, f)), err_msg=f)
    assert not np.array_equal(_png(os.path.join(d_f, 'noise0.png')), _png(os.path.join(d_h, 'noise0.png')))      # the soft edge shows
