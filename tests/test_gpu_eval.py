"""The evaluation kernels and loops on the GPU: functional.eval_metrics / end_select_var_mean against the oracle, fp64 and
the existing per-metric calls; evaluate.test_on_device / test_variance_on_device against the reference's goldens and the
.item() loops; no host synchronisation inside the loop; the test command end to end."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_eval_cpu import SHAPES, VAR_SHAPES, check_metrics, expected_metrics, expected_variance, metric_case, var_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _gpu(arrays, dev):
    return [torch.from_numpy(a).to(dev) for a in arrays]


@pytest.mark.parametrize('T', [1, 5])
@pytest.mark.parametrize('shape', SHAPES + [(1, 3, 397, 600)])
def test_eval_metrics_against_the_oracle_and_the_single_calls(dev, shape, T):
    import t2onet_amd.functional as F
    inp, imgs, first, tgt = metric_case(shape, T)
    want = expected_metrics(inp, imgs, first, tgt)
    d_inp, d_tgt, d_first = _gpu([inp, tgt, first], dev)
    d_imgs = _gpu(imgs, dev)
    got = F.eval_metrics(d_inp, d_imgs, d_first, d_tgt)
    assert got.shape == (4,)
    print(shape, T, got.tolist(), want)
    check_metrics(got.cpu().numpy(), want)
    # the calls it replaces, on the gathered images
    out = torch.stack(d_imgs, 1)[torch.arange(shape[0], device=dev), d_first]
    single = [F.l1_loss(d_inp, d_tgt).item(), F.l1_loss(out, d_tgt).item(), F.ssim(d_inp, d_tgt).item(), F.ssim(out, d_tgt).item()]
    check_metrics(got.cpu().numpy(), single)
    assert torch.equal(F.eval_metrics(d_inp, d_imgs, d_first, d_tgt), got)                 # the same bits from run to run
    # into row 3 of a table: the other rows stay
    table = torch.full((5, 4), -7.0, device=dev)
    F.eval_metrics(d_inp, d_imgs, d_first, d_tgt, out=table[3])
    assert torch.equal(table[3], got) and bool((table[[0, 1, 2, 4]] == -7.0).all())
    # a step outside the table counts as the last one
    wild = torch.full_like(d_first, T + 2)
    assert torch.equal(F.eval_metrics(d_inp, d_imgs, wild, d_tgt), F.eval_metrics(d_inp, d_imgs, torch.full_like(d_first, T - 1), d_tgt))
    plain = F.eval_metrics(d_inp, d_imgs, d_first, d_tgt, with_ssim=False)
    assert torch.equal(plain[:2], got[:2]) and plain[2:].tolist() == [0.0, 0.0]


def test_eval_wrappers_refuse_what_the_kernels_cannot_take(dev):
    import t2onet_amd.functional as F
    img = torch.zeros(1, 3, 8, 8, device=dev)
    first = torch.zeros(1, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match='no CPU'):
        F.eval_metrics(img, [img], first, img, out=torch.zeros(4))                         # the table row too
    with pytest.raises(RuntimeError, match='no CPU'):
        F.end_select_var_mean([[img], [img]], [first, first], out=torch.zeros(1))
    with pytest.raises(ValueError):
        F.eval_metrics(img, [img[:, :, :4]], first, img)
    with pytest.raises(ValueError):
        F.eval_metrics(img, [img], first.int(), img)
    with pytest.raises(RuntimeError, match='T <= 8'):
        F.eval_metrics(img, [img] * 9, first, img)
    with pytest.raises(RuntimeError, match='fewer than two'):
        F.end_select_var_mean([[img]], [first])


@pytest.mark.parametrize('R,B,row', VAR_SHAPES)
def test_end_select_var_mean_against_fp64_and_torch(dev, R, B, row):
    import t2onet_amd.functional as F
    lists, firsts = var_case(R, B, row)
    want = expected_variance(lists, firsts)
    d_lists = [_gpu(l, dev) for l in lists]
    d_firsts = _gpu(firsts, dev)
    got = F.end_select_var_mean(d_lists, d_firsts)
    ends = [torch.stack(l, 1)[torch.arange(B, device=dev), f] for l, f in zip(d_lists, d_firsts)]
    ref = torch.var(torch.cat(ends), 0).mean().item()
    print((R, B, row), got.item(), ref, want)
    np.testing.assert_allclose(got.item(), want, rtol=1e-5)
    np.testing.assert_allclose(got.item(), ref, rtol=1e-5)
    assert torch.equal(F.end_select_var_mean(d_lists, d_firsts), got)
    table = torch.full((3, 1), -7.0, device=dev)
    F.end_select_var_mean(d_lists, d_firsts, out=table[1])
    assert table[:, 0].tolist() == [-7.0, got.item(), -7.0]
    if row % 4 == 0:          # images that start 4 bytes into their storage: the narrow loads, the same value
        shifted = [[torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(B, row) for t in l] for l in d_lists]
        np.testing.assert_allclose(F.end_select_var_mean(shifted, d_firsts).item(), want, rtol=1e-5)


@pytest.fixture(scope='module')
def eval_setup(dev):
    from oracle import synth
    from tests.test_gpu_actor_extra import L, make_model2
    model, opt = make_model2(dev)
    batches = [(synth.images(2, 48, 64, 151 + k), synth.images(2, 48, 64, 161 + k), synth.requests(2, L, 171 + k), ['req'] * 2)
               for k in range(3)]
    return model, opt, batches


def test_on_device_loop_matches_the_golden_and_the_item_loop(dev, eval_setup, golden_dir, monkeypatch):
    from t2onet_amd import evaluate
    model, opt, batches = eval_setup
    extra2 = np.load(os.path.join(golden_dir, 'extra2.npz'))
    avg_init, avg, metrics = evaluate.test_on_device(model, batches, opt, is_test=True, device=dev, verbose=False)
    print(avg_init, avg, metrics)
    assert abs(avg_init - float(extra2['eval_avg_init_dist'])) < 1e-6
    assert abs(avg - float(extra2['eval_avg_dist'])) < 1e-5
    seen = {}
    orig = evaluate.ImageEvaluator.eval
    monkeypatch.setattr(evaluate.ImageEvaluator, 'eval', lambda self: seen.update(orig(self)) or seen)
    evaluate.test(model, batches, opt, is_test=True, device=dev, verbose=False)
    assert sorted(seen) == sorted(metrics) == ['in_L1', 'in_SSIM', 'out_L1', 'out_SSIM']
    for key, v in seen.items():
        assert abs(metrics[key] - v) <= 1e-5 * abs(v) + 1e-6, (key, metrics[key], v)
    # is_test=False: the same two distances, no metrics; a loader without a length (the table doubles)
    res = evaluate.test_on_device(model, iter(batches), opt, device=dev, verbose=False)
    assert res[2] is None and abs(res[0] - avg_init) < 1e-7 and abs(res[1] - avg) < 1e-7


def test_variance_on_device_matches_the_reference(dev, golden_dir):
    from oracle import synth
    from t2onet_amd import evaluate
    from tests.test_gpu_actor_extra import L, make_model2
    var = np.load(os.path.join(golden_dir, 'variance.npz'))
    model, opt = make_model2(dev)
    batches = [(synth.images(1, 48, 64, 181 + k), synth.images(1, 48, 64, 191 + k), synth.requests(1, L, 201 + k), ['req']) for k in range(3)]
    vocab2id = {str(t): i for i, t in enumerate(var['var_vocab'])}
    got = evaluate.test_variance_on_device(model, batches, opt, [str(t) for t in var['var_texts']], vocab2id, device=dev, verbose=False)
    print(got, float(var['var_avg']))
    assert abs(got - float(var['var_avg'])) < 1e-5
    with pytest.raises(ValueError):
        evaluate.test_variance_on_device(model, batches, opt, ['darken it'], vocab2id, device=dev, verbose=False)


def test_no_host_synchronisation_inside_the_loop(dev, eval_setup):
    """Three batches (the first warms every cache outside the guard) with torch's synchronisation check set to 'error': no
    .item(), .cpu(), nonzero or blocking copy between two images.  result() -- the one read -- stays outside."""
    from t2onet_amd import evaluate
    model, opt, batches = eval_setup
    evaluate.test_on_device(model, batches[:1], opt, is_test=True, device=dev, verbose=False)
    on_dev = [(a.to(dev), b.to(dev), x, r) for a, b, x, r in batches]
    seen = []
    mode = torch.cuda.get_sync_debug_mode()
    real_read = evaluate._DeviceTable.read
    try:
        def read(self):                                   # the end of the loop: leave the guarded region for the one copy
            torch.cuda.set_sync_debug_mode(mode)
            seen.append(self.itr)
            return real_read(self)
        evaluate._DeviceTable.read = read
        torch.cuda.set_sync_debug_mode('error')
        res = evaluate.test_on_device(model, on_dev, opt, is_test=True, device=dev, verbose=False)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
        evaluate._DeviceTable.read = real_read
    assert seen == [3] and all(np.isfinite(v) for v in res[:2])


WORDS = ['<NULL>', '<START>', '<END>', '<UNK>', 'make', 'the', 'photo', 'brighter', 'and', 'more', 'colorful', 'please', 'it', 'darker']


def test_test_cli_end_to_end(dev, tmp_path):
    import t2onet_amd
    from PIL import Image
    from t2onet_amd import test_cli
    from t2onet_amd.actor import Actor
    from t2onet_amd.data import short_side_size
    from tests.fivek_tree import write_tree
    img_dir, anno_dir, _, _ = write_tree(str(tmp_path / 'tree'), n_train=0, n_val=2)
    vocab_dir = tmp_path / 'language'
    vocab_dir.mkdir()
    with open(str(vocab_dir / 'FiveK_vocabs_sess_1.json'), 'w') as f:
        json.dump(WORDS + ['word%d' % i for i in range(918 - len(WORDS))], f)
    with open(str(vocab_dir / 'FiveK_operator_vocabs_sess_1.json'), 'w') as f:
        json.dump(['<NULL>', '<START>', '<END>'] + ['op%d' % i for i in range(8)], f)
    torch.manual_seed(5)
    ckpt = str(tmp_path / 'model.pth')
    torch.save(Actor(t2onet_amd.default_options(vocab_dir=str(vocab_dir))).state_dict(), ckpt)
    requests = tmp_path / 'requests.txt'
    requests.write_text('make the photo brighter\nplease make it darker\nmake it more colorful\n')

    def run(save_dir, *more):
        test_cli.main(['--checkpoint', ckpt, '--img_dir', img_dir, '--anno_dir', anno_dir, '--vocab_dir', str(vocab_dir), '--phase', 'val',
                       '--short_size', '64', '--requests', str(requests), '--save_dir', save_dir, '--save_images', '--num_workers', '0']
                      + list(more))
        with open(os.path.join(save_dir, 'metrics.json')) as f:
            return f.read()
    text = run(str(tmp_path / 'out'))
    got = json.loads(text)
    for key in ('in_L1', 'out_L1', 'in_SSIM', 'out_SSIM', 'init_dist', 'dist', 'variance'):
        assert np.isfinite(got[key]), key
    assert got['items'] == 2 and got['checkpoint'] == ckpt and got['phase'] == 'val' and got['variance'] >= 0
    assert [r['request'] for r in got['records']] == ['make it 0', 'make it 1']
    for rec in got['records']:
        assert len(rec['operations']) <= 5
        for name, values in rec['operations']:
            assert len(values) == t2onet_amd.data.ACT2PN[name]
    for k, (h, w) in enumerate([(120, 80), (96, 144)]):
        for tag in ('in', 'out', 'gt'):
            pic = np.asarray(Image.open(str(tmp_path / 'out' / ('val%d_%s.png' % (k, tag)))))
            assert pic.shape == short_side_size(h, w, 64) + (3,)
    assert run(str(tmp_path / 'out2')) == text
    # the first item alone, decoded on the host and resized on the device (the same bytes): its record and its metrics
    one = json.loads(run(str(tmp_path / 'out3'), '--max_items', '1', '--device_resize'))
    assert one['items'] == 1 and one['records'] == got['records'][:1]
    single = json.loads(run(str(tmp_path / 'out4'), '--max_items', '1'))
    assert all(one[key] == single[key] for key in ('in_L1', 'out_L1', 'in_SSIM', 'out_SSIM', 'dist', 'variance'))


def test_train_cli_device_eval_validates_through_the_device_loop(tmp_path, monkeypatch):
    from t2onet_amd import evaluate, train_cli
    calls = []
    real = evaluate.test_on_device
    monkeypatch.setattr(evaluate, 'test_on_device', lambda *a, **kw: calls.append(real(*a, **kw)) or calls[-1])
    monkeypatch.setattr(evaluate, 'test', lambda *a, **kw: pytest.fail('--device_eval must not run the .item() loop'))
    avg = train_cli.main(['--synthetic', '--batch_size', '4', '--img_size', '64', '--num_iters', '2', '--print_every', '2', '--val_items', '8',
                          '--checkpoint_every', '2', '--run_dir', str(tmp_path), '--num_workers', '0', '--device_eval'])
    st = avg['stats']
    assert len(calls) == 1 and calls[0][2] is None and st['val_dist'] == [calls[0][1]] and 0 < st['best_val_dist'] < 1


def test_device_evaluator_on_plain_images_replays_image_evaluator(dev, capsys):
    """update(input, output, gt) -- the T = 1 form -- over three batches, the table growing from one row: the keys and
    running means of ImageEvaluator.eval() on the same images."""
    from oracle import synth
    from t2onet_amd import evaluate
    ours, theirs = evaluate.DeviceEvaluator(device=dev), evaluate.ImageEvaluator()
    for k in range(3):
        a, b, c = (synth.images(2, 33, 70, 300 + 3 * k + j).to(dev) for j in range(3))
        ours.update(a, b, c)
        theirs.update(a, b, c)
    got, want = ours.result(), theirs.eval()
    assert ours.itr == 3 and sorted(got) == sorted(want)
    for key, v in want.items():
        assert abs(got[key] - v) <= 1e-5 * abs(v) + 1e-6, (key, got[key], v)
