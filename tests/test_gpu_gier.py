"""GIER on the device: the masked episode with a gier.MaskTable (no host read) against the same episode with the reference's
list of dicts; gier_cli and train_cli --dataset GIER end to end on a synthetic GIER-layout tree (tests/gier_tree.py)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import synth
from tests import gier_tree
from tests.test_gpu_actor import B, H, W, L, make_model

pytestmark = pytest.mark.gpu


def test_masked_episode_with_a_table_equals_the_dict_path():
    """Eval-mode arg-max episode, B = 4 at 64 x 64 (the shapes of test_episode_with_local_edit_masks): masks for some samples
    and operators only, one of them a count of 2.  The table path runs with host synchronisation forbidden."""
    from t2onet_amd.gier import MaskTable
    dev = torch.device('cuda:0')
    model, opt = make_model(dev)
    model.eval()
    x = synth.requests(B, L, 41).to(dev)
    lengths = (x != opt.null_id).sum(1).cpu()
    img = synth.images(B, H, W, 42).to(dev)
    with torch.no_grad():
        _, _, ops0, _ = model.episode_forward(x, img, None, reinforce_sample=0, lengths=lengths)
    chosen = ops0.tolist()
    box = np.zeros((1, H, W), np.float32)
    box[:, 16:48, 16:48] = 1.0
    two = box.copy()
    two[:, 24:40, 8:56] += 1.0                                          # 0 / 1 / 2: overlapping masks, summed
    assert two.max() == 2.0
    # sample 0: its first and second operator; sample 1: nothing; sample 2: the count-2 mask on its first; sample 3: an
    # operator it may never choose (END)
    mask_dict = [{str(chosen[0][0]): [box], str(chosen[0][1]): [two]}, {}, {str(chosen[2][0]): [two]}, {'2': [box]}]
    table = MaskTable.from_arrays(mask_dict, (H, W), opt.output_vocab_size, dev)
    assert table.planes.shape == (4, H, W) and int((table.slot >= 0).sum()) == 4
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        with torch.no_grad():
            state_t, imgs_t, ops_t, params_t = model.episode_forward(x, img, table, reinforce_sample=0, lengths=lengths)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    with torch.no_grad():                                               # the dict path reads pred_op back at every step
        state_d, imgs_d, ops_d, params_d = model.episode_forward(x, img, mask_dict, reinforce_sample=0, lengths=lengths)
    assert torch.equal(ops_t, ops_d)
    assert len(params_t) == len(params_d) and all(torch.equal(a, b) for a, b in zip(params_t, params_d))
    assert torch.equal(imgs_t, imgs_d)
    assert state_t['masks'].shape == (B, opt.decoder_max_len, 1, H, W) and state_d['masks'].shape == (B, opt.decoder_max_len, 3, H, W)
    assert torch.equal(state_t['masks'].expand(-1, -1, 3, -1, -1), state_d['masks'])
    assert float(state_t['masks'][2, 0].max()) == 2.0 and float(state_t['masks'][1].min()) == 1.0
    # the masks did something: sample 0's first step differs from the global edit outside the box only
    with torch.no_grad():
        _, imgs0, _, _ = model.episode_forward(x, img, None, reinforce_sample=0, lengths=lengths)
    assert torch.equal(imgs_t[1, 0], imgs0[1, 0]) and torch.equal(imgs_t[0, 0, :, 16:48, 16:48], imgs0[0, 0, :, 16:48, 16:48])
    if chosen[0][0] >= 3:
        assert torch.equal(imgs_t[0, 0, :, :16], img[0, :, :16])


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return gier_tree.write_tree(str(tmp_path_factory.mktemp('gier_gpu')), n_train=8, n_val=2)


def gier_model(vocab_dir, dev, favour=None):
    import t2onet_amd
    from t2onet_amd.actor import Actor
    opt = t2onet_amd.default_options(input_dropout_p=0.0, dropout_p=0.0, dataset='GIER', session=3, vocab_dir=vocab_dir)
    m = Actor(opt)
    assert m.lang_encoder.embedding.weight.shape[0] == len(gier_tree.WORDS)
    m.load_state_dict(synth.fill_state_dict(m.state_dict(), seed=7))
    if favour is not None:
        with torch.no_grad():
            m.decoder.out_linear.bias[favour] += 30.0                   # this operator is chosen first
    return m.to(dev), opt


def test_gier_cli_on_a_gier_tree(tree, tmp_path):
    """The GIER scoring command end to end, twice: identical metrics.json; with --load_mask the saved pictures are the direct masked
    episode's (list-of-dicts path, masks from the host union) on the same items."""
    from PIL import Image
    from t2onet_amd import functional as T
    from t2onet_amd import gier, gier_cli
    from t2onet_amd.train import select_end_images
    data_dir, vocab_dir, _, _ = tree
    dev = torch.device('cuda:0')
    model, opt = gier_model(vocab_dir, dev, favour=3)                   # brightness first: every record has a local one
    ckpt = str(tmp_path / 'model.pth')
    torch.save(model.state_dict(), ckpt)
    base = ['--checkpoint', ckpt, '--dataset', 'GIER', '--data_dir', data_dir, '--vocab_dir', vocab_dir, '--data_mode', 'shapeAlign',
            '--phase', 'val', '--num_workers', '0']
    runs = []
    for k in range(2):
        out = str(tmp_path / ('run%d' % k))
        res = gier_cli.main(base + ['--save_dir', out])
        with open(os.path.join(out, 'metrics.json')) as f:
            runs.append(f.read())
        assert res['items'] == 3 and 0 < res['out_L1'] < 1 and 0 < res['in_SSIM'] <= 1 and len(res['records']) == 3
        assert res['records'][0]['name'] == 'va00_va00.jpg' and res['records'][0]['request'] == gier_tree.REQUESTS[0]
    assert runs[0].replace('run0', 'run1') == runs[1].replace('run0', 'run1')
    assert json.loads(runs[0])['records'][0]['operations'][0][0] == 'brightness'
    # local edits
    out = str(tmp_path / 'masked')
    res = gier_cli.main(base + ['--save_dir', out, '--load_mask', '--save_images', '--max_items', '2'])
    assert res['items'] == 2
    ds = gier.GIERDataset(data_dir, vocab_dir, 'val', 'shapeAlign', True, 3)
    model.eval()
    differs = False
    for k in range(2):
        it = ds[k]
        x = it['request_idx'].unsqueeze(0)
        img = it['input'].unsqueeze(0).to(dev)
        assert it['mask_dict'][3].shape == tuple(img.shape[-2:]) and it['mask_dict'][3].max() == 2.0
        mask_dict = [{str(op): [m[None]] for op, m in it['mask_dict'].items()}]
        with torch.no_grad():
            _, imgs, ops, _ = model.episode_forward(x.to(dev), img, mask_dict, reinforce_sample=False, lengths=(x != 0).sum(1))
            _, imgs_g, ops_g, _ = model.episode_forward(x.to(dev), img, None, reinforce_sample=False, lengths=(x != 0).sum(1))
        assert int(ops[0, 0]) == 3
        want = T.to_u8_hwc(select_end_images(imgs, ops, opt.end_id)).cpu().numpy()[0]
        got = np.asarray(Image.open(os.path.join(out, 'va00_va00_req%04d_out.png' % k)))
        np.testing.assert_array_equal(got, want)
        differs = differs or not torch.equal(imgs[:, 0], imgs_g[:, 0])
    assert differs                                                      # the masks changed the pictures: the edit was local


def test_train_cli_on_a_gier_tree(tree, tmp_path):
    """A few iterations of the reference-shaped loop on the GIER plumbing; the checkpoint loads into gier_cli."""
    from t2onet_amd import gier_cli, train_cli
    data_dir, vocab_dir, act_dir, glove = tree
    avg = train_cli.main(['--dataset', 'GIER', '--data_dir', data_dir, '--vocab_dir', vocab_dir, '--act_dir', act_dir, '--data_mode', 'valid',
                          '--word2vec', glove, '--batch_size', '4', '--img_size', '64', '--num_iters', '4', '--print_every', '2',
                          '--checkpoint_every', '4', '--run_dir', str(tmp_path / 'run'), '--num_workers', '0'])
    st = avg['stats']
    assert st['train_iter'] == [4] and len(st['val_dist']) == 1 and 0 < st['best_val_dist'] < 1
    ckpt = str(tmp_path / 'run' / 'seq2seqL1_model' / 'checkpoint_best' / 'model.pth')
    sd = torch.load(ckpt)
    assert len(sd) == 199 and sd['lang_encoder.embedding.weight'].shape[0] == len(gier_tree.WORDS)
    res = gier_cli.main(['--checkpoint', ckpt, '--dataset', 'GIER', '--data_dir', data_dir, '--vocab_dir', vocab_dir, '--phase', 'val',
                         '--max_items', '1', '--num_workers', '0', '--save_dir', str(tmp_path / 'out')])
    assert res['items'] == 1 and np.isfinite(res['out_L1'])


def test_collated_batch_becomes_a_table_with_one_call(tree):
    """GIERDataset.collate output -> MaskTable.from_collated: the run-length form (device union) and the ready-plane form
    (host union) of the same training items give the same table."""
    from t2onet_amd import gier
    data_dir, vocab_dir, _, _ = tree
    dev = torch.device('cuda:0')
    ready = gier.GIERDataset(data_dir, vocab_dir, 'train', 'valid', True, 3, train_img_size=48)
    runs = gier.GIERDataset(data_dir, vocab_dir, 'train', 'valid', 'rle', 3, train_img_size=48)
    picks = [0, 2, 3, 5]
    a = gier.MaskTable.from_collated(runs.collate([runs[i] for i in picks]), len(runs.op_vocab2id), dev)
    b = gier.MaskTable.from_collated(ready.collate([ready[i] for i in picks]), len(ready.op_vocab2id), dev)
    assert a.size == b.size == (48, 48) and a.slot.shape == (4, 11)
    assert torch.equal(a.slot, b.slot) and torch.equal(a.planes, b.planes)
    assert int(a.slot[1, 8]) >= 0 and int(a.slot[0, 8]) == -1 and int(a.planes.max()) >= 2      # tint on the odd record only; masks 0 and 1 overlap: counts of 2 (three blobs may give 3)
