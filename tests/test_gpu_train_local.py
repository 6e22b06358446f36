"""Local edits in the train steps: Trainer.supervised_step / episode_step with a gier.MaskTable.  The yardstick is the
two-launch path (Trainer.fuse_masks = False: mask_select + apply_per_sample per step), which the fused path (operator
kernels reading the uint8 planes, functional.apply_planes) must reproduce bit for bit -- losses, the flat gradient buffer
and the updated parameters; plus train_cli --dataset GIER --load_mask end to end on the synthetic tree."""
import numpy as np
import pytest
import torch

from oracle import synth
from tests import gier_tree
from tests.test_gpu_actor import B, H, W, L
from tests.test_gpu_actor_extra import supervised_inputs
from tests.test_gpu_gier import gier_model

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(autouse=True)
def framework_deterministic():
    """The train steps on the framework's deterministic implementations, as bench.py runs its train legs: the decoder tape
    forms the embedding gradient with index_add_, whose default GPU form adds with float atomics in arrival order -- two
    runs of ONE unchanged step then differ in that gradient's low bits (measured: 1.9e-9) and a bitwise comparison of two
    Trainers would compare noise."""
    import torch.utils.deterministic
    fill = torch.utils.deterministic.fill_uninitialized_memory
    torch.utils.deterministic.fill_uninitialized_memory = False
    torch.use_deterministic_algorithms(True, warn_only=True)
    yield
    torch.use_deterministic_algorithms(False)
    torch.utils.deterministic.fill_uninitialized_memory = fill


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return gier_tree.write_tree(str(tmp_path_factory.mktemp('gier_local')), n_train=8, n_val=2)


@pytest.fixture(scope='module')
def batch():
    x = synth.requests(B, L, 41, vocab=len(gier_tree.WORDS))
    y, img_y, gt_params = supervised_inputs(DEV)
    return dict(x=x.to(DEV), lengths=(x != 0).sum(1), img=synth.images(B, H, W, 42).to(DEV), y=y, img_y=img_y, gt=gt_params)


def make_table(kind, n_vocab):
    """'local': sample 0 every operator under a box, sample 1 nothing, sample 2 every operator under a 0 / 1 / 2 count plane,
    sample 3 an entry for END only (never executed); 'none': no entry at all (every slot -1)."""
    from t2onet_amd.gier import MaskTable
    box = np.zeros((H, W), np.float32)
    box[16:48, 17:48] = 1.0
    two = box.copy()
    two[24:40, 8:56] += 1.0
    ops = (3, 4, 5, 6, 8, 9)
    dicts = [{}, {}, {}, {}] if kind == 'none' else [{op: box for op in ops}, {}, {str(op): [two] for op in ops}, {2: box}]
    return MaskTable.from_arrays(dicts, (H, W), n_vocab, DEV)


def two_steps(vocab_dir, batch, table, fuse, reinforce_sample):
    """A fresh model and Trainer from the one synthetic state dict; one supervised and one episode step, seeded.  Returns
    every number the steps produce: losses, the flat gradients after each step, the parameters after both."""
    from t2onet_amd.train import Trainer
    model, opt = gier_model(vocab_dir, DEV)
    model.train()
    tr = Trainer(model, opt)
    tr.fuse_masks = fuse
    torch.manual_seed(123)
    op_loss, param_loss = tr.supervised_step(batch['x'], batch['y'], batch['img'], batch['img_y'], batch['gt'], batch['lengths'], masks=table)
    g_sup = tr.grads.flat.clone()
    torch.manual_seed(124)
    l1 = tr.episode_step(batch['x'], batch['img'], batch['img_y'][:, -1], reinforce_sample, batch['lengths'], masks=table)
    out = dict(op_loss=op_loss.clone(), param_loss=param_loss.clone(), l1=l1.clone(), g_sup=g_sup, g_ep=tr.grads.flat.clone(),
               params=tr.optimizer.flat_param.clone())
    tr.close()
    return out, opt


def assert_same(a, b, tag):
    for k in a:
        assert torch.isfinite(a[k]).all(), (tag, k)
        assert torch.equal(a[k], b[k]), (tag, k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize('reinforce_sample', [0, 1])
def test_fused_steps_equal_the_two_launch_steps_bit_for_bit(tree, batch, reinforce_sample):
    vocab_dir = tree[1]
    n_vocab = len(gier_tree.OPS)
    fused, _ = two_steps(vocab_dir, batch, make_table('local', n_vocab), True, reinforce_sample)
    plain, _ = two_steps(vocab_dir, batch, make_table('local', n_vocab), False, reinforce_sample)
    assert_same(fused, plain, 'fused vs two-launch')
    assert float(fused['g_sup'].abs().max()) > 0 and float(fused['g_ep'].abs().max()) > 0
    if reinforce_sample == 0:
        # a table without entries is the step without masks, bit for bit; a table with entries is not: the masks act
        empty, _ = two_steps(vocab_dir, batch, make_table('none', n_vocab), True, 0)
        nomask, _ = two_steps(vocab_dir, batch, None, True, 0)
        assert_same(empty, nomask, 'all -1 vs masks=None')
        assert float(fused['l1']) != float(nomask['l1'])


def test_supervised_forward_takes_a_table(tree, batch):
    """A MaskTable as `mask`, fused or not, equals the documented 5-D tensor form built from mask_select on y[:, i]."""
    from t2onet_amd import functional as T
    model, opt = gier_model(tree[1], DEV)
    model.eval()
    table = make_table('local', len(gier_tree.OPS))
    y = batch['y']
    steps = int((y != 0).sum(1).max()) - 2
    five_d = torch.stack([T.mask_select(table.planes, table.slot, y[:, i + 1].contiguous()) for i in range(steps)], 1)
    assert five_d.shape == (B, steps, 1, H, W) and float(five_d.max()) == 2.0 and float(five_d.min()) == 0.0
    args = (batch['x'], y, batch['img'], batch['img_y'], batch['gt'])
    with torch.no_grad():
        want = model.supervised_forward(*args, five_d, batch['lengths'])
        plain = model.supervised_forward(*args, table, batch['lengths'])
        fused = model.supervised_forward(*args, table, batch['lengths'], fuse_masks=True)
        glob = model.supervised_forward(*args, None, batch['lengths'])
    for got in (plain, fused):
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert not torch.equal(want[0], glob[0])
    # the episode: no stacked masks in the fused state, the same pictures
    with torch.no_grad():
        s0, imgs0, ops0, _ = model.episode_forward(batch['x'], batch['img'], table, 0, batch['lengths'])
        s1, imgs1, ops1, _ = model.episode_forward(batch['x'], batch['img'], table, 0, batch['lengths'], fuse_masks=True)
    assert s0['masks'] is not None and s1['masks'] is None
    assert torch.equal(ops0, ops1) and torch.equal(imgs0, imgs1)


def test_train_cli_load_mask_on_a_gier_tree(tree, tmp_path):
    """Four iterations of the loop with the batch's run-length masks as a MaskTable (both steps masked); the checkpoint it
    writes loads into gier_cli --load_mask."""
    from t2onet_amd import gier, gier_cli, train_cli
    data_dir, vocab_dir, act_dir, glove = tree
    # the collate: tensors stacked, every item's own mask_rle dict beside them
    ds = gier._Tuples(gier.GIERDatasetAct(data_dir, vocab_dir, act_dir, 'train', 'valid', 'rle', 3, 64), with_masks=True)
    plain = gier._Tuples(gier.GIERDatasetAct(data_dir, vocab_dir, act_dir, 'train', 'valid', False, 3, 64))
    assert len(ds[0]) == 7 and len(plain[0]) == 6
    col = gier.collate_masks([ds[0], ds[1]])
    assert len(col) == 7 and col[0].shape == (2, 3, 64, 64) and isinstance(col[6], list) and len(col[6]) == 2
    assert any(len(d) > 0 for d in col[6])                                # the tree annotates local operators
    avg = train_cli.main(['--dataset', 'GIER', '--load_mask', '--data_dir', data_dir, '--vocab_dir', vocab_dir, '--act_dir', act_dir,
                          '--data_mode', 'valid', '--word2vec', glove, '--batch_size', '4', '--img_size', '64', '--num_iters', '4',
                          '--print_every', '2', '--checkpoint_every', '4', '--run_dir', str(tmp_path / 'run'), '--num_workers', '0'])
    st = avg['stats']
    assert st['train_iter'] == [4] and len(st['val_dist']) == 1 and 0 < st['best_val_dist'] < 1
    ckpt = str(tmp_path / 'run' / 'seq2seqL1_model' / 'checkpoint_best' / 'model.pth')
    assert len(torch.load(ckpt)) == 199
    res = gier_cli.main(['--checkpoint', ckpt, '--dataset', 'GIER', '--data_dir', data_dir, '--vocab_dir', vocab_dir, '--phase', 'val',
                         '--data_mode', 'shapeAlign', '--load_mask', '--max_items', '1', '--num_workers', '0', '--save_dir', str(tmp_path / 'out')])
    assert res['items'] == 1 and np.isfinite(res['out_L1'])
