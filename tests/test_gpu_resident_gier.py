"""The device-resident GIER training set on the GPU: the item gather (t2o_resident_items.hip) on the cases of
resident_gier_cases.py against its host emulation, numpy and -- for K = 7 -- the existing gather; a captured launch
re-aimed through its index buffer, rows included; gier.ResidentGIER batch by batch against the host loader's collation and
MaskTable.from_rle; both train steps on a resident batch against the loader's batch; train_cli --resident_gier end to end;
shards and the memory refusal.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gier_tree
from tests import resident_gier_cases as GC

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
N_TRAIN = 8
N_ITEMS = 12                                                           # records 0, 2, 4, 6 carry two requests


def on_device(h, w, K):
    store, slots = GC.case(h, w, K)
    return torch.from_numpy(store.copy()).to(DEV), torch.from_numpy(slots.copy()).to(DEV)


@pytest.fixture(scope='module')
def emul():
    from tests.test_resident_gier_cpu import build_emulation
    lib = build_emulation('emul_resident_items')
    lib.emul_gather_items_u8_to_f32.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2
    return lib


@pytest.mark.parametrize('K', GC.KS)
@pytest.mark.parametrize('size', GC.SIZES)
def test_kernel_equals_the_emulation_and_numpy(emul, size, K):
    import t2onet_amd.functional as T
    h, w = size
    store, slots = on_device(h, w, K)
    host_store, host_slots = GC.case(h, w, K)
    guard = 37                                                          # (odd: the planes are not 16-byte aligned)
    for V in GC.VS:
        table = torch.from_numpy(GC.rows(V).copy()).to(DEV) if V else None
        for which, host_index in GC.index_vectors().items():
            index = torch.from_numpy(host_index).to(DEV)
            B = index.numel()
            nx, ny = B * 3 * h * w, B * (K - 1) * 3 * h * w
            big = torch.full((3 * guard + nx + ny,), float('nan'), device=DEV)
            x = big[guard:guard + nx].view(B, 3, h, w)
            ys = big[2 * guard + nx:2 * guard + nx + ny].view(B, K - 1, 3, h, w)
            rbig = torch.full((B * V + 10,), -77, dtype=torch.int32, device=DEV)
            out_rows = rbig[5:5 + B * V].view(B, V)
            got = T.gather_items_u8(store, slots, index, (h, w), rows=table, out=(x, ys, out_rows) if V else (x, ys))
            assert len(got) == (3 if V else 2) and got[0].data_ptr() == x.data_ptr() and got[1].data_ptr() == ys.data_ptr()
            want_x, want_ys = (torch.from_numpy(a.copy()) for a in GC.expected(h, w, K, which))
            assert torch.equal(x.cpu(), want_x) and torch.equal(ys.cpu(), want_ys)          # (equal: no NaN is left)
            assert int(torch.isnan(big).sum()) == 3 * guard            # nothing outside the two tensors was written
            assert torch.equal(out_rows.cpu(), torch.from_numpy(GC.expected_rows(V, which)))
            assert int((rbig == -77).sum()) >= 10 and bool((rbig[:5] == -77).all()) and bool((rbig[5 + B * V:] == -77).all())
            if which == 'repeat':                                       # the emulation, bit for bit
                ex, eys = np.full((B, 3, h, w), np.nan, np.float32), np.full((B, K - 1, 3, h, w), np.nan, np.float32)
                er = np.full((B, V), -77, np.int32)
                rc = emul.emul_gather_items_u8_to_f32(host_store.ctypes.data, host_slots.ctypes.data, host_index.ctypes.data, GC.N, K, B,
                                                      h, w, ex.ctypes.data, eys.ctypes.data if K > 1 else None,
                                                      GC.rows(V).ctypes.data if V else None, V, er.ctypes.data if V else None, None)
                assert rc == 0
                assert x.cpu().numpy().tobytes() == ex.tobytes() and ys.cpu().numpy().tobytes() == eys.tobytes()
                assert out_rows.cpu().numpy().tobytes() == er.tobytes()
            if K <= 8 and which != 'bad':                               # the existing entry: the same thread program
                ref = T.gather_u8(store, slots, index, (h, w))
                assert torch.equal(x, ref[0]) and torch.equal(ys, ref[1])
                assert torch.equal(x.view(torch.int32), ref[0].view(torch.int32)) and torch.equal(ys.view(torch.int32), ref[1].view(torch.int32))


def test_captured_launch_follows_its_index_buffer_rows_included():
    import t2onet_amd.functional as T
    h, w, K, V = 33, 31, 10, 11
    store, slots = on_device(h, w, K)
    table = torch.from_numpy(GC.rows(V).copy()).to(DEV)
    first, second = GC.index_vectors()['repeat'], np.array([0, 3, 4, 5], np.int64)
    index = torch.from_numpy(first).to(DEV)
    out = (torch.empty(4, 3, h, w, device=DEV), torch.empty(4, K - 1, 3, h, w, device=DEV), torch.empty(4, V, dtype=torch.int32, device=DEV))
    T.gather_items_u8(store, slots, index, (h, w), rows=table, out=out)  # (the library is loaded before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                           # one kernel node: a linear graph
        T.gather_items_u8(store, slots, index, (h, w), rows=table, out=out)
    host_store, host_slots = GC.case(h, w, K)
    for vector in (second, first):
        out[0].fill_(-1.0)
        out[1].fill_(-1.0)
        out[2].fill_(-5)
        index.copy_(torch.from_numpy(vector))                           # only the index buffer changes
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[2].cpu(), torch.from_numpy(GC.rows(V)[vector]))
        for b, i in enumerate(vector):
            for k in range(K):
                got = (out[0][b] if k == 0 else out[1][b, k - 1]).cpu().numpy()
                if host_slots[i, k] < 0:
                    assert not got.any()
                else:
                    off = int(host_slots[i, k])
                    want = host_store[off:off + 3 * h * w].reshape(h, w, 3).astype(np.float32).transpose(2, 0, 1) / np.float32(255)
                    np.testing.assert_array_equal(got, want)


def test_wrapper_refuses_what_the_kernel_cannot_take():
    import t2onet_amd.functional as T
    store, slots = on_device(5, 7, 10)
    index = torch.zeros(2, dtype=torch.int64, device=DEV)
    table = torch.zeros(GC.N, 3, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match='no CPU'):
        T.gather_items_u8(store, slots, index.cpu(), (5, 7))
    with pytest.raises(RuntimeError, match='no CPU'):
        T.gather_items_u8(store, slots, index, (5, 7), rows=table.cpu())
    with pytest.raises(RuntimeError, match='no CPU'):
        T.gather_items_u8(store, slots, index, (5, 7), rows=table.to(torch.int64))
    with pytest.raises(ValueError):
        T.gather_items_u8(store, slots, index, (5, 7), rows=table[:GC.N - 1].contiguous())
    with pytest.raises(ValueError):
        T.gather_items_u8(store, slots, index, (5, 7), rows=table, out=(torch.empty(2, 3, 5, 7, device=DEV), torch.empty(2, 9, 3, 5, 7, device=DEV)))
    with pytest.raises(ValueError):
        T.gather_items_u8(store, torch.zeros(1, 17, dtype=torch.int64, device=DEV), index, (5, 7))


# ---------------------------------------------------------------------------------------------- gier.ResidentGIER
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return gier_tree.write_tree(str(tmp_path_factory.mktemp('resident_gier')), n_train=N_TRAIN, n_val=2)


def datasets(tree, S, masks='rle'):
    from t2onet_amd import gier
    data_dir, vocab_dir, act_dir, _ = tree
    return gier.GIERDatasetAct(data_dir, vocab_dir, act_dir, 'train', 'valid', masks, 3, S)


@pytest.fixture(scope='module')
def loader_items():
    """The host loader's items, read once per size and shared: {S: [item 0 .. item 11]} of _Tuples(..., with_masks=True)."""
    return {}


def host_items(loader_items, tree, S):
    from t2onet_amd import gier
    if S not in loader_items:
        ds = gier._Tuples(datasets(tree, S), with_masks=True)
        loader_items[S] = [ds[i] for i in range(len(ds))]
    return loader_items[S]


@pytest.mark.parametrize('S', [16, 64])
def test_fetch_equals_the_loaders_batch_and_its_mask_table(tree, loader_items, S):
    from t2onet_amd import functional as T, gier
    from t2onet_amd import data
    base = datasets(tree, S)
    V = len(gier_tree.OPS)
    rs = gier.ResidentGIER(base, S, 5, DEV, seed=10, num_workers=2, chunk_pictures=7)
    assert len(base) == N_ITEMS and len(rs) == 2
    # every distinct file once: per pair the input, the target and the steps its plan keeps; the two requests of a pair share all
    steps = {}
    for r in range(N_ITEMS):
        steps[base.GIER.ReqId2PairId[r]] = base.get_plan(r)[2]
    assert len(steps) == N_TRAIN and min(steps.values()) < 5 <= max(steps.values())
    assert rs.n_pictures == sum(2 + n for n in steps.values()) < 10 * N_ITEMS
    assert rs.n_pictures == 8 * 2 + 4 * 5 + 4 * 3                      # (odd records are truncated at their third step)
    assert rs.n_planes == 8 + 4 == rs.planes.shape[0]                  # 'brightness' of every pair, 'tint' of the odd ones
    slot = data.resident_slot_bytes(S)
    assert rs.store.numel() == rs.n_pictures * slot and tuple(rs.slots.shape) == (N_ITEMS, 10) and tuple(rs.rows.shape) == (N_ITEMS, V)
    assert rs.nbytes == rs.n_pictures * slot + rs.n_planes * S * S + N_ITEMS * 10 * 8 + N_ITEMS * V * 4 and rs.build_seconds > 0
    slots = rs.slots.cpu()
    assert (slots[slots >= 0] % 16 == 0).all() and len(torch.unique(slots[slots >= 0])) == rs.n_pictures
    assert int((slots < 0).sum()) == sum(8 - steps[base.GIER.ReqId2PairId[r]] for r in range(N_ITEMS))
    assert rs.store.is_cuda and rs.slots.is_cuda and rs.rows.is_cuda and rs.planes.is_cuda and not rs.req_idx.is_cuda
    items = host_items(loader_items, tree, S)
    order = rs.batch_indices(0)
    assert torch.equal(torch.cat(order), torch.randperm(N_ITEMS, generator=torch.Generator().manual_seed(10))[:10])
    batches = list(rs)
    assert len(batches) == 2 and rs.epoch == 1
    twos = 0
    for idx, got in zip(order + [torch.tensor([0, 1, 1, 11, 3])], batches + [rs.fetch(torch.tensor([0, 1, 1, 11, 3]))]):
        want = gier.collate_masks([items[i] for i in idx.tolist()])
        assert len(got) == len(want) == 7
        for g, w in zip(got[:5], want[:5]):
            assert g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous()
            assert torch.equal(g.to(DEV), w.to(DEV))
        assert got[0].is_cuda and got[1].is_cuda and tuple(got[1].shape) == (5, 9, 3, S, S)
        assert list(got[5]) == list(want[5])
        table, ref = got[6], gier.MaskTable.from_rle(want[6], (S, S), V, DEV)
        assert isinstance(table, gier.MaskTable) and table.size == (S, S) and len(table) == 5
        assert table.planes.data_ptr() == rs.planes.data_ptr() and tuple(table.planes.shape) == (12, S, S)   # the whole store, every batch
        assert tuple(table.slot.shape) == (5, V) and table.slot.dtype == torch.int32
        assert torch.equal(table.slot >= 0, ref.slot >= 0)
        for v in range(V):
            op = torch.full((5,), v, dtype=torch.int64, device=DEV)
            mine, theirs = T.mask_select(table.planes, table.slot, op), T.mask_select(ref.planes, ref.slot, op)
            assert torch.equal(mine, theirs)
            if v == gier_tree.OPS.index('brightness'):
                for b, i in enumerate(idx.tolist()):                    # overlapping candidates 0 and 1: a count of 2
                    if int(base.GIER.ReqId2PairId[i]) % 3 == 0:
                        assert float(mine[b].max()) == 2.0
                        twos += 1
                    else:
                        assert float(mine[b].max()) == 1.0
    assert twos > 0
    # the same set without masks: the six fields, the same pictures, neither planes nor rows
    plain = gier.ResidentGIER(datasets(tree, S, False), S, 5, DEV, seed=10, num_workers=0)
    assert plain.rows is None and plain.planes is None and plain.n_planes == 0 and plain.n_pictures == rs.n_pictures
    assert torch.equal(plain.store, rs.store) and torch.equal(plain.slots, rs.slots)
    got = plain.fetch(order[0])
    assert len(got) == 6 and torch.equal(got[0], batches[0][0]) and torch.equal(got[1], batches[0][1])


def test_fetch_uploads_and_launches_nothing_for_the_masks(tree):
    """Sync-free, allocation of the batch's own tensors only: the plane store is handed out as it is."""
    from t2onet_amd import gier
    rs = gier.ResidentGIER(datasets(tree, 16), 16, 4, DEV, seed=3, num_workers=0)
    idx = rs.batch_indices(0)[0]
    warm = rs.fetch(idx)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = rs.fetch(idx)
        nxt = next(iter(rs))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(got[0], warm[0]) and torch.equal(got[1], warm[1]) and torch.equal(got[6].slot, warm[6].slot)
    assert got[6].planes is rs.planes and nxt[0].shape == (4, 3, 16, 16)


# ---------------------------------------------------------------------------------------------- the train steps
@pytest.fixture()
def framework_deterministic():
    """As tests/test_gpu_train_local.py: the framework's deterministic implementations, so that two runs of one step agree
    bit for bit (index_add_ in the decoder tape)."""
    import torch.utils.deterministic
    fill = torch.utils.deterministic.fill_uninitialized_memory
    torch.utils.deterministic.fill_uninitialized_memory = False
    torch.use_deterministic_algorithms(True, warn_only=True)
    yield
    torch.use_deterministic_algorithms(False)
    torch.utils.deterministic.fill_uninitialized_memory = fill


def two_steps(vocab_dir, batch, table):
    from t2onet_amd.train import Trainer
    from tests.test_gpu_gier import gier_model
    model, opt = gier_model(vocab_dir, DEV)
    model.train()
    tr = Trainer(model, opt)
    img_x, img_y, x, y, gt = batch[:5]
    lengths = (x != opt.null_id).sum(1)
    x, y, img_x, img_y, gt = (t.to(DEV) for t in (x, y, img_x, img_y, gt))
    torch.manual_seed(123)
    op_loss, param_loss = tr.supervised_step(x, y, img_x, img_y, gt, lengths, masks=table)
    g_sup = tr.grads.flat.clone()
    torch.manual_seed(124)
    l1 = tr.episode_step(x, img_x, img_y[:, -1], lengths=lengths, masks=table)
    out = dict(op_loss=op_loss.clone(), param_loss=param_loss.clone(), l1=l1.clone(), g_sup=g_sup, g_ep=tr.grads.flat.clone(),
               params=tr.optimizer.flat_param.clone())
    tr.close()
    return out


def test_train_steps_on_a_resident_batch_equal_the_loaders(tree, loader_items, framework_deterministic):
    from t2onet_amd import gier
    S, V = 64, len(gier_tree.OPS)
    rs = gier.ResidentGIER(datasets(tree, S), S, 4, DEV, seed=5, num_workers=0)
    idx = torch.tensor([0, 3, 5, 9])                                    # pairs 0 (count-2 plane), 2, 3 ('tint' too), 6
    got = rs.fetch(idx)
    items = host_items(loader_items, tree, S)
    want = gier.collate_masks([items[i] for i in idx.tolist()])
    resident = two_steps(tree[1], got, got[6])
    loader = two_steps(tree[1], want, gier.MaskTable.from_rle(want[6], (S, S), V, DEV))
    for k in resident:
        assert torch.isfinite(resident[k]).all(), k
        assert torch.equal(resident[k], loader[k]), (k, float((resident[k] - loader[k]).abs().max()))
    assert float(resident['g_sup'].abs().max()) > 0 and float(resident['g_ep'].abs().max()) > 0
    unmasked = two_steps(tree[1], got, None)                            # and the masks act
    assert float(unmasked['l1']) != float(resident['l1'])


def test_train_cli_resident_gier_on_a_gier_tree(tree, tmp_path, capsys):
    from t2onet_amd import gier_cli, train_cli
    data_dir, vocab_dir, act_dir, glove = tree
    avg = train_cli.main(['--dataset', 'GIER', '--resident_gier', '--load_mask', '--data_dir', data_dir, '--vocab_dir', vocab_dir,
                          '--act_dir', act_dir, '--data_mode', 'valid', '--word2vec', glove, '--batch_size', '4', '--img_size', '64',
                          '--num_iters', '4', '--print_every', '2', '--checkpoint_every', '4', '--run_dir', str(tmp_path / 'run'),
                          '--num_workers', '0'])
    st = avg['stats']
    assert st['train_iter'] == [4] and len(st['val_dist']) == 1 and 0 < st['best_val_dist'] < 1
    assert all(np.isfinite(avg[k]) for k in ('op', 'param', 'l1')) and avg['op'] > 0 and avg['l1'] > 0
    assert 'resident GIER set: 12 items, 48 distinct pictures, 12 mask planes, ' in capsys.readouterr().out
    ckpt = str(tmp_path / 'run' / 'seq2seqL1_model' / 'checkpoint_best' / 'model.pth')
    assert len(torch.load(ckpt)) == 199
    res = gier_cli.main(['--checkpoint', ckpt, '--dataset', 'GIER', '--data_dir', data_dir, '--vocab_dir', vocab_dir, '--phase', 'val',
                         '--data_mode', 'shapeAlign', '--load_mask', '--max_items', '1', '--num_workers', '0', '--save_dir', str(tmp_path / 'out')])
    assert res['items'] == 1 and np.isfinite(res['out_L1'])


def test_shards_and_memory_refusal(tree):
    from t2onet_amd import data, gier
    base = datasets(tree, 16)
    shards = [gier.ResidentGIER(base, 16, 3, DEV, seed=3, rank=r, world=2, num_workers=0) for r in (0, 1)]
    seen = [torch.cat(s.batch_indices(4)).tolist() for s in shards]
    assert len(seen[0]) == len(seen[1]) == 6 and not set(seen[0]) & set(seen[1])
    assert len(shards[0]) == len(shards[1]) == 2
    assert torch.equal(shards[0].store, shards[1].store) and torch.equal(shards[0].planes, shards[1].planes)
    need = shards[0].nbytes
    assert need == 48 * data.resident_slot_bytes(16) + 12 * 256 + N_ITEMS * 80 + N_ITEMS * len(gier_tree.OPS) * 4
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    with pytest.raises(ValueError, match='%d bytes' % need):
        gier.ResidentGIER(base, 16, 3, DEV, memory_limit=need - 1)
    assert torch.cuda.memory_allocated(DEV) == before
    with pytest.raises(ValueError, match="phase 'train'"):
        gier.ResidentGIER(gier.GIERDataset(tree[0], tree[1], 'train', 'valid', False, 3, 16), 16, 3, DEV)
    with pytest.raises(ValueError, match='train_img_size'):
        gier.ResidentGIER(base, 32, 3, DEV)
