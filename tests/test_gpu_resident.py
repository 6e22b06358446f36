"""The device-resident training set on the GPU: the gather kernel (t2o_resident.hip) on the cases of resident_cases.py
against numpy and against the path the data step already had (descriptors picked by index_select, then the resize
entry copying same-size sources); a captured launch re-aimed through its index buffer; data.ResidentFiveK batch by batch
against device_batch and the default host collation; train_cli --resident end to end.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from tests import resident_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def on_device(h, w, dev):
    store, slots, _ = RC.case(h, w)
    return torch.from_numpy(store.copy()).to(dev), torch.from_numpy(slots.copy()).to(dev)


def descriptor_path(store, slots, index, h, w):
    """The same batch through what the data step had before the gather: the (N K, 4) int32 descriptor table of the store
    (offset, h, w; 0 x 0 where the slot is absent), its rows picked on the device, one resize launch that copies."""
    import t2onet_amd.functional as T
    N, K = slots.shape
    rec = np.zeros(N * K, T.IMAGE_DESC)
    flat = slots.cpu().numpy().reshape(-1)
    rec['offset'] = np.where(flat >= 0, flat, 0)
    rec['h'], rec['w'] = np.where(flat >= 0, h, 0), np.where(flat >= 0, w, 0)
    table = torch.from_numpy(rec.view(np.int32).reshape(-1, 4).copy()).to(store.device)
    rows = (index[:, None] * K + torch.arange(K, device=index.device)[None, :]).reshape(-1)
    picked = table.index_select(0, rows).contiguous()
    B = index.numel()
    out = T._resize_launch(store, picked.data_ptr(), B * K, h, w).view(B, K, 3, h, w)
    return out[:, 0], out[:, 1:]


@pytest.mark.parametrize('which', ['one', 'repeat', 'batch64'])
@pytest.mark.parametrize('size', RC.SIZES)
def test_gather_against_numpy_and_the_descriptor_path(dev, size, which):
    import t2onet_amd.functional as T
    h, w = size
    store, slots = on_device(h, w, dev)
    index = torch.from_numpy(RC.index_vectors()[which]).to(dev)
    B, K = index.numel(), RC.K
    want_x, want_ys = (torch.from_numpy(a.copy()) for a in RC.expected(h, w, which))
    guard = 37                                                          # (odd: the planes are not 16-byte aligned)
    nx, ny = B * 3 * h * w, B * (K - 1) * 3 * h * w
    big = torch.full((3 * guard + nx + ny,), float('nan'), device=dev)
    x = big[guard:guard + nx].view(B, 3, h, w)
    ys = big[2 * guard + nx:2 * guard + nx + ny].view(B, K - 1, 3, h, w)
    got = T.gather_u8(store, slots, index, (h, w), out=(x, ys))
    assert got[0].data_ptr() == x.data_ptr() and got[1].data_ptr() == ys.data_ptr()
    assert torch.equal(x.cpu(), want_x) and torch.equal(ys.cpu(), want_ys)          # (equal: no NaN is left)
    assert int(torch.isnan(big).sum()) == 3 * guard                    # nothing outside the two tensors was written
    host_slots = RC.case(h, w)[1]
    for b, i in enumerate(RC.index_vectors()[which][:8]):
        for k in range(1, K):
            if host_slots[i, k] < 0:
                assert float(ys[b, k - 1].abs().sum()) == 0.0
    ref_x, ref_ys = descriptor_path(store, slots, index, h, w)
    assert torch.equal(x, ref_x) and torch.equal(ys, ref_ys)
    again = T.gather_u8(store, slots, index, (h, w))                    # fresh tensors from the allocator: equal bits
    assert torch.equal(again[0].view(torch.int32), x.view(torch.int32)) and torch.equal(again[1].view(torch.int32), ys.view(torch.int32))


def test_captured_gather_follows_its_index_buffer(dev):
    import t2onet_amd.functional as T
    h, w = 33, 31
    store, slots = on_device(h, w, dev)
    first, second = RC.index_vectors()['repeat'], np.array([0, 1, 3], np.int64)
    index = torch.from_numpy(first).to(dev)
    x = torch.empty(3, 3, h, w, device=dev)
    ys = torch.empty(3, RC.K - 1, 3, h, w, device=dev)
    T.gather_u8(store, slots, index, (h, w), out=(x, ys))              # (the library is loaded before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                           # one kernel node: a linear graph
        T.gather_u8(store, slots, index, (h, w), out=(x, ys))
    x.fill_(-1.0)
    ys.fill_(-1.0)
    index.copy_(torch.from_numpy(second))
    g.replay()
    torch.cuda.synchronize()
    host_store, host_slots, _ = RC.case(h, w)
    for b, i in enumerate(second):
        for k in range(RC.K):
            got = (x[b] if k == 0 else ys[b, k - 1]).cpu().numpy()
            if host_slots[i, k] < 0:
                assert not got.any()
            else:
                off = int(host_slots[i, k])
                want = host_store[off:off + 3 * h * w].reshape(h, w, 3).astype(np.float32).transpose(2, 0, 1) / np.float32(255)
                np.testing.assert_array_equal(got, want)
    index.copy_(torch.from_numpy(first))
    g.replay()
    want_x, want_ys = RC.expected(h, w, 'repeat')
    np.testing.assert_array_equal(x.cpu().numpy(), want_x)
    np.testing.assert_array_equal(ys.cpu().numpy(), want_ys)


def test_wrapper_refuses_what_the_kernel_cannot_take(dev):
    import t2onet_amd.functional as T
    store, slots = on_device(5, 7, dev)
    index = torch.zeros(2, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match='no CPU'):
        T.gather_u8(store, slots, index.cpu(), (5, 7))
    with pytest.raises(RuntimeError, match='no CPU'):
        T.gather_u8(store, slots.to(torch.int32), index, (5, 7))
    with pytest.raises(ValueError):
        T.gather_u8(store, slots, index, (5, 7), out=(torch.empty(2, 3, 5, 7, device=dev), torch.empty(2, 5, 3, 5, 7, device=dev)))
    with pytest.raises(ValueError):
        T.gather_u8(store, torch.zeros(1, 9, dtype=torch.int64, device=dev), index, (5, 7))


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    from tests import fivek_tree
    return fivek_tree.write_tree(str(tmp_path_factory.mktemp('resident')), n_train=8)


@pytest.mark.parametrize('S', [16, 33])
def test_resident_set_equals_device_batch_and_the_host_loader(dev, tree, S):
    from t2onet_amd import data
    img_dir, anno_dir, act_dir, _ = tree
    raw = data.FiveKAct(img_dir, anno_dir, act_dir, 'train', 1, S, raw=True)
    ref = data.FiveKAct(img_dir, anno_dir, act_dir, 'train', 1, S)
    steps = [sum(im is not None for im in raw[i][1]) - 1 for i in range(len(raw))]
    assert min(steps) < 5                                               # an absent column is exercised
    rs = data.ResidentFiveK(raw, S, 3, dev, seed=10, num_workers=2, chunk_items=3)
    assert len(rs) == 2 and rs.store.is_cuda and rs.slots.is_cuda and not rs.req_idx.is_cuda
    assert rs.nbytes == 8 * 7 * data.resident_slot_bytes(S) == rs.store.numel()
    slots = rs.slots.cpu()
    assert int((slots < 0).sum()) == sum(5 - n for n in steps) and (slots[slots >= 0] % 16 == 0).all()
    order = rs.batch_indices(0)
    assert torch.equal(torch.cat(order), torch.randperm(8, generator=torch.Generator().manual_seed(10))[:6])
    batches = list(rs)
    assert len(batches) == 2
    for idx, got in zip(order, batches):
        items = [raw[i] for i in idx.tolist()]
        want = data.device_batch(data.collate_raw(items), S, dev, images_only=True)
        host = torch.utils.data.default_collate([ref[i] for i in idx.tolist()])
        assert len(got) == len(want) == 6
        for g, w in zip(got, want):
            if torch.is_tensor(w):
                assert g.device == w.device and g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous()
                assert torch.equal(g, w)
            else:
                assert list(g) == list(w)
        assert got[0].is_cuda and got[1].is_cuda and not got[2].is_cuda
        assert torch.equal(got[0].cpu(), host[0]) and torch.equal(got[1].cpu(), host[1])
    # the next iteration is the next epoch: another order; the same seed gives the same orders again
    assert rs.epoch == 1
    second = [b[5] for b in rs]
    assert second != [b[5] for b in batches]
    assert [i.tolist() for i in rs.batch_indices(1)] != [i.tolist() for i in order]
    twin = data.ResidentFiveK(raw, S, 3, dev, seed=10, num_workers=0)
    for e in (0, 1):
        assert [i.tolist() for i in twin.batch_indices(e)] == [i.tolist() for i in rs.batch_indices(e)]
    assert torch.equal(twin.store, rs.store) and torch.equal(twin.slots, rs.slots)
    assert [i.tolist() for i in data.ResidentFiveK(raw, S, 3, dev, seed=11, num_workers=0).batch_indices(0)] != [i.tolist() for i in order]


def test_resident_shards_sync_free_fetch_and_memory_refusal(dev, tree):
    from t2onet_amd import data
    img_dir, anno_dir, act_dir, _ = tree
    raw = data.FiveKAct(img_dir, anno_dir, act_dir, 'train', 1, 16, raw=True)
    shards = [data.ResidentFiveK(raw, 16, 2, dev, seed=3, rank=r, world=2, num_workers=0) for r in (0, 1)]
    seen = [torch.cat(s.batch_indices(4)).tolist() for s in shards]
    assert len(seen[0]) == len(seen[1]) == 4 and not set(seen[0]) & set(seen[1])
    assert len(shards[0]) == len(shards[1]) == 2
    rs = shards[0]
    idx = rs.batch_indices(0)[0]
    warm = rs.fetch(idx)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = rs.fetch(idx)
        it = iter(rs)
        nxt = next(it)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(got[0], warm[0]) and torch.equal(got[1], warm[1]) and nxt[0].shape == (2, 3, 16, 16)
    need = 8 * 7 * data.resident_slot_bytes(16)
    before = torch.cuda.memory_allocated(dev)
    with pytest.raises(ValueError, match='%d bytes' % need):
        data.ResidentFiveK(raw, 16, 2, dev, memory_limit=need - 1)
    assert torch.cuda.memory_allocated(dev) == before
    with pytest.raises(ValueError, match='raw=True'):
        data.ResidentFiveK(data.FiveKAct(img_dir, anno_dir, act_dir, 'train', 1, 16), 16, 2, dev)


def test_train_cli_resident_on_a_fivek_layout_tree(tree, tmp_path, capsys):
    from t2onet_amd import default_options, train_cli
    from t2onet_amd.actor import Actor
    img_dir, anno_dir, act_dir, glove = tree
    avg = train_cli.main(['--img_dir', img_dir, '--anno_dir', anno_dir, '--act_dir', act_dir, '--resident', '--batch_size', '2',
                          '--img_size', '32', '--num_iters', '2', '--checkpoint_every', '2', '--word2vec', glove,
                          '--print_every', '2', '--run_dir', str(tmp_path / 'run'), '--num_workers', '0'])
    assert all(np.isfinite(avg[k]) for k in ('op', 'param', 'l1')) and avg['op'] > 0 and avg['l1'] > 0
    assert 'resident set: 8 items, %d bytes' % (8 * 7 * 3072) in capsys.readouterr().out
    sd = torch.load(os.path.join(str(tmp_path / 'run'), 'seq2seqL1_model', 'checkpoint_iter00000002', 'model.pth'))
    assert len(sd) == 199
    Actor(default_options()).load_state_dict(sd)
    assert avg['stats']['train_iter'] == [2]
