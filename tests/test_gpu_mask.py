"""The mask kernels on the device (t2o_mask.hip) against the numpy oracle: exact comparisons, guard bytes included."""
import numpy as np
import pytest
import torch

from tests import mask_cases as MC
from tests.test_mask_cpu import select_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def run_union(rles, jobs, total):
    from t2onet_amd import functional as T
    out = torch.full((total,), MC.GUARD, dtype=torch.uint8, device=DEV)
    assert T.rle_union_u8(rles, jobs, out=out) is out
    return out


@pytest.mark.parametrize('src', MC.SRC_SIZES)
def test_union_against_the_numpy_oracle(src):
    """Every output size x every selection (empty, single, overlapping, repeated) of one source size, planes at all four
    byte alignments, the bytes between them untouched."""
    planes, rles, jobs, total = MC.source_case(src, 1)
    assert {off % 4 for _, off, _, _ in jobs} == {0, 1, 2, 3}
    np.testing.assert_array_equal(run_union(rles, jobs, total).cpu().numpy(), MC.expected_buffer(planes, jobs, total))


@pytest.mark.parametrize('n_jobs', [1, 7, 64])
def test_union_mixed_jobs_in_one_launch(n_jobs):
    from t2onet_amd import functional as T
    planes, rles, jobs, total = MC.mixed_case(n_jobs)
    want = MC.expected_buffer(planes, jobs, total)
    first = run_union(rles, jobs, total)
    np.testing.assert_array_equal(first.cpu().numpy(), want)
    assert torch.equal(run_union(rles, jobs, total), first)               # equal bits on a second call
    # captured: the tables are uploaded before, the launch alone is recorded; one replay gives the same bytes
    tables = T.pack_rle_union(rles, jobs)
    tables.upload(torch.device(DEV))
    out = torch.full((total,), MC.GUARD, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        T.rle_union_u8(tables, out=out)
    out.fill_(MC.GUARD)
    graph.replay()
    assert torch.equal(out, first)


def test_union_refusals_reach_python():
    from t2onet_amd import functional as T
    planes, rles = MC.mask_set(7, 5)
    out = torch.zeros(64, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match='selection index'):
        T.rle_union_u8(rles, [([6], 0, 5, 9)], out=out)
    with pytest.raises(ValueError, match='outside the output'):
        T.rle_union_u8(rles, [([0], 20, 5, 9)], out=out)
    assert int(out.sum()) == 0


@pytest.mark.parametrize('H,W', [(1, 1), (33, 47), (32, 32)])
def test_mask_select_against_get_gt_mask(H, W):
    from t2onet_amd import functional as T
    from t2onet_amd.actor import Actor
    from t2onet_amd.gier import MaskTable
    B, V, planes, mask_dict, ops, wild = select_case(H, W)
    table = MaskTable.from_arrays(mask_dict, (H, W), V, DEV)
    assert table.planes.shape == (5, H, W) and table.slot.shape == (B, V) and table.size == (H, W)
    actor = Actor.__new__(Actor)
    img = torch.zeros(B, 3, H, W, device=DEV)
    for chosen in (ops, wild):
        want = Actor.get_gt_mask(actor, img, mask_dict, chosen.reshape(B, 1))[:, :1]
        got = T.mask_select(table.planes, table.slot, torch.from_numpy(chosen).to(DEV))
        assert got.shape == (B, 1, H, W) and torch.equal(got, want)
    if H > 1:                                                            # a count of 2 comes through as 2.0
        assert float(T.mask_select(table.planes, table.slot, torch.from_numpy(ops).to(DEV))[3].max()) == 2.0
    # no plane at all: every sample global
    none = MaskTable.from_arrays([{}] * B, (H, W), V, DEV)
    assert none.planes.shape[0] == 0
    assert torch.equal(T.mask_select(none.planes, none.slot, torch.from_numpy(ops).to(DEV)), torch.ones(B, 1, H, W, device=DEV))


def test_mask_table_from_rle_equals_from_arrays():
    """The same masks through run lengths (one upload, one launch) and through ready host planes: same planes, same slots."""
    from t2onet_amd import gier
    size, V = (50, 75), 11
    sets = [MC.mask_set(*src, seed=3) for src in MC.SRC_SIZES]
    items = [{3: (sets[0][1], [4, 5]), '7': (sets[0][1], [3])}, {}, {10: (sets[2][1], [4, 4, 5])}, {7: (sets[3][1], [])}]
    arrays = [{key: gier.resize_and_union_mask_host(rles, ids, size).astype(np.float32) for key, (rles, ids) in it.items()} for it in items]
    a = gier.MaskTable.from_rle(items, size, V, DEV)
    b = gier.MaskTable.from_arrays(arrays, size, V, DEV)
    assert a.size == b.size == size and a.planes.dtype == torch.uint8 and a.slot.dtype == torch.int32
    assert torch.equal(a.slot, b.slot) and torch.equal(a.planes, b.planes)
    assert int(a.planes[0].max()) == 2 and int(a.planes.max()) == 3 and a.slot[0, 3] == 0 and a.slot[0, 7] == 1 and int((a.slot >= 0).sum()) == 4
    # keys of either type, lists whose first entry is the array, and a plane of another size (no plane: a global edit)
    c = gier.MaskTable.from_arrays([{str(k): [v[None]] for k, v in arrays[0].items()}, {'5': [np.zeros((3, 3), np.float32)]}], size, V, DEV)
    assert torch.equal(c.slot[0], a.slot[0]) and int((c.slot[1] >= 0).sum()) == 0 and torch.equal(c.planes, a.planes[:2])
