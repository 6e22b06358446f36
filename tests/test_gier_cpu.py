"""No-GPU checks of t2onet_amd/gier.py: the COCO run-length codec (round trip and hand-written cases from the published
format), the host union against a direct decode + nearest_index + sum, the GIER index against the reference's own class
(tests/golden/gier.npz over the trimmed tree tests/golden/gier/, both from tools/gen_golden_gier.py), and the items of
GIERDataset / GIERDatasetAct on a synthetic GIER-layout tree (tests/gier_tree.py)."""
import json
import os

import numpy as np
import pytest
import torch

from t2onet_amd import gier
from t2onet_amd.edit import nearest_index
from tests import gier_tree
from tests import mask_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


# ------------------------------------------------------------------ codec
@pytest.mark.parametrize('h,w', [(1, 1), (7, 5), (33, 47), (64, 64), (101, 67)])
def test_codec_round_trip(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    for density in (0.1, 0.5, 0.9):
        plane = (rng.random((h, w)) < density).astype(np.uint8)
        counts = gier.rle_encode(plane)
        assert int(counts.sum()) == h * w
        text = gier.rle_to_string(counts)
        rle = {'size': [h, w], 'counts': text}
        np.testing.assert_array_equal(gier.rle_counts(rle), counts)
        np.testing.assert_array_equal(gier.rle_decode(rle), plane)
        np.testing.assert_array_equal(gier.rle_decode({'size': [h, w], 'counts': text.encode()}), plane)            # bytes, as pycocotools returns
        np.testing.assert_array_equal(gier.rle_decode({'size': [h, w], 'counts': [int(c) for c in counts]}), plane)    # uncompressed


def test_codec_hand_written_cases():
    h, w = 6, 4
    # an empty mask: one run of zeros; a full mask: no zeros, then h * w ones
    np.testing.assert_array_equal(gier.rle_decode({'size': [h, w], 'counts': [h * w]}), np.zeros((h, w), np.uint8))
    np.testing.assert_array_equal(gier.rle_decode({'size': [h, w], 'counts': [0, h * w]}), np.ones((h, w), np.uint8))
    # strings worked out by hand from rleToString: 5 bits per character + 48, bit 5 = more, bit 4 of the last group = sign
    assert gier.rle_to_string([15]) == '?'                    # 0b01111: one group
    assert gier.rle_to_string([16]) == '`0'                   # 0b10000 would read as negative: a second, empty group
    assert gier.rle_to_string([24]) == 'h0' and gier.rle_to_string([0, 24]) == '0h0'
    assert gier.rle_to_string([32]) == 'P1'
    for text, counts in (('?', [15]), ('`0', [16]), ('h0', [24]), ('0h0', [0, 24]), ('P1', [32])):
        np.testing.assert_array_equal(gier.rle_counts({'counts': text}), np.array(counts, np.uint32))
    # one pixel at (y, x) = (2, 1): column-major position 1 * 6 + 2 = 8
    one = np.zeros((h, w), np.uint8)
    one[2, 1] = 1
    np.testing.assert_array_equal(gier.rle_encode(one), [8, 1, 15])
    np.testing.assert_array_equal(gier.rle_decode({'size': [h, w], 'counts': gier.rle_to_string([8, 1, 15])}), one)
    # a run that crosses a column boundary: positions 4 .. 8 = rows 4, 5 of column 0 and rows 0 .. 2 of column 1
    cross = np.zeros((h, w), np.uint8)
    cross[4:, 0] = 1
    cross[:3, 1] = 1
    np.testing.assert_array_equal(gier.rle_encode(cross), [4, 5, 15])
    np.testing.assert_array_equal(gier.rle_decode({'size': [h, w], 'counts': [4, 5, 15]}), cross)
    # the delta coding from the FOURTH count on (i > 2): [1, 2, 3, 1, 5, 3] -> 1, 2, 3, 1 - 2 = -1 ('O'), 5 - 3 = 2, 3 - 1 = 2
    assert gier.rle_to_string([1, 2, 3, 1, 5, 3]) == '123O22'
    np.testing.assert_array_equal(gier.rle_counts({'counts': '123O22'}), [1, 2, 3, 1, 5, 3])
    assert gier.rle_to_string([3, 9, 12]) == '39<'            # the third count is NOT a difference
    # counts above 2^15: four characters each, and a large negative difference (sign extension over several groups)
    big = [40000, 3, 2, 70000, 1, 33000, 100000, 494]
    text = gier.rle_to_string(big)
    assert text.startswith('PRW132')                          # 40000 = 16 + 2 * 32 + 7 * 1024 + 1 * 32768 -> 'P' 'R' 'W' '1'
    np.testing.assert_array_equal(gier.rle_counts({'counts': text}), np.array(big, np.uint32))
    plane = gier.rle_decode({'size': [500, 487], 'counts': text})
    assert plane.shape == (500, 487) and int(plane.sum()) == 3 + 70000 + 33000 + 494 and plane[0, 80] == 1 and plane[499, 79] == 0
    with pytest.raises(ValueError):
        gier.rle_decode({'size': [h, w], 'counts': [5, 5]})
    with pytest.raises(ValueError):
        gier.rle_counts({'counts': 'P'})                       # ends inside a count


# ------------------------------------------------------------------ host union
@pytest.mark.parametrize('src', MC.SRC_SIZES)
def test_host_union_against_direct_decode_index_sum(src):
    planes, rles = MC.mask_set(*src, seed=11)
    for oh, ow in MC.OUT_SIZES:
        iy, ix = nearest_index(src[0], oh), nearest_index(src[1], ow)
        for ids in ([], [2], [4, 5], [4, 5, 1], [4, 4, 5]):
            want = np.zeros((oh, ow), np.int64)
            for i in ids:
                want += gier.rle_decode(rles[i])[iy][:, ix].astype(bool)
            got = gier.resize_and_union_mask_host(rles, ids, (oh, ow))
            assert got.dtype == np.uint8 and got.shape == (oh, ow)
            np.testing.assert_array_equal(got, want)
    if src[0] >= 33:                                          # overlapping ids give 2, with the full mask 3: a count, not a union
        full = gier.resize_and_union_mask_host(rles, [4, 5, 1], src)
        assert set(np.unique(full)) == {1, 2, 3}
        assert gier.resize_and_union_mask_host(rles, [4, 5], src).max() == 2


# ------------------------------------------------------------------ index parity with the reference
@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLD, 'gier.npz'))


@pytest.mark.parametrize('mode', ['full', 'shapeAlign', 'valid+global'])
def test_index_matches_the_reference(gold, mode):
    tree = os.path.join(GOLD, 'gier')
    g = gier.GIER(tree, os.path.join(tree, 'language'), 'val', mode, False, 3)
    key = mode.replace('+', '_')
    assert len(g) == len(g.op_data) == int(gold[key + '_len'])
    n_req = len(g.ReqId2PairId)
    np.testing.assert_array_equal([g.ReqId2PairId[r] for r in range(n_req)], gold[key + '_req2pair'])
    np.testing.assert_array_equal([len(g.PairId2ReqId[p]) for p in range(len(g))], gold[key + '_pair2req_len'])
    np.testing.assert_array_equal(np.stack([g.getReqIdx[r] for r in range(n_req)]), gold[key + '_req_idx'])
    infos = [g.get_op_info(p) for p in range(len(g))]
    np.testing.assert_array_equal([i[0] for i in infos], gold[key + '_op_idx'])
    np.testing.assert_array_equal([i[1] for i in infos], gold[key + '_is_local'])
    assert [{str(k): v for k, v in i[2].items()} for i in infos] == json.loads(str(gold[key + '_mask_ids']))
    assert len(g.OpReqId2ReqId) == len(g.OpReqId2OpId) == len(g.getOpReq) == int(gold[key + '_n_op_req'])
    assert len(g.getImgId) == int(gold[key + '_n_imgs'])
    assert g.req_ids == list(range(n_req)) and len(g.vocab2id) == len(g.id2vocab) and g.op_vocab2id['color_bg'] == 10
    assert all(g.OpId2OpIdx(i) == g.op_vocab2id[g.getOp[i]] for i in g.getOp)
    with pytest.raises(ValueError):
        gier.GIER(tree, os.path.join(tree, 'language'), 'val', 'nonsense', False, 3)


# ------------------------------------------------------------------ items on a synthetic tree
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return gier_tree.write_tree(str(tmp_path_factory.mktemp('gier')), n_train=6, n_val=3)


def test_dataset_items_and_collate(tree):
    data_dir, vocab_dir, act_dir, _ = tree
    ds = gier.GIERDataset(data_dir, vocab_dir, 'train', 'valid', True, 3, train_img_size=48)
    assert len(ds) == 9 and len(ds.GIER) == 6                 # even records carry two requests
    it = ds[0]
    assert set(it) == {'input', 'output', 'is_local', 'op_idx', 'request', 'request_idx', 'mask_dict'}
    assert it['input'].shape == it['output'].shape == (3, 48, 48) and it['input'].dtype == torch.float32
    assert it['op_idx'] == [3, 4] + [0] * 8 and it['is_local'] == [1] + [0] * 9             # 'crop' is not in the vocabulary
    # pad_req: START, the tokens (punctuation dropped), END in front of the first 0
    assert it['request_idx'].tolist() == [1, 11, 4, 5, 12, 7, 2] + [0] * 10 and it['request'] == gier_tree.REQUESTS[0]
    # 'a' is dropped (one letter), 'zebra' is unknown -> 3
    assert ds[3]['request'] == gier_tree.REQUESTS[2] and ds[3]['request_idx'].tolist()[:9] == [1, 16, 5, 17, 8, 14, 3, 2, 0]
    assert ds.pad_req([4] * 15) == [1] + [4] * 15 + [2]
    # the mask planes equal the host union at the item's size, as float32; ids [0, 1] overlap: a count of 2
    rles = ds.GIER.load_mask_rles('tr00')
    assert list(it['mask_dict']) == [3] and it['mask_dict'][3].dtype == np.float32
    np.testing.assert_array_equal(it['mask_dict'][3], gier.resize_and_union_mask_host(rles, [0, 1], (48, 48)))
    assert it['mask_dict'][3].max() == 2.0
    odd = ds[2]                                                # record 1: brightness [2] and tint [1, 3, 4]
    assert sorted(odd['mask_dict']) == [3, 8]
    np.testing.assert_array_equal(odd['mask_dict'][8], gier.resize_and_union_mask_host(ds.GIER.load_mask_rles('tr01'), [1, 3, 4], (48, 48)))
    blob = ds.collate([ds[0], ds[2]])
    assert blob['input'].shape == (2, 3, 48, 48) and blob['request_idx'].shape == (2, 17)
    assert isinstance(blob['mask_dict'], list) and sorted(blob['mask_dict'][1]) == [3, 8] and blob['request'][0] == it['request']
    # get_pair_item: every request of the pair
    pair = ds.GIER.get_pair_item(0)
    assert pair['request'] == [gier_tree.REQUESTS[0], gier_tree.REQUESTS[1]] and pair['input'].shape == (3, 48, 48)
    # data_mode intersections on the five families
    assert len(gier.GIER(data_dir, vocab_dir, 'train', 'valid+global', False, 3)) == 3
    assert len(gier.GIER(data_dir, vocab_dir, 'train', 'shapeAlign_nonCrop+global', False, 3)) == 0
    assert len(gier.GIER(data_dir, vocab_dir, 'train', 'full', False, 3)) == 6


def test_validation_items_take_their_own_size_for_masks(tree):
    data_dir, vocab_dir, _, _ = tree
    ds = gier.GIERDataset(data_dir, vocab_dir, 'val', 'shapeAlign', True, 3)
    it = ds[0]
    assert it['input'].shape == (3, 900, 600) and it['output'].shape == (3, 900, 600)          # short side 600
    assert it['mask_dict'][3].shape == (900, 600)                                              # mask_size=None: the item's own size
    fixed = gier.GIERDataset(data_dir, vocab_dir, 'val', 'shapeAlign', True, 3, mask_size=128)  # the reference's (128, 128)
    assert fixed[0]['mask_dict'][3].shape == (128, 128)
    rle = gier.GIERDataset(data_dir, vocab_dir, 'val', 'shapeAlign', 'rle', 3)[0]
    rles, ids = rle['mask_rle'][3]
    assert ids == [0, 1] and len(rles) == gier_tree.N_CAND and 'mask_dict' not in rle
    np.testing.assert_array_equal(gier.resize_and_union_mask_host(rles, ids, (900, 600)), it['mask_dict'][3])


def test_actions(tree):
    data_dir, vocab_dir, act_dir, _ = tree
    ds = gier.GIERDatasetAct(data_dir, vocab_dir, act_dir, 'train', 'valid', False, 3, train_img_size=48)
    assert ds.actions == ['brightness', 'contrast', 'saturation', 'color', 'inpaint', 'tone', 'sharpness', 'white'] and ds.op_max_len == 8
    ops, params, imgs = ds.get_act(0)                           # record 0: nothing truncated
    assert ops.tolist() == [1, 3, 6, 4, 8, 5, 2, 0, 0, 0] and params.shape == (8, 24) and imgs.shape == (8, 3, 48, 48)
    with open(os.path.join(act_dir, 'tr00', 'acts.json')) as f:
        seq = json.load(f)['operation sequence'][0]
    assert params[0, 0] == np.float32(0.4) and (params[0, 1:] == 0).all()
    color = np.array(seq[1][1])
    np.testing.assert_array_equal(params[1], (color / np.abs(color).max()).astype(np.float32))   # max-abs rule
    assert np.abs(params[1]).max() == 1.0
    assert (params[2] == 0).all()                                                                # |7.5| > 5 -> 0
    tone = np.array(seq[3][1])
    np.testing.assert_array_equal(params[3, :8], (tone / np.abs(tone).max()).astype(np.float32))
    assert params[4, 0] == np.float32(-0.3) and (params[5:] == 0).all()
    assert (imgs[:5].flatten(1).max(1).values > 0).all() and (imgs[5:] == 0).all()
    ops1, params1, imgs1 = ds.get_act(2)                        # request 2 = record 1: the fourth step gains < 1 %: three kept
    assert ops1.tolist() == [1, 3, 6, 4, 2, 0, 0, 0, 0, 0] and (params1[3:] == 0).all() and (imgs1[3:] == 0).all()
    it = ds[2]
    assert it['output'].shape == (9, 3, 48, 48) and it['operations'].tolist() == ops1.tolist()
    blob = ds.collate([ds[0], ds[2]])
    assert blob['operations'].shape == (2, 10) and blob['parameters'].shape == (2, 8, 24) and blob['output'].shape == (2, 9, 3, 48, 48)
    tup = gier._Tuples(ds)[2]
    assert len(tup) == 6 and tup[3].tolist() == ops1.tolist() and tup[1].shape == (9, 3, 48, 48)


def test_command_line_flags():
    from t2onet_amd import gier_cli, train_cli
    a = gier_cli.parse_args(['--checkpoint', 'm.pth', '--dataset', 'GIER', '--data_dir', 'data/GIER', '--data_mode', 'shapeAlign', '--load_mask'])
    assert (a.dataset, a.data_dir, a.data_mode, a.load_mask, a.session, a.phase) == ('GIER', 'data/GIER', 'shapeAlign', True, 3, 'test')
    b = gier_cli.parse_args(['--checkpoint', 'm.pth'])
    assert (b.load_mask, b.data_mode, b.vocab_dir, b.max_items) == (False, 'shapeAlign', 'data/language', None)   # the reference's is_load_mask = False
    with pytest.raises(SystemExit):
        gier_cli.parse_args(['--data_dir', 'data/GIER'])                                                          # a checkpoint is required
    c = train_cli.parse_args(['--dataset', 'GIER', '--data_dir', 'data/GIER', '--act_dir', 'output/GIER_actions_set_1', '--data_mode', 'valid'])
    assert (c.dataset, c.data_dir, c.act_dir, c.data_mode, c.session) == ('GIER', 'data/GIER', 'output/GIER_actions_set_1', 'valid', 3)
    d = train_cli.parse_args([])
    assert (d.dataset, d.act_dir, d.session, d.run_dir) == ('FiveK', 'output/actions_set_1', 1, 'output/FiveK_trial_1')   # the FiveK defaults stay
    with pytest.raises(SystemExit):
        train_cli.parse_args(['--dataset', 'GIER', '--synthetic'])
