"""The GIER half of the reference (data/GIER/GIER.py, datasets/GIERdataset.py): the index over the split files, the
request / operator vocabularies, the items the GIER train and test scripts consume, and the local-edit masks.

Masks are what the dataset stores them as: COCO run lengths (`<name>_<name>_mask.json`, a list of {'size': [h, w],
'counts': ...}).  The codec below is written from the published format (cocoapi, common/maskApi.c: rleFrString /
rleToString): counts alternate runs of zeros and ones starting with zeros, in column-major order over size = [h, w]; the
compressed string holds each count in 5-bit groups (bit 5 = "more", bit 4 of the last group = sign), counts from the
fourth on as differences to the count two places earlier.  pycocotools and cv2 are absent here, so parity with those
libraries themselves is unpinned; the codec is held to its own round trip and to hand-written cases, the resize to
edit.nearest_index (OpenCV's published INTER_NEAREST rule).

Host path (`resize_and_union_mask_host`): the reference function in numpy -- every candidate decoded to its native size,
indexed, the annotated ones summed.  Device path (`MaskTable.from_rle`): the run lengths of the ANNOTATED masks only are
uploaded (kilobytes) and functional.rle_union_u8 evaluates every union plane of a batch at its output size in one launch.
Both give a COUNT (masks.sum(0).astype(uint8)): overlapping masks give 2.

Two quirks of the reference, handled on purpose:
  * get_req_item builds masks at (train_img_size, train_img_size) also for the short-side-600 validation images, where
    get_gt_mask's expand_as throws and its `except` silently turns the edit global.  Here mask_size=None (the default)
    means "the item's own image size"; mask_size=(h, w) or an int restores a fixed size.
  * the dataset keys its mask_dict by int operator ids while get_gt_mask looks up str(op): a dict-path episode fed from
    the dataset never finds a mask.  MaskTable accepts both key types.
load_mask_feature (h5 panoptic features) is out of scope.

ResidentGIER (at the end) keeps the training items on the device: every distinct picture file and every distinct union
plane once, a batch and its MaskTable by index in one launch (train_cli --resident_gier).
"""
import copy
import json
import os
from functools import reduce

import numpy as np
import torch
from torch.utils.data import Dataset

from . import data as D

ACTIONS = ['brightness', 'contrast', 'saturation', 'color', 'inpaint', 'tone', 'sharpness', 'white']     # GIERdataset.py:103
ACT2PN = {'brightness': 1, 'contrast': 1, 'saturation': 1, 'color': 24, 'inpaint': 0, 'tone': 8, 'sharpness': 1, 'white': 0}
OP_MAX_LEN = 8


# ------------------------------------------------------------------ COCO RLE codec
def _counts_from_string(s):
    """rleFrString, vectorised: 5-bit groups, little end first; bit 5 = more; bit 4 of the last group = sign."""
    if isinstance(s, str):
        s = s.encode('ascii')
    b = np.frombuffer(bytes(s), dtype=np.uint8).astype(np.int64) - 48
    if b.size == 0:
        return np.zeros(0, np.uint32)
    last = (b & 0x20) == 0
    if not last[-1]:
        raise ValueError('rle_counts: the string ends inside a count')
    ends = np.nonzero(last)[0]
    starts = np.concatenate([[0], ends[:-1] + 1])
    gid = np.repeat(np.arange(len(ends)), ends - starts + 1)
    k = np.arange(b.size) - starts[gid]
    if k.max() > 12:
        raise ValueError('rle_counts: a count of more than 13 groups')
    x = np.add.reduceat((b & 0x1f) << (5 * k), starts)
    neg = (b[ends] & 0x10) != 0
    x = np.where(neg, x - (np.int64(1) << (5 * (k[ends] + 1))), x)
    # counts[i] = x[i] + counts[i - 2] for i > 2: two running sums, one over the odd places, one over the even from 2 on
    out = x.copy()
    out[1::2] = np.cumsum(x[1::2])
    out[2::2] = np.cumsum(x[2::2])
    return (out & 0xffffffff).astype(np.uint32)


def rle_counts(rle):
    """The run lengths of a COCO RLE {'size': [h, w], 'counts': compressed string (str / bytes) or list} as a uint32 array."""
    c = rle['counts']
    if isinstance(c, (str, bytes, bytearray)):
        return _counts_from_string(c)
    return np.asarray(c, dtype=np.int64).astype(np.uint32)


def rle_to_string(counts):
    """rleToString: the compressed form of a sequence of run lengths (fixtures and tests)."""
    counts = [int(c) for c in counts]
    out = []
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5                                    # Python's >> is arithmetic, as C's on a long
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return ''.join(out)


def rle_encode(plane):
    """The uncompressed counts of a binary (h, w) plane: column-major, zeros first (fixtures and tests)."""
    flat = (np.asarray(plane) != 0).T.reshape(-1)
    if flat.size == 0:
        return np.zeros(0, np.uint32)
    change = np.nonzero(flat[1:] != flat[:-1])[0] + 1
    runs = np.diff(np.concatenate([[0], change, [flat.size]]))
    if flat[0]:
        runs = np.concatenate([[0], runs])
    return runs.astype(np.uint32)


def rle_decode(rle):
    """pycocotools.mask.decode for one RLE: a uint8 (h, w) array of 0 / 1.  The numpy oracle of the device path."""
    h, w = int(rle['size'][0]), int(rle['size'][1])
    counts = rle_counts(rle).astype(np.int64)
    if int(counts.sum()) != h * w:
        raise ValueError('rle_decode: the runs add up to %d, the mask has %d pixels' % (int(counts.sum()), h * w))
    flat = np.repeat((np.arange(len(counts)) & 1).astype(np.uint8), counts)
    return np.ascontiguousarray(flat.reshape(w, h).T)


def resize_and_union_mask_host(rles, mask_ids, size):
    """GIER.resize_and_union_mask (GIER.py:288-307) in numpy: every mask decoded, resized to size = (h, w) with
    cv2.INTER_NEAREST's rule (edit.nearest_index), the boolean planes at mask_ids summed -> uint8 (h, w), a COUNT."""
    from .edit import nearest_index
    h, w = int(size[0]), int(size[1])
    planes = []
    for rle in rles:
        m = rle_decode(rle)
        planes.append(m[nearest_index(m.shape[0], h)][:, nearest_index(m.shape[1], w)])
    masks = np.array(planes, dtype=bool).reshape(len(planes), h, w)[list(mask_ids)]
    return masks.sum(0).astype(np.uint8)


# ------------------------------------------------------------------ masks on the device
class MaskTable(object):
    """The masks of a batch where the masked episode reads them: .planes (N,H,W) uint8 on the device, .slot (B,V) int32 on
    the device -- slot[b][operator vocabulary id] = a plane number, or -1 for "no entry: a global edit" -- and .size =
    (H, W).  Actor.episode_forward / episode_decode / forward take one as `mask_dict`: per step ONE functional.mask_select
    on the operators just chosen, no host read and no loop over samples."""

    def __init__(self, planes, slot, size):
        self.planes, self.slot, self.size = planes, slot, (int(size[0]), int(size[1]))

    def __len__(self):
        return self.slot.shape[0]

    @staticmethod
    def _key(key, n_vocab):
        op = int(key)
        if not 0 <= op < n_vocab:
            raise ValueError('MaskTable: operator id %r outside the vocabulary of %d' % (key, n_vocab))
        return op

    @classmethod
    def from_rle(cls, items, size, n_vocab, device=None):
        """items[b] = {operator vocabulary id (int or str): (rles, mask_ids)}: rles the candidate masks of sample b's
        image (COCO RLE dicts, as the mask file holds them), mask_ids the annotated ones.  Only the annotated masks are
        parsed and uploaded; the whole batch costs ONE upload (tables, run ends and the slot table in one pinned buffer)
        and ONE launch."""
        from . import functional as T
        H, W = int(size[0]), int(size[1])
        masks, jobs, seen = [], [], {}
        slot = np.full((len(items), int(n_vocab)), -1, np.int32)
        for b, entry in enumerate(items):
            for key, (rles, mask_ids) in entry.items():
                sel = []
                for i in mask_ids:
                    rle = rles[i]
                    at = seen.get(id(rle))
                    if at is None:
                        at = seen[id(rle)] = len(masks)
                        masks.append(rle)
                    sel.append(at)
                slot[b, cls._key(key, n_vocab)] = len(jobs)
                jobs.append((sel, len(jobs) * H * W, H, W))
        if not jobs:
            dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
            return cls(torch.zeros(0, H, W, dtype=torch.uint8, device=dev), torch.from_numpy(slot).to(dev, non_blocking=True), (H, W))
        out, extra = T.rle_union_u8(masks, jobs, device, extra=slot)
        return cls(out[:len(jobs) * H * W].view(len(jobs), H, W), extra.view(len(items), int(n_vocab)), (H, W))

    @classmethod
    def from_arrays(cls, mask_dict, size, n_vocab, device=None):
        """mask_dict: the reference-style list of dicts of READY masks (Actor.get_gt_mask; GIERDataset.collate's
        'mask_dict'): keys int or str operator ids, a value an array / tensor or a list whose first entry is one, shaped
        (H, W) or (1, H, W) and holding whole numbers 0..255 (a count).  A value of another shape gets no plane, as get_gt_mask's
        failed expand_as makes the edit global.  One upload: the planes and the slot table in one pinned buffer."""
        H, W = int(size[0]), int(size[1])
        planes, entries = [], []
        for b, entry in enumerate(mask_dict):
            for key, value in entry.items():
                value = value[0] if isinstance(value, (list, tuple)) else value
                a = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)
                if a.shape not in ((H, W), (1, H, W)):
                    continue
                u8 = a.astype(np.uint8)
                if not np.array_equal(u8.astype(a.dtype), a):
                    raise ValueError('MaskTable.from_arrays: mask values must be whole numbers 0..255 (a count)')
                entries.append((b, cls._key(key, n_vocab), len(planes)))
                planes.append(u8.reshape(H, W))
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        n, nslot = len(planes), len(mask_dict) * int(n_vocab)
        buf = torch.empty(4 * nslot + n * H * W, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        flat = buf.numpy()
        slot = flat[:4 * nslot].view(np.int32).reshape(len(mask_dict), int(n_vocab))
        slot[:] = -1
        for b, op, p in entries:
            slot[b, op] = p
        for p, plane in enumerate(planes):
            flat[4 * nslot + p * H * W:4 * nslot + (p + 1) * H * W] = plane.reshape(-1)
        d = buf.to(dev, non_blocking=True)
        return cls(d[4 * nslot:].view(n, H, W), d[:4 * nslot].view(torch.int32).view(len(mask_dict), int(n_vocab)), (H, W))

    @classmethod
    def from_collated(cls, blob, n_vocab, device=None):
        """GIERDataset.collate's output as a table: its 'mask_rle' entries (is_load_mask='rle': run lengths, the device
        path) when present, else its ready 'mask_dict' planes."""
        size = tuple(blob['input'].shape[-2:])
        if 'mask_rle' in blob:
            return cls.from_rle(blob['mask_rle'], size, n_vocab, device)
        return cls.from_arrays(blob['mask_dict'], size, n_vocab, device)


# ------------------------------------------------------------------ the index
class GIER(object):
    """data/GIER/GIER.py:28-413.  Directory layout as the reference's: data_dir/{images, masks, splits}.
    is_load_mask: False, True (ready union planes in 'mask_dict', built on the host) or 'rle' ('mask_rle': the run lengths
    and annotated ids per operator, for MaskTable.from_rle).  mask_size: see the module text."""

    def __init__(self, data_dir, vocab_dir, phase, data_mode, is_load_mask, session, train_img_size=128, mask_size=None):
        self.op_max_len = 10
        self.req_max_len = 15
        self.session, self.phase, self.data_mode = session, phase, data_mode
        self.img_dir = os.path.join(data_dir, 'images')
        self.mask_dir = os.path.join(data_dir, 'masks')
        self.feature_dir = os.path.join(data_dir, 'features')
        self.split_dir = os.path.join(data_dir, 'splits')
        self.op_data = self.load_ops(phase, data_mode, session)
        self.vocab2id, self.id2vocab, self.op_vocab2id, self.id2op_vocab = self.load_vocab(vocab_dir)
        self.create_index(self.op_data)
        self.define_ids(len(self.op_data))
        self.train_img_size = train_img_size
        self.is_load_mask = is_load_mask
        self.mask_size = (mask_size, mask_size) if isinstance(mask_size, int) else mask_size

    def _split(self, name):
        with open(os.path.join(self.split_dir, name)) as f:
            return json.load(f)

    def load_ops(self, phase, data_mode, session):
        op_data = self._split('{}_sess_{}.json'.format(phase, session))
        families = {'valid': '{}_Ids_L1Thr_0.06_sess_{}.json', 'shapeAlign_nonCrop': '{}_shapeAlignNonCrop_sess_{}.json',
                    'shapeAlign': '{}_shapeAlign_sess_{}.json', 'global': '{}_global_sess_{}.json'}
        idxs = []
        for mode in data_mode.split('+'):
            if mode == 'full':
                idx = range(len(op_data))
            elif mode in families:
                idx = self._split(families[mode].format(phase, session))
            else:
                raise ValueError('{} is not recognize'.format(mode))
            idxs.append(set(int(i) for i in idx))
        idx = sorted(reduce(lambda x, y: x.intersection(y), idxs))
        return [op_data[i] for i in idx]

    def load_vocab(self, vocab_dir):
        with open(os.path.join(vocab_dir, 'GIER_vocabs_sess_{}.json'.format(self.session))) as f:
            vocab = json.load(f)
        with open(os.path.join(vocab_dir, 'GIER_operator_vocabs_sess_{}.json'.format(self.session))) as f:
            op_vocab = json.load(f)
        vocab2id = {token: i for i, token in enumerate(vocab)}
        id2vocab = {i: token for i, token in enumerate(vocab)}
        op_vocab2id = {token: i for i, token in enumerate(op_vocab)}
        id2op_vocab = {i: token for i, token in enumerate(op_vocab)}
        return vocab2id, id2vocab, op_vocab2id, id2op_vocab

    def req2idx(self, sent):
        ids = np.array([self.vocab2id.get(tok, 3) for tok in D.parse_sent(sent)], dtype=int)
        sent_idx = np.zeros(self.req_max_len, dtype=int)
        sent_idx[:min(len(ids), self.req_max_len)] = ids[:self.req_max_len]
        return sent_idx

    def define_ids(self, id_len):
        self.pair_ids = np.arange(id_len)
        self.req_ids = reduce(lambda x, y: x + y, [self.PairId2ReqId[i] for i in self.pair_ids], [])

    def filter_operator(self, op_list):
        return [op for op in op_list.keys() if op in self.op_vocab2id]

    def create_index(self, op_data):
        imgs = np.unique([name for d in op_data for name in (d['input'], d['output'])]) if op_data else []
        getImgId = {name: i for i, name in enumerate(imgs)}
        ReqId2PairId, ImgId2PairId, OpReqId2ReqId, OpReqId2OpId, OpId2PairId = {}, {}, {}, {}, {}
        getOpReq, getOp, getReq, getReqIdx = {}, {}, {}, {}
        req_id = op_req_id = op_id = 0
        for pair_i, d in enumerate(op_data):
            op_id_start = op_id
            ops = self.filter_operator(d['operator'])
            for op in ops:
                OpId2PairId[op_id] = pair_i
                getOp[op_id] = op
                op_id += 1
            if d['expert_summary'] == [] and d['amateur_summary'] == []:
                raise ValueError('GIER: record %d has no request' % pair_i)       # (the reference stops in pdb here)
            for req in d['expert_summary'] + d['amateur_summary']:
                getReq[req_id] = req
                getReqIdx[req_id] = self.req2idx(req)
                ReqId2PairId[req_id] = pair_i
                ImgId2PairId[getImgId[d['input']]] = pair_i
                ImgId2PairId[getImgId[d['output']]] = pair_i
                for op_i, op in enumerate(ops):
                    OpReqId2ReqId[op_req_id] = req_id
                    OpReqId2OpId[op_req_id] = op_id_start + op_i
                    getOpReq[op_req_id] = op
                    op_req_id += 1
                req_id += 1
        PairId2ReqId = {}
        for req_id, pair_id in ReqId2PairId.items():
            PairId2ReqId.setdefault(pair_id, []).append(req_id)
        self.getImgId, self.getReq, self.getReqIdx, self.getOpReq, self.getOp = getImgId, getReq, getReqIdx, getOpReq, getOp
        self.ImgId2PairId, self.ReqId2PairId, self.PairId2ReqId = ImgId2PairId, ReqId2PairId, PairId2ReqId
        self.OpReqId2ReqId, self.OpReqId2OpId, self.OpId2PairId = OpReqId2ReqId, OpReqId2OpId, OpId2PairId

    def OpId2OpIdx(self, op_id):
        return self.op_vocab2id[self.getOp[op_id]]

    def get_mask(self, pair_id, operator):
        mask_dict = self.op_data[pair_id]['operator'][operator]
        return mask_dict['local'], mask_dict['ids']

    def get_op_info(self, pair_id):
        """(operator_idx (op_max_len), is_local (op_max_len), {operator vocabulary id: mask ids}) -- GIER.py:331-352."""
        operator_idx, is_local_list, mask_dict = [], [], {}
        for op in self.op_data[pair_id]['operator']:
            if op in self.op_vocab2id:
                operator_idx.append(self.op_vocab2id[op])
                is_local, mask_ids = self.get_mask(pair_id, op)
                is_local_list.append(int(is_local))
                if is_local:
                    mask_dict[int(self.op_vocab2id[op])] = mask_ids
        operator_idx += [0] * (self.op_max_len - len(operator_idx))
        is_local_list += [0] * (self.op_max_len - len(is_local_list))
        return operator_idx, is_local_list, mask_dict

    def load_mask_rles(self, name):
        """The candidate masks of image `name` as the mask file holds them (run lengths; nothing is decoded)."""
        with open(os.path.join(self.mask_dir, '{}_{}_mask.json'.format(name, name))) as f:
            return json.load(f)

    def resize_and_union_mask(self, mask_ids, name, size):
        return resize_and_union_mask_host(self.load_mask_rles(name), mask_ids, size)

    def _masks(self, return_dict, mask_dict, input, size):
        if not self.is_load_mask:
            return
        name = input.split('_')[0]
        size = self.mask_size or size
        if self.is_load_mask == 'rle':
            rles = self.load_mask_rles(name) if mask_dict else []
            return_dict['mask_rle'] = {op: (rles, ids) for op, ids in mask_dict.items()}
            return
        return_dict['mask_dict'] = {op: self.resize_and_union_mask(ids, name, size).astype(np.float32) for op, ids in mask_dict.items()}

    def get_req_item(self, req_id):
        """GIER.py:355-388: 'input' / 'output' (3,h,w), 'is_local', 'op_idx', 'request', 'request_idx' (+ masks)."""
        req_idx = self.getReqIdx[req_id].tolist()
        pair_id = self.ReqId2PairId[req_id]
        input, output = self.op_data[pair_id]['input'], self.op_data[pair_id]['output']
        input_path, output_path = os.path.join(self.img_dir, input), os.path.join(self.img_dir, output)
        if self.phase == 'train':
            input_img, output_img = D.load_image(input_path, self.train_img_size), D.load_image(output_path, self.train_img_size)
        else:
            input_img = D.load_image_short_side(input_path)
            output_img = D.load_image(output_path, tuple(input_img.shape[1:]))
        op_idx, is_local, mask_dict = self.get_op_info(pair_id)
        return_dict = {'input': input_img, 'output': output_img, 'is_local': is_local, 'op_idx': op_idx,
                       'request': self.getReq[req_id], 'request_idx': req_idx}
        self._masks(return_dict, mask_dict, input, tuple(input_img.shape[1:]))
        return return_dict

    def get_pair_item(self, pair_id):
        """GIER.py:391-410 (training size for both images, every request of the pair)."""
        d = self.op_data[pair_id]
        input_img = D.load_image(os.path.join(self.img_dir, d['input']), self.train_img_size)
        output_img = D.load_image(os.path.join(self.img_dir, d['output']), self.train_img_size)
        op_idx, is_local, mask_dict = self.get_op_info(pair_id)
        return_dict = {'input': input_img, 'output': output_img, 'is_local': is_local, 'op_idx': op_idx,
                       'request': d['expert_summary'] + d['amateur_summary']}
        self._masks(return_dict, mask_dict, d['input'], tuple(input_img.shape[1:]))
        return return_dict

    def __len__(self):
        return len(self.op_data)


# ------------------------------------------------------------------ datasets
def _pad(idx):
    """pad_req / pad_op (GIERdataset.py:30-46): END (2) in front of the first 0 (appended when there is none), START (1) first."""
    end = np.where(np.array(idx) == 0)[0]
    if len(end) > 0:
        idx.insert(int(end[0]), 2)
    else:
        idx.append(2)
    idx.insert(0, 1)
    return idx


def _collate(batch, arrays=False):
    blob = {}
    for key in batch[0]:
        v = batch[0][key]
        if type(v) in (dict, list, str):
            blob[key] = [b[key] for b in batch]
        elif type(v) == torch.Tensor:
            blob[key] = torch.stack([b[key] for b in batch])
        elif arrays and type(v) == np.ndarray:
            blob[key] = torch.stack([torch.from_numpy(b[key]) for b in batch])
        elif arrays:
            raise TypeError('{} cannot be collated'.format(type(v)))
    return blob


class GIERDataset(Dataset):
    """datasets/GIERdataset.py:19-76: one item per request."""

    def __init__(self, data_dir, vocab_dir, phase, data_mode, is_load_mask, session, train_img_size=128, mask_size=None):
        self.op_max_len, self.req_max_len = OP_MAX_LEN, 15
        self.session, self.phase, self.train_img_size = session, phase, train_img_size
        self.GIER = GIER(data_dir, vocab_dir, phase, data_mode, is_load_mask, session, train_img_size, mask_size)
        self.vocab2id, self.id2vocab, self.op_vocab2id, self.id2op_vocab = \
            self.GIER.vocab2id, self.GIER.id2vocab, self.GIER.op_vocab2id, self.GIER.id2op_vocab

    pad_req = staticmethod(_pad)
    pad_op = staticmethod(_pad)

    def collate(self, batch):
        return _collate(batch)

    def __len__(self):
        return len(self.GIER.ReqId2PairId)

    def _item(self, item):
        dic = self.GIER.get_req_item(item)
        rle = dic.pop('mask_rle', None)                      # shared run-length lists: not copied
        dic = copy.deepcopy(dic)
        if rle is not None:
            dic['mask_rle'] = rle
        dic['request_idx'] = torch.tensor(self.pad_req(dic['request_idx']))
        return dic

    def __getitem__(self, item):
        return self._item(item)


class GIERDatasetAct(GIERDataset):
    """datasets/GIERdataset.py:92-201: GIERDataset + the planned actions of <act_dir>/<data_id>/acts.json."""

    def __init__(self, data_dir, vocab_dir, act_dir, phase, data_mode, is_load_mask, session, train_img_size=128, mask_size=None):
        super().__init__(data_dir, vocab_dir, phase, data_mode, is_load_mask, session, train_img_size, mask_size)
        self.act_dir = act_dir
        self.actions, self.act2pn = list(ACTIONS), dict(ACT2PN)

    def collate(self, batch):
        return _collate(batch, arrays=True)

    def get_plan(self, item):
        """(op_seq (op_max_len+2), params (op_max_len,24), trunc_len, item_dir): 'init distance' and the top 'operation
        sequence', truncated by data.analyze_traj (at most op_max_len = 8), colour / tone parameters divided by their
        largest magnitude, a one-parameter value beyond +-5 replaced by 0; the pictures of the kept steps are
        item_dir/edit{k}.jpg, k < trunc_len.  No picture is read."""
        pair_id = self.GIER.ReqId2PairId[item]
        data_id = self.GIER.op_data[pair_id]['input'].split('_')[0]
        item_dir = os.path.join(self.act_dir, '{}'.format(data_id))
        with open(os.path.join(item_dir, 'acts.json')) as f:
            record = json.load(f)
        seq = record['operation sequence'][0]
        seq_dist = [record['init distance']] + [v[-1] for v in seq]
        trunc_len = min(D.analyze_traj(seq_dist), self.op_max_len)
        seq = seq[:trunc_len]
        params = np.zeros((self.op_max_len, 24), dtype=np.float32)
        op_seq = np.zeros(self.op_max_len + 2, dtype=int)
        for i, act in enumerate(seq):
            op_seq[i + 1] = self.actions.index(act[0]) + 3
            n = self.act2pn[act[0]]
            if act[0] in ('color', 'tone'):
                params[i, :n] = np.array(act[1]) / np.abs(np.array(act[1])).max()
            elif np.abs(act[1][0]) > 5:
                params[i, :n] = np.array([0])
            else:
                params[i, :n] = np.array(act[1])
        op_seq[0] = 1
        op_seq[len(seq) + 1] = 2
        return op_seq, params, trunc_len, item_dir

    def get_act(self, item):
        """(op_seq, params, imgs (op_max_len,3,S,S)): get_plan and the pictures of its steps, zeros beyond the truncation."""
        op_seq, params, trunc_len, item_dir = self.get_plan(item)
        imgs = torch.zeros(self.op_max_len, 3, self.train_img_size, self.train_img_size, dtype=torch.float32)
        for i in range(trunc_len):
            imgs[i] = D.load_image(os.path.join(item_dir, 'edit{}.jpg'.format(i)), self.train_img_size)
        return op_seq, params, imgs

    def __getitem__(self, item):
        dic = self._item(item)
        ops, params, imgs = self.get_act(item)
        dic['output'] = torch.cat([imgs, dic['output'].unsqueeze(0)])       # the last image is the target
        dic['operations'] = ops
        dic['parameters'] = params
        return dic


class _Tuples(Dataset):
    """A GIER dataset as the tuples the train / evaluation loops take: (img_x, img_y, x, req) or, with actions,
    (img_x, img_ys, x, ops, params, req).  with_masks: a trailing dict, the item's 'mask_rle' (batch size 1 loops; batches
    through collate_masks)."""

    def __init__(self, base, with_masks=False):
        self.base, self.with_masks = base, with_masks

    def __len__(self):
        return len(self.base)

    def __getitem__(self, i):
        d = self.base[i]
        if 'operations' in d:
            t = d['input'], d['output'], d['request_idx'], torch.from_numpy(d['operations']), torch.from_numpy(d['parameters']), d['request']
            return t + (d.get('mask_rle', {}),) if self.with_masks else t
        if self.with_masks:
            return d['input'], d['output'], d['request_idx'], d['request'], d.get('mask_rle', {})
        return d['input'], d['output'], d['request_idx'], d['request']


def collate_masks(batch):
    """DataLoader collate for _Tuples(..., with_masks=True): the tensors stacked as the default collate stacks them, each
    item's 'mask_rle' dict kept as it is in a list beside them -- what MaskTable.from_rle takes (the operators differ from
    item to item, so the dicts cannot be merged key by key)."""
    from torch.utils.data import default_collate
    return tuple(default_collate([item[:-1] for item in batch])) + ([item[-1] for item in batch],)


# ------------------------------------------------------------------ the training set on the device
RESIDENT_UNION_JOBS = 65535                      # planes per functional.rle_union_u8 launch of the build


class _Files(Dataset):
    """Decoded pictures by path: all a worker of the resident build does."""

    def __init__(self, paths):
        self.paths = paths

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        return D.decode_image(self.paths[i])


def _collate_files(images):
    """A chunk of decoded pictures as data.collate_raw packs them: one byte buffer headed by its descriptor table, and the
    table as an (n,4) int32 tensor."""
    from . import functional as T
    buffer, descs = T.pack_u8(images, pin=False)
    return buffer, torch.from_numpy(descs.view(np.int32).reshape(-1, 4).copy())


class ResidentGIER(D.ResidentFiveK):
    """The training items of a GIERDatasetAct (phase 'train') on the device, served as batches by index: the GIER form of
    data.ResidentFiveK, whose epoch order, sharding and index staging it keeps (batch_indices, __iter__, __len__).

    Pictures.  GIER has one item per REQUEST: the requests of a pair share all ten pictures, pairs on one input share the
    input and the planned steps of act_dir/<data_id>.  The store holds ONE slot of data.resident_slot_bytes(S) per distinct
    file path (uint8 HWC); .slots (N,10) int64 on the device names them per item -- column 0 the input, 1..8 the planned
    steps (-1 at and beyond get_plan's truncation), 9 the target.  Build: workers decode in chunks; per chunk one upload,
    the resize launch and functional.to_u8_hwc into the store (ResidentFiveK's path), so a gathered picture has the bits of
    data.load_image(path, S).

    Masks (a dataset made with is_load_mask='rle').  One uint8 (S,S) union plane per distinct (input name, mask ids),
    .planes (P,S,S), written by functional.rle_union_u8 launches of at most 65535 jobs straight into the store; .rows
    (N,V) int32 on the device holds, per item and operator vocabulary id, the plane's number or -1.  Without masks there
    are neither planes nor rows.

    fetch / iteration yield [img_x, img_ys (B,9,3,S,S), request_idx, ops, params, requests] -- what
    collate_masks / the default collation of _Tuples(dataset) gives for the same items, the pictures on the device -- and,
    with masks, a MaskTable(planes = the WHOLE plane store, slot = the items' rows) behind them: one small non-blocking
    index upload and ONE functional.gather_items_u8 launch per batch, nothing uploaded or launched for the masks, every
    shape the same for every batch.

    memory_limit: bytes the set may take on the device (.nbytes: pictures, planes and both tables); default half of the
    device's free memory.  A larger set is refused with a ValueError before anything is allocated or decoded.  Reports
    .nbytes, .build_seconds, .n_pictures, .n_planes."""

    K = OP_MAX_LEN + 2

    def __init__(self, dataset, size, batch_size, device=None, seed=0, rank=0, world=1, drop_last=True, num_workers=4,
                 chunk_pictures=64, memory_limit=None, n_vocab=None):
        from torch.utils.data import DataLoader
        from . import functional as T
        import time
        if not isinstance(dataset, GIERDatasetAct) or dataset.phase != 'train':
            raise ValueError("ResidentGIER: the dataset must be a GIERDatasetAct in phase 'train'")
        G = dataset.GIER
        if G.is_load_mask not in (False, None, 'rle'):
            raise ValueError("ResidentGIER: masks are built on the device from run lengths: is_load_mask must be False or 'rle'")
        if size <= 0 or batch_size <= 0 or world <= 0 or not 0 <= rank < world or chunk_pictures <= 0:
            raise ValueError('ResidentGIER: size, batch_size, chunk_pictures and world must be positive and 0 <= rank < world')
        if int(size) != int(dataset.train_img_size):
            raise ValueError('ResidentGIER: size %d is not the dataset\'s train_img_size %d' % (size, dataset.train_img_size))
        tik = time.time()
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        device = torch.device(device)
        N, K, S = len(dataset), self.K, int(size)
        if N == 0:
            raise ValueError('ResidentGIER: empty dataset')
        with_masks = G.is_load_mask == 'rle'
        V = int(n_vocab) if n_vocab is not None else len(dataset.op_vocab2id)
        # ---- the index, from the split and plan files alone: which files, which planes, which item uses which
        paths, where, plans = [], {}, {}
        plane_keys, plane_of = [], {}

        def number(table, order, key):
            at = table.get(key)
            if at is None:
                at = table[key] = len(order)
                order.append(key)
            return at
        picture = np.full((N, K), -1, np.int64)
        rows = np.full((N, V), -1, np.int32) if with_masks else None
        req_idx, ops, params, reqs = [], [], [], []
        for r in range(N):
            pair_id = G.ReqId2PairId[r]
            rec = G.op_data[pair_id]
            name = rec['input'].split('_')[0]
            if name not in plans:
                plans[name] = dataset.get_plan(r)
            op_seq, par, n, item_dir = plans[name]
            picture[r, 0] = number(where, paths, os.path.join(G.img_dir, rec['input']))
            for k in range(n):
                picture[r, 1 + k] = number(where, paths, os.path.join(item_dir, 'edit{}.jpg'.format(k)))
            picture[r, K - 1] = number(where, paths, os.path.join(G.img_dir, rec['output']))
            req_idx.append(torch.tensor(_pad(G.getReqIdx[r].tolist())))
            ops.append(torch.from_numpy(op_seq))
            params.append(torch.from_numpy(par))
            reqs.append(G.getReq[r])
            if with_masks:
                for op, ids in G.get_op_info(pair_id)[2].items():
                    rows[r, MaskTable._key(op, V)] = number(plane_of, plane_keys, (name, tuple(int(i) for i in ids)))
        slot = D.resident_slot_bytes(S)
        self.n_pictures, self.n_planes = len(paths), len(plane_keys)
        self.nbytes = self.n_pictures * slot + self.n_planes * S * S + picture.nbytes + (rows.nbytes if with_masks else 0)
        limit = torch.cuda.mem_get_info(device)[0] // 2 if memory_limit is None else int(memory_limit)
        if self.nbytes > limit:
            raise ValueError('ResidentGIER: %d items at %d x %d (%d distinct pictures, %d mask planes) need %d bytes, more than the '
                             "%d allowed (half of the device's free memory unless memory_limit says otherwise); train without "
                             '--resident_gier' % (N, S, S, self.n_pictures, self.n_planes, self.nbytes, limit))
        self.size, self.batch_size, self.device, self.seed = S, int(batch_size), device, int(seed)
        self.rank, self.world, self.drop_last, self.epoch = int(rank), int(world), bool(drop_last), 0
        # ---- the pictures: decode (workers), upload, resize, to bytes -- chunk by chunk into the store
        self.store = torch.zeros(self.n_pictures * slot, dtype=torch.uint8, device=device)
        cells = self.store.view(self.n_pictures, slot)[:, :3 * S * S]
        loader = DataLoader(_Files(paths), batch_size=int(chunk_pictures), shuffle=False, collate_fn=_collate_files, pin_memory=True,
                            num_workers=max(0, min(int(num_workers), D.RESIDENT_MAX_WORKERS)))
        at = 0
        for buffer, table in loader:
            m = table.shape[0]
            dev_buffer, table_ptr, descs, keep = T.upload_packed(buffer, table, device)
            cells[at:at + m] = T.to_u8_hwc(T._resize_launch(dev_buffer, table_ptr, m, S, S)).view(m, -1)
            at += m
        self.slots = torch.from_numpy(np.where(picture >= 0, picture * slot, -1)).to(device)
        # ---- the union planes: the annotated run lengths of a chunk of planes in one upload, one launch into the store
        self.rows = self.planes = None
        if with_masks:
            self.planes = torch.zeros(self.n_planes, S, S, dtype=torch.uint8, device=device)
            for c0 in range(0, self.n_planes, RESIDENT_UNION_JOBS):
                files, masks, seen, jobs = {}, [], {}, []
                for j, (name, ids) in enumerate(plane_keys[c0:c0 + RESIDENT_UNION_JOBS]):
                    if name not in files:
                        files[name] = G.load_mask_rles(name)
                    sel = [number(seen, masks, (name, i)) for i in ids]
                    jobs.append((sel, (c0 + j) * S * S, S, S))
                T.rle_union_u8([files[name][i] for name, i in masks], jobs, device, out=self.planes.view(-1))
            self.rows = torch.from_numpy(rows).to(device)
        self.req_idx, self.ops, self.params, self.reqs = torch.stack(req_idx), torch.stack(ops), torch.stack(params), reqs
        torch.cuda.synchronize(device)
        self.build_seconds = time.time() - tik

    def fetch(self, idx, staged=None):
        """One batch for the host int64 item numbers `idx`; staged: the same numbers in pinned memory (else they are pinned here)."""
        from . import functional as T
        if staged is None:
            staged = idx.pin_memory()
        index = staged.to(self.device, non_blocking=True)
        out = T.gather_items_u8(self.store, self.slots, index, self.size, rows=self.rows)
        batch = [out[0], out[1], self.req_idx[idx], self.ops[idx], self.params[idx], [self.reqs[i] for i in idx.tolist()]]
        if self.rows is not None:
            batch.append(MaskTable(self.planes, out[2], (self.size, self.size)))
        return batch
