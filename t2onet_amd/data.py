"""The data step in front of the train loop: turning a planned-action
record into the tensors `train_seq2seqL1.py` consumes, as datasets/FiveKdataset.py:54-135 does.

Image decoding is kept behind `load_image` (PIL, bilinear resize to a square like
utils/visual_utils.py:6-14; the reference uses cv2, absent here, so pixel-exact parity of the
decode/resize is NOT claimed).  The record logic -- trajectory truncation, operator ids,
curve-parameter normalisation, outlier handling -- is restated exactly and tested against the
reference's own functions on synthetic records (tests/golden/data.npz).
"""
import json
import os

import numpy as np
import torch
from torch.utils.data import Dataset

ACTIONS = ['brightness', 'contrast', 'saturation', 'color', 'inpaint', 'tone', 'sharpness', 'white']
ACT2PN = {'brightness': 1, 'contrast': 1, 'saturation': 1, 'color': 24, 'inpaint': 0, 'tone': 8, 'sharpness': 1, 'white': 0}
OP_MAX_LEN = 5


def analyze_traj(seq):
    """Number of planned steps to keep: stop at the first step whose distance drop is not more
    than 1 % of the initial distance (FiveKdataset.py:54-64); at least 1."""
    seq = np.array(seq)
    over_shot = (seq[:-1] - seq[1:]) / seq[0]
    stops = np.where(~(over_shot > 0.01))[0]
    trunc_len = int(stops[0]) if len(stops) else len(over_shot)
    return max(trunc_len, 1)


def parse_action_record(record, op_max_len=OP_MAX_LEN):
    """record = the planner's JSON ({'init distance': d0, 'operation sequence': [[(name, params, dist), ...], ...]}).
    Returns (op_seq (op_max_len+2,) int64 = [START, ids..., END, 0...], params (op_max_len,24) float32, n_kept)
    exactly as FiveKAct.get_act (FiveKdataset.py:86-116): curve parameters divided by their max
    magnitude, one-parameter values beyond +-5 replaced by 0."""
    seq = record['operation sequence'][0]
    dists = [record['init distance']] + [v[2] for v in seq]
    trunc_len = min(analyze_traj(dists), op_max_len)
    seq = seq[:trunc_len]
    params = np.zeros((op_max_len, 24), dtype=np.float32)
    op_seq = np.zeros(op_max_len + 2, dtype=np.int64)
    for i, act in enumerate(seq):
        name, values = act[0], np.array(act[1], dtype=np.float64)
        op_seq[i + 1] = ACTIONS.index(name) + 3
        n = ACT2PN[name]
        if name in ('color', 'tone'):
            params[i, :n] = values / np.abs(values).max()
        elif abs(values[0]) > 5:
            params[i, :n] = 0.0
        else:
            params[i, :n] = values
    op_seq[0] = 1
    op_seq[len(seq) + 1] = 2
    return op_seq, params, trunc_len


def resize_linear_u8(img, out_h, out_w):
    """cv2.resize(img, (out_w, out_h)) for a uint8 (H,W,C) image with the default interpolation -- what the
    reference's loaders call (utils/visual_utils.py:9,24,42).  cv2 is absent from this image, so this restates
    OpenCV's published INTER_LINEAR algorithm for 8-bit images (imgproc/resize.cpp): half-pixel centres, NO
    antialiasing when shrinking, 11-bit fixed-point coefficients (cvRound), horizontal pass in int32, vertical pass
    ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2; and OpenCV's special case: an exact 2x shrink in both
    directions is the rounded mean of each 2x2 block (INTER_LINEAR is replaced by the fast INTER_AREA path there).
    Parity with cv2 itself is unpinned (nothing to run it against here); tests/test_data_cpu.py holds it to the
    algorithm's own properties and to float bilinear within one grey level."""
    img = np.ascontiguousarray(img)
    H, W = img.shape[:2]
    if (out_h, out_w) == (H, W):
        return img.copy()
    if H == 2 * out_h and W == 2 * out_w:
        s = img.astype(np.int32)
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)

    def taps(n_src, n_dst):
        f = (np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5
        i0 = np.floor(f).astype(np.int64)
        f = f - i0
        lo = i0 < 0
        f[lo], i0[lo] = 0.0, 0
        hi = i0 >= n_src - 1
        f[hi], i0[hi] = 0.0, n_src - 1
        i1 = np.minimum(i0 + 1, n_src - 1)
        c1 = np.rint(f * 2048.0).astype(np.int32)                  # cvRound: round half to even
        c0 = np.rint((1.0 - f) * 2048.0).astype(np.int32)
        return i0, i1, c0, c1
    x0, x1, a0, a1 = taps(W, out_w)
    y0, y1, b0, b1 = taps(H, out_h)
    src = img.astype(np.int32)
    shape = (1, out_w) + (1,) * (img.ndim - 2)
    rows = src[:, x0] * a0.reshape(shape) + src[:, x1] * a1.reshape(shape)          # (H, out_w, C) int32
    S0, S1 = rows[y0], rows[y1]
    vb = (out_h, 1) + (1,) * (img.ndim - 2)
    out = (((b0.reshape(vb) * (S0 >> 4)) >> 16) + ((b1.reshape(vb) * (S1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def decode_image(path):
    """The decoded file as a uint8 (H,W,3) RGB array (PIL / libjpeg, like cv2's decoder): everything the loaders do
    before the resize.  This part stays on the host; `raw=True` datasets hand it on as it is."""
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'), dtype=np.uint8)


def short_side_size(h, w, short_size=600):
    """(h_new, w_new) of utils/visual_utils.py:34-47: the short side scaled to `short_size`."""
    ratio = short_size / min(h, w)
    return int(np.round(h * ratio)), int(np.round(w * ratio))


def load_image(path, size=None):
    """RGB float tensor (3,H,W) in [0,1] as the reference's loaders produce it (utils/visual_utils.py:6-31:
    cv2.imread -> cv2.resize -> BGR->RGB -> /255).  `size`: None (as is), an int (square, training:
    load_train_img) or (h, w).  Decoding is PIL's (libjpeg, like cv2's); the resize is resize_linear_u8."""
    img = decode_image(path)
    if size is not None:
        h, w = (size, size) if isinstance(size, int) else size
        img = resize_linear_u8(img, h, w)
    return torch.from_numpy(img.astype(np.float32).transpose(2, 0, 1) / 255.0)


def load_image_short_side(path, short_size=600):
    """utils/visual_utils.py:34-47 (full-resolution inference): the short side scaled to `short_size`."""
    img = decode_image(path)
    img = resize_linear_u8(img, *short_side_size(img.shape[0], img.shape[1], short_size))
    return torch.from_numpy(img.astype(np.float32).transpose(2, 0, 1) / 255.0)


def parse_sent(desc):
    """Request text -> tokens as utils/text_utils.py:9-26 cleans them: whitespace split, lower case, punctuation removed
    from every token, one-letter tokens and tokens with non-letters dropped."""
    import string
    table = str.maketrans('', '', string.punctuation)
    words = [w.lower().translate(table) for w in desc.split()]
    return [w for w in words if len(w) > 1 and w.isalpha()]


def txt2idx(sent, vocab2id, max_len):
    """utils/text_utils.py:42-67: (1, max_len) token ids = START (1), the request's tokens (unknown words -> 3) cut to
    max_len - 2, END (2) right behind them, zero padding."""
    body = max_len - 2
    ids = [vocab2id.get(tok, 3) for tok in parse_sent(sent)][:body]
    row = [1] + ids + [2] + [0] * (body - len(ids))
    return torch.tensor(row, dtype=torch.long).unsqueeze(0)


class FiveKAct(Dataset):
    """(img_x, img_ys (6,3,S,S), req_idx, ops (7,), params (5,24), req) per item, like
    datasets/FiveKdataset.py:67-135.  Directory layout as the reference's:
    anno_dir/{phase}_sess_{session}.json, act_dir/{phase}{i}/{i:05d}.json + edit{k}.jpg.
    raw=True: the images stay as decoded -- img_x a uint8 (H,W,3) array, img_ys a list of 6 such arrays with None in the
    unused steps -- for collate_raw + device_batch, which resize them on the GPU."""

    def __init__(self, img_dir, anno_dir, act_dir, phase='train', session=1, train_img_size=128, raw=False):
        self.img_dir, self.act_dir, self.phase, self.size, self.raw = img_dir, act_dir, phase, train_img_size, raw
        with open(os.path.join(anno_dir, '{}_sess_{}.json'.format(phase, session))) as f:
            self.data = json.load(f)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, item):
        dic = self.data[item]
        item_dir = os.path.join(self.act_dir, '{}{}'.format(self.phase, item))
        with open(os.path.join(item_dir, '{:05d}.json'.format(item))) as f:
            ops, params, n = parse_action_record(json.load(f))
        if self.raw:
            imgs = [decode_image(os.path.join(item_dir, 'edit{}.jpg'.format(k))) for k in range(n)] + [None] * (OP_MAX_LEN - n)
            imgs.append(decode_image(os.path.join(self.img_dir, dic['output'])))
            img_x = decode_image(os.path.join(self.img_dir, dic['input']))
            return img_x, imgs, np.array(dic['request_idx']), ops, params, dic['request']
        imgs = torch.zeros(OP_MAX_LEN + 1, 3, self.size, self.size)
        for k in range(n):
            imgs[k] = load_image(os.path.join(item_dir, 'edit{}.jpg'.format(k)), self.size)
        imgs[OP_MAX_LEN] = load_image(os.path.join(self.img_dir, dic['output']), self.size)
        img_x = load_image(os.path.join(self.img_dir, dic['input']), self.size)
        return img_x, imgs, np.array(dic['request_idx']), ops, params, dic['request']


class FiveK(Dataset):
    """(img_x, img_y, req_idx, req) per item with NO planned actions, like datasets/FiveKdataset.py:24-52: the split the
    reference validates and tests on (train_seq2seqL1.py:155-156, batch_size=1).  phase 'train': square training size;
    any other phase: full resolution with the short side scaled to 600 pixels (load_infer_img_short_size_bounded).
    raw=True: both images stay uint8 (H,W,3) arrays as decoded (collate_raw + device_batch resize them on the GPU)."""

    def __init__(self, img_dir, anno_dir, phase='val', session=1, train_img_size=128, short_size=600, raw=False):
        self.img_dir, self.phase, self.size, self.short_size, self.raw = img_dir, phase, train_img_size, short_size, raw
        with open(os.path.join(anno_dir, '{}_sess_{}.json'.format(phase, session))) as f:
            self.data = json.load(f)

    def __len__(self):
        return len(self.data)

    def _load(self, name):
        path = os.path.join(self.img_dir, name)
        if self.raw:
            return decode_image(path)
        return load_image(path, self.size) if self.phase == 'train' else load_image_short_side(path, self.short_size)

    def __getitem__(self, item):
        dic = self.data[item]
        return self._load(dic['input']), self._load(dic['output']), np.array(dic['request_idx']), dic['request']


def collate_raw(items):
    """collate_fn of a DataLoader over a raw=True dataset: every image of the batch packed back to back into one byte
    buffer headed by its descriptor table (functional.pack_u8), in the order of device_batch's output -- all img_x first,
    then item by item the 6 img_ys (FiveKAct; an unused step is an absent descriptor, h = w = 0) or the img_y (FiveK).
    Returns {'buffer': uint8 tensor, 'descs': (n,4) int32 tensor = the table, 'items': B, 'rest': the default collation of
    the items' other fields}.  Unpinned (it runs in workers): DataLoader(pin_memory=True) pins it."""
    from torch.utils.data import default_collate
    from . import functional as T
    act = len(items[0]) == 6
    images = [it[0] for it in items]
    if act:
        images += [im for it in items for im in it[1]]
    else:
        images += [it[1] for it in items]
    buffer, descs = T.pack_u8(images, pin=False)
    table = torch.from_numpy(descs.view(np.int32).reshape(-1, 4).copy())
    return {'buffer': buffer, 'descs': table, 'items': len(items), 'rest': default_collate([tuple(it[2:]) for it in items])}


def device_batch(batch, size=None, device=None, short_size=None, images_only=False):
    """A collate_raw batch as exactly the tensors the default DataLoader batch of the same items holds, on the device:
    [img_x, img_ys (B,6,3,S,S), req_idx, ops, params, reqs] (FiveKAct) or [img_x, img_y, req_idx, reqs] (FiveK).  One
    upload of the packed bytes and one resize launch (functional.resize_u8) replace the per-image host resizes.
    size: int or (h, w) -- every image resized to it.  short_size (instead of size): FiveK(phase != 'train'), one item
    per batch as the reference evaluates: each image to short_side_size of its own shape, one launch of N = 1 per image.
    images_only: leave the other tensors where the collation put them (the train loop reads lengths on the host)."""
    from . import functional as T
    B = batch['items']
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if short_size is None:
        out = T.resize_u8((batch['buffer'], batch['descs']), size, device)
        img_x, second = out[:B], out[B:]
        if second.shape[0] != B:
            second = second.view(B, second.shape[0] // B, *second.shape[1:])
    else:
        if B != 1:
            raise ValueError('device_batch: the short-side form takes one item per batch (images of differing sizes)')
        dev_buffer, table_ptr, descs, keep = T.upload_packed(batch['buffer'], batch['descs'], device)
        if descs.size != 2:
            raise ValueError('device_batch: the short-side form serves FiveK items (img_x, img_y)')
        outs = [T._resize_launch(dev_buffer, table_ptr + i * T.IMAGE_DESC.itemsize, 1,
                                 *short_side_size(int(descs['h'][i]), int(descs['w'][i]), short_size)) for i in range(2)]
        img_x, second = outs
    rest = [v if images_only or not torch.is_tensor(v) else v.to(device, non_blocking=True) for v in batch['rest']]
    return [img_x, second] + rest


class DeviceBatches(object):
    """A DataLoader of collate_raw batches, iterated as device_batch(...) results."""

    def __init__(self, loader, size=None, device=None, short_size=None, images_only=False):
        self.loader, self.kw = loader, dict(size=size, device=device, short_size=short_size, images_only=images_only)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            yield device_batch(batch, **self.kw)


RESIDENT_MAX_WORKERS = 16


def resident_slot_bytes(size):
    """Bytes between two slots of a resident store of size x size pictures: 3 S S rounded up to the 16-byte boundary every
    slot starts on (functional.gather_u8 reads a slot as aligned dwords)."""
    return (3 * size * size + 15) // 16 * 16


def epoch_order(n, seed, epoch, rank=0, world=1):
    """The items rank `rank` of `world` visits in `epoch`, in order: torch.randperm(n) seeded with seed + epoch, made on
    the host; rank r takes every world-th one from the r-th on, all ranks cut to the same n // world."""
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed) + int(epoch)))
    return perm[rank::world][:n // world].contiguous()


class ResidentFiveK(object):
    """The whole training split of a FiveKAct(..., raw=True) on the device, resized once, served as batches by index.

    Build (once, in __init__): a DataLoader of collate_raw chunks (the workers only decode), per chunk one upload
    (functional.upload_packed), the resize launch to (n,3,S,S) fp32 and functional.to_u8_hwc into the store -- byte for
    byte what a batch's resize would hold: trunc((b / 255) * 255) = b for all 256 bytes in fp32.  Kept: the store (N x 7
    slots of resident_slot_bytes(S), dense, on the device), the (N,7) slot table (on the device; -1 = an unused step) and
    the items' small tensors and request strings on the host (the train loop reads lengths there).

    Iterating yields, per batch, [img_x, img_ys, req_idx, ops, params, reqs] equal to
    device_batch(collate_raw(items), S, images_only=True) for the same items in the same order: one small non-blocking
    index upload from pinned memory and one functional.gather_u8 launch; no picture crosses the bus and nothing waits on
    the host.  The order of epoch e is epoch_order(N, seed, e, rank, world); every rank holds the whole set.  Each
    iter() serves the next epoch.

    memory_limit: bytes the store may take; default half of the device's free memory.  A larger store is refused with a
    ValueError before anything is allocated or decoded."""

    K = OP_MAX_LEN + 2

    def __init__(self, dataset, size, batch_size, device=None, seed=0, rank=0, world=1, drop_last=True, num_workers=4,
                 chunk_items=16, memory_limit=None):
        from torch.utils.data import DataLoader
        from . import functional as T
        import time
        if not getattr(dataset, 'raw', False):
            raise ValueError('ResidentFiveK: the dataset must hand out decoded bytes (FiveKAct(..., raw=True))')
        if size <= 0 or batch_size <= 0 or world <= 0 or not 0 <= rank < world:
            raise ValueError('ResidentFiveK: size, batch_size and world must be positive and 0 <= rank < world')
        tik = time.time()
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        device = torch.device(device)
        N, K, S = len(dataset), self.K, int(size)
        if N == 0:
            raise ValueError('ResidentFiveK: empty dataset')
        slot = resident_slot_bytes(S)
        self.nbytes = N * K * slot
        limit = torch.cuda.mem_get_info(device)[0] // 2 if memory_limit is None else int(memory_limit)
        if self.nbytes > limit:
            raise ValueError('ResidentFiveK: %d items at %d x %d need a store of %d bytes, more than the %d allowed (half of the '
                             "device's free memory unless memory_limit says otherwise); train without --resident"
                             % (N, S, S, self.nbytes, limit))
        self.size, self.batch_size, self.device, self.seed = S, int(batch_size), device, int(seed)
        self.rank, self.world, self.drop_last, self.epoch = int(rank), int(world), bool(drop_last), 0
        self.store = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        cells = self.store.view(N, K, slot)[:, :, :3 * S * S]
        slots = torch.arange(N * K, dtype=torch.int64).view(N, K) * slot
        loader = DataLoader(dataset, batch_size=int(chunk_items), shuffle=False, collate_fn=collate_raw, pin_memory=True,
                            num_workers=max(0, min(int(num_workers), RESIDENT_MAX_WORKERS)))
        rest, at = [], 0
        for chunk in loader:
            m = chunk['items']
            dev_buffer, table_ptr, descs, keep = T.upload_packed(chunk['buffer'], chunk['descs'], device)
            if descs.size != m * K:
                raise ValueError('ResidentFiveK: an item must hold %d pictures (FiveKAct)' % K)
            u8 = T.to_u8_hwc(T._resize_launch(dev_buffer, table_ptr, m * K, S, S)).view(m * K, -1)
            cells[at:at + m, 0] = u8[:m]                                   # collate_raw's order: every img_x, then 6 img_ys per item
            cells[at:at + m, 1:] = u8[m:].view(m, K - 1, -1)
            absent = torch.from_numpy(np.ascontiguousarray(descs['h'] == 0))
            slots[at:at + m, 0][absent[:m]] = -1
            slots[at:at + m, 1:][absent[m:].view(m, K - 1)] = -1
            rest.append(chunk['rest'])
            at += m
        self.slots = slots.to(device)
        self.req_idx, self.ops, self.params = (torch.cat([r[j] for r in rest]) for j in range(3))
        self.reqs = [s for r in rest for s in r[3]]
        torch.cuda.synchronize(device)
        self.build_seconds = time.time() - tik

    def __len__(self):
        n = len(self.reqs) // self.world
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def batch_indices(self, epoch):
        """The (host, int64) item numbers of every batch of `epoch` on this rank, in order."""
        order = epoch_order(len(self.reqs), self.seed, epoch, self.rank, self.world)
        return [order[i * self.batch_size:(i + 1) * self.batch_size] for i in range(len(self))]

    def fetch(self, idx, staged=None):
        """One batch for the host int64 item numbers `idx`; staged: the same numbers in pinned memory (else they are pinned here)."""
        from . import functional as T
        if staged is None:
            staged = idx.pin_memory()
        index = staged.to(self.device, non_blocking=True)
        img_x, img_ys = T.gather_u8(self.store, self.slots, index, self.size)
        return [img_x, img_ys, self.req_idx[idx], self.ops[idx], self.params[idx], [self.reqs[i] for i in idx.tolist()]]

    def __iter__(self):
        epoch, self.epoch = self.epoch, self.epoch + 1
        batches = self.batch_indices(epoch)
        if not batches:
            return
        staged = torch.cat(batches).pin_memory()                           # the epoch's indices: one pinned block, a slice per batch
        at = 0
        for idx in batches:
            yield self.fetch(idx, staged[at:at + idx.numel()])
            at += idx.numel()


class SyntheticFiveK(Dataset):
    """FiveK-shaped random items: what bench.py and the tests train on."""

    def __init__(self, n=256, size=128, seed=10, vocab=918, req_len=17):
        self.n, self.size, self.seed, self.vocab, self.req_len = n, size, seed, vocab, req_len

    def __len__(self):
        return self.n

    def __getitem__(self, item):
        g = torch.Generator().manual_seed(self.seed * 100003 + item)
        S = self.size
        img_x = torch.rand(3, S, S, generator=g)
        imgs = torch.rand(OP_MAX_LEN + 1, 3, S, S, generator=g)
        k = int(torch.randint(1, self.req_len - 1, (1,), generator=g))
        x = torch.zeros(self.req_len, dtype=torch.long)
        x[0] = 1
        x[1:1 + k] = torch.randint(4, self.vocab, (k,), generator=g)
        x[1 + k] = 2
        pool = torch.tensor([3, 4, 5, 6, 8, 9])[torch.randperm(6, generator=g)[:OP_MAX_LEN]]
        ops = torch.cat([torch.tensor([1]), pool, torch.tensor([2])])
        params = torch.zeros(OP_MAX_LEN, 24)
        npar = {3: 1, 4: 1, 5: 1, 6: 24, 8: 8, 9: 1}
        for i, o in enumerate(pool.tolist()):
            params[i, :npar[o]] = torch.rand(npar[o], generator=g) * 2 - 1
        return img_x, imgs, x, ops, params, 'synthetic request'
