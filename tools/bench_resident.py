"""One FiveK train batch (64 items x 7 pictures), three ways ("Resident training set"; figures in
profiles/resident_set.txt):

    python tools/bench_resident.py [--runs 20] [--inner 10] [--items 1024] [--out profiles/resident_set.txt]

  (a) gather       functional.gather_u8 out of a resident store of --items items (random bytes, every slot present: the most
                   traffic a batch can cost), a fresh random batch per launch.
  (b) descriptors  the same batches through what the data step had before: the store's (N 7, 4) descriptor table,
                   index_select of the batch's rows, t2o_resize_u8_to_f32 copying same-size sources.  torch.equal to (a)
                   before anything is timed.
  (a) and (b) alternate, --runs runs of --inner launches each between two HIP events after a warm-up run; median and range
  per launch.  GB/s of (a) counts 15 B per pixel (3 read, 12 written) against BASELINE.md's 8 TB/s.
  (c) loader       the whole --device_resize batch from a FiveK-layout tree of 500 x 333 JPEGs written here: decode in
                   DataLoader workers (16, a batch per worker: wall time per batch in steady state; and one process alone),
                   collate_raw, the upload and the resize launch, each per batch; then the same tree as a ResidentFiveK:
                   build time and the wall time of a whole batch fetch, synchronised.
At 128 x 128 and at 256 x 256."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from t2onet_amd import data                     # noqa: E402
from t2onet_amd import functional as T          # noqa: E402

B, K = 64, 7
HBM = 8e12                                      # BASELINE.md, "Roofline denominators"
SRC_H, SRC_W = 333, 500
WORKERS = 16


def summary(xs, unit=1e6, name='us'):
    return '%9.2f %s (%.2f - %.2f)' % (statistics.median(xs) * unit, name, min(xs) * unit, max(xs) * unit)


def bench_gather(S, items, runs, inner, dev, say):
    slot = data.resident_slot_bytes(S)
    store = torch.randint(0, 256, (items * K * slot,), dtype=torch.uint8, device=dev)
    slots = (torch.arange(items * K, dtype=torch.int64, device=dev) * slot).view(items, K)
    rec = np.zeros(items * K, T.IMAGE_DESC)
    rec['offset'], rec['h'], rec['w'] = np.arange(items * K, dtype=np.int64) * slot, S, S
    table = torch.from_numpy(rec.view(np.int32).reshape(-1, 4).copy()).to(dev)
    g = torch.Generator().manual_seed(S)
    batches = [torch.randperm(items, generator=g)[:B].to(dev) for _ in range((runs + 1) * inner)]
    col = torch.arange(K, device=dev)[None, :]
    x, ys = torch.empty(B, 3, S, S, device=dev), torch.empty(B, K - 1, 3, S, S, device=dev)
    flat = torch.empty(B * K, 3, S, S, device=dev)

    def gather(index):
        T.gather_u8(store, slots, index, S, out=(x, ys))

    def descriptors(index):
        picked = table.index_select(0, (index[:, None] * K + col).reshape(-1))
        T._resize_launch(store, picked.data_ptr(), B * K, S, S, flat)

    for index in batches[:3]:                                            # equal before anything is timed
        gather(index)
        descriptors(index)
        both = flat.view(B, K, 3, S, S)
        assert torch.equal(x, both[:, 0]) and torch.equal(ys, both[:, 1:]), 'gather and descriptor path differ'
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, group):
        torch.cuda.synchronize()
        e0.record()
        for index in group:
            fn(index)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / len(group)
    ta, tb = [], []
    for r in range(runs + 1):                                            # run 0 warms both ways up
        group = batches[r * inner:(r + 1) * inner]
        a, b = timed(gather, group), timed(descriptors, group)
        if r:
            ta.append(a)
            tb.append(b)
    nbytes = 15 * B * K * S * S
    rate = nbytes / statistics.median(ta)
    say('%d x %d, batch of %d items x %d pictures out of a %d-item store (%.0f MB), %d runs of %d launches' % (
        S, S, B, K, items, store.numel() / 1e6, runs, inner))
    say('  (a) gather_u8                          %s per batch' % summary(ta))
    say('  (b) index_select + resize_u8_to_f32    %s per batch' % summary(tb))
    say('  (a) moves %.1f MB per batch: %.0f GB/s on 15 B/px = %.0f %% of %.0f TB/s' % (nbytes / 1e6, rate / 1e9, 100 * rate / HBM, HBM / 1e12))
    apart = max(ta) < min(tb) or max(tb) < min(ta)
    say('  ranges %s; median (b) / (a) = %.2f' % ('do not overlap' if apart else 'OVERLAP: no difference beyond the spread of the runs',
                                                  statistics.median(tb) / statistics.median(ta)))


def write_tree(root, n):
    """A FiveK-layout tree (tests/fivek_tree.py's layout) of n train items, 5 planned steps each: 7 JPEGs of 500 x 333 per item."""
    from PIL import Image
    img_dir, anno_dir, act_dir = (os.path.join(root, d) for d in ('images', 'annotations', 'actions'))
    for d in (img_dir, anno_dir, act_dir):
        os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(0)

    def jpeg(path):
        small = (rng.random((SRC_H // 8 + 2, SRC_W // 8 + 2, 3)) * 255).astype(np.uint8)
        Image.fromarray(small).resize((SRC_W, SRC_H), Image.BICUBIC).save(path, format='JPEG', quality=90)
    names = ['brightness', 'contrast', 'saturation', 'tone', 'sharpness']
    items = []
    for i in range(n):
        fin, fout = 'train%d_in.jpg' % i, 'train%d_out.jpg' % i
        jpeg(os.path.join(img_dir, fin))
        jpeg(os.path.join(img_dir, fout))
        items.append({'input': fin, 'output': fout, 'request': 'make it %d' % i, 'request_idx': [1, 5, 6, 2] + [0] * 13})
        d = os.path.join(act_dir, 'train%d' % i)
        os.makedirs(d, exist_ok=True)
        dist, seq = 0.30, []
        for s, name in enumerate(names):
            dist *= 0.6
            seq.append([name, [0.5] * (8 if name == 'tone' else 1), dist])
            jpeg(os.path.join(d, 'edit%d.jpg' % s))
        with open(os.path.join(d, '%05d.json' % i), 'w') as f:
            json.dump({'init distance': 0.30, 'operation sequence': [seq]}, f)
    with open(os.path.join(anno_dir, 'train_sess_1.json'), 'w') as f:
        json.dump(items, f)
    return img_dir, anno_dir, act_dir


def bench_loader(root, dev, say, rounds=2):
    """Leg (c).  The workers are started, and joined, before this process opens the GPU for timing the rest."""
    from torch.utils.data import DataLoader, Subset
    raw = data.FiveKAct(*write_tree(root, B), 'train', 1, 128, raw=True)
    tik = time.perf_counter()
    items = [raw[i] for i in range(B)]
    alone = time.perf_counter() - tik
    n_batches = WORKERS * (rounds + 1)
    loader = DataLoader(Subset(raw, list(range(B)) * n_batches), batch_size=B, collate_fn=data.collate_raw, num_workers=WORKERS)
    t0 = t1 = None
    for i, _ in enumerate(loader):
        if i == WORKERS - 1:                                             # every worker has delivered its first batch
            t0 = time.perf_counter()
    t1 = time.perf_counter()
    workers = (t1 - t0) / (n_batches - WORKERS)
    del loader
    collate = []
    for _ in range(5):
        tik = time.perf_counter()
        batch = data.collate_raw(items)
        collate.append(time.perf_counter() - tik)
    pinned = batch['buffer'].pin_memory()
    say('(c) the --device_resize batch: %d items x %d JPEGs of %d x %d, %.1f MB decoded' % (B, K, SRC_W, SRC_H, pinned.numel() / 1e6))
    say('  decode, one process                    %9.2f ms per batch (%.2f ms per JPEG)' % (alone * 1e3, alone * 1e3 / (B * K)))
    say('  decode + collate_raw, %2d workers       %9.2f ms per batch (steady state, %d batches, a batch per worker)' % (
        WORKERS, workers * 1e3, n_batches - WORKERS))
    say('  collate_raw (pack), one process        %s per batch' % summary(collate, 1e3, 'ms'))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out
    ups = [timed(lambda: pinned.to(dev, non_blocking=True))[0] for _ in range(6)][1:]
    say('  upload from pinned memory              %s per batch' % summary(ups, 1e3, 'ms'))
    dev_buffer, table_ptr, descs, keep = T.upload_packed(pinned, batch['descs'], dev)
    for S in (128, 256):
        out = torch.empty(B * K, 3, S, S, device=dev)
        rs = [timed(lambda: T._resize_launch(dev_buffer, table_ptr, B * K, S, S, out))[0] for _ in range(6)][1:]
        say('  resize launch to %3d x %3d             %s per batch' % (S, S, summary(rs, 1e3, 'ms')))
    for S in (128, 256):                                                 # the same tree resident: what the train loop waits for per batch
        resident = data.ResidentFiveK(raw, S, B, dev, num_workers=0)      # (built in this process: no fork once the GPU is open)
        walls = []
        for _ in range(21):                                              # an epoch of this tree is one batch; the first warms up
            torch.cuda.synchronize()
            tik = time.perf_counter()
            next(iter(resident))
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - tik)
        say('  resident at %3d x %3d: built by one process in %.2f s (%d bytes); whole fetch (host indexing, index upload, gather, synchronised) %s per batch' % (
            S, S, resident.build_seconds, resident.nbytes, summary(walls[1:], 1e3, 'ms')))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--items', type=int, default=1024)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    dev = torch.device('cuda', 0)
    loader_lines = []
    with tempfile.TemporaryDirectory() as root:                          # first: its workers fork before the GPU is opened
        bench_loader(root, dev, loader_lines.append)
    say('tools/bench_resident.py on %s' % torch.cuda.get_device_name(dev))
    for S in (128, 256):
        bench_gather(S, args.items, args.runs, args.inner, dev, say)
    for s in loader_lines:
        say(s)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
