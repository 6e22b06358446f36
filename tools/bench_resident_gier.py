"""One GIER train batch (64 items x 10 pictures + the local-edit masks), resident against today's loader (DESIGN.md,
"Resident GIER training set"; figures in profiles/resident_gier.txt):

    python tools/bench_resident_gier.py [--runs 20] [--inner 10] [--items 1024] [--note TEXT] [--out profiles/resident_gier.txt]

  (a) the new entry against the existing one: functional.gather_items_u8 (no rows) and functional.gather_u8 on the SAME store,
      K = 7, fresh random batches, torch.equal before anything is timed.  The two alternate, --runs runs of --inner launches
      each between two HIP events after a warm-up run; median and range per launch.
  (b) a GIER batch: K = 10 (every slot present: the most traffic a batch can cost), V = the operator vocabulary of the tree
      below, rows gathered in the same launch.  us per batch and GB/s on the 15 B/px moved (3 read, 12 written; the rows
      are B V ints) against BASELINE.md's 8 TB/s.
  (c) the batch `train_cli --dataset GIER --load_mask` forms today, from a GIER-layout tree of 500 x 333 JPEGs written
      here (32 pairs of two requests: 64 items): decode + host resize + collate_masks in 16 DataLoader workers (wall time
      per batch in steady state; and one process alone), MaskTable.from_rle per batch (host parsing, upload, launch,
      synchronised) -- against the whole ResidentGIER fetch (host indexing, index upload, one launch, synchronised) and its
      build time.
At 128 x 128 and at 256 x 256 ((c)'s loader at 128 x 128, the size it trains at).  --note: a line appended as it is (the
train-step time of bench.py --size 128 taken in the same session)."""
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
from t2onet_amd import data, gier               # noqa: E402
from t2onet_amd import functional as T          # noqa: E402

B = 64
HBM = 8e12                                      # BASELINE.md, "Roofline denominators"
SRC_H, SRC_W = 333, 500
WORKERS = 16
WORDS = ['<NULL>', '<START>', '<END>', '<UNK>', 'make', 'the', 'photo', 'brighter', 'and', 'more', 'colorful', 'please', 'sky', 'darker']
OPS = ['<NONE>', '<START>', '<END>', 'brightness', 'contrast', 'saturation', 'hue', 'inpaint_obj', 'tint', 'sharpness', 'color_bg']


def summary(xs, unit=1e6, name='us'):
    return '%9.2f %s (%.2f - %.2f)' % (statistics.median(xs) * unit, name, min(xs) * unit, max(xs) * unit)


def alternate(fns, batches, runs, inner):
    """Every function of `fns` on the same groups of batches, in turn; run 0 warms up.  Seconds per launch, per function."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, group):
        torch.cuda.synchronize()
        e0.record()
        for index in group:
            fn(index)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / len(group)
    times = [[] for _ in fns]
    for r in range(runs + 1):
        group = batches[r * inner:(r + 1) * inner]
        for ts, fn in zip(times, fns):
            t = timed(fn, group)
            if r:
                ts.append(t)
    return times


def bench_gather(S, items, runs, inner, dev, say):
    slot = data.resident_slot_bytes(S)
    K = 10
    store = torch.randint(0, 256, (items * K * slot,), dtype=torch.uint8, device=dev)
    slots10 = (torch.arange(items * K, dtype=torch.int64, device=dev) * slot).view(items, K)
    slots7 = slots10[:, :7].contiguous()                                 # (a): the same store, the first 7 pictures of every item
    V = len(OPS)
    rows = torch.randint(-1, 1000, (items, V), dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(S)
    batches = [torch.randperm(items, generator=g)[:B].to(dev) for _ in range((runs + 1) * inner)]
    x = torch.empty(B, 3, S, S, device=dev)
    ys7, ys10 = torch.empty(B, 6, 3, S, S, device=dev), torch.empty(B, 9, 3, S, S, device=dev)
    x2, ys7b = torch.empty_like(x), torch.empty_like(ys7)
    out_rows = torch.empty(B, V, dtype=torch.int32, device=dev)

    def existing(index):
        T.gather_u8(store, slots7, index, S, out=(x, ys7))

    def items7(index):
        T.gather_items_u8(store, slots7, index, S, out=(x2, ys7b))

    def items10(index):
        T.gather_items_u8(store, slots10, index, S, rows=rows, out=(x, ys10, out_rows))

    for index in batches[:3]:                                            # equal before anything is timed
        existing(index)
        items7(index)
        assert torch.equal(x, x2) and torch.equal(ys7, ys7b), 'the two entries differ'
        items10(index)
        assert torch.equal(x, x2) and torch.equal(ys10[:, :6], ys7b) and torch.equal(out_rows, rows[index]), 'K = 10 differs'
    ta, tb = alternate([existing, items7], batches, runs, inner)
    tc, = alternate([items10], batches, runs, inner)
    say('%d x %d, batch of %d items out of a %d-item store (%.0f MB), %d runs of %d launches' % (S, S, B, items, store.numel() / 1e6, runs, inner))
    say('  (a) K = 7, no rows: gather_u8            %s per batch' % summary(ta))
    say('  (a) K = 7, no rows: gather_items_u8      %s per batch' % summary(tb))
    apart = max(ta) < min(tb) or max(tb) < min(ta)
    say('      ranges %s; median new / existing = %.3f' % ('DO NOT OVERLAP' if apart else 'overlap: no difference beyond the spread of the runs',
                                                         statistics.median(tb) / statistics.median(ta)))
    nbytes = 15 * B * K * S * S
    rate = nbytes / statistics.median(tc)
    say('  (b) K = 10, V = %d, rows in the launch   %s per batch' % (V, summary(tc)))
    say('      moves %.1f MB per batch: %.0f GB/s on 15 B/px = %.0f %% of %.0f TB/s' % (nbytes / 1e6, rate / 1e9, 100 * rate / HBM, HBM / 1e12))


def write_tree(root, pairs):
    """A GIER-layout tree (tests/gier_tree.py's layout): `pairs` records of two requests, 5 planned steps, 5 candidate masks
    (boxes; candidates 0 and 1 overlap), 'brightness' local on every record, 'tint' on every second: 7 JPEGs of 500 x 333 a pair."""
    from PIL import Image
    data_dir, vocab_dir, act_dir = (os.path.join(root, d) for d in ('GIER', 'language', 'actions'))
    for d in ('images', 'masks', 'splits'):
        os.makedirs(os.path.join(data_dir, d), exist_ok=True)
    os.makedirs(vocab_dir, exist_ok=True)
    for name, words in (('GIER_vocabs_sess_3.json', WORDS), ('GIER_operator_vocabs_sess_3.json', OPS)):
        with open(os.path.join(vocab_dir, name), 'w') as f:
            json.dump({w: i for i, w in enumerate(words)}, f)
    rng = np.random.default_rng(0)

    def jpeg(path):
        small = (rng.random((SRC_H // 8 + 2, SRC_W // 8 + 2, 3)) * 255).astype(np.uint8)
        Image.fromarray(small).resize((SRC_W, SRC_H), Image.BICUBIC).save(path, format='JPEG', quality=90)
    recs = []
    for i in range(pairs):
        name = 'tr%03d' % i
        ops = {'brightness': {'local': True, 'ids': [0, 1] if i % 3 == 0 else [2]}, 'contrast': {'local': False, 'ids': []}}
        if i % 2:
            ops['tint'] = {'local': True, 'ids': [1, 3, 4]}
        recs.append({'input': '%s_%s.jpg' % (name, name), 'output': '%s_out.jpg' % name, 'operator': ops,
                     'expert_summary': ['make the sky brighter please'], 'amateur_summary': ['make the photo more colorful']})
        jpeg(os.path.join(data_dir, 'images', recs[-1]['input']))
        jpeg(os.path.join(data_dir, 'images', recs[-1]['output']))
        cands = []
        for k in range(5):
            plane = np.zeros((SRC_H, SRC_W), np.uint8)
            y0, x0 = int(rng.integers(0, SRC_H // 2)), int(rng.integers(0, SRC_W // 2))
            plane[y0:y0 + SRC_H // 3, x0:x0 + SRC_W // 3] = 1
            cands.append(plane)
        cands[1] |= cands[0]
        with open(os.path.join(data_dir, 'masks', '%s_%s_mask.json' % (name, name)), 'w') as f:
            json.dump([{'size': [SRC_H, SRC_W], 'counts': gier.rle_to_string(gier.rle_encode(c))} for c in cands], f)
        d = os.path.join(act_dir, name)
        os.makedirs(d, exist_ok=True)
        dist, seq = 0.30, []
        for s, op in enumerate(['brightness', 'contrast', 'saturation', 'tone', 'sharpness']):
            dist *= 0.6
            seq.append([op, [0.5] * (8 if op == 'tone' else 1), dist])
            jpeg(os.path.join(d, 'edit%d.jpg' % s))
        with open(os.path.join(d, 'acts.json'), 'w') as f:
            json.dump({'init distance': 0.30, 'operation sequence': [seq]}, f)
    with open(os.path.join(data_dir, 'splits', 'train_sess_3.json'), 'w') as f:
        json.dump(recs, f)
    with open(os.path.join(data_dir, 'splits', 'train_Ids_L1Thr_0.06_sess_3.json'), 'w') as f:
        json.dump(list(range(pairs)), f)
    return data_dir, vocab_dir, act_dir


def bench_loader(root, dev, say, rounds=2):
    """Leg (c).  The workers are started, and joined, before this process opens the GPU for timing the rest."""
    from torch.utils.data import DataLoader, Subset
    data_dir, vocab_dir, act_dir = write_tree(root, B // 2)
    V = len(OPS)

    def dataset(S):
        return gier.GIERDatasetAct(data_dir, vocab_dir, act_dir, 'train', 'valid', 'rle', 3, S)
    ds = gier._Tuples(dataset(128), with_masks=True)
    assert len(ds) == B
    tik = time.perf_counter()
    items = [ds[i] for i in range(B)]
    alone = time.perf_counter() - tik
    n_batches = WORKERS * (rounds + 1)
    loader = DataLoader(Subset(ds, list(range(B)) * n_batches), batch_size=B, collate_fn=gier.collate_masks, num_workers=WORKERS)
    t0 = None
    for i, _ in enumerate(loader):
        if i == WORKERS - 1:                                             # every worker has delivered its first batch
            t0 = time.perf_counter()
    workers = (time.perf_counter() - t0) / (n_batches - WORKERS)
    del loader
    batch = gier.collate_masks(items)
    say('(c) the --dataset GIER --load_mask batch at 128 x 128: %d items (%d pairs x 2 requests) x 7 JPEGs of %d x %d + mask files' % (
        B, B // 2, SRC_W, SRC_H))
    say('  decode + host resize + masks, one process           %9.2f ms per batch' % (alone * 1e3))
    say('  the same + collate_masks, %2d workers                %9.2f ms per batch (steady state, %d batches, a batch per worker)' % (
        WORKERS, workers * 1e3, n_batches - WORKERS))
    walls = []
    for _ in range(11):
        torch.cuda.synchronize()
        tik = time.perf_counter()
        gier.MaskTable.from_rle(batch[6], (128, 128), V, dev)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - tik)
    say('  MaskTable.from_rle (parse, upload, launch, synchronised) %s per batch' % summary(walls[1:], 1e3, 'ms'))
    for S in (128, 256):                                                 # the same tree resident: what the train loop waits for per batch
        resident = gier.ResidentGIER(dataset(S), S, B, dev, num_workers=0)   # (built in this process: no fork once the GPU is open)
        walls = []
        for _ in range(21):                                              # an epoch of this tree is one batch; the first warms up
            torch.cuda.synchronize()
            tik = time.perf_counter()
            next(iter(resident))
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - tik)
        say('  resident at %3d x %3d: %d distinct pictures for %d items (10 N = %d), %d planes, %d bytes, built by one process in %.2f s' % (
            S, S, resident.n_pictures, B, 10 * B, resident.n_planes, resident.nbytes, resident.build_seconds))
        say('      whole fetch with its MaskTable (host indexing, index upload, one launch, synchronised) %s per batch' % summary(walls[1:], 1e3, 'ms'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--items', type=int, default=1024)
    ap.add_argument('--note', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    dev = torch.device('cuda', 0)
    loader_lines = []
    with tempfile.TemporaryDirectory() as root:
        bench_loader(root, dev, loader_lines.append)
    say('tools/bench_resident_gier.py on %s' % torch.cuda.get_device_name(dev))
    for S in (128, 256):
        bench_gather(S, args.items, args.runs, args.inner, dev, say)
    for s in loader_lines:
        say(s)
    say('not measured: the real GIER split (its build seconds, resident bytes and deduplication factor); more than one rank')
    if args.note:
        say(args.note)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
