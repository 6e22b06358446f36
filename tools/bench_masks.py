"""Union planes of one batch, two ways (figures in profiles/mask_union.txt):

    python tools/bench_masks.py [--runs 20] [--items 64] [--out profiles/mask_union.txt]

The batch: 64 items, 2 operators each with 3 of the item's 12 candidate masks annotated, synthetic blob masks on
1000 x 1500 sources (compressed COCO run lengths, as a mask file holds them), planes at 128 x 128.
  host    gier.resize_and_union_mask_host per (item, operator), in this process -- the reference's function: every
          candidate decoded to its native size, indexed, the annotated ones summed -- then one upload of the planes.
  device  gier.MaskTable.from_rle: the annotated masks' run lengths parsed and packed (host), one upload, one launch.
          Reported in parts: parse + pack (wall), upload (wall, synchronised), kernel (HIP events).
The same for ONE 600 x 900 plane, and the masked arg-max episode (B = 64, 128 x 128) with the MaskTable against the same
episode with the list of dicts.  Runs alternate between the two ways; median and range are printed."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from t2onet_amd import functional as T          # noqa: E402
from t2onet_amd import gier                     # noqa: E402

SRC = (1000, 1500)
N_CAND, N_SEL, OPS = 12, 3, (3, 8)


def blob(h, w, rng):
    y, x = np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32)
    m = np.zeros((h, w), bool)
    for _ in range(3):
        cy, cx, r = rng.random() * h, rng.random() * w, (0.1 + 0.2 * rng.random()) * max(h, w)
        m |= ((y - cy) ** 2)[:, None] + ((x - cx) ** 2)[None, :] <= r * r
    return m


def make_items(n, seed=0):
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        rles = [{'size': list(SRC), 'counts': gier.rle_to_string(gier.rle_encode(blob(*SRC, rng)))} for _ in range(N_CAND)]
        items.append({op: (rles, [int(i) for i in rng.choice(N_CAND, N_SEL, replace=False)]) for op in OPS})
    return items


def summary(xs):
    return '%9.3f ms (%.3f - %.3f)' % (statistics.median(xs) * 1e3, min(xs) * 1e3, max(xs) * 1e3)


def sync():
    torch.cuda.synchronize()


def host_way(items, size, dev):
    t0 = time.perf_counter()
    planes = [gier.resize_and_union_mask_host(rles, ids, size) for it in items for rles, ids in it.values()]
    t1 = time.perf_counter()
    d = torch.from_numpy(np.stack(planes)).to(dev)
    sync()
    return t1 - t0, time.perf_counter() - t1, d


def device_way(items, size, dev):
    """MaskTable.from_rle in its parts (same calls, timed apart)."""
    H, W = size
    t0 = time.perf_counter()
    masks, jobs, seen = [], [], {}
    for it in items:
        for rles, ids in it.values():
            sel = []
            for i in ids:
                if id(rles[i]) not in seen:
                    seen[id(rles[i])] = len(masks)
                    masks.append(rles[i])
                sel.append(seen[id(rles[i])])
            jobs.append((sel, len(jobs) * H * W, H, W))
    tables = T.pack_rle_union(masks, jobs)
    t1 = time.perf_counter()
    tables.upload(dev)
    out = torch.empty(tables.need, dtype=torch.uint8, device=dev)
    sync()
    t2 = time.perf_counter()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    T.rle_union_u8(tables, out=out)
    e1.record()
    sync()
    return t1 - t0, t2 - t1, e0.elapsed_time(e1) * 1e-3, tables.host.numel(), out.view(len(jobs), H, W)


def bench_union(items, size, runs, dev, say):
    host, dev_parts, dev_total = [], [], []
    for r in range(runs + 1):                                 # run 0 warms both ways up
        a = host_way(items, size, dev)
        t0 = time.perf_counter()
        table = gier.MaskTable.from_rle(items, size, 11, dev)
        sync()
        whole = time.perf_counter() - t0
        b = device_way(items, size, dev)
        assert torch.equal(a[2], b[4]) and torch.equal(a[2], table.planes)
        if r:
            host.append(a[:2])
            dev_parts.append(b[:3])
            dev_total.append(whole)
    n = sum(len(it) for it in items)
    say('%d planes of %d x %d from %d x %d sources, %d runs' % (n, size[0], size[1], SRC[0], SRC[1], runs))
    say('  host    decode + resize + union %s   upload of %d plane bytes %s' % (summary([h[0] for h in host]), n * size[0] * size[1], summary([h[1] for h in host])))
    say('  host    total                   %s' % summary([h[0] + h[1] for h in host]))
    say('  device  parse + pack            %s   upload of %d table bytes %s   kernel %s' % (
        summary([d[0] for d in dev_parts]), b[3], summary([d[1] for d in dev_parts]), summary([d[2] for d in dev_parts])))
    say('  device  MaskTable.from_rle, whole call, synchronised  %s' % summary(dev_total))
    ht, dt = [h[0] + h[1] for h in host], dev_total
    say('  ranges %s: host %.3f - %.3f ms, device %.3f - %.3f ms' % ('do not overlap' if max(dt) < min(ht) or max(ht) < min(dt) else 'OVERLAP',
                                                                     min(ht) * 1e3, max(ht) * 1e3, min(dt) * 1e3, max(dt) * 1e3))


def bench_episode(runs, dev, say, Bn=64, S=128):
    import t2onet_amd
    from t2onet_amd.actor import Actor
    opt = t2onet_amd.default_options(input_dropout_p=0.0, dropout_p=0.0)
    torch.manual_seed(3)
    model = Actor(opt).to(dev).eval()
    g = torch.Generator().manual_seed(5)
    img = torch.rand(Bn, 3, S, S, generator=g).to(dev)
    x = torch.zeros(Bn, 17, dtype=torch.long)
    x[:, 0], x[:, 1:9], x[:, 9] = 1, torch.randint(4, 900, (Bn, 8), generator=g), 2
    lengths = (x != 0).sum(1)
    x = x.to(dev)
    rng = np.random.default_rng(7)
    mask_dict = [{str(op): [(rng.random((1, S, S)) < 0.5).astype(np.float32)] for op in (3, 4, 5, 6, 8, 9)} for _ in range(Bn)]
    table = gier.MaskTable.from_arrays(mask_dict, (S, S), opt.output_vocab_size, dev)

    def run(md):
        sync()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = model.episode_forward(x, img, md, reinforce_sample=0, lengths=lengths, stack=False)
        sync()
        return time.perf_counter() - t0, out
    ta, tb = [], []
    for r in range(runs + 2):
        a, oa = run(table)
        b, ob = run(mask_dict)
        assert torch.equal(oa[2], ob[2]) and all(torch.equal(p, q) for p, q in zip(oa[1], ob[1]))
        if r > 1:
            ta.append(a)
            tb.append(b)
    say('masked arg-max episode, B = %d, %d x %d, a mask for every operator of every sample, %d runs' % (Bn, S, S, runs))
    say('  MaskTable (mask_select per step)      %s' % summary(ta))
    say('  list of dicts (get_gt_mask per step)  %s' % summary(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--items', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda', torch.cuda.current_device())
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('tools/bench_masks.py on %s' % torch.cuda.get_device_name(dev))
    items = make_items(args.items)
    bench_union(items, (128, 128), args.runs, dev, say)
    bench_union([{3: items[0][3]}], (600, 900), args.runs, dev, say)
    bench_episode(args.runs, dev, say)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
