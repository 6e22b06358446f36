"""What the local-edit masks cost the planner (recorded, no threshold) -> profiles/planner_mask.txt.

  * one sweep round (t2o_op_candidates_multi_l1: 64 jobs x 64 candidates) and one Adam iteration (t2o_fit_multi_l1_adam: 64
    jobs, two launches) at SIZE x SIZE, through the unmasked entry point and through the masked one with mask_index = -1
    (which runs the unmasked kernels), with all-ones planes and with blob planes: device-event times, the variants
    ALTERNATING inside each of REPS rounds, median and range per variant.  Expectation from the bytes: 25 instead of 24 per
    pixel and job.
  * plan_cli --dataset GIER on 8 synthetic pairs (the tree the tests use) at SIZE x SIZE, --local beside the global search on
    the same pairs: seconds per pair end to end (decode, union planes, search, JPEG + record writes), second run of two.

    python tools/bench_planner_mask.py [--size 256] [--reps 20] [--out profiles/planner_mask.txt]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import t2onet_amd.functional as T  # noqa: E402
from t2onet_amd import plan_cli  # noqa: E402


def blob(h, w):
    yy, xx = np.mgrid[:h, :w]
    return ((((yy + 0.5) / h - 0.5) ** 2 + ((xx + 0.5) / w - 0.5) ** 2) <= 0.326 ** 2).astype(np.uint8)      # a third of the plane


def alternate(variants, reps):
    """variants: [(name, fn)] -> {name: sorted ms}; every round runs each variant once, in turn, timed by device events."""
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {k: sorted(v) for k, v in ms.items()}


def report(title, ms, per, unit, lines):
    lines.append(title)
    base = None
    for name, v in ms.items():
        med = v[len(v) // 2] / per
        base = med if base is None else base
        lines.append('  %-34s median %8.4f %s  range %8.4f .. %8.4f  (x %.3f of the first row)' % (name, med, unit, v[0] / per, v[-1] / per, med / base))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--fit_steps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'planner_mask.txt'))
    args = ap.parse_args(argv)
    S, J, C = args.size, 64, 64
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator().manual_seed(5)
    imgs = torch.rand(8, 3, S, S, generator=g).to(dev)
    tgts = torch.rand(8, 3, S, S, generator=g).to(dev)
    ones = torch.ones(8, S, S, dtype=torch.uint8, device=dev)
    blobs = torch.from_numpy(np.stack([np.roll(blob(S, S), 7 * k, 1) for k in range(8)])).to(dev)
    idx = [k % 8 for k in range(J)]
    lines = ['%s, torch %s, %d x %d, %d jobs, %d alternating rounds' % (torch.cuda.get_device_name(dev), torch.__version__, S, S, J, args.reps)]

    sweep_ops = [(0, 1, 2, 3, 5, 0, 1, 2)[k % 8] for k in range(J)]
    cand = torch.zeros(J, C, 24, device=dev)
    cand[:, :, 0] = torch.linspace(-0.5, 0.5, C, device=dev)
    for k, op in enumerate(sweep_ops):
        if op in (3, 5):
            cand[k] = torch.rand(C, 24, generator=g).to(dev) + 0.5

    def sweep(**kw):
        return lambda: T.candidates_multi_l1(sweep_ops, idx, imgs, tgts[0], cand, **kw)
    ms = alternate([('unmasked entry point', sweep()),
                    ('masked entry, mask_index = -1', sweep(masks=blobs, mask_index=[-1] * J)),
                    ('masked entry, all-ones planes', sweep(masks=ones, mask_index=idx)),
                    ('masked entry, blob planes', sweep(masks=blobs, mask_index=idx))], args.reps)
    report('one sweep round (%d jobs x %d candidates, operators 0 1 2 3 5), ms per launch pair:' % (J, C), ms, 1, 'ms', lines)

    fit_ops = [(3, 5, 6, 0, 1, 2)[k % 6] for k in range(J)]
    start = torch.zeros(J, 24, device=dev)
    for k, op in enumerate(fit_ops):
        if op in (3, 5):
            start[k, :24 if op == 3 else 8] = 1.0
    N = args.fit_steps

    def fit(**kw):
        return lambda: T.fit_multi_l1(fit_ops, idx, imgs, tgts, idx, start, steps=N, check_every=0, **kw)
    ms = alternate([('unmasked entry point', fit()),
                    ('masked entry, mask_index = -1', fit(masks=blobs, mask_index=[-1] * J)),
                    ('masked entry, all-ones planes', fit(masks=ones, mask_index=idx)),
                    ('masked entry, blob planes', fit(masks=blobs, mask_index=idx))], args.reps)
    report('one Adam iteration (%d jobs, operators 3 5 6 0 1 2; a %d-step solve / %d, closing evaluation included), ms:' % (J, N, N), ms, N, 'ms', lines)

    from tests import gier_tree
    with tempfile.TemporaryDirectory() as root:
        data_dir, vocab_dir, _, _ = gier_tree.write_tree(os.path.join(root, 'tree'), n_train=8, n_val=1)
        common = ['--dataset', 'GIER', '--data_dir', data_dir, '--vocab_dir', vocab_dir, '--data_mode', 'valid', '--img_size', str(S),
                  '--pairs_per_batch', '8', '--overwrite']
        lines.append('plan_cli --dataset GIER, 8 synthetic pairs at %d x %d in one batch, beam 3 (second of two runs):' % (S, S))
        for tag, extra in (('global search [0,1,2,3,5,6]', []), ('--local      [0,1,2,3,5,6,7]', ['--local'])):
            save = os.path.join(root, 'acts_' + ('local' if extra else 'global'))
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = plan_cli.main(common + extra + ['--save_dir', save])
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            lines.append('  %-32s %7.3f s per pair (%d pairs, %.2f s)' % (tag, dt / n, n, dt))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
