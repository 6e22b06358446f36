"""The evaluation loop without a host read per image ("Evaluation metrics on the device").

Part one -- the metrics of ONE 600 x 900 image (B = 1, five step images, END at step 2), HIP events around the calls:
  fused     functional.eval_metrics: two launches, the three images read once
  separate  the five calls it replaces: train.select_end_images on the stacked steps, l1_loss twice, ssim twice
            (no .item(): device work and its enqueue only)
Part two -- wall time of a whole pass over --items synthetic 600 x 900 items at batch size 1 with one seeded Actor:
  test_on_device(is_test=True) against evaluate.test(is_test=True), alternating, --runs runs each after one warm-up run
  each; every run ends with its host read, so the clock stops after the device has finished.
The values of the two loops are compared first (1e-5 relative).  Nothing is asserted about the times.

    python tools/bench_eval.py [--out profiles/eval_loop.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import t2onet_amd                                # noqa: E402
import t2onet_amd.functional as T                # noqa: E402
from t2onet_amd import evaluate                  # noqa: E402
from t2onet_amd.actor import Actor               # noqa: E402
from t2onet_amd.train import first_end_step, select_end_images   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--height', type=int, default=600)
    ap.add_argument('--width', type=int, default=900)
    ap.add_argument('--items', type=int, default=32)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=50)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_eval: needs the GPU (a CPU run says nothing about these times)')
    dev = torch.device('cuda', torch.cuda.current_device())
    h, w = args.height, args.width
    g = torch.Generator().manual_seed(0)
    lines = []

    def say(line):                               # shown as it is known: a long run is not silent
        lines.append(line)
        print(line, flush=True)
    say('evaluation metrics and loop at %d x %d, %s' % (h, w, torch.cuda.get_device_name(dev)))

    # ---- part one: the metrics of one image
    inp, tgt = (torch.rand(1, 3, h, w, generator=g).to(dev) for _ in range(2))
    steps = [torch.rand(1, 3, h, w, generator=g).to(dev) for _ in range(5)]
    pred_ops = torch.tensor([[5, 4, 2, 6, 8]], device=dev)                  # END (2) at step 2
    first = first_end_step(pred_ops, 2)
    row = torch.zeros(4, device=dev)

    def fused():
        T.eval_metrics(inp, steps, first, tgt, out=row)

    def separate():
        out = select_end_images(torch.stack(steps, 1), pred_ops, 2)
        return T.l1_loss(inp, tgt), T.l1_loss(out, tgt), T.ssim(inp, tgt), T.ssim(out, tgt)

    times = {'fused': [], 'separate': []}
    with torch.no_grad():
        for _ in range(5):
            fused()
            sep = separate()
        torch.cuda.synchronize()
        say('part one: fused %s' % ['%.6f' % v for v in row.tolist()])
        say('          separate %s' % ['%.6f' % v.item() for v in sep])
        for _ in range(args.reps):
            for name, fn in (('fused', fused), ('separate', separate)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b) * 1e3)
    for name in ('fused', 'separate'):
        t = np.array(times[name])
        say('  %-9s median %8.1f us   min %8.1f   max %8.1f   (HIP events, %d calls, alternating)'
                     % (name, np.median(t), t.min(), t.max(), args.reps))
    say('  separate / fused (medians): %.2fx' % (np.median(times['separate']) / np.median(times['fused'])))

    # ---- part two: the whole loop
    torch.manual_seed(3)
    opt = t2onet_amd.default_options(print_every=10 ** 9)
    model = Actor(opt).to(dev).eval()
    items = []
    for _ in range(args.items):
        x = torch.zeros(1, opt.encoder_max_len, dtype=torch.long)
        k = int(torch.randint(2, opt.encoder_max_len - 2, (1,), generator=g))
        x[0, 0], x[0, 1 + k] = 1, 2
        x[0, 1:1 + k] = torch.randint(4, opt.input_vocab_size, (k,), generator=g)
        items.append((torch.rand(1, 3, h, w, generator=g), torch.rand(1, 3, h, w, generator=g), x, ['synthetic request']))

    def on_device():
        return evaluate.test_on_device(model, items, opt, is_test=True, device=dev, verbose=False)

    seen = {}
    real_eval = evaluate.ImageEvaluator.eval
    evaluate.ImageEvaluator.eval = lambda self: seen.update(real_eval(self)) or seen

    def with_items():
        return evaluate.test(model, items, opt, is_test=True, device=dev, verbose=False)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):                          # (ImageEvaluator.eval prints)
        res_dev = on_device()
        res_item = with_items()
    same = all(abs(a - b) <= 1e-5 * abs(b) + 1e-6 for a, b in zip(res_dev[:2], res_item)) and \
        all(abs(res_dev[2][key] - seen[key]) <= 1e-5 * abs(seen[key]) + 1e-6 for key in seen)
    say('part two: %d items, batch size 1; values of the two loops agree (1e-5): %s' % (args.items, same))
    say('  on device %s' % {key: round(v, 6) for key, v in res_dev[2].items()})
    loops = {'test_on_device': [], 'evaluate.test': []}
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(args.runs):
            loops['test_on_device'].append(timed(on_device))
            loops['evaluate.test'].append(timed(with_items))
    for name in ('test_on_device', 'evaluate.test'):
        t = np.array(loops[name])
        say('  %-15s runs %s s   -> %6.2f ms per item (median run)' % (name, ' '.join('%.3f' % v for v in t), 1e3 * np.median(t) / args.items))
    say('  evaluate.test / test_on_device (median runs): %.3fx; spread of the three runs: %.1f %% / %.1f %%'
                 % (np.median(loops['evaluate.test']) / np.median(loops['test_on_device']),
                    100 * (max(loops['test_on_device']) - min(loops['test_on_device'])) / np.median(loops['test_on_device']),
                    100 * (max(loops['evaluate.test']) - min(loops['evaluate.test'])) / np.median(loops['evaluate.test'])))
    text = '\n'.join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    if not same:
        raise SystemExit('bench_eval: the two loops differ')


if __name__ == '__main__':
    main()
