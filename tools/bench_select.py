"""The mask planes of a local edit from a rule: the selection kernel (functional.select_u8) against a device-to-device
copy of the same byte count and against what had to be done without it ("selections").  Run by hand; not a
test and not part of bench.py.

Workload: one generated 4000 x 6000 uint8 RGB picture already on the device (random bytes over a smooth ramp, so that
every colour measure takes all its values) and one random plane behind it.  Cases: each term kind alone (one plane), a
four-term selection (one plane), and four planes in one launch (lum, sat, hue, linear; the jobs share the photo).

  kernel   functional.select_u8: one launch; bytes moved by the kernel's model = (3 + 1 + plane terms) B/px per plane, the 3
           only where the plane has a colour term (the photo is not read otherwise)
  copy     torch's device-to-device copy of HALF that many bytes (read + written = the same bytes moved): the yardstick
  host     the route without the kernel: the planes built by the numpy oracle on the CPU (tests/select_cases.py) and
           uploaded; timed once per case, the upload alone as well

kernel and copy are timed with device events around one call after warm-up, alternating, --reps times; median and range.
The kernel's bytes are compared with the host oracle's first (they must be equal).  No ratio is asserted.

    python tools/bench_select.py [--out profiles/select_u8.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import t2onet_amd.functional as T                # noqa: E402
from tests import select_cases as SC             # noqa: E402


def picture(h, w):
    rng = np.random.default_rng(5)
    ramp = (np.arange(w, dtype=np.int64)[None, :, None] * 255 // max(w - 1, 1) + np.arange(h, dtype=np.int64)[:, None, None] * 64 // max(h - 1, 1))
    noise = rng.integers(-96, 97, (h, w, 3))
    return np.clip(ramp // 2 + 64 + noise, 0, 255).astype(np.uint8)


def cases(h, w, plane):
    m = min(h, w)
    lum, sat, hue = ('lum', 0, 128, 255, 32), ('sat', 0, 0, 96, 48), ('hue', 0, 1365, 171, 128)
    lin, wide = ('linear', 0, 0, 0, 0, h - 1), ('linear', 0, 0, 0, w - 1, h - 1)
    rad = ('radial', 0, w // 2, h // 2, m // 8, m // 2)
    return [('lum', [[lum]]), ('sat', [[sat]]), ('hue', [[hue]]), ('linear, den < 2^24', [[lin]]), ('linear, den >= 2^24', [[wide]]),
            ('radial, den < 2^24', [[rad]]), ('plane', [[('plane', 0, plane)]]), ('four terms: lum * !sat * hue * linear', [[lum, ('sat', 1, 0, 96, 48), hue, lin]]),
            ('four planes: lum, sat, hue, linear', [[lum], [sat], [hue], [lin]])]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--height', type=int, default=4000)
    ap.add_argument('--width', type=int, default=6000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no_host', action='store_true', help='skip the host column (and the byte comparison with it)')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_select: needs the GPU (a CPU run says nothing about these times)')
    dev = torch.device('cuda', torch.cuda.current_device())
    h, w = args.height, args.width
    n = h * w
    img = picture(h, w)
    host_src = np.concatenate([img.reshape(-1), np.random.default_rng(6).integers(0, 256, n, dtype=np.uint8)])
    src = torch.from_numpy(host_src).to(dev)
    lines = ['selections of one %d x %d uint8 RGB picture (%.1f Mpx), %s; %d timed calls each after %d warm-up calls, alternating'
             % (h, w, n / 1e6, torch.cuda.get_device_name(dev), args.reps, args.warmup)]
    all_equal = True
    for name, planes in cases(h, w, 3 * n):
        jobs = [(0, k * n, h, w, terms) for k, terms in enumerate(planes)]
        moved = sum((3 * any(t[0] in ('lum', 'sat', 'hue') for t in terms) + 1 + sum(t[0] == 'plane' for t in terms)) * n for terms in planes)
        out = torch.empty(len(planes) * n, dtype=torch.uint8, device=dev)
        a_copy = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        b_copy = torch.empty_like(a_copy)
        fns = {'kernel': lambda: T.select_u8(src, jobs, out=out), 'copy': lambda: b_copy.copy_(a_copy)}
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.reps):
            for key, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[key].append(a.elapsed_time(b))
        lines.append('%s: %d plane%s, %.0f MB moved' % (name, len(planes), 's' if len(planes) > 1 else '', moved / 1e6))
        med = {}
        for key in fns:
            t = np.array(times[key])
            med[key] = float(np.median(t))
            lines.append('  %-7s median %8.3f ms   min %8.3f   max %8.3f   -> %8.1f GB/s' % (key, med[key], t.min(), t.max(), moved / (med[key] * 1e-3) / 1e9))
        lines.append('  kernel rate / copy rate = %.2f' % (med['copy'] / med['kernel']))
        if not args.no_host:
            t0 = time.perf_counter()
            ref = np.concatenate([SC.selection(terms, img, host_src).reshape(-1) for terms in planes])
            t1 = time.perf_counter()
            up = torch.from_numpy(ref).to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            equal = bool(torch.equal(up, out))
            all_equal = all_equal and equal
            lines.append('  host    once   %8.1f ms numpy on the CPU + %6.2f ms upload of %d MB; kernel bytes equal the host oracle\'s: %s'
                         % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, ref.size // 1000000, equal))
            del up, ref
        print('\n'.join(lines[-(4 + (not args.no_host)):]), flush=True)
        del out, a_copy, b_copy
    lines.append('not measured: real photos through the decoder, apply_cli end to end on a shoot, the kernel\'s share of peak')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    if not all_equal:
        raise SystemExit('bench_select: the kernel\'s bytes differ from the host oracle\'s')


if __name__ == '__main__':
    main()
