"""The connected region around a seed pixel of a photo's size: the union-find kernels (functional.region_u8) on pictures
that stress them in different ways, against a device copy of the workspace's size and against the host route (DESIGN.md,
"magic-wand regions").  Run by hand; not a test and not part of bench.py.  Nothing gates on a time: nobody had measured this
kernel when the tool was written; a content that costs more than ten times the all-passing one is reported as a finding.

Workload: one generated 4000 x 6000 RGB picture per content, already on the device, seed and tolerance per content:
  all         every pixel passes: one component, the most unions on one root
  half        the left half passes
  serpentine  a one-pixel path through every second row, connectors at alternating ends: the longest chains
  noise50     two colours, 50 % of the pixels pass (ragged components; with 8 steps far above the threshold)
  noise59     the same at 59 %, just below the threshold of 4 steps (0.593)
  gradient    a smooth diagonal gradient plus noise of +-2, tolerance 40

  kernel      functional.region_u8, three launches, for conn = 4 and conn = 8; the split by kernel of ONE further call comes
              from the torch profiler
  copy        a device copy of 4 bytes per pixel (the size of the parent array): what one pass over the workspace costs
  host        scipy.ndimage.label on the CPU of this machine where it imports (else a numpy labelling by repeated
              dilation), from the boolean pass plane to the 0/255 plane, timed once; the upload is not included

The device routes are timed with HIP events around one whole call after warm-up, alternating, --reps times.  The kernel's
bytes are compared with the host route's first (they must be equal).

    python tools/bench_region.py [--out profiles/region_u8.txt]
"""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import t2onet_amd.functional as T                # noqa: E402

A, B = (200, 120, 40), (20, 30, 220)


def paint(mask):
    return np.where(mask[:, :, None], np.array(A, np.uint8)[None, None, :], np.array(B, np.uint8)[None, None, :])


def contents(h, w):
    """[(name, photo (h, w, 3) uint8, seed_x, seed_y, tol)], one at a time (each is 72 MB at full size)."""
    yield 'all', paint(np.ones((h, w), bool)), w // 2, h // 2, 10
    m = np.zeros((h, w), bool)
    m[:, :w // 2] = True
    yield 'half', paint(m), w // 4, h // 2, 10
    m = np.zeros((h, w), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = True
    yield 'serpentine', paint(m), w // 2, (h - 1) // 2 * 2, 10
    for share, seed in ((0.50, 50), (0.59, 59)):
        m = np.random.default_rng(seed).random((h, w)) < share
        m[h // 2, w // 2] = True
        yield 'noise%d' % seed, paint(m), w // 2, h // 2, 10
    yy, xx = np.mgrid[:h, :w]
    g = (40 + 170 * (xx * h + yy * w) // (2 * h * w)).astype(np.int64)
    img = np.stack([g, g + 10, 255 - g], -1) + np.random.default_rng(3).integers(-2, 3, (h, w, 3))
    yield 'gradient', np.clip(img, 0, 255).astype(np.uint8), w // 2, h // 2, 40


def host_label(ok, sx, sy, conn):
    """The 0/255 plane of the seed's component of the boolean plane `ok` on the CPU -> (plane, which route)."""
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        labels, _ = ndimage.label(ok, structure=np.ones((3, 3), int) if conn == 8 else None)
        return np.where(labels == labels[sy, sx], 255, 0).astype(np.uint8), 'scipy.ndimage.label'
    sel = np.zeros_like(ok)
    sel[sy, sx] = True
    while True:                                                      # dilate under the mask until nothing changes
        grown = sel.copy()
        grown[1:] |= sel[:-1]; grown[:-1] |= sel[1:]; grown[:, 1:] |= sel[:, :-1]; grown[:, :-1] |= sel[:, 1:]
        if conn == 8:
            grown[1:, 1:] |= sel[:-1, :-1]; grown[1:, :-1] |= sel[:-1, 1:]; grown[:-1, 1:] |= sel[1:, :-1]; grown[:-1, :-1] |= sel[1:, 1:]
        grown &= ok
        if (grown == sel).all():
            return np.where(sel, 255, 0).astype(np.uint8), 'numpy dilation'
        sel = grown


def kernel_split(fn):
    from torch.autograd import DeviceType
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        if e.device_type == DeviceType.CUDA and 'k_region_' in e.key:
            split[re.findall(r'k_region_(\w+)', e.key)[0]] = getattr(e, 'device_time_total', getattr(e, 'cuda_time_total', 0.0)) / 1e3
    return split


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
        raise SystemExit('bench_region: needs the GPU (a CPU run says nothing about these times)')
    dev = torch.device('cuda', torch.cuda.current_device())
    h, w = args.height, args.width
    lines = ['the connected region around a seed of one %d x %d RGB picture (%.1f Mpx), %s; %d timed calls each after %d warm-up calls, alternating'
             % (h, w, h * w / 1e6, torch.cuda.get_device_name(dev), args.reps, args.warmup),
             'kernel workspace: %d bytes (4 per pixel); %d launches per call'
             % (T._lib.load().t2o_region_workspace_bytes(T.region_jobs([(0, 0, h, w, 0, 0, 0, 4)]), 1), T.REGION_LAUNCHES)]
    words = torch.zeros(h * w, dtype=torch.int32, device=dev)
    words2 = torch.empty_like(words)
    out = torch.empty(h * w, dtype=torch.uint8, device=dev)
    all_equal, medians = True, {}
    for name, rgb, sx, sy, tol in contents(h, w):
        pic = torch.from_numpy(np.ascontiguousarray(rgb).reshape(-1)).to(dev)
        d = np.abs(rgb.astype(np.int16) - rgb[sy, sx].astype(np.int16)[None, None, :]).max(axis=2) <= tol
        lines.append('%s (seed %d, %d; tol %d; %.1f %% of the pixels pass):' % (name, sx, sy, tol, 100.0 * d.mean()))
        first = len(lines)
        for conn in (4, 8):
            job = [(0, 0, h, w, sx, sy, tol, conn)]
            routes = {'kernel': lambda: T.region_u8(pic, job, out=out), 'copy': lambda: words2.copy_(words)}
            for _ in range(args.warmup):
                for fn in routes.values():
                    fn()
            torch.cuda.synchronize()
            times = {r: [] for r in routes}
            for _ in range(args.reps):
                for r, fn in routes.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    times[r].append(a.elapsed_time(b))
            t = {r: np.array(v) for r, v in times.items()}
            medians[name, conn] = float(np.median(t['kernel']))
            split = kernel_split(routes['kernel'])
            got = out.cpu().numpy().reshape(h, w)
            lines.append('  conn %d: %d pixels selected' % (conn, int((got == 255).sum())))
            for r in routes:
                lines.append('    %-8s median %9.3f ms   min %9.3f   max %9.3f' % (r, np.median(t[r]), t[r].min(), t[r].max()))
            lines.append('    by kernel, one profiled call: ' + ', '.join('%s %.3f ms' % (k, split[k]) for k in ('tile', 'border', 'resolve') if k in split))
            if not args.no_host:
                t0 = time.perf_counter()
                want, route = host_label(d, sx, sy, conn)
                host_ms = (time.perf_counter() - t0) * 1e3
                equal = bool(np.array_equal(want, got))
                all_equal = all_equal and equal
                lines.append('    %-8s once   %9.1f ms (%s on the CPU, no upload); kernel bytes equal its bytes: %s' % ('host', host_ms, route, equal))
        print('\n'.join(lines[first - 1:]), flush=True)
        del pic
    base = {conn: medians['all', conn] for conn in (4, 8)}
    slow = [(n, c, m / base[c]) for (n, c), m in medians.items() if m > 10.0 * base[c]]
    lines.append('finding: ' + ('; '.join('%s with conn %d costs %.1f x the all-passing picture' % s for s in slow) if slow
                                else 'no content costs more than ten times the all-passing picture (the largest ratio: %.1f x)'
                                % max(m / base[c] for (n, c), m in medians.items())))
    lines.append('not measured: real photos, several jobs in one call, pictures of other sizes, the share of peak')
    text = '\n'.join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print('\n'.join(lines[-2:]))
    if not all_equal:
        raise SystemExit('bench_region: the kernel\'s bytes differ from the host route\'s')


if __name__ == '__main__':
    main()
