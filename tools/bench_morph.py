"""Moving a plane's boundary at a photo's size: the morph kernels (functional.morph_u8) on one synthetic plane, all three modes
at R = 2, 8 and 64, against a device copy of the plane's bytes and against a host route ("grow, shrink, border").
Run by hand; not a test and not part of bench.py.  Nothing gates on a time: nobody had measured these kernels when the tool
was written.  The ratios to the copy and to the host route are written down as measured, never asserted.

Workload: one generated 4000 x 6000 plane already on the device -- a wand-like blob (an ellipse with a ragged rim and a few
holes) plus scattered specks --, hard 0 / 255.

  kernel      functional.morph_u8, two launches, in place (what edit_image does) from a fresh copy of the plane made outside
              the timed span; the split by kernel of ONE further call of each variant comes from the torch profiler
  copy        a device-to-device copy of the plane's 1 byte per pixel, timed in the same rounds
  host        scipy.ndimage.distance_transform_edt or cv2.distanceTransform on the CPU of this machine where one of them
              imports, for the GROW of each radius, timed once; the upload is not included.  Which one ran is reported;
              without either the column is left out.  Where it ran, the kernel's GROW is compared with it (it must be equal).

The device routes are timed with HIP events around one whole call after warm-up; the nine variants and the copy alternate
inside each round, --reps rounds; median, min and max are reported.

    python tools/bench_morph.py [--out profiles/morph_u8.txt]
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

RADII = (2, 8, 64)


def plane(h, w):
    yy, xx = np.mgrid[:h, :w]
    rng = np.random.default_rng(3)
    rim = 1.0 + 0.05 * np.sin(np.arctan2(yy - h * 0.45, xx - w * 0.5) * 23.0)
    m = (((yy - h * 0.45) / (h * 0.3)) ** 2 + ((xx - w * 0.5) / (w * 0.25)) ** 2 <= rim).astype(np.uint8) * 255
    for _ in range(6):                                               # holes in the blob
        y, x, r = int(rng.integers(h // 3, h // 2)), int(rng.integers(w // 3, 2 * w // 3)), int(rng.integers(5, 60))
        m[y - r:y + r, x - r:x + r] = 0
    ys, xs = rng.integers(0, h, 4000), rng.integers(0, w, 4000)     # specks
    m[ys, xs] = 255
    return m


def host_grow(m, radius):
    """The host's Euclidean grow -> (plane or None, which route)."""
    try:
        from scipy import ndimage
        d = ndimage.distance_transform_edt(m < 128)
        return np.where(d <= radius, 255, 0).astype(np.uint8), 'scipy.ndimage.distance_transform_edt'
    except ImportError:
        pass
    try:
        import cv2
        d = cv2.distanceTransform((m < 128).astype(np.uint8), cv2.DIST_L2, cv2.DIST_MASK_PRECISE)
        return np.where(d <= radius, 255, 0).astype(np.uint8), 'cv2.distanceTransform (DIST_MASK_PRECISE)'
    except ImportError:
        return None, 'neither scipy nor cv2 imports here'


def kernel_split(fn):
    from torch.autograd import DeviceType
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        if e.device_type == DeviceType.CUDA and 'k_morph_' in e.key:
            split[re.findall(r'k_morph_(\w+)', e.key)[0]] = getattr(e, 'device_time_total', getattr(e, 'cuda_time_total', 0.0)) / 1e3
    return split


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--height', type=int, default=4000)
    ap.add_argument('--width', type=int, default=6000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no_host', action='store_true', help='skip the host column (and the byte comparison with it)')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_morph: needs the GPU (a CPU run says nothing about these times)')
    dev = torch.device('cuda', torch.cuda.current_device())
    h, w = args.height, args.width
    m = plane(h, w)
    src = torch.from_numpy(m.reshape(-1)).to(dev)
    work, dup = src.clone(), torch.empty_like(src)
    lines = ['moving the boundary of one %d x %d plane (%.1f Mpx, %.1f %% set), %s; %d rounds after %d warm-up rounds, the variants and the copy '
             'alternating inside a round' % (h, w, h * w / 1e6, 100.0 * (m >= 128).mean(), torch.cuda.get_device_name(dev), args.reps, args.warmup)]
    variants = [(mode, r) for r in RADII for mode in T.MORPH_MODES]
    for mode in T.MORPH_MODES:
        need = T._lib.load().t2o_morph_workspace_bytes(T.morph_jobs([(0, 0, h, w, 2, mode)]), 1)
        lines.append('workspace for %-6s %d bytes (%.2f per pixel); 2 launches per call' % (mode + ':', need, need / (h * w)))
    times = {v: [] for v in variants + ['copy']}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    for rnd in range(args.warmup + args.reps):
        for mode, r in variants:
            work.copy_(src)                                          # outside the timed span
            t = timed(lambda: T.morph_u8(work, [(0, 0, h, w, r, mode)]))
            if rnd >= args.warmup:
                times[mode, r].append(t)
        t = timed(lambda: dup.copy_(src))
        if rnd >= args.warmup:
            times['copy'].append(t)
    copy = np.array(times['copy'])
    lines.append('    %-16s median %9.3f ms   min %9.3f   max %9.3f' % ('copy', np.median(copy), copy.min(), copy.max()))
    med = {}
    for mode, r in variants:
        t = np.array(times[mode, r])
        med[mode, r] = float(np.median(t))
        work.copy_(src)
        split = kernel_split(lambda: T.morph_u8(work, [(0, 0, h, w, r, mode)]))
        lines.append('    %-6s R = %-3d    median %9.3f ms   min %9.3f   max %9.3f   %6.1f x the copy   by kernel, one profiled call: %s'
                     % (mode, r, med[mode, r], t.min(), t.max(), med[mode, r] / np.median(copy),
                        ', '.join('%s %.3f ms' % (k, split[k]) for k in ('cols', 'rows') if k in split)))
    print('\n'.join(lines), flush=True)
    all_equal = True
    # the three modes agree with each other on the device: BORDER = GROW and not SHRINK
    for r in RADII:
        outs = {}
        for mode in T.MORPH_MODES:
            outs[mode] = T.morph_u8(src, [(0, 0, h, w, r, mode)], out=torch.empty_like(src))
        same = bool(torch.equal(outs['border'], outs['grow'] & ~outs['shrink']))
        all_equal = all_equal and same
        lines.append('R = %d: border equals grow and not shrink on the device: %s' % (r, same))
        if not args.no_host:
            t0 = time.perf_counter()
            want, route = host_grow(m, r)
            host_ms = (time.perf_counter() - t0) * 1e3
            if want is None:
                lines.append('    host: %s' % route)
            else:
                equal = bool(np.array_equal(want.reshape(-1), outs['grow'].cpu().numpy()))
                all_equal = all_equal and equal
                lines.append('    host grow once %9.1f ms (%s on the CPU, no upload): %.0f x the kernel; kernel bytes equal its bytes: %s'
                             % (host_ms, route, host_ms / med['grow', r], equal))
    for mode in T.MORPH_MODES:
        lines.append('R = 64 over R = 2, %s: %.1f x' % (mode, med[mode, 64] / med[mode, 2]))
    lines.append('not measured: real photos, several jobs in one call, soft planes, pictures of other sizes, the share of peak, a counter run')
    text = '\n'.join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print('\n'.join(lines[-(3 + 2 * len(RADII) + 1):]))
    if not all_equal:
        raise SystemExit('bench_morph: the kernel\'s bytes differ between its modes or from the host route\'s')


if __name__ == '__main__':
    main()
