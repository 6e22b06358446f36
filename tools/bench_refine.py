"""Refining one mask plane of a photo's size: the integer guided-filter kernels (functional.refine_u8) against what a user
can do today ("refined masks").  Run by hand; not a test and not part of bench.py.

Workload: one generated 4000 x 6000 RGB photo (smooth colour fields with hard edges and noise) and one 0/255 plane of blocks
and a disc whose edges lie a few pixels beside the photo's, both already on the device; radius 2, 8, 32, 64, E = 26.

  kernel      functional.refine_u8: four launches
  fw-pool     the same card through the framework, the same filter in fp32: luminance from the bytes, the four box means by
              F.avg_pool2d over a (1, 2r+1) and a (2r+1, 1) window on replicate-padded tensors, a = cov / (var + E),
              b = mean_p - a mean_I, the two box means again, a I + b, round, clamp, -> uint8
  fw-cumsum   the same with every box sum as differences of a cumsum along each axis of the replicate-padded tensor
  host        the numpy int64 oracle of the integer definition on the CPU plus the upload of its result (timed once)

The three device routes are timed with HIP events around one whole call after warm-up, alternating, --reps times.  The
kernel's bytes are compared with the host oracle's first (they must be equal).  The framework routes are NOT exact and are
not the oracle: how many of their bytes differ from the kernel's, and by how much, is reported.  The condition, per radius:
the kernel's slowest call is faster than the fastest call of the FASTER framework route (ranges that do not overlap).

    python tools/bench_refine.py [--out profiles/refine_u8.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import t2onet_amd.functional as T                # noqa: E402

RADII = [2, 8, 32, 64]
EPS2 = 26


def plane(h, w):
    """0/255: blocks with edges off any tile border, and a disc."""
    m = np.zeros((h, w), np.uint8)
    m[h // 10:h // 3 + 1, w // 12:w // 2 - 3] = 255
    m[h // 2 + 5:h - h // 7, w // 3 + 1:w // 3 + w // 9] = 255
    yy, xx = np.ogrid[:h, :w]
    m[(yy - 2 * h // 3) ** 2 + (xx - 3 * w // 4) ** 2 <= (min(h, w) // 5) ** 2] = 255
    return m


def photo(h, w):
    """The plane's shapes 4 pixels further up and left, as colour fields on a gradient, plus noise of +-6."""
    rng = np.random.default_rng(5)
    m = np.roll(plane(h, w), (-4, -4), (0, 1)) > 0
    yy, xx = np.mgrid[:h, :w]
    base = np.stack([40 + 60 * xx // w, 60 + 50 * yy // h, 90 + 0 * xx], -1)
    img = np.where(m[..., None], np.array([210, 180, 120]), base) + rng.integers(-6, 7, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def host_box(a, r):
    h, w = a.shape
    k = 2 * r + 1
    p = a[np.clip(np.arange(-r, h + r), 0, h - 1)][:, np.clip(np.arange(-r, w + r), 0, w - 1)]
    c = np.zeros((h + k, w + k), np.int64)
    c[1:, 1:] = p.cumsum(0).cumsum(1)
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def host_refine(rgb, m, r, E):
    """The integer definition of include/t2onet_hip.h in numpy int64."""
    c = rgb.astype(np.int64)
    I = (69 * c[..., 0] + 172 * c[..., 1] + 15 * c[..., 2] + 128) >> 8
    p = m.astype(np.int64)
    n = (2 * r + 1) ** 2
    SI, Sp, SII, SIp = host_box(I, r), host_box(p, r), host_box(I * I, r), host_box(I * p, r)
    den = n * SII - SI * SI + E * n * n
    A = (2 * (n * SIp - SI * Sp) * 1024 + den) // (2 * den)
    del SII, SIp, den
    B = (2 * ((Sp << 10) - A * SI) + n) // (2 * n)
    del SI, Sp
    d = n << 10
    return np.clip((2 * (host_box(A, r) * I + host_box(B, r)) + d) // (2 * d), 0, 255).astype(np.uint8)


def box_pool(x, r):
    """Box MEANS of (1, C, h, w) fp32 over (2r+1)^2 with replicated borders: two one-dimensional average pools."""
    k = 2 * r + 1
    x = F.avg_pool2d(F.pad(x, (r, r, 0, 0), mode='replicate'), (1, k), stride=1)
    return F.avg_pool2d(F.pad(x, (0, 0, r, r), mode='replicate'), (k, 1), stride=1)


def box_cumsum(x, r):
    """The same through cumulative sums along each axis of the replicate-padded tensor."""
    k = 2 * r + 1
    c = F.pad(F.pad(x, (r, r, 0, 0), mode='replicate'), (1, 0, 0, 0)).cumsum(3)
    x = (c[..., k:] - c[..., :-k]) / k
    c = F.pad(F.pad(x, (0, 0, r, r), mode='replicate'), (0, 0, 1, 0)).cumsum(2)
    return (c[:, :, k:] - c[:, :, :-k]) / k


def framework(rgb, m, h, w, r, E, box):
    c = rgb.view(h, w, 3).to(torch.float32)
    I = torch.floor((69.0 * c[..., 0] + 172.0 * c[..., 1] + 15.0 * c[..., 2] + 128.0) / 256.0)
    p = m.view(h, w).to(torch.float32)
    mean = box(torch.stack([I, p, I * I, I * p]).unsqueeze(0), r)[0]
    a = (mean[3] - mean[0] * mean[1]) / (mean[2] - mean[0] * mean[0] + float(E))
    b = mean[1] - a * mean[0]
    ab = box(torch.stack([a, b]).unsqueeze(0), r)[0]
    return (ab[0] * I + ab[1]).round_().clamp_(0, 255).to(torch.uint8)


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
        raise SystemExit('bench_refine: needs the GPU (a CPU run says nothing about these times)')
    dev = torch.device('cuda', torch.cuda.current_device())
    h, w = args.height, args.width
    m, rgb = plane(h, w), photo(h, w)
    src = torch.from_numpy(m.reshape(-1)).to(dev)
    pic = torch.from_numpy(rgb.reshape(-1)).to(dev)
    out = torch.empty_like(src)
    lines = ['refining one %d x %d uint8 plane (%.1f Mpx) under its RGB photo, E = %d, %s; %d timed calls each after %d warm-up calls, alternating'
             % (h, w, h * w / 1e6, EPS2, torch.cuda.get_device_name(dev), args.reps, args.warmup),
             'kernel workspace: %d bytes (%d per pixel of the padded plane)'
             % (T._lib.load().t2o_refine_workspace_bytes(T.refine_jobs([(0, 0, 0, h, w, 2, EPS2)]), 1), 20)]
    all_equal, all_hold = True, True
    for r in RADII:
        job = [(0, 0, 0, h, w, r, EPS2)]
        routes = {'kernel': lambda: T.refine_u8(pic, src, job, out=out),
                  'fw-pool': lambda: framework(pic, src, h, w, r, EPS2, box_pool),
                  'fw-cumsum': lambda: framework(pic, src, h, w, r, EPS2, box_cumsum)}
        lines.append('radius %d (%d x %d window):' % (r, 2 * r + 1, 2 * r + 1))
        first = len(lines)
        with torch.no_grad():
            for _ in range(args.warmup):
                got = {name: fn() for name, fn in routes.items()}
            torch.cuda.synchronize()
            for name in ('fw-pool', 'fw-cumsum'):
                d = (got[name].view(-1).to(torch.int16) - out.to(torch.int16)).abs()
                lines.append('  %-10s differs from the kernel in %d of %d bytes, by at most %d' % (name, int((d > 0).sum().item()), h * w, int(d.max().item())))
            del got, d
            times = {name: [] for name in routes}
            for _ in range(args.reps):
                for name, fn in routes.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    times[name].append(a.elapsed_time(b))
        if not args.no_host:
            t0 = time.perf_counter()
            up = torch.from_numpy(host_refine(rgb, m, r, EPS2)).to(dev)
            torch.cuda.synchronize()
            host_ms = (time.perf_counter() - t0) * 1e3
            equal = bool(torch.equal(up.view(-1), out))
            all_equal = all_equal and equal
            lines.append('  kernel bytes equal the host oracle\'s: %s' % equal)
        t = {name: np.array(v) for name, v in times.items()}
        for name in routes:
            lines.append('  %-10s median %9.3f ms   min %9.3f   max %9.3f' % (name, np.median(t[name]), t[name].min(), t[name].max()))
        if not args.no_host:
            lines.append('  %-10s once   %9.1f ms (numpy int64 on the CPU + upload)' % ('host', host_ms))
        best = min(('fw-pool', 'fw-cumsum'), key=lambda name: np.median(t[name]))
        hold = bool(t['kernel'].max() < t[best].min())
        all_hold = all_hold and hold
        lines.append('  condition, the kernel\'s slowest call below the fastest call of %s: %s   median %s / kernel = %.2fx'
                     % (best, 'holds' if hold else 'FAILS', best, np.median(t[best]) / np.median(t['kernel'])))
        print('\n'.join(lines[first - 1:]), flush=True)
    lines.append('the condition %s at all four radii' % ('holds' if all_hold else 'FAILS'))
    lines.append('not measured: real photos, several planes in one call, planes of other sizes, the kernels one by one, their share of peak')
    text = '\n'.join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(lines[-2])
    if not all_equal:
        raise SystemExit('bench_refine: the kernel\'s bytes differ from the host oracle\'s')
    if not all_hold:
        raise SystemExit('bench_refine: the kernel is not clear of the framework route at some radius')


if __name__ == '__main__':
    main()
