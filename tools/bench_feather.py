"""Feathering one mask plane of a photo's size: the integer Gaussian kernels (functional.feather_u8) against what a user
can do today ("feathered masks").  Run by hand; not a test and not part of bench.py.

Workload: one generated 4000 x 6000 uint8 plane -- 0/255 blocks and a disc -- already on the device, sigma 2, 8, 32, 64.

  kernel     functional.feather_u8: two launches, 1 byte read + 2 written, then 2 read + 1 written per pixel
  framework  the same card through the framework: uint8 -> fp32, F.pad(replicate) + F.conv2d with a (1, 2R+1) kernel,
             the same with a (2R+1, 1) kernel, round, clamp, -> uint8 (the Gaussian of feather_weights / 65536 in fp32)
  host       the numpy oracle of the integer definition on the CPU plus the upload of its result (timed once per sigma)

kernel and framework are timed with HIP events around one whole call after warm-up, alternating, --reps times.  GB/s =
6 B/px over the time, for every column: the traffic the TASK needs by the kernel's model.  The kernel's bytes are compared
with the host oracle's first (they must be equal); the framework's differ by its fp32 rounding, the largest difference is
reported.  The condition, stated on the medians of this run with the run-to-run range beside them: the kernel is not
slower than the framework route at any of the four sigma.

    python tools/bench_feather.py [--out profiles/feather_u8.txt]
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

SIGMAS = [2, 8, 32, 64]


def plane(h, w):
    """0/255: blocks with edges off any tile border, and a disc."""
    m = np.zeros((h, w), np.uint8)
    m[h // 10:h // 3 + 1, w // 12:w // 2 - 3] = 255
    m[h // 2 + 5:h - h // 7, w // 3 + 1:w // 3 + w // 9] = 255
    yy, xx = np.ogrid[:h, :w]
    m[(yy - 2 * h // 3) ** 2 + (xx - 3 * w // 4) ** 2 <= (min(h, w) // 5) ** 2] = 255
    return m


def taps_of(sigma):
    w = T.feather_weights(sigma).astype(np.int64)
    if len(w) == 1:
        w[0] = 65536
    return np.concatenate([w[:0:-1], w])


def host_feather(m, sigma):
    """The integer definition in numpy; every value fits uint32."""
    taps = taps_of(sigma).astype(np.uint32)
    R = len(taps) // 2
    h, w = m.shape
    mp = np.pad(m.astype(np.uint32), ((0, 0), (R, R)), mode='edge')
    a = np.zeros((h, w), np.uint32)
    for k, t in enumerate(taps):
        a += t * mp[:, k:k + w]
    tp = np.pad((a + np.uint32(128)) >> np.uint32(8), ((R, R), (0, 0)), mode='edge')
    b = np.zeros((h, w), np.uint32)
    for k, t in enumerate(taps):
        b += t * tp[k:k + h, :]
    return ((b + np.uint32(1 << 23)) >> np.uint32(24)).astype(np.uint8)


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
        raise SystemExit('bench_feather: needs the GPU (a CPU run says nothing about these times)')
    dev = torch.device('cuda', torch.cuda.current_device())
    h, w = args.height, args.width
    m = plane(h, w)
    src = torch.from_numpy(m.reshape(-1)).to(dev)
    out = torch.empty_like(src)
    task_bytes = 6.0 * h * w
    lines = ['feathering one %d x %d uint8 plane (%.1f Mpx), %s; %d timed calls each after %d warm-up calls, alternating; GB/s on 6 B/px'
             % (h, w, h * w / 1e6, torch.cuda.get_device_name(dev), args.reps, args.warmup)]
    all_equal, all_hold = True, True
    for sigma in SIGMAS:
        taps = taps_of(sigma)
        R = len(taps) // 2
        k = torch.from_numpy((taps.astype(np.float64) / 65536.0).astype(np.float32)).to(dev)
        kx, ky = k.view(1, 1, 1, -1), k.view(1, 1, -1, 1)
        job = [(0, 0, h, w, sigma)]

        def kernel():
            T.feather_u8(src, job, out=out)

        def framework():
            x = src.view(1, 1, h, w).to(torch.float32)
            x = F.conv2d(F.pad(x, (R, R, 0, 0), mode='replicate'), kx)
            x = F.conv2d(F.pad(x, (0, 0, R, R), mode='replicate'), ky)
            return x.round_().clamp_(0, 255).to(torch.uint8)

        with torch.no_grad():
            for _ in range(args.warmup):
                kernel()
                fw = framework()
            torch.cuda.synchronize()
            diff = int((fw.view(-1).to(torch.int16) - out.to(torch.int16)).abs().max().item())
            del fw
            times = {'kernel': [], 'framework': []}
            for _ in range(args.reps):
                for name, fn in (('kernel', kernel), ('framework', framework)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    times[name].append(a.elapsed_time(b))
        lines.append('sigma %g (R = %d): largest |framework - kernel| = %d' % (sigma, R, diff))
        if not args.no_host:
            t0 = time.perf_counter()
            ref = host_feather(m, sigma)
            up = torch.from_numpy(ref).to(dev)
            torch.cuda.synchronize()
            host_ms = (time.perf_counter() - t0) * 1e3
            equal = bool(torch.equal(up.view(-1), out))
            all_equal = all_equal and equal
            lines.append('  kernel bytes equal the host oracle\'s: %s' % equal)
        med = {}
        for name in ('kernel', 'framework'):
            t = np.array(times[name])
            med[name] = float(np.median(t))
            lines.append('  %-10s median %9.3f ms   min %9.3f   max %9.3f   -> %8.1f GB/s'
                         % (name, med[name], t.min(), t.max(), task_bytes / (med[name] * 1e-3) / 1e9))
        if not args.no_host:
            lines.append('  %-10s once   %9.1f ms (numpy on the CPU + upload)   -> %8.3f GB/s' % ('host', host_ms, task_bytes / (host_ms * 1e-3) / 1e9))
        hold = med['kernel'] <= med['framework']
        all_hold = all_hold and hold
        lines.append('  condition, kernel not slower than framework: %s   framework / kernel = %.2fx' % ('holds' if hold else 'FAILS', med['framework'] / med['kernel']))
        print('\n'.join(lines[-6:]), flush=True)
    lines.append('the condition %s at all four sigma' % ('holds' if all_hold else 'FAILS'))
    lines.append('not measured: several planes in one call, planes of other sizes, the kernels\' share of peak, real selections')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    if not all_equal:
        raise SystemExit('bench_feather: the kernel\'s bytes differ from the host oracle\'s')
    if not all_hold:
        raise SystemExit('bench_feather: the kernel is slower than the framework route at some sigma')


if __name__ == '__main__':
    main()
