"""Removing a region of a photo's size: the push-pull fill kernels (functional.fill_u8) on a picture with holes of
different sizes, against a device copy of the photo's bytes and against a host route ("removing a region").
Run by hand; not a test and not part of bench.py.  Nothing gates on a time: nobody had measured these kernels when the
tool was written.  The ratios to the copy and to the host route are written down as measured, never asserted.

Workload: one generated 4000 x 6000 RGB picture (a smooth diagonal gradient plus noise of +-2), already on the device, and
a hard 0 / 255 plane with ONE centred rectangular hole of 0 %, 1 %, 10 % or 50 % of the frame.

  kernel      functional.fill_u8, three launches, out of place and in place (what edit_image does); the split by kernel of
              ONE further call of each comes from the torch profiler
  copy        a device-to-device copy of the photo's 3 bytes per pixel: the memory floor of writing a picture once
  host        cv2.inpaint (Telea, radius 3) on the CPU of this machine where cv2 imports, else the int64 numpy oracle of
              tests/fill_cases.py (the same definition as the kernels'), timed once; the upload is not included.  Which one
              ran is reported.  The kernel's bytes are compared with the numpy oracle's when that is the host route (they
              must be equal); cv2.inpaint is another algorithm, so only its time is reported.

The device routes are timed with HIP events around one whole call after warm-up, alternating, --reps times; median, min and
max are reported.

    python tools/bench_fill.py [--out profiles/fill_u8.txt]
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

SHARES = (0.0, 0.01, 0.10, 0.50)


def picture(h, w):
    yy, xx = np.mgrid[:h, :w]
    g = (40 + 170 * (xx * h + yy * w) // (2 * h * w)).astype(np.int16)
    img = np.stack([g, g + 10, 255 - g], -1) + np.random.default_rng(3).integers(-2, 3, (h, w, 3), dtype=np.int16)
    return np.clip(img, 0, 255).astype(np.uint8)


def hole(h, w, share):
    """A centred rectangle of the frame's aspect that covers `share` of it, as a hard plane."""
    m = np.zeros((h, w), np.uint8)
    hh, ww = int(round(h * share ** 0.5)), int(round(w * share ** 0.5))
    m[(h - hh) // 2:(h - hh) // 2 + hh, (w - ww) // 2:(w - ww) // 2 + ww] = 255
    return m


def host_fill(photo, plane):
    """The host route -> (picture, which route, comparable with the kernel byte for byte)."""
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        return cv2.inpaint(photo, plane, 3, cv2.INPAINT_TELEA), 'cv2.inpaint (Telea, radius 3)', False
    from tests import fill_cases
    return fill_cases.oracle(photo, plane), 'the int64 numpy oracle of tests/fill_cases.py', True


def kernel_split(fn):
    from torch.autograd import DeviceType
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        if e.device_type == DeviceType.CUDA and 'k_fill_' in e.key:
            split[re.findall(r'k_fill_(\w+)', e.key)[0]] = getattr(e, 'device_time_total', getattr(e, 'cuda_time_total', 0.0)) / 1e3
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
        raise SystemExit('bench_fill: needs the GPU (a CPU run says nothing about these times)')
    dev = torch.device('cuda', torch.cuda.current_device())
    h, w = args.height, args.width
    need = T._lib.load().t2o_fill_workspace_bytes(T.fill_jobs([(0, 0, 0, h, w)]), 1)
    lines = ['removing a region of one %d x %d RGB picture (%.1f Mpx), %s; %d timed calls each after %d warm-up calls, alternating'
             % (h, w, h * w / 1e6, torch.cuda.get_device_name(dev), args.reps, args.warmup),
             'kernel workspace: %d bytes (%.2f per pixel); %d launches per call' % (need, need / (h * w), T.FILL_LAUNCHES)]
    rgb = picture(h, w)
    pic = torch.from_numpy(rgb.reshape(-1)).to(dev)
    work = pic.clone()                                               # the picture the in-place route fills again and again
    out, dup = torch.empty_like(pic), torch.empty_like(pic)
    job, here = [(0, 0, 0, h, w)], [(0, 0, 0, h, w)]
    all_equal, ratios, top_share = True, [], []
    for share in SHARES:
        m = hole(h, w, share)
        plane = torch.from_numpy(m.reshape(-1)).to(dev)
        work.copy_(pic)
        routes = {'kernel': lambda: T.fill_u8(pic, plane, job, out=out), 'in place': lambda: T.fill_u8(work, plane, here, out=work),
                  'copy': lambda: dup.copy_(pic)}
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
        first = len(lines)
        lines.append('hole of %g %% of the frame (%d pixels with M > 0, %d of %d tiles hold one):'
                     % (100 * share, int((m > 0).sum()), sum(bool(m[y:y + 64, x:x + 64].any()) for y in range(0, h, 64) for x in range(0, w, 64)),
                        ((h + 63) // 64) * ((w + 63) // 64)))
        for r in routes:
            lines.append('    %-8s median %9.3f ms   min %9.3f   max %9.3f' % (r, np.median(t[r]), t[r].min(), t[r].max()))
        for r in ('kernel', 'in place'):
            split = kernel_split(routes[r])
            top_share.append(split.get('top', 0.0) / max(sum(split.values()), 1e-9))
            lines.append('    %s by kernel, one profiled call: ' % r + ', '.join('%s %.3f ms' % (k, split[k]) for k in ('pull', 'top', 'push') if k in split))
        got = out.cpu().numpy().reshape(h, w, 3)
        same = bool(np.array_equal(got, work.cpu().numpy().reshape(h, w, 3)))
        all_equal = all_equal and same
        lines.append('    in place equals out of place: %s; ratio to the copy: kernel %.2f x, in place %.2f x'
                     % (same, np.median(t['kernel']) / np.median(t['copy']), np.median(t['in place']) / np.median(t['copy'])))
        if not args.no_host:
            t0 = time.perf_counter()
            want, route, comparable = host_fill(rgb, m)
            host_ms = (time.perf_counter() - t0) * 1e3
            ratios.append(host_ms / np.median(t['kernel']))
            if comparable:
                equal = bool(np.array_equal(want, got))
                all_equal = all_equal and equal
                lines.append('    %-8s once   %9.1f ms (%s on the CPU, no upload): %.0f x the kernel; kernel bytes equal its bytes: %s'
                             % ('host', host_ms, route, ratios[-1], equal))
            else:
                lines.append('    %-8s once   %9.1f ms (%s on the CPU, no upload; another algorithm, bytes not compared): %.0f x the kernel'
                             % ('host', host_ms, route, ratios[-1]))
        print('\n'.join(lines[first:]), flush=True)
    lines.append('finding: the one-workgroup top pass takes %.0f - %.0f %% of the kernels\' time (it does not shrink with the hole; it runs levels 6..K '
                 'through global memory, a fence and a barrier per level)' % (100 * min(top_share), 100 * max(top_share)))
    lines.append('not measured: real photos, several jobs in one call, soft planes, pictures of other sizes, the share of peak')
    text = '\n'.join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print('\n'.join(lines[-2:]))
    if not all_equal:
        raise SystemExit('bench_fill: the kernel\'s bytes differ between its routes or from the host route\'s')


if __name__ == '__main__':
    main()
