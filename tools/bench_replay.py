"""A known operator list on one 8-bit photo at native size: the fused replay kernel against the materialised path it
replaces ("8-bit replay at native size").

Workload: one generated 4000 x 6000 uint8 RGB picture already on the device, the six-operator list [0,1,2,3,5,6]
(brightness, contrast, saturation, color curve, tone curve, sharpness) with mid-range parameters.

  fused         functional.replay_u8: one launch, 3 bytes read + 3 bytes written per pixel
  materialised  t2o_resize_u8_to_f32 at the picture's own size (u8 -> f32), t2o_op_fwd per step with every fp32 image
                written to and read back from memory, t2o_f32_to_u8_hwc (f32 -> u8): 8 launches

Both columns are timed with HIP events around one whole call after warm-up, alternating, --reps times; the bytes of the
two paths are compared first (they must be equal).  GB/s = 6 B/px over the time, for both columns: the traffic the TASK
needs, not what the materialised path moves.

    python tools/bench_replay.py [--out profiles/replay_u8.txt]

--masked runs the LOCAL-edit leg instead ("masked replay"): the same picture and list with a mask on every
step, four columns timed the same way in one alternating loop:

  (a) materialised masked   t2o_resize_u8_to_f32 -> t2o_op_fwd WITH the mask ((1,1,h,w) fp32) per step -> t2o_f32_to_u8_hwc
  (b) masked, all 255       functional.replay_u8_masked, one all-255 plane named by every step
  (c) masked, 1/16 region   the same call, the plane 255 on a centred (h/4) x (w/4) rectangle and 0 elsewhere
  (d) replay_u8             the unmasked kernel

and states two conditions on the medians of this run, the run-to-run range beside them: (b) is not slower than (a), (c)
is not slower than (b).  (b) / (d) is reported, not bounded.  The bytes of (a) and (b) are compared first, (b) against (d)
as well (an all-255 mask is no mask), and (c) against the materialised path under the same plane.

    python tools/bench_replay.py --masked [--out profiles/replay_u8_masked.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import t2onet_amd.functional as T                # noqa: E402

OPS = [0, 1, 2, 3, 5, 6]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--height', type=int, default=4000)
    ap.add_argument('--width', type=int, default=6000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--masked', action='store_true', help='the local-edit leg (replay_u8_masked)')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_replay: needs the GPU (a CPU run says nothing about these times)')
    dev = torch.device('cuda', torch.cuda.current_device())
    h, w = args.height, args.width
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    params = np.zeros((1, 8, 24), np.float32)
    params[0, :6, 0] = [0.3, 0.4, 0.5, 0.0, 0.0, 0.8]
    params[0, 3] = rng.uniform(0.9, 1.1, 24)
    params[0, 4, :8] = rng.uniform(0.5, 2.0, 8)
    par = torch.from_numpy(params).to(dev)
    buffer, descs = T.pack_u8([img])
    dev_buffer, table_ptr, descs, _keep = T.upload_packed(buffer, descs, dev)
    offset = int(descs[0]['offset'])
    out_fused = torch.empty(img.size, dtype=torch.uint8, device=dev)
    out_mat = torch.empty(1, h, w, 3, dtype=torch.uint8, device=dev)
    x0 = torch.empty(1, 3, h, w, device=dev)
    rows = [par[0, k:k + 1] for k in range(len(OPS))]

    def fused():
        T.replay_u8(dev_buffer, [(offset, 0, h, w, OPS)], par, out=out_fused)

    def materialised():
        x = T._resize_launch(dev_buffer, table_ptr, 1, h, w, out=x0)
        for op, row in zip(OPS, rows):
            x = T.operator_apply(op, x, row)
        T.to_u8_hwc(x, out=out_mat)

    if args.masked:
        return masked_leg(args, dev, img, par, rows, dev_buffer, table_ptr, offset, fused, out_fused, out_mat, x0)

    with torch.no_grad():
        for _ in range(args.warmup):
            fused()
            materialised()
        torch.cuda.synchronize()
        equal = bool(torch.equal(out_fused, out_mat.view(-1)))
        times = {'fused': [], 'materialised': []}
        for _ in range(args.reps):
            for name, fn in (('fused', fused), ('materialised', materialised)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
    task_bytes = 6.0 * h * w
    lines = ['8-bit replay of %s on one %d x %d picture (%.1f Mpx), %s; %d timed calls each after %d warm-up calls, alternating'
             % (OPS, h, w, h * w / 1e6, torch.cuda.get_device_name(dev), args.reps, args.warmup),
             'bytes of the two paths equal: %s' % equal]
    for name in ('fused', 'materialised'):
        t = np.array(times[name])
        lines.append('%-13s median %8.3f ms   min %8.3f   max %8.3f   -> %7.1f GB/s on 6 B/px (median)'
                     % (name, np.median(t), t.min(), t.max(), task_bytes / (np.median(t) * 1e-3) / 1e9))
    lines.append('materialised / fused (medians): %.2fx' % (np.median(times['materialised']) / np.median(times['fused'])))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    if not equal:
        raise SystemExit('bench_replay: the two paths differ')


def masked_leg(args, dev, img, par, rows, dev_buffer, table_ptr, offset, fused, out_fused, out_mat, x0):
    h, w = img.shape[:2]
    full = torch.full((h * w,), 255, dtype=torch.uint8, device=dev)
    region = torch.zeros(h, w, dtype=torch.uint8, device=dev)
    region[h // 2 - h // 8:h // 2 - h // 8 + h // 4, w // 2 - w // 8:w // 2 - w // 8 + w // 4] = 255
    region = region.view(-1)
    full_f = torch.ones(1, 1, h, w, device=dev)
    region_f = (region.view(1, 1, h, w).to(torch.float32) / 255.0).contiguous()
    out_b = torch.empty(img.size, dtype=torch.uint8, device=dev)
    out_c = torch.empty(img.size, dtype=torch.uint8, device=dev)
    job = [(offset, 0, h, w, OPS, [0] * len(OPS))]

    def materialised_masked(mask_f=full_f):
        x = T._resize_launch(dev_buffer, table_ptr, 1, h, w, out=x0)
        for op, row in zip(OPS, rows):
            x = T.operator_apply(op, x, row, mask_f)
        T.to_u8_hwc(x, out=out_mat)

    def masked_full():
        T.replay_u8_masked(dev_buffer, job, par, full, [0], out=out_b)

    def masked_region():
        T.replay_u8_masked(dev_buffer, job, par, region, [0], out=out_c)

    legs = [('(a) materialised masked', materialised_masked), ('(b) masked, all 255', masked_full),
            ('(c) masked, 1/16 region', masked_region), ('(d) replay_u8', fused)]
    with torch.no_grad():
        materialised_masked(region_f)
        masked_region()
        torch.cuda.synchronize()
        equal_c = bool(torch.equal(out_c, out_mat.view(-1)))
        for _ in range(args.warmup):
            for _, fn in legs:
                fn()
        torch.cuda.synchronize()
        equal_ab = bool(torch.equal(out_b, out_mat.view(-1)))
        equal_bd = bool(torch.equal(out_b, out_fused))
        times = {name: [] for name, _ in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
    med = {name: float(np.median(times[name])) for name, _ in legs}
    lo = {name: float(np.min(times[name])) for name, _ in legs}
    hi = {name: float(np.max(times[name])) for name, _ in legs}
    lines = ['masked 8-bit replay of %s, a mask on every step, on one %d x %d picture (%.1f Mpx), %s; %d timed calls each after '
             '%d warm-up calls, alternating' % (OPS, h, w, h * w / 1e6, torch.cuda.get_device_name(dev), args.reps, args.warmup),
             'bytes equal: (a) = (b): %s   (b) = (d): %s   (c) = materialised under the same plane: %s' % (equal_ab, equal_bd, equal_c)]
    for name, _ in legs:
        px_bytes = 6.0 if name.startswith('(d)') else 7.0
        lines.append('%-24s median %8.3f ms   min %8.3f   max %8.3f   -> %7.1f GB/s on %d B/px (median)'
                     % (name, med[name], lo[name], hi[name], px_bytes * h * w / (med[name] * 1e-3) / 1e9, px_bytes))
    A, B, C, D = [name for name, _ in legs]
    ok_ba, ok_cb = med[B] <= med[A], med[C] <= med[B]
    lines.append('condition 1, (b) not slower than (a): %s   (b) %.3f [%.3f .. %.3f] against (a) %.3f [%.3f .. %.3f] ms, (a) / (b) = %.2fx'
                 % ('holds' if ok_ba else 'FAILS', med[B], lo[B], hi[B], med[A], lo[A], hi[A], med[A] / med[B]))
    lines.append('condition 2, (c) not slower than (b): %s   (c) %.3f [%.3f .. %.3f] against (b) %.3f [%.3f .. %.3f] ms, (b) / (c) = %.2fx'
                 % ('holds' if ok_cb else 'FAILS', med[C], lo[C], hi[C], med[B], lo[B], hi[B], med[B] / med[C]))
    lines.append('reported, not bounded: (b) / (d) = %.2fx   ((b) %.3f [%.3f .. %.3f] against (d) %.3f [%.3f .. %.3f] ms)'
                 % (med[B] / med[D], med[B], lo[B], hi[B], med[D], lo[D], hi[D]))
    lines.append('not measured: real photos through the decoder, masks larger than the L2 working set, '
                 'the kernel\'s share of peak')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    if not (equal_ab and equal_bd and equal_c):
        raise SystemExit('bench_replay: the masked paths differ')
    if not (ok_ba and ok_cb):
        raise SystemExit('bench_replay: a condition of the masked leg fails')


if __name__ == '__main__':
    main()
