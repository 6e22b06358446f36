"""An operator list that repeats the sharpness on one 8-bit photo at native size: the stencils replay kernel
(functional.replay_u8_stencils) against the materialised path, the only other way to these bytes ("replay
with several sharpness steps").

Workload: the generated 4000 x 6000 uint8 RGB picture of tools/bench_replay.py, already on the device, mid-range parameters.

  (a) materialised [0,6,1,6,5]        t2o_resize_u8_to_f32 at the picture's own size, t2o_op_fwd per step with every fp32
                                      image written to and read back from memory, t2o_f32_to_u8_hwc: 7 launches
  (b) stencils     [0,6,1,6,5]        functional.replay_u8_stencils: one launch, 3 bytes read + 3 written per pixel
  (c1) stencils    [0,6,1,2,5]        one sharpness, same length: the new kernel on a list the old one takes
  (c2) replay_u8   [0,6,1,2,5]        the old kernel on it
  (d) stencils     [0,6,1,6,5]        (b) with every step under one mask plane, 255 on a centred (h/4) x (w/4) rectangle

All columns are timed with HIP events around one whole call after warm-up, in one alternating loop, --reps times; the
bytes of (a) and (b), of (c1) and (c2), and of (d) and the materialised path under the same plane are compared first
(they must be equal).  GB/s = 6 B/px over the time for every column: the traffic the TASK needs.  One condition on the
medians: (b) is faster than (a).  (b) / (a), (c1) / (c2) and (d) / (b) are reported, not bounded.

    python tools/bench_replay_stencils.py [--out profiles/replay_u8_stencils.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import t2onet_amd.functional as T                # noqa: E402

TWO = [0, 6, 1, 6, 5]
ONE = [0, 6, 1, 2, 5]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--height', type=int, default=4000)
    ap.add_argument('--width', type=int, default=6000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_replay_stencils: needs the GPU (a CPU run says nothing about these times)')
    dev = torch.device('cuda', torch.cuda.current_device())
    h, w = args.height, args.width
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    params = np.zeros((1, 8, 24), np.float32)
    params[0, :5, 0] = [0.3, 0.8, 0.4, 0.5, 0.0]                 # brightness, sharpness, contrast, sharpness | saturation, tone
    params[0, 4, :8] = rng.uniform(0.5, 2.0, 8)
    par = torch.from_numpy(params).to(dev)
    rows = [par[0, k:k + 1] for k in range(5)]
    buffer, descs = T.pack_u8([img])
    dev_buffer, table_ptr, descs, _keep = T.upload_packed(buffer, descs, dev)
    offset = int(descs[0]['offset'])
    region = torch.zeros(h, w, dtype=torch.uint8, device=dev)
    region[h // 2 - h // 8:h // 2 - h // 8 + h // 4, w // 2 - w // 8:w // 2 - w // 8 + w // 4] = 255
    region = region.view(-1)
    region_f = (region.view(1, 1, h, w).to(torch.float32) / 255.0).contiguous()
    outs = {k: torch.empty(img.size, dtype=torch.uint8, device=dev) for k in ('b', 'c1', 'c2', 'd')}
    out_mat = torch.empty(1, h, w, 3, dtype=torch.uint8, device=dev)
    x0 = torch.empty(1, 3, h, w, device=dev)

    def materialised(mask_f=None):
        x = T._resize_launch(dev_buffer, table_ptr, 1, h, w, out=x0)
        for op, row in zip(TWO, rows):
            x = T.operator_apply(op, x, row, mask_f)
        T.to_u8_hwc(x, out=out_mat)

    def stencils_two():
        T.replay_u8_stencils(dev_buffer, [(offset, 0, h, w, TWO)], par, out=outs['b'])

    def stencils_one():
        T.replay_u8_stencils(dev_buffer, [(offset, 0, h, w, ONE)], par, out=outs['c1'])

    def old_one():
        T.replay_u8(dev_buffer, [(offset, 0, h, w, ONE)], par, out=outs['c2'])

    def stencils_region():
        T.replay_u8_stencils(dev_buffer, [(offset, 0, h, w, TWO, [0] * 5)], par, region, [0], out=outs['d'])

    legs = [('(a) materialised [0,6,1,6,5]', materialised), ('(b) stencils [0,6,1,6,5]', stencils_two),
            ('(c1) stencils [0,6,1,2,5]', stencils_one), ('(c2) replay_u8 [0,6,1,2,5]', old_one),
            ('(d) stencils, 1/16 region mask', stencils_region)]
    with torch.no_grad():
        materialised(region_f)
        stencils_region()
        torch.cuda.synchronize()
        equal_d = bool(torch.equal(outs['d'], out_mat.view(-1)))
        for _ in range(args.warmup):
            for _, fn in legs:
                fn()
        torch.cuda.synchronize()
        equal_ab = bool(torch.equal(outs['b'], out_mat.view(-1)))
        equal_c = bool(torch.equal(outs['c1'], outs['c2']))
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
    prop = torch.cuda.get_device_properties(dev)
    lines = ['8-bit replay with several sharpness steps on one %d x %d picture (%.1f Mpx); %d timed calls each after %d warm-up '
             'calls, alternating' % (h, w, h * w / 1e6, args.reps, args.warmup),
             'machine: %s, %d CUs, %.0f GB; torch %s, HIP %s' % (prop.name, prop.multi_processor_count, prop.total_memory / 2 ** 30,
                                                                 torch.__version__, torch.version.hip),
             'bytes equal: (a) = (b): %s   (c1) = (c2): %s   (d) = materialised under the same plane: %s' % (equal_ab, equal_c, equal_d)]
    for name, _ in legs:
        lines.append('%-32s median %8.3f ms   min %8.3f   max %8.3f   -> %7.1f GB/s on 6 B/px (median)'
                     % (name, med[name], lo[name], hi[name], 6.0 * h * w / (med[name] * 1e-3) / 1e9))
    A, B, C1, C2, D = [name for name, _ in legs]
    ok = med[B] < med[A]
    lines.append('condition, (b) faster than (a): %s   (b) / (a) = %.3f   ((b) %.3f [%.3f .. %.3f] against (a) %.3f [%.3f .. %.3f] ms)'
                 % ('holds' if ok else 'FAILS', med[B] / med[A], med[B], lo[B], hi[B], med[A], lo[A], hi[A]))
    lines.append('reported, not bounded: (c1) / (c2) = %.2fx   (b) / (c2) = %.2fx   (d) / (b) = %.2fx'
                 % (med[C1] / med[C2], med[B] / med[C2], med[D] / med[B]))
    lines.append('not measured: real photos through the decoder, more than two sharpness steps (R > 2), the kernel\'s share of peak')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    if not (equal_ab and equal_c and equal_d):
        raise SystemExit('bench_replay_stencils: the paths differ')
    if not ok:
        raise SystemExit('bench_replay_stencils: (b) is not faster than (a)')


if __name__ == '__main__':
    main()
