"""The data step of one train batch, host path against device path ("Data step on the device").

Workload: 64 items x 7 images, generated, ALREADY DECODED 500 x 333 uint8 images, resized to 128 x 128 and to 256 x 256
and converted to (3,S,S) fp32 in [0,1].  JPEG decoding is outside BOTH columns: it stays on the host either way.

  host    data.resize_linear_u8 + astype(float32).transpose / 255 per image (what data.load_image does after decoding),
          in one process, then spread over 16 worker processes (results returned to the parent, as a DataLoader's are)
  device  functional.pack_u8 (memcpy into one pinned buffer), the single host-to-device copy, k_resize_u8_f32 -- timed
          separately; the kernel with HIP events over --launches launches after warm-up

    python tools/bench_data_step.py [--out profiles/data_step.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from t2onet_amd import data                      # noqa: E402

ITEMS, PER_ITEM, SRC_H, SRC_W = 64, 7, 333, 500
_IMAGES = None


def _host_one(job):
    i, size = job
    return data.resize_linear_u8(_IMAGES[i], size, size).astype(np.float32).transpose(2, 0, 1) / 255.0


def _best(fn, reps):
    times = []
    for _ in range(reps):
        tik = time.perf_counter()
        fn()
        times.append(time.perf_counter() - tik)
    return min(times)


def main(argv=None):
    global _IMAGES
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--workers', type=int, default=16)
    args = ap.parse_args(argv)
    n = ITEMS * PER_ITEM
    rng = np.random.default_rng(0)
    _IMAGES = [rng.integers(0, 256, (SRC_H, SRC_W, 3), dtype=np.uint8) for _ in range(n)]
    lines = ['data step of one train batch: %d items x %d decoded %d x %d uint8 images = %d resizes; JPEG decode is outside both columns'
             % (ITEMS, PER_ITEM, SRC_W, SRC_H, n)]

    host = {}
    import multiprocessing as mp
    for size in (128, 256):                       # (the workers are forked, and gone, before the GPU is opened)
        jobs = [(i, size) for i in range(n)]
        one = _best(lambda: [_host_one(j) for j in jobs], args.reps)
        with mp.get_context('fork').Pool(args.workers) as pool:
            pool.map(_host_one, jobs[:args.workers])                                  # start-up outside the timing
            many = _best(lambda: pool.map(_host_one, jobs, chunksize=PER_ITEM), args.reps)
        host[size] = (one, many)

    import torch
    import t2onet_amd.functional as T
    dev = torch.device('cuda:0')
    pack = _best(lambda: T.pack_u8(_IMAGES), args.reps)
    buffer, descs = T.pack_u8(_IMAGES)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, count):
        fn()
        torch.cuda.synchronize()
        start.record()
        for _ in range(count):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / count * 1e-3

    h2d = timed(lambda: buffer.to(dev, non_blocking=True), 10)
    dev_buffer, table_ptr, _, _keep = T.upload_packed(buffer, descs, dev)
    mb = buffer.numel() / 1e6
    for size in (128, 256):
        out = torch.empty(n, 3, size, size, device=dev)
        kern = timed(lambda: T._resize_launch(dev_buffer, table_ptr, n, size, size, out), args.launches)
        ref = torch.from_numpy(np.stack([_host_one((i, size)) for i in range(0, n, 37)]))
        assert torch.equal(out[::37].cpu(), ref), 'device result differs from the host path'
        whole = _best(lambda: (T.resize_u8(_IMAGES, size, dev), torch.cuda.synchronize()), args.reps)
        one, many = host[size]
        total = pack + h2d + kern
        lines += ['',
                  '%d x %d' % (size, size),
                  '  host, 1 process            %9.2f ms  (%8.0f img/s)' % (one * 1e3, n / one),
                  '  host, %2d processes         %9.2f ms  (%8.0f img/s)' % (args.workers, many * 1e3, n / many),
                  '  device: pack (pinned)      %9.2f ms  (%.1f MB, %.1f GB/s memcpy)' % (pack * 1e3, mb, mb / pack * 1e-3),
                  '  device: H2D                %9.2f ms  (%.1f GB/s)' % (h2d * 1e3, mb / h2d * 1e-3),
                  '  device: k_resize_u8_f32    %9.3f ms  (HIP events, mean of %d launches)' % (kern * 1e3, args.launches),
                  '  device: pack + H2D + kernel%9.2f ms  (%8.0f img/s); resize_u8() wall time %.2f ms' % (total * 1e3, n / total, whole * 1e3),
                  '  upload share of H2D + kernel: %.0f %% -- the device column is %s' % (
                      100 * h2d / (h2d + kern), 'bound by the upload' if h2d > kern else 'bound by the kernel')]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
