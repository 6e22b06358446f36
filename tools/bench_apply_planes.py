"""What reading the uint8 mask planes in place costs or saves (recorded, no threshold) -> profiles/apply_planes.txt.

  * one masked per-sample operator step at B = 64, 128 x 128 and 256 x 256: functional.apply_planes (fused: the operator
    kernels read the planes) beside mask_select + apply_per_sample (two launches, a (B,1,H,W) fp32 mask in between), forward
    alone and forward + backward; device-event times, the variants ALTERNATING inside each of REPS rounds, median and range
    per variant.  The batch mixes the operators as the actor's choice does (every executor operator, a quarter sharpness).
    Expectation from the bytes: forward 25 instead of 33 per pixel, backward 37 instead of 40.
  * one Trainer.episode_step at --step_size with a MaskTable (fused, then two-launch) beside the unmasked step, synthetic
    weights, eager (a masked step bypasses the captured graphs): the step kernels are a small part of it.

    python tools/bench_apply_planes.py [--reps 30] [--step_batch 64] [--step_size 128] [--out profiles/apply_planes.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import t2onet_amd  # noqa: E402
import t2onet_amd.functional as T  # noqa: E402
from tools.bench_planner_mask import alternate, blob, report  # noqa: E402


def operator_step(S, B, reps, lines, dev):
    g = torch.Generator().manual_seed(5)
    img = torch.rand(B, 3, S, S, generator=g).to(dev)
    gout = torch.randn(B, 3, S, S, generator=g).to(dev)
    op_id = torch.tensor([(0, 1, 2, 6, 3, 5, 6, 0)[b % 8] for b in range(B)], dtype=torch.int32, device=dev)
    pred_op = (op_id + 3).long()
    param = torch.zeros(B, 24, device=dev)
    param[:, 0] = torch.linspace(-0.4, 0.4, B, device=dev)
    curves = (op_id == 3) | (op_id == 5)
    param[curves] = torch.rand(int(curves.sum()), 24, generator=g).to(dev) + 0.5
    planes = torch.from_numpy(np.stack([np.roll(blob(S, S), 5 * k, 1) for k in range(B)])).to(dev)
    slot = torch.full((B, 11), -1, dtype=torch.int32, device=dev)
    slot[torch.arange(B, device=dev), pred_op] = torch.arange(B, dtype=torch.int32, device=dev)
    slot[::4] = -1                                                          # every fourth sample: a global edit

    def fused():
        return T.apply_planes(op_id, pred_op, x, p, planes, slot)

    def two():
        return T.apply_per_sample(op_id, x, p, T.mask_select(planes, slot, pred_op))

    x, p = img, param
    with torch.no_grad():
        assert torch.equal(fused(), two())
        ms = alternate([('mask_select + apply_per_sample', two), ('apply_planes (fused)', fused)], reps)
    report('forward, B = %d at %d x %d, ms:' % (B, S, S), ms, 1, 'ms', lines)
    x, p = img.clone().requires_grad_(True), param.clone().requires_grad_(True)

    def both(fn):
        def run():
            x.grad = p.grad = None
            fn().backward(gout)
        return run
    ms = alternate([('mask_select + apply_per_sample', both(two)), ('apply_planes (fused)', both(fused))], reps)
    report('forward + backward (image and parameter gradients), B = %d at %d x %d, ms:' % (B, S, S), ms, 1, 'ms', lines)


def episode_step(S, B, reps, lines, dev):
    from oracle import synth
    from t2onet_amd.actor import Actor
    from t2onet_amd.gier import MaskTable
    from t2onet_amd.train import Trainer
    opt = t2onet_amd.default_options(batch_size=B, input_dropout_p=0.0, dropout_p=0.0)
    model = Actor(opt)
    model.load_state_dict(synth.fill_state_dict(model.state_dict(), seed=7))
    model = model.to(dev).train()
    tr = Trainer(model, opt, lr=0.0)
    x = synth.requests(B, 17, 41)
    lengths = (x != 0).sum(1)
    x = x.to(dev)
    img, tgt = synth.images(B, S, S, 42).to(dev), synth.images(B, S, S, 43).to(dev)
    plane = blob(S, S).astype(np.float32)
    table = MaskTable.from_arrays([{op: np.roll(plane, 3 * b, 1) for op in (3, 4, 5, 6, 8, 9)} if b % 4 else {} for b in range(B)],
                                  (S, S), opt.output_vocab_size, dev)

    def step(masks, fuse):
        def run():
            tr.fuse_masks = fuse
            torch.manual_seed(9)
            tr.episode_step(x, img, tgt, 1, lengths, masks=masks)
        return run
    ms = alternate([('unmasked', step(None, True)), ('MaskTable, two launches per step', step(table, False)),
                    ('MaskTable, fused', step(table, True))], reps)
    report('Trainer.episode_step (eager, %d decoder steps), B = %d at %d x %d, ms:' % (opt.decoder_max_len, B, S, S), ms, 1, 'ms', lines)
    tr.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--step_batch', type=int, default=64)
    ap.add_argument('--step_size', type=int, default=128)
    ap.add_argument('--step_reps', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'apply_planes.txt'))
    args = ap.parse_args(argv)
    dev = torch.device('cuda', torch.cuda.current_device())
    lines = ['%s, torch %s, %d alternating rounds (%d for the train step)' % (torch.cuda.get_device_name(dev), torch.__version__, args.reps,
                                                                               args.step_reps)]
    for S in (128, 256):
        operator_step(S, args.batch, args.reps, lines, dev)
    episode_step(args.step_size, args.step_batch, args.step_reps, lines, dev)
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
