"""Time one planner parameter fit per operator: the reference's procedure (scipy Nelder-Mead, one
executor call + .item() per evaluation -- here already on the HIP kernels) vs the GPU-native
'sweep' optimiser, one full beam search, and the FiveK generator's six-operator search ('sweep' against 'batched',
and beam_search_pairs over 8 pairs): milliseconds, kernel launches, best distance."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import t2onet_amd  # noqa: E402
from t2onet_amd import planner  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 128
ex = t2onet_amd.Executor(t2onet_amd.default_options()).cuda()
g = torch.Generator().manual_seed(3)
img = torch.rand(1, 3, S, S, generator=g).cuda()
truth = {0: torch.tensor([[0.3]]), 1: torch.tensor([[-0.25]]), 2: torch.tensor([[0.4]]),
         5: torch.tensor([[0.7, 0.9, 1.1, 1.3, 1.2, 1.0, 0.9, 0.8]])}
for op, p in truth.items():
    tgt, _ = ex.execute(img, op, None, specified_param=p.cuda())
    for optm in ['Nelder-Mead', 'sweep']:
        planner.get_param(img, tgt, None, op, ex, None, 'L1', optm)          # warm up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q, _ = planner.get_param(img, tgt, None, op, ex, None, 'L1', optm)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out, _ = ex.execute(img, op, None, specified_param=q)
        print('size %d op %d %-12s %8.2f ms  residual L1 %.2e' % (S, op, optm, dt * 1e3, planner.get_dist(out, tgt).item()), flush=True)
mid, _ = ex.execute(img, 0, None, specified_param=torch.tensor([[0.25]]).cuda())
tgt2, _ = ex.execute(mid, 1, None, specified_param=torch.tensor([[0.3]]).cuda())
names = ['brightness', 'contrast', 'saturation', 'color', 'inpaint', 'tone', 'sharpness', 'white']
for optm in ['Nelder-Mead', 'sweep']:
    planner.beam_search(img, tgt2, None, ex, None, 3, [0, 1, 2], names, 3, 1e-3, 'L1', optm)      # warm up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    actions, _ = planner.beam_search(img, tgt2, None, ex, None, 3, [0, 1, 2], names, 3, 1e-3, 'L1', optm)
    torch.cuda.synchronize()
    print('beam search (3 ops, beam 3) %-12s %8.1f ms  best dist %.2e' % (optm, (time.perf_counter() - t0) * 1e3, actions[0][-1][2]))


# ---- the FiveK generator's search: beam 3 over the six operators, max_step 6 (preprocess/gen_greedy_seqs_FiveK.py:38-41):
# 'sweep' (1-parameter sweeps batched, every curve / sharpness fit a serial 300-iteration Adam loop) against 'batched'
# (those fits in one device-resident solve per beam step), and beam_search_pairs over P = 8 pairs in lock-step.
def count_kernels(fn):
    from torch.autograd import DeviceType
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA and not e.key.startswith(('Memcpy', 'Memset')))


def timed(fn, reps):
    fn()                                                                   # warm up
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], out


SIX = [0, 1, 2, 3, 5, 6]
P = 8
ins = [torch.rand(1, 3, S, S, generator=g).cuda() for _ in range(P)]
outs = []
for k, x in enumerate(ins):                                                # colour curve -> sharpness -> contrast, a little different per pair
    curve = (torch.rand(1, 24, generator=g) * 0.6 + 0.7).cuda()
    y, _ = ex.execute(x, 3, None, specified_param=curve)
    y, _ = ex.execute(y, 6, None, specified_param=torch.tensor([[0.2 + 0.02 * k]]).cuda())
    y, _ = ex.execute(y, 1, None, specified_param=torch.tensor([[0.3 - 0.02 * k]]).cuda())
    outs.append(y)
for optm, reps in (('sweep', 3), ('batched', 5)):
    def run(optm=optm):
        return planner.beam_search(ins[0], outs[0], None, ex, None, 3, SIX, names, 6, 1e-2, 'L1', optm)
    ms, (actions, _) = timed(run, reps)
    print('six-operator search %dx%d (beam 3, max_step 6) %-8s %9.1f ms  %6d kernels  best dist %.3e  (%s)' % (
        S, S, optm, ms, count_kernels(run), actions[0][-1][2], '>'.join(a[0] for a in actions[0])), flush=True)


def run_pairs():
    return planner.beam_search_pairs(ins, outs, None, ex, None, 3, SIX, names, 6, 1e-2, 'L1')


ms, res = timed(run_pairs, 3)
print('beam_search_pairs P=%d %dx%d                       %9.1f ms = %.1f ms per pair  %6d kernels  best dists %s' % (
    P, S, S, ms, ms / P, count_kernels(run_pairs), ' '.join('%.2e' % r[0][0][-1][2] for r in res)), flush=True)
