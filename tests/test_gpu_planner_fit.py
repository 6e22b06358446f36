"""The batched, device-resident planner fits (t2o_fit_multi_l1_adam), the 'batched' beam search built on them, the
lock-step search over several pairs and the action-set generator, on the GPU."""
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref, synth

pytestmark = pytest.mark.gpu
OPT = cpu_ref.default_opt()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['brightness', 'contrast', 'saturation', 'color', 'inpaint', 'tone', 'sharpness', 'white']
FIVEK_OPS = [0, 1, 2, 3, 5, 6]


@pytest.fixture(scope='module')
def executor():
    import t2onet_amd
    return t2onet_amd.Executor(t2onet_amd.default_options()).to('cuda:0')


def _record(tag, lines):
    """The measured figures of a run, printed (pytest -s shows them)."""
    print('## ' + tag)
    for line in lines:
        print(line)


def _start(ops):
    p = torch.zeros(len(ops), 24)
    for k, op in enumerate(ops):
        if op in (3, 5):
            p[k, :cpu_ref.OP_NPARAM[op]] = 1.0
    return p


def _adam_fp64(op, img, tgt, p0, steps, lr):
    """torch.optim.Adam in fp64 on the oracle's operator: the arithmetic the batched solve is held to."""
    p = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr)
    img, tgt = img.double(), tgt.double()
    for _ in range(steps):
        opt.zero_grad()
        cpu_ref.l1_loss(cpu_ref.operator_apply(op, img, p, None, OPT), tgt).backward()
        opt.step()
    return p.detach()


@pytest.mark.parametrize('shape', [(37, 53), (128, 128)])
def test_fixed_step_arithmetic_against_fp64_adam(executor, shape):
    """K = 20 Adam iterations, stop rule off, operators 3 / 5 / 6 on two images and two targets: the returned
    parameters against torch.optim.Adam in fp64 on the oracle's operators (same start, lr, betas).  Bound: the distance
    (max |p - p64| over all jobs) of the serial fp32 path -- executor.value_and_grad + torch.optim.Adam, planner._fit_adam
    -- from the same fp64 run, times 2: the two fp32 solves differ in summation order only.  `dist` against
    get_dist(execute(img, op, p), target): 1e-6, the bound of test_multi_job_sweep_equals_single_job_launches.

    Both distances are printed by the test (run it with -s)."""
    import t2onet_amd.functional as T
    from t2onet_amd import planner
    H, W = shape
    K, lr = 20, 2e-2
    imgs = synth.images(2, H, W, 71)
    tgts = synth.images(2, H, W, 72)
    jobs = [(0, 0, 3), (1, 1, 3), (0, 1, 5), (1, 0, 5), (0, 0, 6), (1, 1, 6), (1, 0, 3), (0, 1, 6)]     # (image, target, operator)
    ops = [j[2] for j in jobs]
    start = _start(ops)
    got, dist = T.fit_multi_l1(ops, [j[0] for j in jobs], imgs.cuda(), tgts.cuda(), [j[1] for j in jobs], start.cuda(),
                               steps=K, lr=lr, check_every=0)
    got, dist = got.cpu(), dist.cpu()
    d_batched = d_serial = 0.0
    for k, (i, t, op) in enumerate(jobs):
        n = cpu_ref.OP_NPARAM[op]
        assert float(got[k, n:].abs().max()) == 0.0 if n < 24 else True               # the padding stays zero
        ref = _adam_fp64(op, imgs[i:i + 1], tgts[t:t + 1], start[k:k + 1, :n], K, lr)
        serial, _ = planner._fit_adam(imgs[i:i + 1].cuda(), tgts[t:t + 1].cuda(), op, executor, start[k:k + 1, :n], steps=K, lr=lr,
                                      check_every=10 ** 9)
        d_batched = max(d_batched, float((got[k:k + 1, :n].double() - ref).abs().max()))
        d_serial = max(d_serial, float((serial.cpu().double() - ref).abs().max()))
        assert float((ref - start[k:k + 1, :n].double()).abs().max()) > 0.05           # K steps of lr 2e-2 moved the parameters
        out = planner.execute(imgs[i:i + 1].cuda(), op, got[k:k + 1, :n].cuda(), executor)
        want = planner.get_dist(out, tgts[t:t + 1].cuda()).item()
        assert abs(float(dist[k]) - want) < 1e-6, (k, float(dist[k]), want)
    _record('fixed-step arithmetic %dx%d' % (H, W),
            ['K=%d lr=%g, %d jobs (operators 3, 5, 6; 2 images x 2 targets), max |p - p_fp64| over all jobs:' % (K, lr, len(jobs)),
             '  batched solve (t2o_fit_multi_l1_adam)      %.3e' % d_batched,
             '  serial fp32 path (planner._fit_adam)       %.3e' % d_serial,
             '  bound = 2 x serial                         %.3e' % (2 * d_serial)])
    assert d_batched <= 2 * d_serial, (d_batched, d_serial)


def _jobs64():
    ops = [3, 5, 6, 0, 1, 2]
    return [(k % 3, (k // 3) % 2, ops[(k + k // 6) % 6]) for k in range(64)]


@pytest.mark.parametrize('shape', [(37, 53), (128, 128)])
def test_a_job_does_not_depend_on_its_neighbours(shape):
    """Every job fitted alone == the same job inside a 9-job launch == inside a 64-job launch, bit for bit, parameters
    and dist (with the stop rule live); and two runs of one launch are bit-identical."""
    import t2onet_amd.functional as T
    H, W = shape
    imgs = synth.images(3, H, W, 81).cuda()
    tgts = synth.images(2, H, W, 82).cuda()
    jobs = _jobs64()
    start = _start([j[2] for j in jobs]).cuda()
    kw = dict(steps=30, lr=2e-2, check_every=10, tol=1e-6)

    def run(sel):
        return T.fit_multi_l1([jobs[k][2] for k in sel], [jobs[k][0] for k in sel], imgs, tgts, [jobs[k][1] for k in sel],
                              start[sel], **kw)
    p64, d64 = run(list(range(64)))
    again_p, again_d = run(list(range(64)))
    assert torch.equal(p64, again_p) and torch.equal(d64, again_d)
    nine = list(range(20, 29))
    p9, d9 = run(nine)
    assert torch.equal(p9, p64[nine]) and torch.equal(d9, d64[nine])
    for k in ([0, 5, 21, 22, 23, 40, 63] if shape == (128, 128) else range(64)):
        p1, d1 = run([k])
        assert torch.equal(p1[0], p64[k]) and torch.equal(d1[0], d64[k]), (k, jobs[k])
    assert float((p64 - start).abs().max()) > 0.1


def test_stop_rule_freezes_per_job(executor):
    """The serial fit's rule on the device, per job: the first check records the loss, a later check freezes the job if
    the loss fell by less than tol since the previous one.  (a) a job that starts at its optimum (target = the operator at
    the start parameters) is frozen at iteration 2 check_every -- its parameters are those of a steps = 2 check_every run
    -- while a far-off job in the same launch keeps moving; (b) with tol above any possible improvement EVERY job stops
    at 2 check_every, not at check_every and not later; with a negative tol none does."""
    import t2onet_amd.functional as T
    from t2onet_amd import planner
    H, W, ce = 37, 53, 10
    imgs = synth.images(2, H, W, 91).cuda()
    far = synth.images(1, H, W, 92).cuda()
    ops = [5, 5, 3, 3, 6]
    start = _start(ops).cuda()
    at_opt = planner.execute(imgs[0:1], 5, start[0:1, :8], executor)
    tgts = torch.cat([at_opt, far])
    img_index, tgt_index = [0, 1, 1, 0, 1], [0, 1, 1, 1, 1]

    def run(steps, check_every, tol=1e-6):
        return T.fit_multi_l1(ops, img_index, imgs, tgts, tgt_index, start, steps=steps, lr=2e-2, check_every=check_every, tol=tol)
    free = {s: run(s, 0)[0] for s in (ce, 2 * ce, 3 * ce, 4 * ce)}
    p, d = run(4 * ce, ce)
    assert torch.equal(p[0], free[2 * ce][0]) and float(d[0]) < 1e-6
    for k in (1, 2, 3):                                                    # curves far from a noise target: still improving, never frozen
        assert torch.equal(p[k], free[4 * ce][k]) and not torch.equal(p[k], free[2 * ce][k])
    p_all, _ = run(4 * ce, ce, tol=10.0)
    for k in (1, 2, 3, 4):
        assert torch.equal(p_all[k], free[2 * ce][k])
        assert not torch.equal(p_all[k], free[ce][k]) and not torch.equal(p_all[k], free[3 * ce][k])
    p_none, _ = run(4 * ce, ce, tol=-10.0)
    assert torch.equal(p_none, free[4 * ce])


def _chain_targets(executor, size=128):
    from t2onet_amd import planner
    dev = 'cuda:0'
    chains = [[(0, synth.uniform((1, 1), 101, 0.2, 0.3)), (1, synth.uniform((1, 1), 102, 0.2, 0.3))],
              [(5, synth.op_params(5, 1, 103, 'mid')), (2, synth.uniform((1, 1), 104, 0.2, 0.3))],
              [(3, synth.op_params(3, 1, 105, 'mid')), (6, synth.uniform((1, 1), 106, 0.2, 0.4)), (1, synth.uniform((1, 1), 107, 0.2, 0.3))]]
    inputs, targets = [], []
    for c, chain in enumerate(chains):
        img = synth.images(1, size, size, 110 + c).to(dev)
        x = img
        for op, p in chain:
            x = planner.execute(x, op, p.to(dev), executor)
        inputs.append(img)
        targets.append(x)
    return inputs, targets


def test_batched_search_quality_and_pairs(executor):
    """Targets built from known chains (brightness -> contrast, tone -> saturation, colour -> sharpness -> contrast),
    beam 3 over [0,1,2,3,5,6]: the best final distance of 'batched' may exceed that of 'sweep' by at most 10 % plus 1e-5
    (the two differ in summation order, but an L1 objective has kinks where Adam trajectories can part).
    beam_search_pairs over the three pairs returns, per pair, exactly the single-pair 'batched' actions."""
    from t2onet_amd import planner
    inputs, targets = _chain_targets(executor)
    args = (None, executor, None, 3, FIVEK_OPS, NAMES, 6, 1e-2, 'L1')
    singles, lines, figures = [], [], []
    for c, (img, tgt) in enumerate(zip(inputs, targets)):
        a_sweep, _ = planner.beam_search(img, tgt, *args, 'sweep')
        a_batched, I_batched = planner.beam_search(img, tgt, *args, 'batched')
        singles.append((a_batched, I_batched))
        ds, db = a_sweep[0][-1][2], a_batched[0][-1][2]
        lines.append('chain %d: best distance sweep %.6e (%s)  batched %.6e (%s)  ratio %.4f' % (
            c, ds, '>'.join(a[0] for a in a_sweep[0]), db, '>'.join(a[0] for a in a_batched[0]), db / ds))
        figures.append((ds, db))
        init = planner.get_dist(img, tgt).item()
        assert db < init and len(I_batched[0]) == len(a_batched[0])
        out = I_batched[0][-1]
        assert abs(planner.get_dist(out, tgt).item() - db) < 1e-6
    _record('search quality 128x128', lines)
    for (ds, db), line in zip(figures, lines):
        assert db <= 1.10 * ds + 1e-5, line
    together = planner.beam_search_pairs(inputs, targets, *args)
    assert len(together) == 3
    for (a_one, I_one), (a_all, I_all) in zip(singles, together):
        assert a_all == a_one                                               # names, parameter lists and distances, exactly
        assert all(torch.equal(x, y) for s, t in zip(I_one, I_all) for x, y in zip(s, t))
    with pytest.raises(NotImplementedError):
        planner.beam_search_pairs(inputs, targets, None, executor, None, 3, FIVEK_OPS, NAMES, 6, 1e-2, 'self-disc')


def _kernels(prof):
    from torch.autograd import DeviceType
    evs = [e for e in prof.key_averages() if e.device_type == DeviceType.CUDA]
    return [(e.key, e.count) for e in evs if not e.key.startswith(('Memcpy', 'Memset'))]


def test_launch_structure(executor):
    """One fit of 9 jobs x 300 iterations issues at most 2 x 300 + 8 kernels, every one of them this library's fit
    kernels; a 'batched' beam step runs no framework optimiser kernel."""
    import t2onet_amd.functional as T
    from t2onet_amd import planner
    from torch.profiler import profile, ProfilerActivity
    H = W = 128
    imgs = synth.images(3, H, W, 121).cuda()
    tgts = synth.images(1, H, W, 122).cuda()
    ops = [3, 5, 6] * 3
    idx = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    start = _start(ops).cuda()
    T.fit_multi_l1(ops, idx, imgs, tgts, [0] * 9, start, steps=2)          # (library load, first-launch work)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        T.fit_multi_l1(ops, idx, imgs, tgts, [0] * 9, start, steps=300, check_every=0)
        torch.cuda.synchronize()
    ks = _kernels(prof)
    total = sum(c for _, c in ks)
    print('fit_multi_l1, 9 jobs x 300 steps: %d kernels %s' % (total, ks))
    assert 600 <= total <= 2 * 300 + 8, ks
    assert all('k_fit_' in k for k, _ in ks), ks
    img = synth.images(1, H, W, 123).cuda()
    tgt = synth.images(1, H, W, 124).cuda()
    planner.beam_search(img, tgt, None, executor, None, 3, FIVEK_OPS, NAMES, 1, 1e-2, 'L1', 'batched')
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        planner.beam_search(img, tgt, None, executor, None, 3, FIVEK_OPS, NAMES, 1, 1e-2, 'L1', 'batched')
        torch.cuda.synchronize()
    ks = _kernels(prof)
    print('one batched beam step: %d kernels' % sum(c for _, c in ks))
    assert any('k_fit_adam' in k for k, _ in ks) and any('k_candidates_multi_l1' in k for k, _ in ks), ks
    optimiser = [k for k, _ in ks if 'k_fit_' not in k and any(w in k.lower() for w in ('adam', 'multi_tensor', 'foreach', 'lerp', 'addcdiv', 'addcmul'))]
    assert not optimiser, optimiser
    assert sum(c for k, c in ks if 'k_fit_' in k) <= 2 * 300 + 8


def test_get_param_batched(executor):
    from t2onet_amd import planner
    img = synth.images(1, 64, 64, 31).cuda()
    k_true = torch.tensor([[0.6, 0.8, 1.0, 1.2, 1.4, 1.2, 1.0, 0.8]], device='cuda')
    tgt = planner.execute(img, 5, k_true, executor)
    p, ok = planner.get_param(img, tgt, None, 5, executor, None, 'L1', 'batched')
    assert ok and p.shape == (1, 8)
    assert planner.get_dist(planner.execute(img, 5, p, executor), tgt).item() < 3e-3   # (test_curve_fit_and_beam_search's bound for 'sweep')
    p0, _ = planner.get_param(img, planner.execute(img, 0, torch.tensor([[0.37]], device='cuda'), executor), None, 0, executor, None, 'L1', 'batched')
    assert p0.shape == (1, 1) and abs(p0.item() - 0.37) < 2e-3


def test_generator_output_trains(tmp_path):
    """plan_cli over a FiveK-layout tree (--limit 4), FiveKAct over what it wrote, one supervised and one episode step of
    the trainer on that batch: finite losses.  A second run finds every record in place and plans nothing."""
    import t2onet_amd
    from t2onet_amd import plan_cli, data
    from t2onet_amd.actor import Actor
    from t2onet_amd.train import Trainer
    from tests import fivek_tree
    img_dir, anno_dir, _, _ = fivek_tree.write_tree(str(tmp_path / 'data'), n_train=6, n_val=1)
    save_dir = str(tmp_path / 'actions_set_1')
    argv = ['--img_dir', img_dir, '--anno_dir', anno_dir, '--save_dir', save_dir, '--img_size', '64', '--limit', '4', '--pairs_per_batch', '3']
    assert plan_cli.main(argv) == 4
    assert sorted(os.listdir(save_dir)) == ['train0', 'train1', 'train2', 'train3']
    assert plan_cli.main(argv) == 0
    assert plan_cli.main(argv + ['--start', '3']) == 2 and os.path.exists(plan_cli.record_path(save_dir, 'train', 5))
    ds = data.FiveKAct(img_dir, anno_dir, save_dir, 'train', 1, 64)
    items = [ds[i] for i in range(4)]
    dev = torch.device('cuda:0')
    img_x = torch.stack([it[0] for it in items]).to(dev)
    img_y = torch.stack([it[1] for it in items]).to(dev)
    x = torch.stack([torch.as_tensor(it[2]) for it in items]).to(dev)
    y = torch.stack([torch.as_tensor(it[3]) for it in items]).to(dev)
    gt = torch.stack([torch.as_tensor(it[4]) for it in items]).to(dev)
    for it in items:
        n = int((it[3] > 2).sum())
        assert 1 <= n <= 5 and set(it[3][1:1 + n].tolist()) <= {o + 3 for o in FIVEK_OPS} and it[3][n + 1] == 2
    opt = t2onet_amd.default_options(batch_size=4)
    torch.manual_seed(7)
    model = Actor(opt).to(dev).train()
    tr = Trainer(model, opt, graph_encoder=False)
    lengths = (x != opt.null_id).sum(1).cpu()
    op_loss, param_loss = tr.supervised_step(x, y, img_x, img_y, gt, lengths)
    l1 = tr.episode_step(x, img_x, img_y[:, -1], lengths=lengths)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in (op_loss, param_loss, l1))
