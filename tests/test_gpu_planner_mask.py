"""The planner under local-edit masks, on the GPU: the two masked kernels (t2o_op_candidates_multi_l1_masked,
t2o_fit_multi_l1_adam_masked) against the fp64 oracle and against the unmasked kernels, the beam search that uses a pair's
planes, and plan_cli --dataset GIER --local end to end.  Mask values are uint8 COUNTS (0, 1, 2), m = float(byte)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import cpu_ref, synth
from tests import planner_mask_cases as PM

pytestmark = pytest.mark.gpu
OPT = cpu_ref.default_opt()
NAMES = ['brightness', 'contrast', 'saturation', 'color', 'inpaint', 'tone', 'sharpness', 'white']
FIVEK_OPS = [0, 1, 2, 3, 5, 6]
GIER_OPS = [0, 1, 2, 3, 5, 6, 7]
SWEEP_OPS = [0, 1, 2, 3, 5, 7]
PLANE = {n: k for k, n in enumerate(PM.PLANES)}                           # zeros 0, ones 1, blob 2, twos 3


@pytest.fixture(scope='module')
def executor():
    import t2onet_amd
    return t2onet_amd.Executor(t2onet_amd.default_options()).to('cuda:0')


def _record(tag, lines):
    print('## ' + tag)
    for line in lines:
        print(line)


def _planes(H, W):
    host = PM.planes(H, W)
    return host, torch.from_numpy(host).cuda()


def _m64(host, k, H, W):
    return None if k < 0 else torch.from_numpy(host[k].astype(np.float64)).view(1, 1, H, W)


def _start(ops):
    p = torch.zeros(len(ops), 24)
    for k, op in enumerate(ops):
        if op in (3, 5):
            p[k, :cpu_ref.OP_NPARAM[op]] = 1.0
    return p


def _sweep_params(ops, C, seed):
    rows = []
    for k, op in enumerate(ops):
        p = torch.zeros(C, 1) if op == 7 else synth.op_params(op, C, seed + k, 'mid')
        rows.append(torch.cat([p, torch.zeros(C, 24 - p.shape[1])], 1))
    return torch.stack(rows)


# ------------------------------------------------------------------ 1. the sweep against the oracle
@pytest.mark.parametrize('shape', PM.SHAPES)
def test_masked_sweep_matches_oracle(shape):
    """Operators 0, 1, 2, 3, 5, 7 x {no mask, all 0, all 1, blob, 2s} in ONE launch per shape (30 jobs x 9 candidates: two
    candidate groups, the second partial; at 37 x 53 plane 1 starts at an odd byte and the last workgroup is partial):
    loss[j, c] against l1_loss(operator_apply(op, img, p, mask, OPT), target) in fp64.  Bound: rtol 1e-5, atol 1e-6, the
    one of test_gpu_planner.py::test_candidate_sweep_matches_oracle for the unmasked kernel."""
    import t2onet_amd.functional as T
    H, W = shape
    imgs = synth.images(2, H, W, 11)
    tgt = synth.images(1, H, W, 12)
    host, planes = _planes(H, W)
    C = 9
    jobs = [(k % 2, op, mk) for k, op in enumerate(SWEEP_OPS) for mk in (-1, 0, 1, 2, 3)]
    params = _sweep_params([j[1] for j in jobs], C, 300)
    got = T.candidates_multi_l1([j[1] for j in jobs], [j[0] for j in jobs], imgs.cuda(), tgt.cuda(), params.cuda(), masks=planes,
                                mask_index=[j[2] for j in jobs]).cpu().numpy()
    ref = np.zeros((len(jobs), C))
    for k, (i, op, mk) in enumerate(jobs):
        n = cpu_ref.OP_NPARAM[op]
        for c in range(C):
            out = cpu_ref.operator_apply(op, imgs[i:i + 1].double(), params[k, c:c + 1, :n].double(), _m64(host, mk, H, W), OPT)
            ref[k, c] = cpu_ref.l1_loss(out, tgt.double()).item()
    worst = np.abs(got - ref).max()
    print('masked sweep %dx%d: max |loss - fp64| = %.3e over %d jobs x %d candidates' % (H, W, worst, len(jobs), C))
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ 2. neutral masks are exact
@pytest.mark.parametrize('shape', PM.SHAPES)
def test_neutral_masks_are_exact(shape):
    """Jobs with mask_index -1, and jobs under the all-ones plane (z 1 + x 0 = z for finite fp32), through the masked entry
    points equal the unmasked entry points bit for bit -- sweep losses, fit parameters and dist -- both when the whole call
    is neutral and when a blob job in the same launch makes the masked instantiation run."""
    import t2onet_amd.functional as T
    H, W = shape
    imgs = synth.images(2, H, W, 21).cuda()
    tgts = synth.images(2, H, W, 22).cuda()
    _, planes = _planes(H, W)
    C = 9
    ops = SWEEP_OPS
    idx = [k % 2 for k in range(len(ops))]
    params = _sweep_params(ops, C, 320).cuda()
    plain = T.candidates_multi_l1(ops, idx, imgs, tgts[0], params)
    for index in ([-1] * 6, [PLANE['ones']] * 6, [-1, PLANE['ones']] * 3):
        assert torch.equal(T.candidates_multi_l1(ops, idx, imgs, tgts[0], params, masks=planes, mask_index=index), plain), index
    assert torch.equal(T.candidates_multi_l1(ops, idx, imgs, tgts[0], params, mask_index=[-1] * 6), plain)      # no planes at all
    mixed = T.candidates_multi_l1(ops + [0], idx + [0], imgs, tgts[0], torch.cat([params, params[:1]]), masks=planes,
                                  mask_index=[-1, PLANE['ones']] * 3 + [PLANE['blob']])
    assert torch.equal(mixed[:6], plain)
    if H * W > 1:
        assert not torch.equal(mixed[6], plain[0])                          # the blob did something
    fops = [3, 5, 6, 0, 1, 2]
    start = _start(fops).cuda()
    kw = dict(steps=30, lr=2e-2, check_every=10, tol=1e-6)
    p0, d0 = T.fit_multi_l1(fops, idx, imgs, tgts, [1, 0] * 3, start, **kw)
    for index in ([-1] * 6, [PLANE['ones']] * 6, [PLANE['ones'], -1] * 3):
        p, d = T.fit_multi_l1(fops, idx, imgs, tgts, [1, 0] * 3, start, masks=planes, mask_index=index, **kw)
        assert torch.equal(p, p0) and torch.equal(d, d0), index
    p, d = T.fit_multi_l1(fops + [3], idx + [0], imgs, tgts, [1, 0] * 3 + [1], torch.cat([start, start[:1]]), masks=planes,
                          mask_index=[-1, PLANE['ones']] * 3 + [PLANE['blob']], **kw)
    assert torch.equal(p[:6], p0) and torch.equal(d[:6], d0)
    if H * W > 1:
        assert not torch.equal(p[6], p0[0])


# ------------------------------------------------------------------ 3. the all-zero plane
@pytest.mark.parametrize('shape', PM.SHAPES)
def test_all_zero_plane(shape, executor):
    """Under an all-zero plane the gradient is exactly zero and Adam's step is 0 / (0 + eps): the fit returns its start
    parameters bit for bit and dist = l1_loss(clamp(img), target) to 1e-6; the sweep's loss is one number for every
    candidate."""
    import t2onet_amd.functional as T
    from t2onet_amd import planner
    H, W = shape
    imgs = synth.images(2, H, W, 31).cuda()
    tgts = synth.images(2, H, W, 32).cuda()
    _, planes = _planes(H, W)
    fops = [3, 5, 6, 0, 1, 2]
    idx = [k % 2 for k in range(6)]
    start = _start(fops)
    start[3:, 0] = torch.tensor([0.3, -0.2, 0.1])                           # (start values other than the defaults, too)
    start = start.cuda()
    p, d = T.fit_multi_l1(fops, idx, imgs, tgts, [1, 0] * 3, start, steps=20, lr=2e-2, check_every=0, masks=planes,
                          mask_index=[PLANE['zeros']] * 6)
    assert torch.equal(p, start)
    for k in range(6):
        want = planner.get_dist(imgs[idx[k]:idx[k] + 1].clamp(0, 1), tgts[[1, 0][k % 2]][None]).item()
        assert abs(float(d[k]) - want) < 1e-6, (k, float(d[k]), want)
    C = 9
    loss = T.candidates_multi_l1(SWEEP_OPS, idx, imgs, tgts[0], _sweep_params(SWEEP_OPS, C, 340).cuda(), masks=planes,
                                 mask_index=[PLANE['zeros']] * 6)
    assert bool((loss == loss[:, :1]).all())
    for k in range(6):
        assert abs(float(loss[k, 0]) - planner.get_dist(imgs[idx[k]:idx[k] + 1], tgts[0:1]).item()) < 1e-6


# ------------------------------------------------------------------ 4. fit arithmetic
def _adam_fp64(op, img, tgt, p0, mask, steps, lr):
    p = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr)
    img, tgt = img.double(), tgt.double()
    for _ in range(steps):
        opt.zero_grad()
        cpu_ref.l1_loss(cpu_ref.operator_apply(op, img, p, mask, OPT), tgt).backward()
        opt.step()
    return p.detach()


def _adam_serial_fp32(executor, op, img, tgt, p0, mask, steps, lr):
    """The serial fp32 solve: Executor.execute under the plane through autograd + torch.optim.Adam, same start / lr / betas."""
    from t2onet_amd import planner
    p = p0.clone().cuda().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        out, _ = executor.execute(img, op, mask, specified_param=p)
        planner.get_dist(out, tgt).backward()
        opt.step()
    return p.detach()


@pytest.mark.parametrize('shape', [(37, 53), (64, 64)])
def test_masked_fixed_step_arithmetic_against_fp64_adam(executor, shape):
    """The construction of test_gpu_planner_fit.py::test_fixed_step_arithmetic_against_fp64_adam under masks: K = 20 Adam
    iterations, stop rule off, operators 3 / 5 / 6 and brightness on two images x two targets x the blob and the 2s plane:
    the returned parameters against torch.optim.Adam in fp64 on the oracle's MASKED operator.  Bound: the distance (max
    |p - p64| over all jobs) from that fp64 run of a serial fp32 solve built here (Executor.execute(img, op, mask,
    specified_param=p) under autograd + torch.optim.Adam), times 2: the two fp32 solves differ in summation order only.
    dist against get_dist(execute(... masked ...), target): 1e-6.  Both distances are printed (run with -s)."""
    import t2onet_amd.functional as T
    from t2onet_amd import planner
    H, W = shape
    K, lr = 20, 2e-2
    imgs, tgts = synth.images(2, H, W, 71), synth.images(2, H, W, 72)
    host, planes = _planes(H, W)
    B, S = PLANE['blob'], PLANE['twos']
    jobs = [(0, 0, 3, B), (1, 1, 3, S), (0, 1, 5, S), (1, 0, 5, B), (0, 0, 6, S), (1, 1, 6, B), (1, 0, 3, S), (0, 1, 6, B),
            (0, 1, 0, B), (1, 0, 0, S), (1, 1, 5, S), (0, 0, 0, S)]          # (image, target, operator, plane)
    ops = [j[2] for j in jobs]
    start = _start(ops)
    got, dist = T.fit_multi_l1(ops, [j[0] for j in jobs], imgs.cuda(), tgts.cuda(), [j[1] for j in jobs], start.cuda(), steps=K, lr=lr,
                               check_every=0, masks=planes, mask_index=[j[3] for j in jobs])
    got, dist = got.cpu(), dist.cpu()
    d_batched = d_serial = 0.0
    for k, (i, t, op, mk) in enumerate(jobs):
        n = cpu_ref.OP_NPARAM[op]
        assert n == 24 or float(got[k, n:].abs().max()) == 0.0              # the padding stays zero
        maskf = planes[mk].float().view(1, 1, H, W)
        ref = _adam_fp64(op, imgs[i:i + 1], tgts[t:t + 1], start[k:k + 1, :n], _m64(host, mk, H, W), K, lr)
        serial = _adam_serial_fp32(executor, op, imgs[i:i + 1].cuda(), tgts[t:t + 1].cuda(), start[k:k + 1, :n], maskf, K, lr)
        d_batched = max(d_batched, float((got[k:k + 1, :n].double() - ref).abs().max()))
        d_serial = max(d_serial, float((serial.cpu().double() - ref).abs().max()))
        assert float((ref - start[k:k + 1, :n].double()).abs().max()) > 0.05   # K steps of lr 2e-2 moved the parameters
        out = planner.execute(imgs[i:i + 1].cuda(), op, got[k:k + 1, :n].cuda(), executor, maskf)
        want = planner.get_dist(out, tgts[t:t + 1].cuda()).item()
        assert abs(float(dist[k]) - want) < 1e-6, (k, float(dist[k]), want)
    _record('masked fixed-step arithmetic %dx%d' % (H, W),
            ['K=%d lr=%g, %d jobs (operators 3, 5, 6, 0; 2 images x 2 targets x blob / 2s plane), max |p - p_fp64| over all jobs:' % (K, lr, len(jobs)),
             '  batched solve (t2o_fit_multi_l1_adam_masked)   %.3e' % d_batched,
             '  serial fp32 solve (execute + autograd + Adam)  %.3e' % d_serial,
             '  bound = 2 x serial                             %.3e' % (2 * d_serial)])
    assert d_batched <= 2 * d_serial, (d_batched, d_serial)


# ------------------------------------------------------------------ 5. job independence
def _jobs64():
    ops = [3, 5, 6, 0, 1, 2]
    return [(k % 3, (k // 3) % 2, ops[(k + k // 6) % 6], (k % 5) - 1) for k in range(64)]     # plane -1, 0, 1, 2, 3 in turn


@pytest.mark.parametrize('shape', [(37, 53), (64, 64)])
def test_a_masked_job_does_not_depend_on_its_neighbours(shape):
    """Stop rule live, planes mixed (none, 0s, 1s, blob, 2s): every job fitted alone == inside a 9-job launch == inside a
    64-job launch, bit for bit, parameters and dist; two runs of one launch are bit-identical."""
    import t2onet_amd.functional as T
    H, W = shape
    imgs = synth.images(3, H, W, 81).cuda()
    tgts = synth.images(2, H, W, 82).cuda()
    _, planes = _planes(H, W)
    jobs = _jobs64()
    start = _start([j[2] for j in jobs]).cuda()
    kw = dict(steps=30, lr=2e-2, check_every=10, tol=1e-6)

    def run(sel):
        return T.fit_multi_l1([jobs[k][2] for k in sel], [jobs[k][0] for k in sel], imgs, tgts, [jobs[k][1] for k in sel], start[sel],
                              masks=planes, mask_index=[jobs[k][3] for k in sel], **kw)
    p64, d64 = run(list(range(64)))
    again_p, again_d = run(list(range(64)))
    assert torch.equal(p64, again_p) and torch.equal(d64, again_d)
    nine = list(range(20, 29))
    p9, d9 = run(nine)
    assert torch.equal(p9, p64[nine]) and torch.equal(d9, d64[nine])
    for k in ([0, 5, 21, 22, 23, 24, 40, 63] if shape == (64, 64) else range(64)):
        p1, d1 = run([k])
        assert torch.equal(p1[0], p64[k]) and torch.equal(d1[0], d64[k]), (k, jobs[k])
    moved = [k for k in range(64) if jobs[k][3] != PLANE['zeros']]
    assert float((p64[moved] - start[moved]).abs().max()) > 0.1


# ------------------------------------------------------------------ 6. the search uses the mask
def _local_pair():
    H = W = 64
    img = synth.images(1, H, W, 131)
    plane = PM.plane('blob', H, W)
    m = torch.from_numpy(plane.astype(np.float32)).view(1, 1, H, W)
    tgt = cpu_ref.operator_apply(0, img, torch.tensor([[0.4]]), m, OPT)
    return img.cuda(), tgt.cuda(), torch.from_numpy(plane).cuda()


def _replay(executor, img, actions, planes):
    from t2onet_amd import planner
    dists, I = [], img
    for name, params, _ in actions:
        op = NAMES.index(name)
        plane = planes.get(op)
        mask = None if plane is None else plane.float().view(1, 1, *plane.shape)
        I = planner.execute(I, op, torch.tensor([params], device=img.device), executor, mask)
        dists.append(I)
    return dists


def test_the_search_uses_the_mask(executor):
    """A 64 x 64 pair whose target is the oracle's brightness at +0.4 under the blob (33.5 % of the pixels) only.  Oracle,
    fp64, on these very images, brightness swept over [-2, 2] in steps of 1e-3: under the blob the best distance is 0.0 (at
    +0.4); as a global edit it is 3.597e-2, at 0.0 -- the initial distance, a global brightness cannot help at all.
    So: the masked search's first step takes brightness under the mask with dist < err = 1e-2 and stops there; the search
    without masks on the same pair ends at a distance at least 5 x larger.  Replaying every returned (name, params) through
    Executor.execute under the planes reproduces every recorded dist to 1e-6."""
    from t2onet_amd import planner
    img, tgt, plane = _local_pair()
    err = 1e-2
    args = (None, executor, None, 3, GIER_OPS, NAMES, len(GIER_OPS), err, 'L1')
    (local, I_local), = planner.beam_search_pairs([img], [tgt], *args, masks=[{0: plane}])
    best = local[0]
    assert len(best) == 1 and best[0][0] == 'brightness' and best[0][2] < err, best
    assert abs(best[0][1][0] - 0.4) < 2e-3
    (glob, I_glob), = planner.beam_search_pairs([img], [tgt], *args)
    print('masked search: %s dist %.3e;  global search: %s dist %.3e' % ([a[0] for a in best], best[-1][2], [a[0] for a in glob[0]], glob[0][-1][2]))
    assert glob[0][-1][2] >= 5 * best[-1][2] and glob[0][-1][2] > err
    assert all(a[0] != 'white' for seq in glob for a in seq)                 # white is a candidate only under a plane
    for actions, Is, planes in ((local, I_local, {0: plane}), (glob, I_glob, {})):
        for seq, imgs in zip(actions, Is):
            outs = _replay(executor, img, seq, planes)
            for (name, params, dist), out, rec in zip(seq, outs, imgs):
                assert abs(planner.get_dist(out, tgt).item() - dist) < 1e-6, (name, dist)
                assert torch.equal(out, rec)
    single, _ = planner.beam_search(img, tgt, *args, 'batched', masks={0: plane})
    assert single == local
    with pytest.raises(NotImplementedError):
        planner.beam_search(img, tgt, *args, 'sweep', masks={0: plane})
    with pytest.raises(ValueError):
        planner.beam_search_pairs([img], [tgt], *args, masks=[{0: plane.float()}])


def test_white_and_shared_planes_in_the_search(executor):
    """A pair that annotates ONE plane for brightness, tone and white (stored once in the launch tensor) and whose target
    is white under the 2s plane: `white` rides in the sweep launch, wins the first step with the parameter list [0.0], and
    its replay under the plane gives the recorded distance."""
    from t2onet_amd import planner
    H = W = 64
    img = synth.images(1, H, W, 141)
    host = PM.plane('twos', H, W)
    m = torch.from_numpy(host.astype(np.float32)).view(1, 1, H, W)
    tgt = cpu_ref.operator_apply(7, img, torch.zeros(1, 1), m, OPT).cuda()
    img, plane = img.cuda(), torch.from_numpy(host).cuda()
    masks = {0: plane, 5: plane, 7: plane}
    beam = planner._Beam(img, tgt, 3, GIER_OPS, NAMES, 1e-2, False, masks)
    stacked, plane_of = planner._gather_planes([beam])
    assert stacked.shape == (1, H, W) and plane_of == [{0: 0, 5: 0, 7: 0}]
    (actions, Is), = planner.beam_search_pairs([img], [tgt], None, executor, None, 3, GIER_OPS, NAMES, len(GIER_OPS), 1e-2, 'L1', masks=[masks])
    assert actions[0][0][0] == 'white' and actions[0][0][1] == [0.0] and actions[0][0][2] < 1e-6 and len(actions[0]) == 1
    out = _replay(executor, img, actions[0], masks)[0]
    assert torch.equal(out, Is[0][0]) and abs(planner.get_dist(out, tgt).item() - actions[0][0][2]) < 1e-6


# ------------------------------------------------------------------ 7. nothing else moved
def _two_pairs(executor, size=64):
    from t2onet_amd import planner
    dev = 'cuda:0'
    chains = [[(0, synth.uniform((1, 1), 101, 0.2, 0.3)), (1, synth.uniform((1, 1), 102, 0.2, 0.3))],
              [(5, synth.op_params(5, 1, 103, 'mid')), (2, synth.uniform((1, 1), 104, 0.2, 0.3))]]
    inputs, targets = [], []
    for c, chain in enumerate(chains):
        img = synth.images(1, size, size, 110 + c).to(dev)
        x = img
        for op, p in chain:
            x = planner.execute(x, op, p.to(dev), executor)
        inputs.append(img)
        targets.append(x)
    return inputs, targets


def test_no_masks_is_todays_search(executor):
    """beam_search_pairs(..., masks=None), masks=[None] * P and masks=[{}] * P: identical actions, torch.equal images."""
    from t2onet_amd import planner
    inputs, targets = _two_pairs(executor)
    args = (None, executor, None, 3, FIVEK_OPS, NAMES, 3, 1e-2, 'L1')
    base = planner.beam_search_pairs(inputs, targets, *args)
    for masks in (None, [None, None], [{}, {}]):
        again = planner.beam_search_pairs(inputs, targets, *args, masks=masks)
        for (a0, I0), (a1, I1) in zip(base, again):
            assert a1 == a0
            assert all(torch.equal(x, y) for s, t in zip(I0, I1) for x, y in zip(s, t))


def _kernels(prof):
    from torch.autograd import DeviceType
    evs = [e for e in prof.key_averages() if e.device_type == DeviceType.CUDA]
    return [(e.key, e.count) for e in evs if not e.key.startswith(('Memcpy', 'Memset'))]


def _one_step(executor, img, tgt, masks):
    """One 'batched' beam step profiled as test_gpu_planner_fit.py::test_launch_structure does -> (planner kernel
    launches by family, host synchronisations)."""
    from t2onet_amd import planner
    from torch.profiler import profile, ProfilerActivity

    def step():
        return planner.beam_search(img, tgt, None, executor, None, 3, FIVEK_OPS, NAMES, 1, 1e-2, 'L1', 'batched', masks=masks)
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    ks = _kernels(prof)
    fam = {f: sum(c for k, c in ks if f in k) for f in ('k_fit_eval', 'k_fit_adam', 'k_fit_dist', 'k_fit_init', 'k_candidates_multi_l1',
                                                        'k_candidates_finalize')}
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        try:
            torch.cuda.set_sync_debug_mode('warn')
            step()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    # (every synchronising call warns "called a synchronizing CUDA operation"; the one-per-process notice that the debug
    # mode is a prototype is not one of them)
    syncs = sum('called a synchronizing' in str(w.message) for w in caught)
    return fam, syncs, ks


def test_masked_step_has_the_launch_structure_of_the_unmasked_one(executor):
    """A masked beam step issues exactly the planner launches of the unmasked one (3 sweep rounds, 2 x 300 + 3 fit kernels)
    and performs the same number of host synchronisations: one for the sweep fits, one for the Adam fits, the rest the
    per-candidate parameter reads of _Beam.advance, the same in both."""
    H = W = 64
    img = synth.images(1, H, W, 123).cuda()
    tgt = synth.images(1, H, W, 124).cuda()
    _, planes = _planes(H, W)
    fam0, syncs0, ks0 = _one_step(executor, img, tgt, None)
    fam1, syncs1, ks1 = _one_step(executor, img, tgt, {0: planes[PLANE['blob']], 3: planes[PLANE['twos']], 6: planes[PLANE['blob']]})
    print('unmasked step: %s, %d syncs;  masked step: %s, %d syncs' % (fam0, syncs0, fam1, syncs1))
    assert fam1 == fam0 and fam0['k_fit_eval'] == 301 and fam0['k_fit_adam'] == 300 and fam0['k_candidates_multi_l1'] == 3
    assert syncs1 == syncs0 and syncs0 >= 2
    assert {k for k, _ in ks1 if 'k_fit_eval' in k} != {k for k, _ in ks0 if 'k_fit_eval' in k}, ks1      # the masked instantiation ran
    optimiser = [k for k, _ in ks1 if 'k_fit_' not in k and any(w in k.lower() for w in ('adam', 'multi_tensor', 'foreach', 'lerp', 'addcdiv', 'addcmul'))]
    assert not optimiser, optimiser


# ------------------------------------------------------------------ python-side validation
def test_wrong_planes_are_python_errors():
    import t2onet_amd.functional as T
    H, W = 37, 53
    imgs, tgt = synth.images(1, H, W, 151).cuda(), synth.images(1, H, W, 152).cuda()
    _, planes = _planes(H, W)
    params = _sweep_params([0], 3, 360).cuda()
    start = _start([3]).cuda()
    for masks, index in ((planes, [4]), (planes, [-2]), (None, [0]), (planes.float(), [0]), (planes.cpu(), [0]), (planes[:, :, :50], [0]),
                         (planes[:, :36], [0]), (planes[0], [0]), (planes, [0, 1])):
        with pytest.raises(ValueError):
            T.candidates_multi_l1([0], [0], imgs, tgt, params, masks=masks, mask_index=index)
        with pytest.raises(ValueError):
            T.fit_multi_l1([3], [0], imgs, tgt, [0], start, steps=1, masks=masks, mask_index=index)


# ------------------------------------------------------------------ 8. end to end
def test_gier_generator_output_trains(tmp_path):
    """plan_cli --dataset GIER --local --img_size 64 --pairs_per_batch 4 over the synthetic GIER tree (--data_mode at its
    default, 'global', as the reference: the tree's odd records): a record for every pair of the index, none on a second
    run, GIERDatasetAct loads every item, and train_cli --dataset GIER --act_dir <that> runs two iterations to a checkpoint."""
    from t2onet_amd import gier, plan_cli, train_cli
    from tests import gier_tree
    data_dir, vocab_dir, _, glove = gier_tree.write_tree(str(tmp_path / 'tree'))
    save_dir = str(tmp_path / 'GIER_actions_set_1')
    argv = ['--dataset', 'GIER', '--local', '--img_size', '64', '--pairs_per_batch', '4', '--data_dir', data_dir, '--vocab_dir', vocab_dir,
            '--save_dir', save_dir]
    index = gier.GIER(data_dir, vocab_dir, 'train', 'global', False, 3, 64)
    names = sorted(d['input'].split('_')[0] for d in index.op_data)
    assert plan_cli.main(argv) == len(names) == 4
    assert sorted(os.listdir(save_dir)) == names
    assert plan_cli.main(argv) == 0
    for i, d in enumerate(index.op_data):
        with open(plan_cli.gier_record_path(save_dir, d['input'].split('_')[0])) as f:
            rec = json.load(f)
        assert rec['local operators'] == ['brightness', 'tone'] and rec['request'] == d['expert_summary'] + d['amateur_summary']
        seq = rec['operation sequence'][0]
        assert 1 <= len(seq) <= 7 and seq[-1][2] < rec['init distance']
        assert all(os.path.exists(os.path.join(save_dir, d['input'].split('_')[0], 'edit%d.jpg' % k)) for k in range(len(seq)))
    ds = gier.GIERDatasetAct(data_dir, vocab_dir, save_dir, 'train', 'global', False, 3, 64)
    assert len(ds) == 4
    for item in range(len(ds)):
        d = ds[item]
        n = int((d['operations'] > 2).sum())
        assert 1 <= n <= 7 and set(d['operations'][1:1 + n].tolist()) <= {o + 3 for o in GIER_OPS} and d['operations'][n + 1] == 2
        assert d['output'].shape == (9, 3, 64, 64) and np.isfinite(d['parameters']).all()
    avg = train_cli.main(['--dataset', 'GIER', '--data_dir', data_dir, '--vocab_dir', vocab_dir, '--act_dir', save_dir, '--data_mode', 'global',
                          '--word2vec', glove, '--batch_size', '4', '--img_size', '64', '--num_iters', '2', '--print_every', '2',
                          '--checkpoint_every', '2', '--run_dir', str(tmp_path / 'run'), '--num_workers', '0'])
    assert avg['stats']['train_iter'] == [2]
    assert os.path.exists(str(tmp_path / 'run' / 'seq2seqL1_model' / 'checkpoint_best' / 'model.pth'))
