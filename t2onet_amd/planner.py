"""Operation planning on the GPU (utils/beam_search.py:65-264 -- SURVEY.md 8(f) rank 1).

The reference fits one operator's parameter per candidate step with scipy Nelder-Mead at batch 1:
every objective evaluation is an `executor.execute(..., specified_param=...)` plus a `.item()`
host sync (`get_param_naive`, beam_search.py:65-91).  Same surface here (`get_param`, `execute`,
`get_dist`, `beam_search` with the reference's arguments), plus a GPU-native optimiser:

  optimizer='sweep'   1-parameter per-pixel operators: three rounds of a 64-candidate sweep, each round
                      shrinking the bracket around the best candidate.  Inside beam_search every such fit of a
                      step -- all beams x all 1-parameter operations -- runs in ONE launch per round
                      (t2o_op_candidates_multi_l1) with the bracket update on the device: 3 launches and ONE
                      host sync per beam step instead of one per candidate fit;
                      curve operators (8 / 24 parameters) and sharpness: Adam on the fused
                      operator+L1 forward/backward kernels with no per-iteration sync.
  optimizer='batched' the same sweep for the 1-parameter operators; EVERY other candidate of a beam step -- curve
                      operators, sharpness, all beams -- in one device-resident Adam solve (fit_adam_batch ->
                      t2o_fit_multi_l1_adam: two launches per iteration for all jobs together, stop rule on the
                      device): one host sync for the sweep fits and one for the Adam fits per beam step.
                      beam_search_pairs runs that search for several same-size pairs in lock-step, the Adam fits
                      of all pairs sharing launches (what plan_cli generates FiveK action sets with).
  'Nelder-Mead' | 'adam' | 'lbfgs'  the reference's procedures, objective evaluated by the HIP kernels.

Local edits (GIER; preprocess/gen_greedy_seqs_GIER.py:60-65: a mask belongs to an operator): beam_search /
beam_search_pairs(..., masks=...) take per pair {executor operator: (H,W) uint8 plane}.  A candidate of such an operator
is fitted, scored and executed under its plane -- out = clamp(process(x) m + x (1 - m)), m = float(byte), a count as
functional.rle_union_u8 / mask_select make it -- by the masked forms of the same two kernels, in the same launches and
with the same two host syncs per beam step; every other candidate is global.  `white` (7) is a candidate only under a
plane and rides in the sweep launch.  optimizer='batched' only.  The reference's own masked search is not in its
checkout; these semantics are this project's.

Only dist_type 'L1' is supported (the discriminator distances belong to the out-of-scope
T2ONet+D variant).
"""
import numpy as np
import torch

from . import functional as T

PER_PIXEL_SWEEP_OPS = (0, 1, 2)        # one parameter, bounded range: bracket sweep
WHITE = 7                              # no parameter to fit: scored in the sweep launch, a candidate only under a mask
SWEEP_C = 64


def get_dist(x1, x2, dist_type='L1'):
    if dist_type != 'L1':
        raise NotImplementedError("only dist_type 'L1' is on this path")
    return T.l1_loss(x1, x2)                       # == (x1 - x2).norm(1) / x1.numel()  (beam_search.py:163-165)


def execute(I, operation, param, executor, mask=None):
    img, _ = executor.execute(I, operation, mask, features=None, specified_param=param, has_noise=False)
    return img


def _initial_param(operation, executor):
    n = executor.get_param_num(operation)
    if operation in (0, 1, 2, 6):
        return torch.zeros(n)
    if operation in (3, 5):
        return torch.ones(n)
    raise AssertionError('the operation is not global operation')          # beam_search.py:147


def _fit_sweep_1d(I0, I1, operation, executor, rounds=3):
    ub, lb, _ = executor.get_param_bnd(operation)
    lo, hi = float(lb), float(ub)
    best = None
    for _ in range(rounds):
        cand = torch.linspace(lo, hi, SWEEP_C, device=I0.device).view(-1, 1)
        loss = T.candidates_l1(operation, I0, I1, cand)
        i = int(torch.argmin(loss))                                      # the only host sync of the round
        best = cand[i:i + 1]
        step = (hi - lo) / (SWEEP_C - 1)
        lo, hi = max(float(lb), float(best) - step), min(float(ub), float(best) + step)
    return best.clone(), True


def fit_sweep_batch(images, jobs, target, executor, rounds=3, masks=None):
    """1-parameter fits of many (image, operator) jobs at once.  images: list of (1,3,H,W); jobs: list of
    (image index, operation) or, with masks (N,H,W) uint8 on the device, (image index, operation, plane index or -1): that
    job is fitted under its plane (functional.candidates_multi_l1).  `white` (7) has nothing to fit: it rides in the launch
    with the bracket [0, 0], every candidate the same picture, and returns the parameter 0.
    Returns (params (J,1), dists (J,)) on the device -- no host synchronisation here."""
    dev = target.device
    imgs = torch.cat([im.reshape(1, 3, *im.shape[-2:]) for im in images], 0)
    ops = [jb[1] for jb in jobs]
    idx = [jb[0] for jb in jobs]
    planes = [jb[2] if len(jb) > 2 else -1 for jb in jobs]
    kw = {} if masks is None and all(k < 0 for k in planes) else dict(masks=masks, mask_index=planes)
    bnd = [(0.0, 0.0) if op == WHITE else executor.get_param_bnd(op) for op in ops]
    lb = torch.tensor([float(b[1]) for b in bnd], device=dev).view(-1, 1)
    ub = torch.tensor([float(b[0]) for b in bnd], device=dev).view(-1, 1)
    lo, hi = lb.clone(), ub.clone()
    t = torch.linspace(0.0, 1.0, SWEEP_C, device=dev).view(1, -1)
    best = best_loss = None
    for _ in range(rounds):
        cand = lo + (hi - lo) * t                                        # (J, C)
        loss = T.candidates_multi_l1(ops, idx, imgs, target, cand.unsqueeze(-1), **kw)
        best_loss, i = loss.min(dim=1, keepdim=True)
        best = cand.gather(1, i)
        step = (hi - lo) / (SWEEP_C - 1)
        lo, hi = torch.maximum(lb, best - step), torch.minimum(ub, best + step)
    return best, best_loss.view(-1)


def fit_adam_batch(images, jobs, targets, executor, steps=300, lr=2e-2, check_every=50, tol=1e-6, masks=None):
    """Adam fits of many jobs at once, the sibling of fit_sweep_batch for operators of any parameter count.  images:
    list of (1,3,H,W); targets: list of (1,3,H,W) of that size (or one tensor); jobs: list of (image index, operation)
    -- target 0 --, (image index, operation, target index) or, with masks (N,H,W) uint8 on the device, (image index,
    operation, target index, plane index or -1): that job is fitted under its plane (functional.fit_multi_l1).  Start
    values, step size and stop rule are _fit_adam's as
    'sweep' uses it.  Returns (params (J,24) zero padded, dists (J,)) on the device -- no host synchronisation here;
    more than 64 jobs go in chunks of 64 (the kernel's limit), which does not change any job's result."""
    targets = [targets] if torch.is_tensor(targets) else list(targets)
    dev = targets[0].device
    imgs = torch.cat([im.reshape(1, 3, *im.shape[-2:]) for im in images], 0)
    tgts = torch.cat([t.reshape(1, 3, *t.shape[-2:]) for t in targets], 0)
    jobs = [(jb[0], jb[1], jb[2] if len(jb) > 2 else 0, jb[3] if len(jb) > 3 else -1) for jb in jobs]
    masked = masks is not None or any(jb[3] >= 0 for jb in jobs)
    start = torch.zeros(len(jobs), T.PARAM_PAD)
    for k, (_, op, _, _) in enumerate(jobs):
        p0 = _initial_param(op, executor)
        start[k, :p0.numel()] = p0
    start = start.to(dev)
    out_p, out_d = [], []
    for c0 in range(0, len(jobs), T.FIT_MAX_JOBS):
        chunk = jobs[c0:c0 + T.FIT_MAX_JOBS]
        kw = dict(masks=masks, mask_index=[jb[3] for jb in chunk]) if masked else {}
        p, d = T.fit_multi_l1([jb[1] for jb in chunk], [jb[0] for jb in chunk], imgs, tgts, [jb[2] for jb in chunk],
                              start[c0:c0 + T.FIT_MAX_JOBS], steps=steps, lr=lr, check_every=check_every, tol=tol, **kw)
        out_p.append(p)
        out_d.append(d)
    return (out_p[0], out_d[0]) if len(out_p) == 1 else (torch.cat(out_p), torch.cat(out_d))


def _fit_adam(I0, I1, operation, executor, param0, steps=300, lr=2e-2, check_every=50, tol=1e-6):
    """Adam on the operator's parameters against mean |execute(I0) - I1| (beam_search.py:65-91 with a first-order
    optimiser).  One library call per iteration: executor.value_and_grad (loss + parameter gradient, no separate forward,
    no image gradient, no autograd graph)."""
    n = param0.shape[-1]
    padded = torch.zeros(1, I0.shape[0], T.PARAM_PAD, device=I0.device)
    padded[0, :, :n] = param0.to(I0.device)
    param = padded[0, :, :n].requires_grad_(True)                        # a view: Adam's in-place update lands in `padded`
    opt = torch.optim.Adam([param], lr=lr)
    prev = None
    for it in range(steps):
        loss, _, gparams, _ = executor.value_and_grad(I0, [operation], padded, I1, want_image_grad=False)
        param.grad = gparams[0, :, :n]
        opt.step()
        if (it + 1) % check_every == 0:                                  # one sync per check_every iterations
            cur = loss.item()
            if prev is not None and prev - cur < tol:
                break
            prev = cur
    return param.detach().clone(), True


def _fit_scipy(I0, I1, operation, executor, param0, method):
    from scipy.optimize import minimize

    def func(p):                                                         # beam_search.py:76-86
        param = torch.tensor(np.asarray(p, dtype=np.float32)[None], device=I0.device)
        return get_dist(execute(I0, operation, param, executor), I1).item()
    res = minimize(func, param0.numpy(), method=method)
    return torch.tensor([list(res.x)], dtype=torch.float, device=I0.device), bool(res.success)


def get_param(I0, I1, txt, operation, executor, discriminator=None, dist_type='L1', optimizer='sweep'):
    """Parameter of `operation` that best maps I0 to I1 -> (param (1,n), success_flag)."""
    if dist_type != 'L1' or discriminator is not None:
        raise NotImplementedError("only dist_type 'L1' without a discriminator is on this path")
    param0 = _initial_param(operation, executor)
    if optimizer == 'Nelder-Mead':
        return _fit_scipy(I0, I1, operation, executor, param0, 'Nelder-Mead')
    if optimizer in ('sweep', 'batched') and operation in PER_PIXEL_SWEEP_OPS:
        return _fit_sweep_1d(I0, I1, operation, executor)
    if optimizer == 'batched':
        if I0.shape[0] != 1:
            raise ValueError("optimizer='batched' fits one image pair per job")
        params, _ = fit_adam_batch([I0], [(0, operation)], [I1], executor)
        return params[:, :param0.numel()].clone(), True
    if optimizer in ('sweep', 'adam'):
        lr = 1e-2 if optimizer == 'adam' else 2e-2
        return _fit_adam(I0, I1, operation, executor, param0.view(1, -1).repeat(I0.shape[0], 1), lr=lr)
    if optimizer == 'lbfgs':
        param = param0.view(1, -1).repeat(I0.shape[0], 1).to(I0.device).requires_grad_(True)
        opt = torch.optim.LBFGS([param], lr=1)

        def closure():
            opt.zero_grad()
            loss, _ = executor.run_sequence_fused(I0, [operation], [param], I1)
            loss.backward()
            return loss
        opt.step(closure)
        return param.detach(), True
    raise ValueError('unknown optimizer %r' % (optimizer,))


class _Beam:
    """The beam of one image pair (beam_search.py:196-264): surviving sequences, their images, the early exit."""

    def __init__(self, I_0, I_gt, beam_size, operations, operation_names, err, replace, masks=None):
        self.I_gt, self.beam_size, self.operations, self.names, self.err, self.replace = I_gt, beam_size, operations, operation_names, err, replace
        self.masks = _check_planes(masks, I_gt)       # {executor operator: (H,W) uint8 plane}: that operator is a LOCAL edit
        self.min_dist = float('inf')
        self.sequences = [[[], float('inf')]]
        self.I_buff = [I_0]
        self.done = False

    def candidates(self):
        """(beam, operation) pairs of this step, in the reference's visiting order."""
        pairs = []
        for j in range(len(self.I_buff)):
            used = [self.names.index(v[0]) for v in self.sequences[j][0]]
            pairs += [(j, operation) for operation in self.operations
                      if (self.replace or operation not in used) and (operation != WHITE or WHITE in self.masks)]
        return pairs

    def mask_of(self, operation):
        """What executor.execute takes for this operator: its plane as (1,1,H,W) fp32 -- a count, not divided by 255, as
        functional.mask_select hands the episode -- or None for a global edit."""
        plane = self.masks.get(operation)
        return None if plane is None else plane.float().view(1, 1, *plane.shape)

    def advance(self, pairs, fitted, fit_one, executor):
        """One step.  fitted: {(beam, operation): (param (1,n), dist)} from the batched fits -- their images are executed
        only if they enter the beam; every other pair is fitted by fit_one(I, operation) -> param."""
        all_candidates, I_tmp_list, tmp_min_dists = [], [], []
        no_update, finished = True, False
        for j, operation in pairs:
            I = self.I_buff[j]
            if (j, operation) in fitted:
                param, dist = fitted[(j, operation)]
                I_out = None
            else:
                param = fit_one(I, operation)
                I_out = execute(I, operation, param, executor, self.mask_of(operation))
                dist = get_dist(I_out, self.I_gt).item()
            if dist < self.min_dist:
                if I_out is None:
                    I_out = execute(I, operation, param, executor, self.mask_of(operation))
                tmp_min_dists.append(dist)
                all_candidates.append([self.sequences[j][0] + [(self.names[operation], param[0].tolist(), dist, I_out)], dist])
                I_tmp_list.append(I_out)
                no_update = False
                finished = finished or dist < self.err
        self.min_dist = min(tmp_min_dists) if tmp_min_dists else self.min_dist
        if len(all_candidates) < self.beam_size:
            all_candidates += self.sequences
            I_tmp_list += self.I_buff
        order = np.argsort(np.array([v[1] for v in all_candidates]))
        self.sequences = [all_candidates[i] for i in order][:self.beam_size]
        self.I_buff = [I_tmp_list[i] for i in order][:self.beam_size]
        self.done = no_update or finished

    def result(self):
        actions = [[act[:-1] for act in seq[0]] for seq in self.sequences]
        Is = [[act[-1] for act in seq[0]] for seq in self.sequences]
        return actions, Is


def _check_planes(masks, like):
    """A pair's annotation {executor operator: plane} (None -> {}): every plane a (H,W) uint8 tensor on the images' device."""
    if not masks:
        return {}
    for op, plane in masks.items():
        if not (torch.is_tensor(plane) and plane.dtype == torch.uint8 and plane.device == like.device
                and tuple(plane.shape) == tuple(like.shape[-2:])):
            raise ValueError('masks[%r]: a (%d,%d) uint8 plane on %s is expected' % ((op,) + tuple(like.shape[-2:]) + (like.device,)))
    return {int(op): plane for op, plane in masks.items()}


def _gather_planes(beams):
    """The planes of these beams' pairs in ONE (N,H,W) tensor -- what the masked launches take -- and, per beam,
    {operator: plane number}.  A plane that several operators (or pairs) share is stored once.  (None, [{}, ...]) when no
    pair annotates anything: the unmasked entry points run."""
    planes, at, plane_of = [], {}, []
    for beam in beams:
        own = {}
        for op, plane in beam.masks.items():
            key = (plane.data_ptr(), plane.stride())
            if key not in at:
                at[key] = len(planes)
                planes.append(plane)
            own[op] = at[key]
        plane_of.append(own)
    return (torch.stack(planes).contiguous() if planes else None), plane_of


def _sweep_fits(beam, pairs, executor, fitted, masks=None, plane_of=None):
    """The 1-parameter candidates of a step (and `white`, which has none) through the batched sweep: one host sync per
    64 jobs.  masks / plane_of: _gather_planes' tensor and this beam's {operator: plane number}."""
    batch = [pr for pr in pairs if pr[1] in PER_PIXEL_SWEEP_OPS or pr[1] == WHITE]
    for c0 in range(0, len(batch), 64):                                  # (the kernel takes 64 jobs per launch)
        chunk = batch[c0:c0 + 64]
        if masks is None:
            params, dists = fit_sweep_batch(beam.I_buff, chunk, beam.I_gt, executor)
        else:
            params, dists = fit_sweep_batch(beam.I_buff, [(j, op, plane_of.get(op, -1)) for j, op in chunk], beam.I_gt, executor,
                                            masks=masks)
        params, dists = params.cpu(), dists.cpu()                        # the one host sync of these fits
        for k, pr in enumerate(chunk):
            fitted[pr] = (params[k:k + 1].to(beam.I_gt.device), float(dists[k]))


def _adam_fits(beams, pairs_of, executor, fitted_of, masks=None, plane_of=None):
    """Every candidate of this step that the sweep does not take, of all beams of all pairs, in one fit_adam_batch:
    one host sync.  masks / plane_of: _gather_planes' tensor and per beam {operator: plane number}."""
    images, jobs, owner = [], [], []
    for t, (beam, pairs) in enumerate(zip(beams, pairs_of)):
        base = len(images)
        images += beam.I_buff
        for pr in pairs:
            if pr[1] not in PER_PIXEL_SWEEP_OPS and pr[1] != WHITE:
                jobs.append((base + pr[0], pr[1], t) if masks is None else (base + pr[0], pr[1], t, plane_of[t].get(pr[1], -1)))
                owner.append((t, pr))
    if not jobs:
        return
    params, dists = fit_adam_batch(images, jobs, [beam.I_gt for beam in beams], executor, masks=masks)
    params, dists = params.cpu(), dists.cpu()                            # the one host sync of these fits
    for k, (t, pr) in enumerate(owner):
        n = executor.get_param_num(pr[1])
        fitted_of[t][pr] = (params[k:k + 1, :n].to(beams[t].I_gt.device), float(dists[k]))


def _check_l1(dist_type, discriminator, who):
    if dist_type != 'L1' or discriminator is not None:
        # (checked before any fit: the batched fits score candidates with the L1 kernels directly and would otherwise
        # answer a non-L1 request with L1 distances)
        raise NotImplementedError('%s: L1 distance without a discriminator only (the FiveK planner, beam_search.py:196-264)' % who)


def beam_search(I_0, I_gt, txt, executor, discriminator, beam_size, operations, operation_names, max_step, err,
                dist_type='L1', optimizer='sweep', replace=False, masks=None):
    """Beam search over operator sequences (beam_search.py:196-264).  Returns (actions, Is):
    per surviving sequence the list of (name, param list, dist) and the list of intermediate images.
    masks: None or {executor operator: (H,W) uint8 GPU plane} -- the pair's local edits (gen_greedy_seqs_GIER.py:60-65: a
    mask belongs to an operator): a candidate of such an operator is fitted, scored and executed under its plane,
    out = clamp(process(x) m + x (1 - m)) with m = float(byte), every other candidate is global.  `white` (7) is a
    candidate only under a plane.  optimizer='batched' only."""
    _check_l1(dist_type, discriminator, 'beam_search')
    if masks and optimizer != 'batched':
        raise NotImplementedError("beam_search: masks are fitted by optimizer='batched' only (got %r)" % (optimizer,))
    beam = _Beam(I_0, I_gt, beam_size, operations, operation_names, err, replace, masks)
    planes, plane_of = _gather_planes([beam])

    def fit_one(I, operation):
        return get_param(I, I_gt, txt, operation, executor, None, dist_type, optimizer)[0]
    for _ in range(max_step):
        pairs = beam.candidates()
        fitted = {}
        if optimizer in ('sweep', 'batched'):
            _sweep_fits(beam, pairs, executor, fitted, planes, plane_of[0])
        if optimizer == 'batched':
            _adam_fits([beam], [pairs], executor, [fitted], planes, plane_of)
        beam.advance(pairs, fitted, fit_one, executor)
        if beam.done:
            break
    return beam.result()


def beam_search_pairs(inputs, targets, txt, executor, discriminator, beam_size, operations, operation_names, max_step, err,
                      dist_type='L1', replace=False, masks=None):
    """beam_search(..., optimizer='batched') for P image pairs of one size in lock-step: every pair keeps its own beam
    and its own early exit, the sweeps run per pair, and the multi-parameter fits of all pairs of a step share one
    fit_adam_batch (64 jobs per launch).  inputs / targets: lists of (1,3,H,W).  Returns [(actions, Is)] per pair,
    each exactly what the single-pair search returns.  masks: None or, per pair, None or {executor operator: (H,W) uint8
    GPU plane} as in beam_search; the planes of all live pairs of a step are gathered once into the tensor that step's
    launches take."""
    _check_l1(dist_type, discriminator, 'beam_search_pairs')
    if len(inputs) != len(targets):
        raise ValueError('one target per input')
    masks = [None] * len(inputs) if masks is None else list(masks)
    if len(masks) != len(inputs):
        raise ValueError('one mask entry (None or a dict) per input')
    beams = [_Beam(I_0, I_gt, beam_size, operations, operation_names, err, replace, m) for I_0, I_gt, m in zip(inputs, targets, masks)]
    for _ in range(max_step):
        live = [beam for beam in beams if not beam.done]
        if not live:
            break
        pairs_of = [beam.candidates() for beam in live]
        fitted_of = [{} for _ in live]
        planes, plane_of = _gather_planes(live)
        for beam, pairs, fitted, own in zip(live, pairs_of, fitted_of, plane_of):
            _sweep_fits(beam, pairs, executor, fitted, planes, own)
        _adam_fits(live, pairs_of, executor, fitted_of, planes, plane_of)
        for beam, pairs, fitted in zip(live, pairs_of, fitted_of):
            beam.advance(pairs, fitted, None, executor)
    return [beam.result() for beam in beams]
