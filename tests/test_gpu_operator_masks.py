"""The mask operand of the operator kernels (t2o_kernels.hip) against fp64 autograd of the oracle's
clamp(process(x, p) * m + x * (1 - m), 0, 1): static operators, the per-sample (OP_DYNAMIC) launch the actor's local-edit
path uses with its (B,3,H,W) masks, the fused-L1 forms (t2o_op_fwd_l1 / t2o_op_bwd_l1, called directly: nothing in the
package passes them a mask), a three-step local-edit chain, and the bitwise identities of the blend.

Kernel instantiation -> the case that reaches it (H*W % 4 == 0 -> V = 4, else V = 1; W % 4 == 0 -> strips, else LDS tiles):
  k_point_fwd/bwd<op, V=4, MASKED, L1=false>      static (a) on (9,20) (4,256) (1,4) (5,260) (6,500) (4,264) (18,66) (2,130)
  k_point_fwd/bwd<op, V=1, MASKED, L1=false>      static (a) on (23,19) (17,70) (1,1) (1,7) (5,1)
  k_point_fwd/bwd<OP_DYNAMIC, V=4 / 1, MASKED>    per-sample (b) on (9,20) (5,260) (18,66) / (23,19) (1,7); chain (d)
  k_point_fwd/bwd<op, V=4 / 1, MASKED, L1=true>   fused L1 (c) on (9,20) (5,260) / (23,19)
  k_sharp_fwd_strip<DYN=false, WIDE=false / true> (a) op 6 on (9,20) (4,256) (1,4) / (5,260) (6,500) (4,264); L1: (c)
  k_sharp_fwd_strip<DYN=true, WIDE=false / true>  (b) on (9,20) / (5,260); (d) on (9,20)
  k_sharp_bwd_strip<DYN=false, WIDE, MASKED=true> (a) op 6, the same shapes; L1: (c) on (9,20) / (5,260)
  k_sharp_bwd_strip<DYN=true, WIDE, MASKED=true>  (b) on (9,20) / (5,260); (d) on (9,20)
  k_sharp_fwd/bwd<DYN=false, vec_tile=1>          (a) op 6 on (23,19) (17,70) (18,66) and the tiny shapes; L1: (c) on (23,19)
  k_sharp_fwd/bwd<DYN=true, vec_tile=1>           (b) on (23,19) (18,66) (1,7); (d) on (18,66)
  (k_sharp_fwd/bwd<.., vec_tile=4> is never launched: W % 4 == 0 always takes the strip kernels, sharp_uses_strips)
MASKED = false strip backward and every unmasked form stay with tests/test_gpu_operators.py; (e) ties the two together bit
for bit through the all-ones mask.

Tolerances are those of tests/test_gpu_operators.py (test_vs_oracle_ragged_sizes, test_sharpness_strip_kernels): output rtol
1e-5 + atol 2e-6, image gradient rtol 1e-5 + atol 5e-6, parameter gradient rtol 2e-4 + atol 1e-4 * max(1, max |g|); fused L1:
loss 1e-6, image gradient rtol 1e-5 + atol 1e-5 / n + 1e-9, parameter gradient rtol 2e-4 + atol 1e-6 * gloss.

Clamp edge: an element whose fp64 value under the clamp lies within 1e-5 of 0 or 1 (and not on it: the clamp is inclusive
and elements exactly on a bound are compared as they are) may sit on the other side of the clamp in fp32.  Its gradient is
then blocked where the reference passes it, or the reverse, and everything that depends on it moves with it: its own pixel
for the HSV operators, its 5-point neighbourhood for sharpness, the parameter gradient.  Nothing is left out for it: such an
element may take either side, the side is read off the image gradient where the element acts, and image gradient and
parameter gradient are then both held to the fp64 gradients of that side (clamp_alternatives / settle).  Each case asserts
that at most ceil(0.001 * numel) of its elements are in the band; counted on the CPU from the fp64 reference alone: static
230 of 5,675,376 (worst 1 of 1,560), per-sample 18 of 252,072 (worst 4 of 35,100), fused L1 1 of 138,024, chain 3 of 49,248.

Measured on the MI355X, worst |error| over each group (share of the tolerance): static out 9.2e-7 (0.37), gimg 8.1e-6 (0.62,
an element of size ~1; 'strong' on operators 0 and 2 stays inside the 5e-6 floor), gparam 1.2e-5 (0.01); per-sample out
5.7e-7, gimg 7.7e-7, gparam 4.0e-6; fused L1 out 5.4e-7, loss 4.9e-8, gimg 2.0e-9 (0.05), gparam 1.7e-8; chain out 5.2e-7,
loss 1.1e-8, gimg 1.9e-10, gparam 9.4e-9.  Each test prints its group's worst figures (pytest -s)."""
import math

import numpy as np
import pytest
import torch

from oracle import cpu_ref, synth
from tests.test_block_programs_cpu import operator_apply64, oracle_fwd_bwd

pytestmark = pytest.mark.gpu

OPT = cpu_ref.default_opt()
OPS = [0, 1, 2, 3, 5, 6, 7]
DYN_OPS = [0, 1, 2, 3, 5, 6, 7, -1, 6]
SHAPES = [(9, 20), (4, 256), (1, 4), (5, 260), (6, 500), (4, 264), (23, 19), (17, 70), (18, 66), (1, 1), (1, 7), (5, 1),
          (2, 130)]
DYN_SHAPES = [(9, 20), (5, 260), (23, 19), (18, 66), (1, 7)]
L1_SHAPES = [(9, 20), (5, 260), (23, 19)]
BAND = 1e-5
SEED_IMG, SEED_GOUT, SEED_TGT = 61, 62, 68
MASK_SEED = {('soft', 1): 63, ('soft', 3): 64, ('hard', 1): 65, ('hard', 3): 66}
MASK_KINDS = [('soft', 1), ('soft', 3), ('hard', 1), ('hard', 3), ('box', 1), ('box', 3), ('mix', 3)]
WORST = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def executor(dev):
    import t2onet_amd
    ex = t2onet_amd.Executor(t2onet_amd.default_options())
    ex.load_state_dict(synth.fill_state_dict(ex.state_dict(), seed=3))
    return ex.to(dev)


# ------------------------------------------------------------------ inputs
def box_mask(B, C, H, W):
    """0 everywhere, 1 on rows [H/4, H - H/4) x columns [W/4 + 1, W - W/4): edges off the 4-pixel quads."""
    m = torch.zeros(B, C, H, W)
    m[:, :, H // 4:H - H // 4, W // 4 + 1:W - W // 4] = 1.0
    return m


def mix_mask(B, H, W):
    """What Actor.get_gt_mask produces: all-ones (3,H,W) for samples without a local edit (odd ones here), a box for the rest."""
    m = box_mask(B, 3, H, W)
    m[1::2] = 1.0
    return m


def make_mask(kind, C, B, H, W):
    if kind == 'box':
        return box_mask(B, C, H, W)
    if kind == 'mix':
        return mix_mask(B, H, W)
    return synth.masks(B, C, H, W, MASK_SEED[(kind, C)], soft=(kind == 'soft'))


def dyn_params(ops, seed0, sharp_setting='mid'):
    params = torch.zeros(len(ops), 24)
    for b, op in enumerate(ops):
        if op >= 0:
            params[b, :cpu_ref.OP_NPARAM[op]] = synth.op_params(op, 1, seed0 + b, sharp_setting if op == 6 else 'mid')[0]
    return params


# ------------------------------------------------------------------ the clamp-edge guard (fp64, CPU)
def _edge(pre):
    return ((pre.abs() < BAND) & (pre != 0)) | (((pre - 1).abs() < BAND) & (pre != 1))


def _pre64(op, x, p, m):
    """The fp64 value under the final clamp."""
    out = cpu_ref.process(op, x, p, OPT)
    return out if m is None else out * m + x * (1 - m)


def clamp_alternatives(pre, wrt, gup):
    """For every element e of `pre` (fp64 value under a clamp, part of an autograd graph) in the clamp-edge band: what the
    gradients w.r.t. the tensors `wrt` change by when e sits on the other side of the clamp, i.e. when the gradient gup[e]
    arriving at the clamp's output is blocked where the reference passes it (value inside [0,1]) or the reverse:
    -/+ gup[e] * d pre[e] / d wrt.  -> list of [delta per tensor of wrt]."""
    alts = []
    for idx in _edge(pre.detach()).nonzero():
        idx = tuple(int(i) for i in idx)
        gs = torch.autograd.grad(pre[idx], wrt, retain_graph=True, allow_unused=True)
        g = float(gup[idx]) * (-1.0 if 0.0 <= float(pre[idx].detach()) <= 1.0 else 1.0)
        alts.append([torch.zeros_like(w) if d is None else g * d for d, w in zip(gs, wrt)])
    return alts


def settle(gots, refs, alts):
    """The references with, for every clamp-edge element, the side of the clamp that the computed gradients took: decided
    where that element acts (the support of its delta, first tensor that has one), then applied to every tensor -- the
    image gradient and the parameter gradients must agree on it."""
    refs = [r.clone() for r in refs]
    for alt in alts:
        for got, ref, d in zip(gots, refs, alt):
            sup = d != 0
            if sup.any():
                got = got.detach().cpu().double()
                if float((got - ref - d)[sup].abs().max()) < float((got - ref)[sup].abs().max()):
                    refs = [r + dd for r, dd in zip(refs, alt)]
                break
    return refs


def single_op_refs(op, img, p, mask, gup, gots, refs):
    """settle() for one operator application.  -> (references, number of clamp-edge elements)."""
    x = img.double().requires_grad_(True)
    pp = p.double().requires_grad_(True)
    pre = _pre64(op, x, pp, None if mask is None else mask.double())
    if not _edge(pre.detach()).any():
        return refs, 0
    alts = clamp_alternatives(pre, [x, pp], gup.double() if torch.is_tensor(gup) else gup(pre.detach()))
    return settle(gots, refs, alts), len(alts)


def check_cap(tag, edge, numel):
    cap = math.ceil(0.001 * numel)
    assert edge <= cap, '%s: %d of %d elements in the clamp-edge band (cap %d)' % (tag, edge, numel, cap)


# ------------------------------------------------------------------ comparison that reports every miss
class Report:
    def __init__(self, group):
        self.group, self.fails = group, []
        self.worst = WORST.setdefault(group, {})

    def close(self, tag, what, got, ref, rtol, atol):
        """|got - ref| <= atol + rtol |ref|."""
        got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
        ref = np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref, dtype=np.float64)
        assert got.shape == ref.shape, (tag, what, got.shape, ref.shape)
        if got.size == 0:
            return
        tol = np.asarray(atol, dtype=np.float64) + rtol * np.abs(ref)
        err = np.abs(got - ref)
        bad = ~(err <= tol)                                   # (a NaN is a miss)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.nanmax(np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0)))
        w = self.worst.setdefault(what, [0.0, 0.0, ''])
        if float(np.nanmax(err)) > w[0]:
            w[0], w[2] = float(np.nanmax(err)), tag
        w[1] = max(w[1], float(ratio))
        if bad.any():
            self.fails.append('%s %s: %d of %d miss, max |err| %.3e = %.2f x tolerance' % (tag, what, int(bad.sum()), bad.size,
                                                                                       float(np.nanmax(err)), float(ratio)))

    def equal(self, tag, what, a, b):
        if not torch.equal(a, b):
            d = (a.double() - b.double()).abs()
            self.fails.append('%s %s: not bit-identical (%d elements, max |diff| %.3e)' % (tag, what, int((a != b).sum()), float(d.max())))

    def finish(self):
        print('\n[%s] worst so far: %s' % (self.group, ', '.join('%s %.3e (%.2f x tol, %s)' % (k, v[0], v[1], v[2])
                                                                  for k, v in sorted(self.worst.items()))))
        assert not self.fails, '%d comparisons miss:\n%s' % (len(self.fails), '\n'.join(self.fails[:40]))


def compare_grads(rep, tag, op, img, p, mask, gout, out, gimg, gparam, o64, gi64, gp64, gimg_atol=5e-6):
    """The three comparisons of one operator application against fp64.  -> number of clamp-edge elements."""
    (gi64, gp64), edge = single_op_refs(op, img, p, mask, gout, [gimg, gparam], [gi64, gp64])
    rep.close(tag, 'out', out, o64, 1e-5, 2e-6)
    rep.close(tag, 'gimg', gimg, gi64, 1e-5, gimg_atol)
    scale = max(1.0, float(gp64.abs().max())) if gp64.numel() else 1.0
    rep.close(tag, 'gparam', gparam, gp64, 2e-4, 1e-4 * scale)
    return edge


# ------------------------------------------------------------------ launches
def run_static(executor, dev, op, img_d, p, mask_d, gout_d):
    x = img_d.clone().requires_grad_(True)
    pp = p.to(dev).clone().requires_grad_(True)
    out, _ = executor.execute(x, op, mask_d, specified_param=pp)
    out.backward(gout_d)
    return out.detach(), x.grad, pp.grad


def run_dynamic(executor, dev, ops_d, img_d, p24, mask_d, gout_d):
    x = img_d.clone().requires_grad_(True)
    pp = p24.to(dev).clone().requires_grad_(True)
    out, _ = executor.execute_per_sample(x, ops_d, mask_d, specified_param=pp)
    out.backward(gout_d)
    return out.detach(), x.grad, pp.grad


# ------------------------------------------------------------------ (a) static operators
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('op', OPS)
def test_static_masked_vs_fp64(executor, dev, op, shape):
    """execute(x, op, mask): every mask kind at both channel counts, 'mid' and 'strong' (clamp active under the blend);
    output, image gradient and parameter gradient against fp64 autograd."""
    H, W = shape
    B = 2
    img = synth.images(B, H, W, SEED_IMG)
    gout = synth.uniform((B, 3, H, W), SEED_GOUT, -1.0, 1.0)
    img_d, gout_d = img.to(dev), gout.to(dev)
    rep = Report('static')
    for si, setting in enumerate(['mid', 'strong']):
        p = synth.op_params(op, B, 400 + 10 * op + si, setting)
        for kind, C in MASK_KINDS:
            tag = 'op%d %dx%d %s %s%d' % (op, H, W, setting, kind, C)
            mask = make_mask(kind, C, B, H, W)
            o64, gi64, gp64 = oracle_fwd_bwd(op, img, p, mask, gout, torch.float64)
            out, gimg, gparam = run_static(executor, dev, op, img_d, p, mask.to(dev), gout_d)
            check_cap(tag, compare_grads(rep, tag, op, img, p, mask, gout, out, gimg, gparam, o64, gi64, gp64), img.numel())
    rep.finish()


# ------------------------------------------------------------------ (b) per-sample launch
@pytest.mark.parametrize('shape', DYN_SHAPES)
def test_per_sample_masked_vs_fp64(executor, dev, shape):
    """execute_per_sample with a mask, forward AND backward (the actor's local-edit path always passes (B,3,H,W) masks to
    this launch): each sample against fp64 of its own operator; gparam columns past the operator's parameter count are
    exactly 0; the identity sample returns its image and its gradient bit for bit whatever its mask."""
    H, W = shape
    ops = DYN_OPS
    B = len(ops)
    img = synth.images(B, H, W, SEED_IMG)
    gout = synth.uniform((B, 3, H, W), SEED_GOUT, -1.0, 1.0)
    params = dyn_params(ops, 500)
    img_d, gout_d = img.to(dev), gout.to(dev)
    ops_d = torch.tensor(ops, dtype=torch.int32, device=dev)
    rep = Report('per-sample')
    for kind, C in [('soft', 1), ('soft', 3), ('mix', 3)]:
        mask = make_mask(kind, C, B, H, W)
        out, gimg, gparam = run_dynamic(executor, dev, ops_d, img_d, params, mask.to(dev), gout_d)
        out, gimg, gparam = out.cpu(), gimg.cpu(), gparam.cpu()
        edge = 0
        for b, op in enumerate(ops):
            tag = 'op%d sample %d %dx%d %s%d' % (op, b, H, W, kind, C)
            if op < 0:
                rep.equal(tag, 'out', out[b], img[b])
                rep.equal(tag, 'gimg', gimg[b], gout[b])
                rep.equal(tag, 'gparam', gparam[b], torch.zeros(24))
                continue
            n = cpu_ref.OP_NPARAM[op]
            sl = slice(b, b + 1)
            o64, gi64, gp64 = oracle_fwd_bwd(op, img[sl], params[sl, :n], mask[sl], gout[sl], torch.float64)
            edge += compare_grads(rep, tag, op, img[sl], params[sl, :n], mask[sl], gout[sl], out[sl], gimg[sl],
                                      gparam[sl, :n], o64, gi64, gp64)
            rep.equal(tag, 'gparam columns past the parameter count', gparam[b, n:], torch.zeros(24 - n))
        check_cap('%dx%d %s%d' % (H, W, kind, C), edge, img.numel())
    rep.finish()


# ------------------------------------------------------------------ (c) fused L1 with a mask
@pytest.mark.parametrize('shape', L1_SHAPES)
@pytest.mark.parametrize('op', [0, 1, 2, 3, 5, 6])
def test_fused_l1_masked_vs_fp64(dev, op, shape):
    """t2o_op_fwd_l1 / t2o_op_bwd_l1 with a mask (k_point_fwd/bwd<OP, V, MASKED = true, L1 = true>, the strip and LDS-tile
    stencil kernels with target and mask together), through the C ABI: out, loss, gimg and gparam against fp64 autograd of
    3 * mean |operator(x, p, m) - target|."""
    import t2onet_amd.functional as T
    from t2onet_amd import _lib
    lib = _lib.load()
    H, W = shape
    B, gl = 2, 3.0
    n = cpu_ref.OP_NPARAM[op]
    numel = B * 3 * H * W
    img, tgt = synth.images(B, H, W, SEED_IMG), synth.images(B, H, W, SEED_TGT)
    p = synth.op_params(op, B, 400 + 10 * op, 'mid')
    img_d, tgt_d, p_d = img.to(dev), tgt.to(dev), p.to(dev)
    gloss = torch.full((1,), gl, device=dev)
    st = T._stream(dev)
    rep = Report('fused-L1')
    for kind, C in [('soft', 1), ('hard', 3)]:
        tag = 'op%d %dx%d %s%d' % (op, H, W, kind, C)
        mask = make_mask(kind, C, B, H, W)
        x = img.double().requires_grad_(True)
        pp = p.double().requires_grad_(True)
        o64 = operator_apply64(op, x, pp, mask.double())
        l64 = (o64 - tgt.double()).abs().mean()
        (gl * l64).backward()
        mask_d = mask.to(dev)
        out = torch.full_like(img_d, float('nan'))
        loss = torch.full((1,), float('nan'), device=dev)
        gimg = torch.full_like(img_d, float('nan'))
        gparam = torch.full((B, n), float('nan'), device=dev)
        ws = T.workspace(B, H, W, dev)
        rc = lib.t2o_op_fwd_l1(op, img_d.data_ptr(), p_d.data_ptr(), n, mask_d.data_ptr(), C, tgt_d.data_ptr(), out.data_ptr(),
                               loss.data_ptr(), ws.data_ptr(), ws.numel(), B, H, W, st)
        _lib.check(rc, 't2o_op_fwd_l1')
        rc = lib.t2o_op_bwd_l1(op, img_d.data_ptr(), p_d.data_ptr(), n, mask_d.data_ptr(), C, tgt_d.data_ptr(), gloss.data_ptr(),
                               gimg.data_ptr(), gparam.data_ptr(), n, ws.data_ptr(), ws.numel(), B, H, W, st)
        _lib.check(rc, 't2o_op_bwd_l1')
        (gi64, gp64), edge = single_op_refs(op, img, p, mask, lambda pre: gl / numel * torch.sign(pre.clamp(0, 1) - tgt.double()),
                                            [gimg, gparam], [x.grad, pp.grad])
        check_cap(tag, edge, numel)
        rep.close(tag, 'out', out, o64, 1e-5, 2e-6)
        rep.close(tag, 'loss', loss, l64.reshape(1), 0.0, 1e-6)
        rep.close(tag, 'gimg', gimg, gi64, 1e-5, 1e-5 / numel + 1e-9)
        rep.close(tag, 'gparam', gparam, gp64, 2e-4, 1e-6 * gl)
    rep.finish()


# ------------------------------------------------------------------ (d) a three-step local-edit chain
# Every sample meets sharpness exactly once: under the ones/box mix (samples 0, 3), under the soft mask (1, 4), unmasked
# (2, 5); white (7) under a soft mask and an identity step (-1) are in.
# A clamp that acts leaves channels at exactly 0 or 1, and the next operator maps those to within 1e-6 of the bound again
# (a curve gives 1 - 1e-11 at 1, the HSV operators 9e-7 at 0): with images over (0,1) and 'mid' sharpness the fp64 chain
# alone puts 2,085 of 21,384 elements into the clamp-edge band, where fp32 and fp64 may legitimately disagree.  The chain is
# about gradients flowing through masked steps, the acting clamp is (a)'s 'strong' setting, so the images stay in
# (0.25, 0.75) and sharpness takes its gentle range: at most 2 of 21,384 and 0 of 3,240 elements in the band (counted on
# the CPU, both mask pairs).
CHAIN_OPS = [[6, 0, 1, 6, 3, 5],
             [7, 6, 2, 3, 6, 1],
             [1, 2, 6, -1, 0, 6]]
CHAIN_SEED = 520
CHAIN_RANGE = (0.25, 0.75)
CHAIN_SETTING = 'neg'                       # of sharpness; every other operator 'mid'


def _chain64(img_b, tgt_b, ops_b, params_b, masks_b, numel):
    """One sample's chain in fp64, operator by operator as cpu_ref.run_sequence runs it (with operator_apply64's 64-bit
    sharpness / contrast forms); its share of mean |x3 - target| over the whole batch.
    -> x3, [x0.grad, p_a.grad, p_b.grad, p_c.grad], clamp_alternatives of the three clamps."""
    x0 = img_b.double().requires_grad_(True)
    ps = [p.double().requires_grad_(True) for p in params_b]
    cur, pres, outs = x0, [], []
    for op, p, m in zip(ops_b, ps, masks_b):
        if op >= 0:
            m64 = None if m is None else m.double()
            pres.append(_pre64(op, cur, p[:, :cpu_ref.OP_NPARAM[op]], m64))
            cur = operator_apply64(op, cur, p[:, :cpu_ref.OP_NPARAM[op]], m64)
            cur.retain_grad()
        else:
            pres.append(None)
        outs.append(cur)
    loss = (cur - tgt_b.double()).abs().sum() / numel
    loss.backward(retain_graph=True)
    alts = []
    for k, pre in enumerate(pres):
        if pre is not None:
            alts += clamp_alternatives(pre, [x0] + ps, outs[k].grad)
    return cur.detach(), [x0.grad] + [p.grad if p.grad is not None else torch.zeros_like(p) for p in ps], alts


@pytest.mark.parametrize('shape', [(18, 66), (9, 20)])
@pytest.mark.parametrize('mask_pair', ['mix3-soft1', 'hard3-soft3'])
def test_local_edit_chain_vs_fp64(dev, shape, mask_pair):
    """x1 = apply_per_sample(ops_a, x0, p_a, m_a); x2 = apply_per_sample(ops_b, x1, p_b, m_b);
    x3 = apply_per_sample(ops_c, x2, p_c, None); loss = l1_loss(x3, target): x0.grad and the three parameter gradients
    against the fp64 chain of each sample.  'mix3-soft1': m_a the ones/box mix (C = 3), m_b soft (C = 1) -- what the
    actor's local-edit episodes pass; the three planes of such a mask are equal, so a wrong plane index cannot show.
    'hard3-soft3': m_a hard, m_b soft, both with three different planes -- where it does (the soft one second: white
    under a hard mask writes exact ones, which the contrast after it puts into the clamp-edge band).

    Tolerances: the output as everywhere (rtol 1e-5 + atol 2e-6).  The gradients are those of a mean over n elements, so
    they are O(1 / n) and a fixed absolute floor would compare nothing; x1 and x2 carry fp32 rounding into the next
    operator's derivative, so the single-operator 1e-5 does not transfer either.  The bound is the one the project's
    chain-against-fp64 test (test_chain6_gradients_vs_fp64_oracle, six operators) holds: rtol 2e-4 + atol 2e-5 * max |g|."""
    import t2onet_amd.functional as T
    H, W = shape
    B = 6
    numel = B * 3 * H * W
    img, tgt = synth.uniform((B, 3, H, W), SEED_IMG, *CHAIN_RANGE), synth.images(B, H, W, SEED_TGT)
    params = [dyn_params(ops, CHAIN_SEED + 10 * k, CHAIN_SETTING) for k, ops in enumerate(CHAIN_OPS)]
    masks = {'mix3-soft1': [mix_mask(B, H, W), make_mask('soft', 1, B, H, W), None],
             'hard3-soft3': [make_mask('hard', 3, B, H, W), make_mask('soft', 3, B, H, W), None]}[mask_pair]
    x0 = img.to(dev).clone().requires_grad_(True)
    ps = [p.to(dev).clone().requires_grad_(True) for p in params]
    cur = x0
    for ops, p, m in zip(CHAIN_OPS, ps, masks):
        cur = T.apply_per_sample(torch.tensor(ops, dtype=torch.int32, device=dev), cur, p, None if m is None else m.to(dev))
    loss = T.l1_loss(cur, tgt.to(dev))
    loss.backward()
    x3, gots = cur.detach().cpu(), [x0.grad.cpu()] + [p.grad.cpu() for p in ps]
    rep = Report('chain')
    outs, refs, edge = [], [], 0
    for b in range(B):
        sl = slice(b, b + 1)
        ops_b = [ops[b] for ops in CHAIN_OPS]
        o64, r, alts = _chain64(img[sl], tgt[sl], ops_b, [p[sl] for p in params], [None if m is None else m[sl] for m in masks], numel)
        # the same chain through cpu_ref.run_sequence itself (identity steps dropped: it has none)
        live = [k for k in range(3) if ops_b[k] >= 0]
        seq, _ = cpu_ref.run_sequence(img[sl].double(), [ops_b[k] for k in live],
                                      [params[k][sl, :cpu_ref.OP_NPARAM[ops_b[k]]].double() for k in live], OPT,
                                      masks=[None if masks[k] is None else masks[k][sl].double() for k in live])
        assert float((seq.detach() - o64).abs().max()) < 1e-12
        outs.append(o64)
        refs.append(settle([g[sl] for g in gots], r, alts))
        edge += len(alts)
    tag = 'chain %dx%d %s' % (H, W, mask_pair)
    check_cap(tag, edge, numel)
    o64 = torch.cat(outs)
    rep.close(tag, 'out', x3, o64, 1e-5, 2e-6)
    rep.close(tag, 'loss', loss.detach().reshape(1), (o64 - tgt.double()).abs().mean().reshape(1), 0.0, 1e-6)
    g64 = torch.cat([r[0] for r in refs])
    rep.close(tag, 'gimg', gots[0], g64, 2e-4, 2e-5 * float(g64.abs().max()))
    for k in range(3):
        gk = torch.cat([r[1 + k] for r in refs])
        rep.close(tag + ' step %d' % k, 'gparam', gots[1 + k], gk, 2e-4, 2e-5 * max(float(gk.abs().max()), 1e-6))
        for b in range(B):
            n = cpu_ref.OP_NPARAM[CHAIN_OPS[k][b]] if CHAIN_OPS[k][b] >= 0 else 0
            rep.equal(tag + ' step %d sample %d' % (k, b), 'gparam columns past the parameter count', gots[1 + k][b, n:],
                      torch.zeros(24 - n))
    rep.finish()


# ------------------------------------------------------------------ (e) bitwise identities
@pytest.mark.parametrize('shape', L1_SHAPES)
def test_mask_bitwise_identities(executor, dev, shape):
    """Forward and backward, static and per-sample: an all-ones mask (C = 1, 3) is the unmasked result; an all-zero mask
    returns the image, the output gradient and a zero parameter gradient; a C = 1 mask and its plane repeated three times,
    and a (1,3,H,W) mask broadcast over the batch and its materialised copy, give identical bits; so do two runs."""
    H, W = shape
    rep = Report('identities')
    launches = [('op%d' % op, op, 2) for op in OPS] + [('per-sample', None, len(DYN_OPS))]
    for name, op, B in launches:
        img_d = synth.images(B, H, W, SEED_IMG).to(dev)
        gout_d = synth.uniform((B, 3, H, W), SEED_GOUT, -1.0, 1.0).to(dev)
        if op is None:
            p = dyn_params(DYN_OPS, 500)
            ops_d = torch.tensor(DYN_OPS, dtype=torch.int32, device=dev)
            run = lambda m: run_dynamic(executor, dev, ops_d, img_d, p, m, gout_d)
        else:
            p = synth.op_params(op, B, 400 + 10 * op, 'mid')
            run = lambda m: run_static(executor, dev, op, img_d, p, m, gout_d)
        tag = '%s %dx%d' % (name, H, W)
        names = ('out', 'gimg', 'gparam')
        plain = run(None)
        for C in (1, 3):
            for q, a, b in zip(names, run(torch.ones(B, C, H, W, device=dev)), plain):
                rep.equal(tag + ' ones%d' % C, q, a, b)
            o, gi, gp = run(torch.zeros(B, C, H, W, device=dev))
            rep.equal(tag + ' zeros%d' % C, 'out', o, img_d)
            rep.equal(tag + ' zeros%d' % C, 'gimg', gi, gout_d)
            rep.equal(tag + ' zeros%d' % C, 'gparam', gp, torch.zeros_like(gp))
        m1 = synth.masks(B, 1, H, W, MASK_SEED[('soft', 1)]).to(dev)
        r1 = run(m1)
        for q, a, b in zip(names, run(m1.repeat(1, 3, 1, 1)), r1):
            rep.equal(tag + ' C=1 against its plane repeated', q, a, b)
        for q, a, b in zip(names, run(m1), r1):
            rep.equal(tag + ' second run', q, a, b)
        m3 = synth.masks(1, 3, H, W, MASK_SEED[('soft', 3)]).to(dev)
        for q, a, b in zip(names, run(m3), run(m3.repeat(B, 1, 1, 1))):
            rep.equal(tag + ' (1,3,H,W) broadcast against its copy', q, a, b)
    rep.finish()
