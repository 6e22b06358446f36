"""Inputs and fp64 references for the four kernel groups that end every train step: the operators' parameter heads
(t2o_heads.hip), the episode loss (k_l1_* / k_end_l1_* in t2o_kernels.hip), the flat Adam step and the graph fill kernel
(t2o_optim.hip).  Pure numpy / CPU torch: tests/test_step_cases_cpu.py checks the references themselves, the GPU tests
(tests/test_gpu_step_*.py) hold the kernels to them.

u = 2^-24 (half an fp32 ulp of 1) throughout."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref

U = 2.0 ** -24
D = 512
PAD = 24
HEAD_OPS = (0, 1, 2, 3, 5, 6, 7)
N_PARAM = cpu_ref.OP_NPARAM
ATTR = cpu_ref.OP_ATTRS
DEFAULT_CONSTS = (2.0, -0.2, 0.8, 1.5)                       # brightness_range, saturation lo, hi, sharpness_range
OTHER_CONSTS = (1.25, -0.375, 0.625, 2.75)                   # (fp32-exact, so the kernel's floats are the reference's numbers)
HEAD_KEYS = ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias')


def opt_of(consts):
    """The oracle's options with these constants AS THE KERNELS RECEIVE THEM: fp32 (-0.2f is 0.6 u off -0.2)."""
    consts = [float(np.float32(c)) for c in consts]
    return cpu_ref.default_opt(brightness_range=consts[0], saturation_range=(consts[1], consts[2]), sharpness_range=consts[3])


# ----------------------------------------------------------------------------------------------------------------------
# parameter heads
# ----------------------------------------------------------------------------------------------------------------------
def dyadic_heads(seed):
    """Weights on which fc1 is EXACT in fp32 under any summation order: W1, W2 multiples of 2^-8 in [-2^-4, 2^-4], b1 odd
    multiples of 2^-15 (so |pre| >= 2^-15: no unit sits on the LeakyReLU kink), b2 multiples of 2^-8.  With features on the
    2^-6 grid in [-1, 1] every product is a multiple of 2^-14 below 2^-4 and every partial sum of 512 of them plus the bias
    a multiple of 2^-15 below 2^6: 21 bits."""
    rng = np.random.default_rng(seed)
    sd = {}
    for op in HEAD_OPS:
        n = N_PARAM[op]
        sd[ATTR[op] + '.fc1.weight'] = rng.integers(-16, 17, (D, D)).astype(np.float32) * np.float32(2.0 ** -8)
        sd[ATTR[op] + '.fc1.bias'] = (2 * rng.integers(-64, 64, D) + 1).astype(np.float32) * np.float32(2.0 ** -15)
        sd[ATTR[op] + '.fc2.weight'] = rng.integers(-16, 17, (n, D)).astype(np.float32) * np.float32(2.0 ** -8)
        sd[ATTR[op] + '.fc2.bias'] = rng.integers(-16, 17, n).astype(np.float32) * np.float32(2.0 ** -8)
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def dyadic_features(B, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(-64, 65, (B, D)).astype(np.float32) * np.float32(2.0 ** -6))


def default_init_heads(seed, scale=1.0):
    """nn.Linear's default initialisation (uniform +-1/sqrt(fan_in)) from a numpy stream, times `scale`."""
    rng = np.random.default_rng(seed)
    k = 1.0 / math.sqrt(D)
    sd = {}
    for op in HEAD_OPS:
        n = N_PARAM[op]
        for key, shape in zip(HEAD_KEYS, ((D, D), (D,), (n, D), (n,))):
            sd[ATTR[op] + '.' + key] = torch.from_numpy((rng.uniform(-k, k, shape) * scale).astype(np.float32))
    return sd


def random_features(B, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, (B, D)).astype(np.float32))


def gout_of(B, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, (B, PAD)).astype(np.float32))


MIXED = [0, 1, 2, 3, 5, 6, -1, 4, 3, 5, 0, 2, 7]               # the operator test's pattern, with op 7


def op_layout(name, B):
    """(B,) int32 operator ids.  'mixed': period 13, every head; 'run<k>': operator k owns samples 0..68 (a whole 64-sample
    ballot chunk and five stragglers in the next), the rest mixed; 'none': only identity / inpaint rows; 'all<k>'."""
    if name == 'mixed':
        ids = (MIXED * (B // len(MIXED) + 1))[:B]
    elif name.startswith('run'):
        ids = (MIXED * (B // len(MIXED) + 1))[:B]
        ids[:min(B, 69)] = [int(name[3:])] * min(B, 69)
    elif name == 'none':
        ids = ([-1, 4, 4, -1, -1] * (B // 5 + 1))[:B]
    elif name.startswith('all'):
        ids = [int(name[3:])] * B
    else:
        raise KeyError(name)
    return torch.tensor(ids, dtype=torch.int32)


# gradient cases (dyadic inputs): (name, B, layout, consts).  B = 1, 64, 65, 128, 130 are the ballot boundaries of the
# weight-gradient kernels; 'all<k>' puts every sample on one head; 'none' selects no head at all.
HEAD_GRAD_CASES = (
    ('b1', 1, 'mixed', DEFAULT_CONSTS),
    ('b64_mixed', 64, 'mixed', DEFAULT_CONSTS),
    ('b65_run6', 65, 'run6', OTHER_CONSTS),
    ('b128_mixed', 128, 'mixed', OTHER_CONSTS),
    ('b130_run3', 130, 'run3', DEFAULT_CONSTS),
    ('b130_run2', 130, 'run2', OTHER_CONSTS),
    ('b9_none', 9, 'none', DEFAULT_CONSTS),
) + tuple(('b3_all%d' % k, 3, 'all%d' % k, OTHER_CONSTS if k % 2 else DEFAULT_CONSTS) for k in HEAD_OPS)


def head_grad_case(name):
    """-> (sd, op_ids, ctx, gout, consts) of a gradient case: dyadic weights and features."""
    i, (_, B, layout, consts) = next((i, c) for i, c in enumerate(HEAD_GRAD_CASES) if c[0] == name)
    return dyadic_heads(40 + i), op_layout(layout, B), dyadic_features(B, 60 + i), gout_of(B, 80 + i), consts


def heads_reference(sd, op_ids, ctx, consts, gout=None):
    """The heads in fp64, operator group by operator group: pre / hidden / raw / param as (B, .) arrays (zero rows for op -1
    or 4) and, with gout, the fp64 autograd gradients of (param * gout).sum(): gctx, dpre (at fc1's pre-activation) and
    the 28 head gradients (exact zeros for heads no sample selected)."""
    opt = opt_of(consts)
    B = ctx.shape[0]
    w = {k: v.double().requires_grad_(gout is not None) for k, v in sd.items()}
    x = ctx.double().requires_grad_(gout is not None)
    out = {k: torch.zeros(B, n, dtype=torch.float64) for k, n in (('pre', D), ('hidden', D), ('raw', PAD))}
    param = torch.zeros(B, PAD, dtype=torch.float64)
    pres = []
    for op in HEAD_OPS:
        idx = (op_ids == op).nonzero().flatten()
        if idx.numel() == 0:
            continue
        a, n = ATTR[op], N_PARAM[op]
        pre = F.linear(x[idx], w[a + '.fc1.weight'], w[a + '.fc1.bias'])
        if gout is not None:
            pre.retain_grad()
        hid = F.leaky_relu(pre, 0.01)
        raw = F.linear(hid, w[a + '.fc2.weight'], w[a + '.fc2.bias'])
        param[idx, :n] = cpu_ref.regress(op, raw, opt)
        pres.append((idx, pre))
        out['pre'][idx] = pre.detach()
        out['hidden'][idx] = hid.detach()
        out['raw'][idx, :n] = raw.detach()
    ref = {k: v.numpy() for k, v in out.items()}
    ref['param'] = param.detach().numpy()
    if gout is not None:
        if pres:
            (param * gout.double()).sum().backward()
        dpre = torch.zeros(B, D, dtype=torch.float64)
        for idx, pre in pres:
            dpre[idx] = pre.grad
        ref['dpre'] = dpre.numpy()
        ref['gctx'] = (torch.zeros_like(x) if x.grad is None else x.grad).numpy()
        ref['gw'] = {k: (torch.zeros_like(v) if v.grad is None else v.grad).numpy() for k, v in w.items()}
    return ref


# The kernels' dot products (row_dot / k_heads_fc1): a lane multiplies 8 weight-feature pairs (1 rounding each), adds them
# as ((p0+p1)+(p2+p3)) + ((p4+p5)+(p6+p7)) (3 additions on every product's path), the 64 lanes meet in 6 shuffle levels
# (6 more) and the bias is added last (1): 11 roundings on every product's path, 1 on the bias.  So
#   |fl(dot + b) - (dot + b)| <= ((1 + u)^11 - 1) sum|w_i x_i| + u |b|  <=  12 u (sum|w_i x_i| + |b|)
# for 11 * 11 / 2 * u << 1.  K = 12 is the bound, not a fit.
K_DOT = 12


def dot_bound(wabs, xabs, babs):
    """K_DOT u (sum_i |w_ji| |x_bi| + |b_j|) for every (sample, row): the fp32 dot product's worst-case error."""
    return K_DOT * U * (xabs @ wabs.T + babs[None, :])


def forward_bounds(sd, op_ids, ctx, hidden_gpu):
    """Per-element error bounds of the fused forward against fp64, layer by layer:
      hidden: against lrelu(W1 ctx + b1) in fp64.  E_pre = dot_bound; a unit whose fp64 pre-activation lies at least E_pre
              below zero is negative in fp32 too and carries 0.01 E_pre plus the product with 0.01f (one rounding, and 0.01f is
              0.37 u off 0.01: 2 u |h|); any other unit carries at most E_pre (LeakyReLU is 1-Lipschitz across the kink);
      raw:    against W2 hidden_gpu + b2 in fp64 from the kernel's OWN fp32 hidden -- one dot product, dot_bound again.
    Returns (hidden64, E_hidden, raw_from_gpu_hidden64, E_raw, E_raw_total) with E_raw_total = E_raw + |W2| E_hidden, the
    bound of raw against the all-fp64 raw; rows of op -1 / 4 all zero with zero bounds."""
    B = ctx.shape[0]
    x = ctx.double().numpy()
    hg = np.asarray(hidden_gpu, dtype=np.float64)
    hid = np.zeros((B, D)); e_hid = np.zeros((B, D))
    raw = np.zeros((B, PAD)); e_raw = np.zeros((B, PAD)); e_tot = np.zeros((B, PAD))
    for op in HEAD_OPS:
        idx = (op_ids == op).nonzero().flatten().numpy()
        if idx.size == 0:
            continue
        a, n = ATTR[op], N_PARAM[op]
        w1, b1 = sd[a + '.fc1.weight'].double().numpy(), sd[a + '.fc1.bias'].double().numpy()
        w2, b2 = sd[a + '.fc2.weight'].double().numpy(), sd[a + '.fc2.bias'].double().numpy()
        p = x[idx] @ w1.T + b1
        e = dot_bound(np.abs(w1), np.abs(x[idx]), np.abs(b1))
        h = np.where(p > 0, p, 0.01 * p)
        hid[idx] = h
        e_hid[idx] = np.where(p < -e, 0.01 * e, e) + 2 * U * np.abs(h)
        raw[idx, :n] = hg[idx] @ w2.T + b2
        e_raw[idx, :n] = dot_bound(np.abs(w2), np.abs(hg[idx]), np.abs(b2))
        e_tot[idx, :n] = e_raw[idx, :n] + e_hid[idx] @ np.abs(w2).T
    return hid, e_hid, raw, e_raw, e_tot


def regress64(op, f, consts):
    return cpu_ref.regress(op, torch.as_tensor(f, dtype=torch.float64), opt_of(consts)).numpy()


def regress_slope_sup(op, f, e, consts):
    """sup |regressor'| over [f - e, f + e]: tanh' and sigmoid' peak at 0 and fall off monotonically on both sides, so the sup
    sits at the point of the interval nearest 0 (for saturation: per branch, the slopes differ left and right of 0)."""
    br, lo, hi, sh = consts
    near = np.clip(0.0, f - e, f + e)
    sech2 = 1.0 - np.tanh(near) ** 2
    sig = 1.0 / (1.0 + np.exp(-near))
    if op == 0:
        return sech2 * br
    if op == 1:
        return sech2
    if op == 2:
        right = np.where(f + e > 0, (1.0 - np.tanh(np.maximum(f - e, 0.0)) ** 2) * abs(hi), 0.0)
        left = np.where(f - e < 0, (1.0 - np.tanh(np.minimum(f + e, 0.0)) ** 2) * abs(lo), 0.0)
        return np.maximum(left, right)
    if op == 6:
        return sig * (1 - sig) * sh
    if op == 7:
        return sig * (1 - sig)
    return np.ones_like(f)


def regress_scale(op, consts):
    br, lo, hi, sh = consts
    return {0: 2 * br, 1: 1.0, 2: max(abs(lo), abs(hi)), 6: sh, 7: 1.0}.get(op, 0.0)


def param_bound(op, consts):
    """|param_gpu - regressor64(raw_gpu)| allowed, the regressor evaluated at the kernel's own fp32 raw: tanhf is good to
    2 ulp of a value below 1 (4 u), expf to 1 ulp and the sigmoid adds two roundings (4 u); the remaining arithmetic is at
    most four roundings of numbers no larger than the output range (op 0: * 0.5, + 0.5, * 2r, - r): 8 u * range covers
    both.  Curves (3, 5) copy raw: exact."""
    return 8 * U * regress_scale(op, consts)


def param_bound_end_to_end(op, raw64, e_raw, consts):
    """|param_gpu - param64| allowed when raw itself is off by at most e_raw: through the regressor's derivative, plus
    param_bound."""
    return regress_slope_sup(op, raw64, e_raw, consts) * e_raw + param_bound(op, consts)


# ----------------------------------------------------------------------------------------------------------------------
# L1 and END-select L1
# ----------------------------------------------------------------------------------------------------------------------
L1_SIZES = (1, 3, 4, 5, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 8196, 12287, 12289, 64 * 3 * 128 * 128)
L1_REL_BOUND = 64 * U        # (52 + ceil(nblk / 256)) u: 32 adds per thread, 8 reduce levels, the finaliser's strided adds + 8
#                              levels, the subtraction, 1/n and the last product; nblk <= 384 at these sizes (53.5 u)


def l1_pair(n, seed):
    """pred, target: fp32 multiples of 2^-24 in [0, 1) (differences are exact, never denormal), with ties."""
    rng = np.random.default_rng(seed)
    p = rng.random(n, dtype=np.float32)
    t = rng.random(n, dtype=np.float32)
    tie = rng.random(n) < 0.1
    t[tie] = p[tie]
    return p, t


def l1_loss64(p, t):
    return float(np.abs(p.astype(np.float64) - t.astype(np.float64)).mean())


def l1_grad32(p, t, gloss):
    """sign(p - t) * fl32(gloss * fl32(1 / fl32(n))), the kernels' arithmetic in numpy fp32; ties give 0."""
    gs = np.float32(gloss) * (np.float32(1.0) / np.float32(p.size))
    return np.sign(p - t).astype(np.float32) * gs


# (name, B, T, sample shape, first): first is 'zero', 'last', 'mixed' or an explicit list
END_CASES = (
    ('scalar_3x5x7', 5, 2, (3, 5, 7), 'mixed'),                   # row 105, row % 4 = 1: k_end_l1_*<1>
    ('scalar_3x1x1', 7, 8, (3, 1, 1), 'mixed'),                   # row 3: a float4 would span two samples
    ('scalar_straddle', 3, 2, (3, 25, 33), [1, 0, 1]),            # row 2475: the forward's 2048-float workgroups cut samples
    ('b1_t1', 1, 1, (3, 5, 7), 'zero'),                           # one sample, one step image (scalar kernels)
    ('b1_t1_vec', 1, 1, (3, 4, 4), 'zero'),                       # ... and on the float4 kernels
    ('b1_t8', 1, 8, (3, 5, 7), [5]),                              # one sample, every other step image all zeros
    ('t1_b5', 5, 1, (3, 8, 8), 'zero'),
    ('t8_last', 4, 8, (3, 8, 8), 'last'),
    ('t8_zero', 4, 8, (3, 8, 8), 'zero'),
    ('vector_straddle', 30, 2, (3, 20, 12), 'mixed'),             # row 720, 21600 floats: 8192-float workgroups cut samples
    ('multi_wg', 6, 8, (3, 64, 64), [7, 0, 3, 3, 1, 6]),          # 73728 floats: 9 forward, 18 backward workgroups
)


def end_case(name):
    """-> (imgs: list of T (B, *shape) fp32 arrays, first (B,) int64, target).  A twentieth of the elements are ties; where
    B > 1 the selected image of sample 0 equals its target everywhere (with B = 1 that would leave nothing to check)."""
    _, B, T, shape, first = next(c for c in END_CASES if c[0] == name)
    rng = np.random.default_rng(sum(map(ord, name)))
    imgs = [rng.random((B,) + shape, dtype=np.float32) for _ in range(T)]
    tgt = rng.random((B,) + shape, dtype=np.float32)
    if first == 'zero':
        f = np.zeros(B, dtype=np.int64)
    elif first == 'last':
        f = np.full(B, T - 1, dtype=np.int64)
    elif first == 'mixed':
        f = (np.arange(B, dtype=np.int64) * 3 + 1) % T
    else:
        f = np.asarray(first, dtype=np.int64)
    tie = rng.random((B,) + shape) < 0.05
    for b in range(B):
        imgs[f[b]][b][tie[b]] = tgt[b][tie[b]]
    if B > 1:
        imgs[f[0]][0] = tgt[0]
    return imgs, f, tgt


def end_gather(imgs, first):
    return np.stack([imgs[first[b]][b] for b in range(len(first))])


# ----------------------------------------------------------------------------------------------------------------------
# Adam
# ----------------------------------------------------------------------------------------------------------------------
# The C ABI takes lr, beta1, beta2, eps as fp32: those fp32 values ARE the hyper-parameters (0.999f is 0.99900001287..., so
# 1 - beta2 is 1.3e-5 relative off 0.001); the reference evaluates the same formulas from them in fp64.
def hyper(lr, b1, b2, eps):
    return tuple(float(np.float32(v)) for v in (lr, b1, b2, eps))


ADAM_DEFAULT = hyper(1e-3, 0.9, 0.999, 1e-8)
ADAM_HYPERS = (ADAM_DEFAULT, hyper(3e-2, 0.5, 0.9, 1e-3), hyper(1e-5, 0.95, 0.9999, 1e-12))
ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_SIZES = (1, 2, 3, 4, 5, 7, 1023, 1025, 1026, 1027, 3073, 3074, 3075)
ADAM_BIG = 2 * 4 * 4096 * 256 + 1203             # every thread of the capped 4096-workgroup launch loops twice, then a 3-float tail
ADAM_GUARD = 8


def adam_state(n, seed):
    """p, g, m, v (fp32, n + ADAM_GUARD floats: the guard elements after n must stay untouched).  |g| spread over
    1e-8 .. 1e4 with exact zeros, m of g's size, v of g^2's; a tenth of the elements have m = v = g = 0."""
    rng = np.random.default_rng(seed)
    N = n + ADAM_GUARD
    mag = 10.0 ** rng.uniform(-8, 4, N)
    g = (mag * rng.choice([-1.0, 1.0], N)).astype(np.float32)
    m = (mag * rng.uniform(-1, 1, N)).astype(np.float32)
    v = (mag * mag * rng.uniform(0.0, 2.0, N)).astype(np.float32)
    p = rng.uniform(-2, 2, N).astype(np.float32)
    gz = rng.random(N) < 0.1
    g[gz] = 0.0
    allz = rng.random(N) < 0.1
    g[allz] = 0.0; m[allz] = 0.0; v[allz] = 0.0
    return p, g, m, v


def adam_reference(p, g, m, v, step, hp):
    """One Adam step in fp64 from fp32 state -> (p', m', v', bounds) with the per-element rounding counts of the issue:
         m' : 3 u (|m| + |g|)                         g - m, * (1 - b1), + m
         v' : 4 u v'                                  v * b2 | g * g, * (1 - b2) | +   (all terms non-negative)
         p' : 2 u |p'| + 16 u |D| + 8 u lr_c (|m| + |g|) / denom,   D = lr_c m' / denom the fp64 update."""
    lr, b1, b2, eps = hp
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    m1 = m + (g - m) * (1.0 - b1)
    v1 = v * b2 + g * g * (1.0 - b2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    lr_c = lr / bc1
    denom = np.sqrt(v1) / math.sqrt(bc2) + eps
    delta = lr_c * m1 / denom
    p1 = p - delta
    bounds = dict(m=3 * U * (np.abs(m) + np.abs(g)), v=4 * U * v1,
                  p=2 * U * np.abs(p1) + 16 * U * np.abs(delta) + 8 * U * lr_c * (np.abs(m) + np.abs(g)) / denom)
    return p1, m1, v1, bounds


def torch_adam_step(p, g, m, v, step, hp):
    """torch.optim.Adam(foreach=False) in fp32 on the CPU from the same state -> (p', m', v')."""
    lr, b1, b2, eps = hp
    q = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    q.grad = torch.from_numpy(g.copy())
    opt.state[q] = {'step': torch.tensor(float(step - 1)), 'exp_avg': torch.from_numpy(m.copy()), 'exp_avg_sq': torch.from_numpy(v.copy())}
    opt.step()
    st = opt.state[q]
    return q.detach().numpy(), st['exp_avg'].numpy(), st['exp_avg_sq'].numpy()


TRAJ_N, TRAJ_STEPS = 4099, 20


def adam_trajectory_inputs(seed=77):
    """p0 and 20 gradients (fp32), magnitudes spread over four decades per element, signs drifting."""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(-1, 1, TRAJ_N).astype(np.float32)
    mag = 10.0 ** rng.uniform(-3, 1, TRAJ_N)
    gs = [(mag * rng.normal(0.3, 1.0, TRAJ_N)).astype(np.float32) for _ in range(TRAJ_STEPS)]
    return p0, gs


def adam_trajectory64(p0, gs, hp):
    p = p0.astype(np.float64); m = np.zeros_like(p); v = np.zeros_like(p)
    lr, b1, b2, eps = hp
    for t, g in enumerate(gs, 1):
        g = g.astype(np.float64)
        m = m + (g - m) * (1.0 - b1)
        v = v * b2 + g * g * (1.0 - b2)
        p = p - (lr / (1.0 - b1 ** t)) * m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + eps)
    return p


def adam_trajectory_torch32(p0, gs, hp):
    lr, b1, b2, eps = hp
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    for g in gs:
        q.grad = torch.from_numpy(g.copy())
        opt.step()
    return q.detach().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# graph fills
# ----------------------------------------------------------------------------------------------------------------------
def fill_bytes(buf, offset, value, elem, width, height=1, pitch=0):
    """The memset node's semantics on a host byte array: `height` rows of `width` elements of `elem` bytes, rows `pitch`
    bytes apart, each element the low `elem` bytes of value (little endian)."""
    pat = np.frombuffer(int(value & ((1 << (8 * elem)) - 1)).to_bytes(elem, 'little'), dtype=np.uint8)
    for r in range(height):
        o = offset + r * pitch
        buf[o:o + width * elem] = np.tile(pat, width)
    return buf
