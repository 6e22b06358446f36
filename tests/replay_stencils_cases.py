"""Shared cases of the stencils replay tests (tests/test_replay_stencils_cpu.py on the host emulation,
tests/test_gpu_replay_stencils.py on the kernel): operator lists that repeat the sharpness, their sizes and mask cases.
Pictures, parameters, the oracle and the per-byte interval condition are tests/replay_cases.py's, the mask patterns
tests/replay_mask_cases.py's."""
import numpy as np

from tests import replay_cases as RC
from tests import replay_mask_cases as MC

# a 1 x 1 picture under an 8-pixel ring, pictures narrower than the ring, tile edges inside the picture, 31/33-pixel sides
SIZES = list(RC.SIZES) + [(3, 3), (40, 70), (65, 33)]

# name -> operator list
LISTS = {
    'ss': [6, 6], 's_b_s': [6, 0, 6], 'c_ss_b': [1, 6, 6, 0], 's_end_s': [6, -1, 6], 'three': [0, 6, 1, 6, 3, 6, 5],
    'five': [6, 0, 6, 1, 6, 5, 6, 6], 'eight': [6] * 8, 'white_ss': [7, 6, 6],
    'none': [0, 1, 3, 5, 7], 'one': [0, 1, 6, 3, 5],               # the new kernel serves these too
}
NAMES = sorted(LISTS)
# the lists the oracle interval is asked of: at most two sharpness steps, their parameter forced to 0.3 (a sharpness
# multiplies an error by up to 1 + 8 p; the fp32 oracle's own distance from fp64 stays under 1.7e-6 for these)
ORACLE_NAMES = ['ss', 's_b_s', 'c_ss_b']
ORACLE_SHARP = 0.3

# mask cases: name -> (pattern of mask 0, which steps name a mask: a function of the list -> mask_of)
def _all0(ops):
    return [0] * len(ops)


def _sharp_only(ops):
    return [0 if op == 6 else -1 for op in ops]


def _front_of_sharp(ops):
    """Mask 0 on every step that stands directly in front of a sharpness (none: on the first step)."""
    m = [0 if k + 1 < len(ops) and ops[k + 1] == 6 else -1 for k in range(len(ops))]
    return m if 0 in m else [0] + [-1] * (len(ops) - 1)


def _two(ops):
    """Two planes: sharpness steps under mask 0, every other step under mask 1."""
    return [0 if op == 6 else 1 for op in ops]


MASK_CASES = {
    'soft_all': ('soft', _all0), 'blocks_all': ('blocks', _all0), 'zeros_all': ('zeros', _all0), 'full_all': ('full', _all0),
    'soft_sharp': ('soft', _sharp_only), 'blocks_sharp': ('blocks', _sharp_only),
    'soft_front': ('soft', _front_of_sharp), 'blocks_front': ('blocks', _front_of_sharp),
    'two_planes': ('blocks', _two),
}
MASK_NAMES = sorted(MASK_CASES)


# white turns the zeros outside the picture into ones: with a sharpness parameter above 0 the clamp hides which of the
# two the stencil read at the picture's border (1 + p > 1 either way), with one below 0 it shows
FORCED_SHARP = {'white_ss': -0.15}


def params_for(name, seed, sharp=None):
    """RC.params_for with every sharpness row forced to `sharp` when given (default: FORCED_SHARP's for the list)."""
    ops = LISTS[name]
    p = RC.params_for(ops, seed)
    sharp = FORCED_SHARP.get(name) if sharp is None else sharp
    if sharp is not None:
        for k, op in enumerate(ops):
            if op == 6:
                p[k, 0] = sharp
    return p


def mask_case(name, case, h, w, seed=0):
    """-> (mask_of, planes) of list `name` under mask case `case` on an (h, w) picture."""
    pattern, rule = MASK_CASES[case]
    mask_of = rule(LISTS[name])
    planes = [MC.mask(pattern, h, w, seed)]
    if max(mask_of) == 1:
        planes.append(MC.mask('soft', h, w, seed + 1))
    return mask_of, planes


def numpy_chain(img, ops, params):
    """An independent fp32 restatement for unmasked lists of white (7), identity (-1) and sharpness (6): full-image
    arrays, np.pad with zeros, the stencil in sharp_delta's order ((((-up) - left) + 4 c) - right) - down, clip after
    each step.  Returns (3, h, w) float32 before quantisation."""
    f = np.float32
    x = img.astype(f).transpose(2, 0, 1) / f(255.0)
    for k, op in enumerate(ops):
        if op == 6:
            z = np.pad(x, ((0, 0), (1, 1), (1, 1)))
            c, up, le, ri, dn = z[:, 1:-1, 1:-1], z[:, :-2, 1:-1], z[:, 1:-1, :-2], z[:, 1:-1, 2:], z[:, 2:, 1:-1]
            x = c + f(params[k, 0]) * (((((-up) - le) + f(4.0) * c) - ri) - dn)
        elif op == 7:
            x = np.ones_like(x)
        else:
            assert op == -1, op
        assert x.dtype == f
        x = np.clip(x, f(0), f(1))
    return x
