"""Shared cases of the 8-bit replay tests (tests/test_replay_cpu.py on the host emulation, tests/test_gpu_replay.py on the
kernel): pictures, operator lists with their parameters, the fp32 oracle and the per-byte interval condition."""
import numpy as np
import torch

TILE = 32                                       # kReplayTile of t2onet_amd/csrc/t2o_replay_math.h (asserted by the CPU test)
SIZES = [(1, 1), (1, 7), (9, 1), (37, 50), (TILE - 1, TILE + 1), (TILE + 1, 2 * TILE + 1)]
BOUND = 1e-5                                    # what the chain tests hold against the same oracle (tests/test_gpu_operators.py:288,361)

# name -> (ops, forced parameter of single-parameter steps or None)
LISTS = {
    'brightness': ([0], None), 'contrast': ([1], None), 'saturation': ([2], None), 'color': ([3], None),
    'tone': ([5], None), 'sharpness': ([6], None), 'white': ([7], None),
    'sharp_first': ([6, 0, 1, 3, 5], None), 'sharp_middle': ([0, 1, 6, 3, 5], None), 'sharp_last': ([0, 2, 3, 5, 6], None),
    'with_end': ([0, -1, 5, 6], None), 'end_only': ([-1], None),
    'steps0': ([], None), 'steps8': ([1, 0, 2, 3, 5, 6, 1, 0], None),
    # parameters that drive the clamp: below 0 and above 1
    'clamp_sharp': ([6], 1.5), 'clamp_bright_up': ([0], 2.0), 'clamp_bright_down': ([0], -2.0),
    'clamp_contrast_neg': ([1], -1.0), 'clamp_contrast_pos': ([1], 1.0), 'clamp_chain': ([1, 6, 0], 1.5),
}


def picture(h, w, seed):
    """Seeded noise holding exact 0, exact 255 and grey (r = g = b) pixels."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h * w, 3), dtype=np.uint8)
    idx = np.arange(h * w)
    img[idx % 5 == 0] = img[idx % 5 == 0][:, :1]            # grey
    img[idx % 11 == 3] = 0
    img[idx % 13 == 4] = 255
    return np.ascontiguousarray(img.reshape(h, w, 3))


def params_for(ops, seed, forced=None):
    """(8, 24) float32 parameter rows for `ops` inside each operator's range (oracle.cpu_ref.param_range)."""
    rng = np.random.default_rng(seed)
    p = np.zeros((8, 24), np.float32)
    for k, op in enumerate(ops):
        if op == 3:
            p[k] = rng.uniform(0.9, 1.1, 24)
        elif op == 5:
            p[k, :8] = rng.uniform(0.5, 2.0, 8)
        elif op >= 0:
            lo, hi = {0: (-0.5, 0.5), 1: (-0.6, 0.6), 2: (-0.2, 0.8), 6: (0.2, 1.2), 7: (0.0, 1.0)}[op]
            p[k, 0] = rng.uniform(lo, hi) if forced is None else forced
    return p


def oracle(img, ops, params):
    """The fp32 oracle's image BEFORE quantisation, (3, h, w) float32: / 255, then Executor.execute per step."""
    from oracle import cpu_ref
    x = torch.from_numpy(img.astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)).unsqueeze(0)
    n = cpu_ref.OP_NPARAM
    rows = [None if op < 0 else torch.from_numpy(params[k:k + 1, :n[op]].copy()) for k, op in enumerate(ops)]
    out, _ = cpu_ref.run_sequence(x, list(ops), rows, cpu_ref.default_opt())
    assert out.dtype == torch.float32
    return out[0].numpy()


def interval(o):
    """Per byte: trunc(255 (o - 1e-5)) .. trunc(255 (o + 1e-5)), as (h, w, 3) integer arrays."""
    o = o.astype(np.float64).transpose(1, 2, 0)
    return np.trunc(255.0 * (o - BOUND)).astype(np.int64), np.trunc(255.0 * (o + BOUND)).astype(np.int64)


def assert_in_interval(got_hwc, o, what=''):
    lo, hi = interval(o)
    g = got_hwc.astype(np.int64)
    bad = (g < lo) | (g > hi)
    assert not bad.any(), '%s: %d bytes outside the oracle interval, first at %s: got %d, allowed %d..%d (o = %r)' % (
        what, int(bad.sum()), tuple(np.argwhere(bad)[0]), g[bad][0], lo[bad][0], hi[bad][0], o.transpose(1, 2, 0)[bad][0])
