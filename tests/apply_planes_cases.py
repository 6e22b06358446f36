"""Shared inputs of the apply_planes tests (tests/test_apply_planes_cpu.py, tests/test_gpu_apply_planes.py): a batch whose
samples run every supported operator and the identity row, a small plane stack with every kind of content, slot tables
that mix a plane, -1 and a number that is not a plane, and the shapes at which the per-sample launch changes path."""
import numpy as np
import torch

from oracle import synth

B, V, N = 9, 11, 5
OP_ID = np.array([0, 1, 2, 3, 5, 6, 7, -1, 6], np.int32)           # executor indices; -1 = identity
PRED_OP = (OP_ID + 3).astype(np.int64)                             # operator vocabulary ids: the identity row is END = 2
PLANES = ['box', 'count', 'zeros', 'ones', 'random']
# pointwise V = 4 + narrow strips; V = 4 + wide strips (two 248-column segments); V = 1 + LDS tiles, two tile rows, odd H*W;
# V = 4 + LDS tiles, two tile columns; a single ragged row, odd H*W
SHAPES = [(9, 20), (5, 260), (23, 19), (18, 66), (1, 7)]


def planes(H, W):
    """(N,H,W) uint8: a box with edges off the 4-pixel quads (box_mask of test_gpu_operator_masks.py), a count plane with
    0 / 1 / 2 (two overlapping regions), all zeros, all ones, a seeded hard random plane."""
    out = np.zeros((N, H, W), np.uint8)
    out[0, H // 4:H - H // 4, W // 4 + 1:W - W // 4] = 1
    out[1, :H - H // 3, :W - W // 3] += 1
    out[1, H // 3:, W // 3:] += 1
    out[3] = 1
    out[4] = (np.random.default_rng(1234 + 31 * H + W).random((H, W)) < 0.5).astype(np.uint8)
    return out


def slots(kind='mixed', pred_op=PRED_OP):
    """(B,V) int32.  'mixed': every sample's chosen column holds a plane, -1, or N (not a plane number: all ones), the other
    columns hold planes the call must not read for that sample; 'none': every entry -1."""
    s = np.full((B, V), -1, np.int32)
    if kind == 'none':
        return s
    rng = np.random.default_rng(77)
    s[:] = rng.integers(0, N, size=(B, V))
    chosen = [0, 1, 4, 2, N, 1, 3, -1, 0]        # brightness box, contrast count, saturation random, color zeros, tone "N",
    for b in range(B):                           # sharpness count, white ones, identity -1, sharpness box
        if 0 <= pred_op[b] < V:
            s[b, pred_op[b]] = chosen[b]
    return s


def pred_op_outside():
    """The extra case: one sample's operator id equals V (outside the table: all ones); its executor index stays valid."""
    p = PRED_OP.copy()
    p[0] = V
    return p


def tensors(H, W, seed=0):
    """img (B,3,H,W), param (B,24) -- each row holds its operator's parameters, zero padded -- and a seeded gout."""
    img = synth.images(B, H, W, 40 + seed)
    param = torch.zeros(B, 24)
    for b, op in enumerate(OP_ID):
        if op >= 0 and op != 7:
            p = synth.op_params(int(op), 1, 500 + 7 * b + seed, 'strong' if b % 2 else 'mid')
            param[b, :p.shape[1]] = p[0]
    g = torch.Generator().manual_seed(900 + seed)
    gout = torch.randn(B, 3, H, W, generator=g)
    return img, param, gout


def select_host(stack, slot, pred_op):
    """t2o_mask_select on the host: (B,1,H,W) float32 = float(byte) of the chosen plane, ones for no plane."""
    n, H, W = stack.shape
    out = np.ones((len(pred_op), 1, H, W), np.float32)
    for b, op in enumerate(pred_op):
        if 0 <= op < slot.shape[1] and 0 <= slot[b, op] < n:
            out[b, 0] = stack[slot[b, op]].astype(np.float32)
    return out
