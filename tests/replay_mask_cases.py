"""Shared cases of the MASKED 8-bit replay tests (tests/test_replay_mask_cpu.py on the host emulation,
tests/test_gpu_replay_mask.py on the kernel): mask patterns, operator lists with the steps that name a mask, the fp32
oracle with masks.  Pictures, parameters, sizes and the per-byte interval condition are tests/replay_cases.py's."""
import numpy as np
import torch

from tests import replay_cases as RC

PATTERNS = ['zeros', 'full', 'soft', 'blocks', 'one_pixel', 'border']
T = RC.TILE


def mask(pattern, h, w, seed=0):
    """(h, w) uint8 mask plane: 0 leaves a pixel, 255 applies the operator."""
    m = np.zeros((h, w), np.uint8)
    if pattern == 'full':
        m[:] = 255
    elif pattern == 'soft':
        m[:] = np.random.default_rng(1000 + seed).integers(0, 256, (h, w), dtype=np.uint8)
    elif pattern == 'blocks':
        # 0/255 rectangles with edges at 31, 32 and 33 in both directions: on both sides of a tile border
        m[:T - 1, :T + 1] = 255
        m[T:, T - 1:] = 255
        m[T + 1:, :T] = 255
    elif pattern == 'one_pixel':
        y, x = (T, T) if h > T and w > T else (h - 1, w - 1)
        m[y, x] = 255
    elif pattern == 'border':
        m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 255
    else:
        assert pattern == 'zeros', pattern
    return m


def _sharp(name, k):
    ops = RC.LISTS[name][0]
    return ops, [0 if i == k else -1 for i in range(len(ops))]


# name -> (ops, mask_of): mask_of[k] = which of the case's masks (0 = the pattern's, 1 = a second pattern's) step k
# names, -1 = none.  The operators are RC.LISTS'.  sharp_first has no step in front of its sharpness and sharp_last none
# behind it: those two of the nine sharpness variants do not exist.
LISTS = {
    'm_brightness': ([0], [0]), 'm_contrast': ([1], [0]), 'm_saturation': ([2], [0]), 'm_color': ([3], [0]),
    'm_tone': ([5], [0]), 'm_sharpness': ([6], [0]), 'm_white': ([7], [0]),
    'sharp_first_self': _sharp('sharp_first', 0), 'sharp_first_behind': _sharp('sharp_first', 2),
    'sharp_middle_front': _sharp('sharp_middle', 1), 'sharp_middle_self': _sharp('sharp_middle', 2),
    'sharp_middle_behind': _sharp('sharp_middle', 3),
    'sharp_last_front': _sharp('sharp_last', 1), 'sharp_last_self': _sharp('sharp_last', 4),
    'two_masks': (RC.LISTS['sharp_middle'][0], [0, -1, -1, 1, -1]),
    'with_end_masked': (RC.LISTS['with_end'][0], [-1, -1, 0, -1]),
    'steps8_masked': (RC.LISTS['steps8'][0], [0] * 8),
}
NAMES = sorted(LISTS)
assert LISTS['sharp_first_self'][0][0] == 6 and LISTS['sharp_middle_self'][0][2] == 6 and LISTS['sharp_last_self'][0][4] == 6
assert LISTS['with_end_masked'][0][1] == -1


def masks_for(name, pattern, h, w, seed=0):
    """The mask planes a case needs: the pattern's, and for a list with a second mask the NEXT pattern's."""
    n = max(LISTS[name][1]) + 1
    return [mask(PATTERNS[(PATTERNS.index(pattern) + i) % len(PATTERNS)], h, w, seed + i) for i in range(n)]


def mask_f32(m):
    """(1, 1, h, w) float32 = byte / 255, as the kernel converts it."""
    return torch.from_numpy(m.astype(np.float32) / np.float32(255.0))[None, None]


def oracle(img, ops, params, mask_of, planes):
    """The fp32 oracle's image BEFORE quantisation, (3, h, w) float32: / 255, then Executor.execute per step with the
    mask operand ((1, 1, h, w) fp32, None for unmasked steps)."""
    from oracle import cpu_ref
    x = torch.from_numpy(img.astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)).unsqueeze(0)
    n = cpu_ref.OP_NPARAM
    rows = [None if op < 0 else torch.from_numpy(params[k:k + 1, :n[op]].copy()) for k, op in enumerate(ops)]
    masks = [None if i < 0 else mask_f32(planes[i]) for i in mask_of]
    out, _ = cpu_ref.run_sequence(x, list(ops), rows, cpu_ref.default_opt(), masks=masks)
    assert out.dtype == torch.float32
    return out[0].numpy()


def pack_masks(planes, first_pad=1):
    """The planes back to back in one buffer, each at another residue modulo 4, 0xA5 between them ->
    (buffer, offsets)."""
    pos, offsets = first_pad, []
    for i, m in enumerate(planes):
        offsets.append(pos)
        pos += m.size + 1 + 2 * (i % 2)
    buf = np.full(pos + 4, 0xA5, np.uint8)
    for off, m in zip(offsets, planes):
        buf[off:off + m.size] = m.reshape(-1)
    return buf, offsets
