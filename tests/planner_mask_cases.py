"""Cases shared by tests/test_planner_mask_cpu.py (host emulation) and tests/test_gpu_planner_mask.py (device): the mask
planes the masked planner kernels are held to, as uint8 counts -- what functional.rle_union_u8 / gier.MaskTable make."""
import numpy as np

SHAPES = [(1, 1), (37, 53), (64, 64)]
PLANES = ['zeros', 'ones', 'blob', 'twos']


def _disc(h, w, cy, cx, r):
    """An ellipse around (cy, cx) * (h, w) with half axes r * (h, w): r = 0.326 covers pi r^2 = a third of the plane."""
    yy, xx = np.mgrid[:h, :w]
    return (((yy + 0.5) / h - cy) ** 2 + ((xx + 0.5) / w - cx) ** 2 <= r * r).astype(np.uint8)


def plane(name, h, w):
    """(h, w) uint8: all 0, all 1, a 0/1 blob of about a third of the pixels, or two overlapping blobs summed (0 / 1 / 2)."""
    if name == 'zeros':
        return np.zeros((h, w), np.uint8)
    if name == 'ones':
        return np.ones((h, w), np.uint8)
    if name == 'blob':
        return _disc(h, w, 0.5, 0.5, 0.326)
    if name == 'twos':
        m = _disc(h, w, 0.4, 0.4, 0.3) + _disc(h, w, 0.6, 0.6, 0.3)
        if h * w == 1:
            m[:] = 2
        return m
    raise KeyError(name)


def planes(h, w):
    """The four planes stacked (4, h, w): plane k starts at byte k h w -- odd for odd h w."""
    return np.stack([plane(n, h, w) for n in PLANES])
