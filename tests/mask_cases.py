"""Cases shared by tests/test_mask_cpu.py (host emulation) and tests/test_gpu_mask.py (device): run-length masks, union jobs
laid out in one byte buffer with guard bytes, and the numpy oracle of what every byte of that buffer must hold."""
import numpy as np

from t2onet_amd import gier
from t2onet_amd.edit import nearest_index

SRC_SIZES = [(7, 5), (33, 47), (64, 64), (101, 67)]
OUT_SIZES = [(1, 1), (5, 9), (32, 32), (50, 75), (128, 128)]
PATTERNS = ['empty', 'full', 'pixel', 'stripes', 'blob_a', 'blob_b']
GUARD = 0xA5
# indices into PATTERNS: empty selection, single ones, overlapping blobs (-> 2), with the full mask (-> 3), a repeated id
SELECTIONS = [[], [0], [1], [2], [3], [4], [4, 5], [4, 5, 1], [4, 4, 5], [5, 5, 5]]


def blob(h, w, rng):
    """A smooth random region: a few discs, clipped to the plane."""
    yy, xx = np.mgrid[:h, :w]
    m = np.zeros((h, w), bool)
    for _ in range(3):
        cy, cx, r = rng.random() * h, rng.random() * w, (0.15 + 0.25 * rng.random()) * max(h, w)
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m.astype(np.uint8)


def pattern(name, h, w, seed):
    rng = np.random.default_rng(seed)
    if name == 'empty':
        return np.zeros((h, w), np.uint8)
    if name == 'full':
        return np.ones((h, w), np.uint8)
    if name == 'pixel':
        m = np.zeros((h, w), np.uint8)
        m[h // 2, w // 3] = 1
        return m
    if name == 'stripes':
        m = np.zeros((h, w), np.uint8)
        m[:, 1::2] = 1
        return m
    return blob(h, w, rng)


def mask_set(h, w, seed=0):
    """The six patterns at one source size -> (planes, RLE dicts): compressed strings and uncompressed lists alternate."""
    planes = [pattern(n, h, w, seed + 7 * k) for k, n in enumerate(PATTERNS)]
    planes[5] = planes[5].copy()
    planes[5][::2] |= planes[4][::2]                            # blob_b overlaps blob_a on the even rows
    rles = []
    for k, p in enumerate(planes):
        counts = gier.rle_encode(p)
        rles.append({'size': [h, w], 'counts': gier.rle_to_string(counts) if k % 2 == 0 else [int(c) for c in counts]})
    return planes, rles


def union_oracle(planes, ids, oh, ow):
    """decode -> nearest_index on both axes -> boolean planes at ids -> sum -> uint8, on already decoded planes."""
    out = np.zeros((oh, ow), np.int64)
    for i in ids:
        p = planes[i]
        out += (p[nearest_index(p.shape[0], oh)][:, nearest_index(p.shape[1], ow)] != 0)
    return out.astype(np.uint8)


def layout(specs, base_align=0, gaps=None):
    """specs: [(mask indices, oh, ow)].  Planes laid out one after the other with `gaps[i]` guard bytes in front of plane
    i (default: 0, 1, 2, 3, 0, ... so that planes abut and start at every byte alignment) after `base_align` leading bytes
    -> (jobs for rle_union_u8, total bytes)."""
    pos, jobs = base_align, []
    for i, (ids, oh, ow) in enumerate(specs):
        pos += (i % 4) if gaps is None else gaps[i]
        jobs.append((list(ids), pos, oh, ow))
        pos += oh * ow
    return jobs, pos + 5


def expected_buffer(planes, jobs, total):
    buf = np.full(total, GUARD, np.uint8)
    for ids, off, oh, ow in jobs:
        buf[off:off + oh * ow] = union_oracle(planes, ids, oh, ow).reshape(-1)
    return buf


def source_case(src, align):
    """Every output size x every selection for the mask set of one source size, the first plane at byte alignment `align`."""
    planes, rles = mask_set(*src, seed=src[0])
    specs = [(sel, oh, ow) for (oh, ow) in OUT_SIZES for sel in SELECTIONS]
    jobs, total = layout(specs, base_align=align)
    return planes, rles, jobs, total


def mixed_case(n_jobs, seed=0):
    """n_jobs planes of mixed output sizes over masks of ALL source sizes in one table; planes abut at odd offsets."""
    rng = np.random.default_rng(seed)
    planes, rles, first = [], [], []
    for src in SRC_SIZES:
        p, r = mask_set(*src, seed=src[1])
        first.append(len(planes))
        planes += p
        rles += r
    specs = []
    for j in range(n_jobs):
        f = first[j % len(SRC_SIZES)]
        sel = [f + k for k in SELECTIONS[(j * 3 + 1) % len(SELECTIONS)]]
        if j % 5 == 4:
            sel.append(first[(j + 1) % len(SRC_SIZES)] + 4)             # masks of two source sizes in one union
        oh, ow = OUT_SIZES[int(rng.integers(len(OUT_SIZES)))] if n_jobs > 1 else (50, 75)
        specs.append((sel, oh, ow))
    jobs, total = layout(specs, base_align=1, gaps=[int(g) for g in rng.integers(0, 4, n_jobs)])
    return planes, rles, jobs, total


def gt_mask_reference(mask_dict, ops, H, W):
    """Actor.get_gt_mask(...)[:, :1] for float masks, in numpy: the entry of str(op) when there is one, else ones."""
    out = np.ones((len(mask_dict), 1, H, W), np.float32)
    for b, entry in enumerate(mask_dict):
        v = entry.get(str(int(ops[b])))
        if v is not None:
            out[b, 0] = np.asarray(v[0], np.float32).reshape(H, W)
    return out
