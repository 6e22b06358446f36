"""Shared cases of the mask refine tests (tests/test_refine_cpu.py on the host emulation, tests/test_gpu_refine.py on the
kernels): the numpy int64 oracle of the arithmetic in include/t2onet_hip.h, photo and plane patterns, and calls of up to 4
jobs laid out in byte buffers with guard bytes around every photo, plane and destination.  Integers throughout: every
comparison is exact."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A
F = 10
RADII = [0, 1, 2, 7, 64]
EPS2 = [1, 26, 65025]
PATTERNS = ['random', 'step', 'anti', 'contrast1', 'zeros', 'full', 'const127']


def tile_constants():
    """kRefineRowW, kRefineRowH, kRefineColW, kRefineColH as t2o_refine_math.h declares them."""
    with open(os.path.join(ROOT, 't2onet_amd', 'csrc', 't2o_refine_math.h')) as f:
        text = f.read()
    return {k: int(v) for k, v in re.findall(r'\b(kRefine(?:Row|Col)[WH]) = (\d+)', text)}


TILES = tile_constants()
assert sorted(TILES) == ['kRefineColH', 'kRefineColW', 'kRefineRowH', 'kRefineRowW'], TILES
# one pixel past a tile of the row passes in each direction, and of the column passes
SIZES = [(1, 1), (1, 5), (3, 1), (5, 7), (37, 53), (64, 64), (TILES['kRefineRowH'] + 1, TILES['kRefineRowW'] + 1),
         (TILES['kRefineColH'] + 1, TILES['kRefineColW'] + 1)]


def lum(rgb):
    """The guide: t2o_select_u8's luminance of an (h, w, 3) uint8 picture, int64."""
    c = rgb.astype(np.int64)
    return (69 * c[..., 0] + 172 * c[..., 1] + 15 * c[..., 2] + 128) >> 8


def box(a, r):
    """(2r+1)^2 box sums of an int64 (h, w) array with replicated borders."""
    h, w = a.shape
    k = 2 * r + 1
    p = a[np.clip(np.arange(-r, h + r), 0, h - 1)][:, np.clip(np.arange(-r, w + r), 0, w - 1)]
    c = np.zeros((h + k, w + k), np.int64)
    c[1:, 1:] = p.cumsum(0).cumsum(1)
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


_oracle = {}
PEAK = {'A': 0, 'num': 0}                                       # the largest |A| and 64-bit intermediate any oracle call met


def refine(I, p, r, E):
    """The definition on int64 arrays (h, w); every bound of the header asserted."""
    n = (2 * r + 1) ** 2
    SI, Sp, SII, SIp = box(I, r), box(p, r), box(I * I, r), box(I * p, r)
    assert max(SI.max(), Sp.max(), SII.max(), SIp.max()) < 1 << 31
    den = n * SII - SI * SI + E * n * n
    assert den.min() > 0
    num = 2 * (n * SIp - SI * Sp) * (1 << F) + den
    assert np.abs(num).max() < 9.3e15
    A = num // (2 * den)
    assert np.abs(A).max() <= 65281
    B = (2 * ((Sp << F) - A * SI) + n) // (2 * n)
    assert np.abs(B).max() < 1.7e7
    TA = box(A, r)
    assert np.abs(TA).max() < 1 << 31
    d = n << F
    PEAK['A'] = max(PEAK['A'], int(np.abs(A).max()))
    PEAK['num'] = max(PEAK['num'], int(np.abs(num).max()))
    return np.clip((2 * (TA * I + box(B, r)) + d) // (2 * d), 0, 255).astype(np.uint8)


def oracle(rgb, plane, r, E):
    """refine of a uint8 (h, w, 3) photo and a uint8 (h, w) plane; computed once per input."""
    key = (rgb.shape, int(r), int(E), rgb.tobytes(), plane.tobytes())
    if key not in _oracle:
        _oracle[key] = refine(lum(rgb), plane.astype(np.int64), int(r), int(E))
    return _oracle[key]


def grey(v):
    """An (h, w) array of luminances -> an (h, w, 3) photo whose luminance is exactly v (R = G = B: 69 + 172 + 15 = 256)."""
    return np.repeat(np.asarray(v, np.uint8)[..., None], 3, -1)


def case(pattern, h, w, seed=0):
    """(photo (h, w, 3) uint8, plane (h, w) uint8) of a pattern."""
    rng = np.random.default_rng(3000 + seed)
    photo = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    plane = np.zeros((h, w), np.uint8)
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    if pattern == 'random':
        plane[:] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif pattern == 'step':                                      # a full-contrast guide edge, the plane's step 3 px beside it
        photo = grey(np.where(x >= w // 2, 230, 20))
        plane[:] = np.where(x >= w // 2 + 3, 255, 0)
    elif pattern == 'anti':                                      # the plane falls where the guide rises: cov, A, numerators < 0
        photo = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        plane[:] = 255 - lum(photo)
        plane[::3, ::2] = 0
    elif pattern == 'contrast1':                                 # a guide step of ONE byte under a 0/255 plane: the largest |A| at E = 1
        photo = grey(np.where(x >= w // 2, 101, 100))
        plane[:] = np.where(x >= w // 2, 255, 0)
    elif pattern == 'full':
        plane[:] = 255
    elif pattern == 'const127':
        plane[:] = 127
    else:
        assert pattern == 'zeros', pattern
    return photo, plane


def specs():
    """Every size with every radius, E and the patterns walking along: (h, w, r, E, pattern, seed).  'contrast1' runs at
    E = 1, where |A| is largest; the two mid sizes also meet it at every radius."""
    out = []
    for s, (h, w) in enumerate(SIZES):
        for g, r in enumerate(RADII):
            pattern = PATTERNS[(2 * s + g) % len(PATTERNS)]
            out.append((h, w, r, 1 if pattern == 'contrast1' else EPS2[(s + g) % 3], pattern, 10 * s + g))
    for h, w in [(37, 53), (64, 64)]:
        for g, r in enumerate(RADII):
            out.append((h, w, r, 1, 'contrast1', 100 + g))
            out.append((h, w, r, EPS2[g % 3], 'anti', 200 + g))
    return out


class Call(object):
    """One refine_u8 call: .photo / .src / .out the byte buffers as they are before it (out is src for a call inside one
    buffer), .jobs = [(photo_offset, src_offset, out_offset, h, w, radius, eps2)], .want = the destination buffer after it
    by the oracle."""

    def __init__(self, photo, src, out, jobs):
        self.photo, self.src, self.out, self.jobs = photo, src, out, jobs
        self.want = out.copy()
        for po, so, oo, h, w, r, E in jobs:
            self.want[oo:oo + h * w] = oracle(photo[po:po + 3 * h * w].reshape(h, w, 3), src[so:so + h * w].reshape(h, w), r, E).reshape(-1)


def _place(pos, residue):
    while pos % 4 != residue:
        pos += 1
    return pos


def _photo_buffer(photos, residues):
    offsets, pos = [], 1
    for im, res in zip(photos, residues):
        po = _place(pos, res)
        offsets.append(po)
        pos = po + im.size + 1
    buf = np.full(pos + 4, 0x3C, np.uint8)
    for im, po in zip(photos, offsets):
        buf[po:po + im.size] = im.reshape(-1)
    return buf, offsets


def separate_call(group, residues=None, first=0):
    """The photos of `group` (specs) in one buffer, the planes in another, the destinations in a third full of GUARD.
    residues: per job (photo, source, destination) address residues modulo 4; by default they rotate with `first`."""
    made = [case(p, h, w, seed) for h, w, _, _, p, seed in group]
    if residues is None:
        residues = [((first + i) % 4, (first + 2 * i + 1) % 4, (first + 3 * i + 2) % 4) for i in range(len(group))]
    photo, pos_ = _photo_buffer([m[0] for m in made], [r[0] for r in residues])
    jobs, pos_s, pos_o = [], 1, 2
    for (_, m), po, (h, w, r, E, _, _), res in zip(made, pos_, group, residues):
        so, oo = _place(pos_s, res[1]), _place(pos_o, res[2])
        jobs.append((po, so, oo, h, w, r, E))
        pos_s, pos_o = so + m.size + 1, oo + m.size + 1              # one byte at least between two planes
    src = np.full(pos_s + 4, 0xC3, np.uint8)
    for (_, m), job in zip(made, jobs):
        src[job[1]:job[1] + m.size] = m.reshape(-1)
    return Call(photo, src, np.full(pos_o + 4, GUARD, np.uint8), jobs)


def in_place_call(group, first=0):
    """Every job of `group` in place in ONE plane buffer: destination = source, GUARD between the planes."""
    made = [case(p, h, w, seed) for h, w, _, _, p, seed in group]
    photo, pos_ = _photo_buffer([m[0] for m in made], [(first + 3 * i) % 4 for i in range(len(group))])
    jobs, pos = [], 1
    for i, ((_, m), po, (h, w, r, E, _, _)) in enumerate(zip(made, pos_, group)):
        so = _place(pos, (first + i) % 4)
        jobs.append((po, so, so, h, w, r, E))
        pos = so + m.size + 1
    buf = np.full(pos + 4, GUARD, np.uint8)
    for (_, m), job in zip(made, jobs):
        buf[job[1]:job[1] + m.size] = m.reshape(-1)
    return Call(photo, buf, buf, jobs)


def mixed_call():
    """FOUR mixed jobs in one plane buffer of random bytes: job 0 writes a 37 x 53 plane over the first rows of the plane
    that job 1 READS (job 1 writes elsewhere), job 2 runs in place, job 3 is a small one at radius 64: every job must see
    the bytes from before the call.  The photos lie in a buffer of their own."""
    h, w = 37, 53
    n = h * w
    rng = np.random.default_rng(78)
    photos = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), case('step', h, w, 1)[0], rng.integers(0, 256, (9, 31, 3), dtype=np.uint8),
              rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)]
    photo, po = _photo_buffer(photos, [1, 2, 3, 0])
    a = 3
    b = a + n + 2                                                # job 0's destination
    s1 = b + 5 * w + 3                                           # job 1's source: starts inside it, ends behind it
    o1 = s1 + n + 6
    d = o1 + n + 5                                               # job 2, in place
    e = d + 9 * 31 + 2
    f = e + 35 + 1
    buf = rng.integers(0, 256, f + 35 + 8, dtype=np.uint8)
    jobs = [(po[0], a, b, h, w, 2, 26), (po[1], s1, o1, h, w, 7, 1), (po[2], d, d, 9, 31, 1, 65025), (po[3], e, f, 5, 7, 64, 26)]
    assert b < s1 < b + n < s1 + n
    return Call(photo, buf, buf, jobs)


def residue_calls():
    """The two smallest sizes at 16 residue triples each, four jobs to a call: every residue of every one of the three
    offsets, in varied combinations."""
    out = []
    for s, (h, w) in enumerate(SIZES[:2]):
        triples = [(k % 4, k // 4, (k + k // 4 + 1) % 4) for k in range(16)]
        for i in range(0, 16, 4):
            group = [(h, w, RADII[(i + q) % len(RADII)], EPS2[q % 3], 'random', 300 + 16 * s + i + q) for q in range(4)]
            out.append(('residues_%dx%d_%d' % (h, w, i // 4), separate_call(group, triples[i:i + 4])))
    return out


_calls = []


def calls():
    """The specs four to a call (mixed sizes and radii in one call), alternately into a separate output and in place, the
    residue calls, then the mixed call: [(name, Call)].  Built once."""
    if not _calls:
        sp = specs()
        assert np.gcd(7, len(sp)) == 1
        order = [sp[(7 * i) % len(sp)] for i in range(len(sp))]         # neighbours in specs() share a size: a call mixes sizes
        for n, i in enumerate(range(0, len(order), 4)):
            group = order[i:i + 4]
            make = in_place_call if n % 3 == 2 else separate_call
            _calls.append(('%s_%d' % (make.__name__, n), make(group, first=n)))
        _calls.extend(residue_calls())
        _calls.append(('mixed_call', mixed_call()))
    return _calls
