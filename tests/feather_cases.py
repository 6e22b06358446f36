"""Shared cases of the mask feather tests (tests/test_feather_cpu.py on the host emulation, tests/test_gpu_feather.py on
the kernels): the numpy int64 oracle of the arithmetic in include/t2onet_hip.h, plane patterns, and calls of up to 4 jobs
laid out in byte buffers with guard bytes around every plane.  Integers throughout: every comparison is exact."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A
SIGMAS = [0, 0.1, 0.5, 2.5, 7, 20, 64]
PATTERNS = ['zeros', 'full', 'random', 'vedge', 'hedge', 'one_pixel', 'border']


def tile_constants():
    """kFeatherRowW, kFeatherRowH, kFeatherColW, kFeatherColH as t2o_feather_math.h declares them."""
    with open(os.path.join(ROOT, 't2onet_amd', 'csrc', 't2o_feather_math.h')) as f:
        text = f.read()
    return {k: int(v) for k, v in re.findall(r'\b(kFeather(?:Row|Col)[WH]) = (\d+)', text)}


TILES = tile_constants()
assert sorted(TILES) == ['kFeatherColH', 'kFeatherColW', 'kFeatherRowH', 'kFeatherRowW'], TILES
# two tiles plus one pixel in each direction, of whichever pass has the larger tile
BIG = (2 * max(TILES['kFeatherRowH'], TILES['kFeatherColH']) + 1, 2 * max(TILES['kFeatherRowW'], TILES['kFeatherColW']) + 1)
SIZES = [(1, 1), (1, 7), (7, 1), (5, 9), (33, 65), BIG]


def plane(pattern, h, w, seed=0):
    m = np.zeros((h, w), np.uint8)
    if pattern == 'full':
        m[:] = 255
    elif pattern == 'random':
        m[:] = np.random.default_rng(2000 + seed).integers(0, 256, (h, w), dtype=np.uint8)
    elif pattern == 'vedge':                                     # a hard vertical edge: left of it 0, from it on 255
        m[:, w // 2:] = 255
    elif pattern == 'hedge':
        m[h // 2:, :] = 255
    elif pattern == 'one_pixel':
        m[h // 2, w // 2] = 255
    elif pattern == 'border':
        m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 255
    else:
        assert pattern == 'zeros', pattern
    return m


def weights_int(sigma):
    """functional.feather_weights as int64 with the centre of the copy (R = 0) at its true value 65536."""
    import t2onet_amd.functional as T
    w = T.feather_weights(sigma).astype(np.int64)
    if len(w) == 1:
        assert w[0] == 0                                         # 65536 modulo 2^16
        w[0] = 65536
    assert w[0] + 2 * w[1:].sum() == 65536 and (w >= 0).all()
    return w


_oracle = {}


def oracle(m, sigma):
    """The definition in int64: row pass, (a + 128) >> 8, column pass, (b + 2^23) >> 24, replicated borders; both
    accumulator bounds asserted.  Computed once per (plane, sigma)."""
    key = (m.shape, float(sigma), m.tobytes())
    if key not in _oracle:
        w = weights_int(sigma)
        R = len(w) - 1
        taps = np.concatenate([w[:0:-1], w])                     # w_R .. w_1 w_0 w_1 .. w_R
        h, wd = m.shape
        mp = np.pad(m.astype(np.int64), ((0, 0), (R, R)), mode='edge')
        a = np.zeros((h, wd), np.int64)
        for k, t in enumerate(taps):
            a += t * mp[:, k:k + wd]
        assert a.min() >= 0 and a.max() <= 255 * 65536
        t16 = (a + 128) >> 8
        assert t16.max() <= 65280
        tp = np.pad(t16, ((R, R), (0, 0)), mode='edge')
        b = np.zeros((h, wd), np.int64)
        for k, t in enumerate(taps):
            b += t * tp[k:k + h, :]
        assert b.min() >= 0 and b.max() <= 65280 * 65536 and b.max() + (1 << 23) < (1 << 32)
        out = (b + (1 << 23)) >> 24
        assert out.max() <= 255
        _oracle[key] = out.astype(np.uint8)
    return _oracle[key]


def specs():
    """Every size with every sigma, the patterns walking along (each size meets all seven): (h, w, sigma, pattern, seed)."""
    out = []
    for s, (h, w) in enumerate(SIZES):
        for g, sigma in enumerate(SIGMAS):
            out.append((h, w, sigma, PATTERNS[(s + g) % len(PATTERNS)], 10 * s + g))
    return out


class Call(object):
    """One feather_u8 call: .src / .out the byte buffers as they are before it (out is src for a call inside one buffer),
    .jobs = [(src_offset, out_offset, h, w, sigma)], .want = the destination buffer after it by the oracle."""

    def __init__(self, src, out, jobs):
        self.src, self.out, self.jobs = src, out, jobs
        self.want = out.copy()
        for so, oo, h, w, sigma in jobs:
            self.want[oo:oo + h * w] = oracle(src[so:so + h * w].reshape(h, w), sigma).reshape(-1)


def _place(pos, residue):
    while pos % 4 != residue:
        pos += 1
    return pos


def separate_call(group, first=0):
    """The planes of `group` (specs) in a source buffer, their destinations in another one full of GUARD; job i's source
    starts at residue (first + i) mod 4 and its destination at residue (first + 2 i + 1) mod 4."""
    planes = [plane(p, h, w, seed) for h, w, _, p, seed in group]
    jobs, pos_s, pos_o = [], 1, 2
    for i, (m, (h, w, sigma, _, _)) in enumerate(zip(planes, group)):
        so, oo = _place(pos_s, (first + i) % 4), _place(pos_o, (first + 2 * i + 1) % 4)
        jobs.append((so, oo, h, w, sigma))
        pos_s, pos_o = so + m.size + 1, oo + m.size + 1              # one byte at least between two planes
    src = np.full(pos_s + 4, 0xC3, np.uint8)
    for m, (so, _, _, _, _) in zip(planes, jobs):
        src[so:so + m.size] = m.reshape(-1)
    return Call(src, np.full(pos_o + 4, GUARD, np.uint8), jobs)


def in_place_call(group, first=0):
    """Every job of `group` in place in ONE buffer: destination = source, GUARD between the planes."""
    planes = [plane(p, h, w, seed) for h, w, _, p, seed in group]
    jobs, pos = [], 1
    for i, (m, (h, w, sigma, _, _)) in enumerate(zip(planes, group)):
        so = _place(pos, (first + i) % 4)
        jobs.append((so, so, h, w, sigma))
        pos = so + m.size + 1
    buf = np.full(pos + 4, GUARD, np.uint8)
    for m, (so, _, _, _, _) in zip(planes, jobs):
        buf[so:so + m.size] = m.reshape(-1)
    return Call(buf, buf, jobs)


def overlap_call():
    """One buffer of random bytes; job 0 writes a 33 x 65 plane over the first rows of the plane that job 1 READS (job 1
    writes elsewhere), and job 2 is in place: every job must see the bytes from before the call."""
    h, w = 33, 65
    n = h * w
    a = 3
    b = a + n + 2                                                # job 0's destination
    s1 = b + 5 * w + 3                                           # job 1's source: starts inside it, ends behind it
    o1 = s1 + n + 6
    d = o1 + n + 5
    buf = np.random.default_rng(77).integers(0, 256, d + 9 * 31 + 8, dtype=np.uint8)
    jobs = [(a, b, h, w, 2.5), (s1, o1, h, w, 7), (d, d, 9, 31, 20)]
    assert b < s1 < b + n < s1 + n
    return Call(buf, buf, jobs)


def calls():
    """The specs four to a call (mixed sizes and sigmas in one call), alternately into a separate output and in place,
    then the overlapping call: [(name, Call)]."""
    sp = specs()
    assert np.gcd(11, len(sp)) == 1
    order = [sp[(11 * i) % len(sp)] for i in range(len(sp))]        # neighbours in specs() share a size: a call mixes sizes
    out = []
    for n, i in enumerate(range(0, len(order), 4)):
        group = order[i:i + 4]
        make = in_place_call if n % 3 == 2 else separate_call
        out.append(('%s_%d' % (make.__name__, n), make(group, first=n)))
    out.append(('overlap_call', overlap_call()))
    return out
