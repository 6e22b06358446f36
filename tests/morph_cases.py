"""Shared cases of the mask morph tests (tests/test_morph_cpu.py on the host emulation, tests/test_gpu_morph.py on the
kernels): the oracle -- the definition of include/t2onet_hip.h restated in numpy int64, the minimum of the squared distances
to every pixel of the set, with no separable pass and no threshold table --, plane patterns, and calls of up to 4 jobs laid
out in byte buffers with guard bytes around every plane.  Integers throughout: every comparison is exact."""
import numpy as np

GUARD = 0x5A
MODES = ('grow', 'shrink', 'border')
RADII = [0, 1, 2, 5, 25, 64]
INF = np.int64(1) << 40
COL_TILE, ROW_TILE = (64, 64), (8, 256)                      # (rows, columns) of the two passes' tiles (t2o_morph_math.h)


def sqdist(member):
    """(h, w) bool -> (h, w) int64: the least squared distance from each pixel to a True pixel, INF where there is none.
    Brute force over every (pixel, member) pair, in row chunks."""
    h, w = member.shape
    ys, xs = np.nonzero(member)
    out = np.full((h, w), INF, np.int64)
    if not len(ys):
        return out
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    rows = max(1, (1 << 22) // (w * len(ys)))
    X = np.arange(w, dtype=np.int64)
    for y0 in range(0, h, rows):
        Y = np.arange(y0, min(y0 + rows, h), dtype=np.int64)
        d = (Y[:, None, None] - ys) ** 2 + (X[None, :, None] - xs) ** 2
        out[y0:y0 + len(Y)] = d.min(-1)
    return out


_oracle = {}


def oracle(plane, radius, mode):
    """The definition: S = plane >= 128; GROW Dout <= R^2; SHRINK in S and Din > R^2; BORDER GROW and not SHRINK.  Computed
    once per (plane, radius, mode); the two distance maps once per plane."""
    assert plane.dtype == np.uint8 and plane.ndim == 2 and mode in MODES and 0 <= int(radius) <= 64
    pk = (plane.shape, plane.tobytes())
    key = pk + (int(radius), mode)
    if key not in _oracle:
        S = plane >= 128
        r2 = np.int64(radius) ** 2

        def dist(which):
            if pk + (which,) not in _oracle:
                _oracle[pk + (which,)] = sqdist(S if which == 'out' else ~S)
            return _oracle[pk + (which,)]
        grow = (dist('out') <= r2) if mode != 'shrink' else None
        shrink = (S & (dist('in') > r2)) if mode != 'grow' else None
        on = grow if mode == 'grow' else shrink if mode == 'shrink' else grow & ~shrink
        _oracle[key] = np.where(on, 255, 0).astype(np.uint8)
    return _oracle[key]


def disc_offsets(radius):
    """The lattice points of the closed disc, as a set of (dy, dx)."""
    return {(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if dy * dy + dx * dx <= radius * radius}


def corners(h, w):
    """A plane with single set pixels and a small block on the corners of both passes' tiles, as far as they lie inside."""
    m = np.zeros((h, w), np.uint8)
    for ty in (COL_TILE[0], 2 * COL_TILE[0], ROW_TILE[0]):
        for tx in (COL_TILE[1], ROW_TILE[1]):
            for y, x in ((ty - 1, tx - 1), (ty, tx), (ty - 1, tx), (ty, tx - 1)):
                if 0 <= y < h and 0 <= x < w and (y + x) % 2 == 0:
                    m[y, x] = 255
    m[0, 0] = m[h - 1, w - 1] = 200
    m[h // 3:h // 3 + 9, w // 4:w // 4 + 7] = 255
    return m


def blob(h, w, seed):
    """A wand-like blob that touches the top of the frame, a hole in it, and scattered specks."""
    yy, xx = np.mgrid[:h, :w]
    m = np.where((yy - h // 5) ** 2 * 4 + (xx - w // 2) ** 2 <= (w // 4) ** 2, 255, 0).astype(np.uint8)
    m[h // 6:h // 6 + 3, w // 2:w // 2 + 4] = 0
    rng = np.random.default_rng(seed)
    m[rng.integers(0, h, 12), rng.integers(0, w, 12)] = 255
    return m


def cases():
    """[(name, plane, radius, mode)]"""
    out = []
    rng = np.random.default_rng(5)
    # the radius exceeds the frame
    for n, (h, w) in enumerate([(1, 1), (1, 7), (7, 1), (2, 2), (5, 9)]):
        m = np.zeros((h, w), np.uint8)
        m[(h - 1) // 2, w - 1] = 255
        for mode in MODES:
            out.append(('tiny_%dx%d_%s' % (h, w, mode), m, 64, mode))
        out.append(('tiny_%dx%d_inverse' % (h, w), 255 - m, 64, MODES[n % 3]))
    # features on the tile corners, every mode, every radius
    for n, (h, w) in enumerate([(63, 65), (64, 64), (65, 63), (129, 67)]):
        m = corners(h, w)
        for k, mode in enumerate(MODES):
            out.append(('corner_%dx%d_%s' % (h, w, mode), m, RADII[(n + 2 * k) % 6], mode))
            out.append(('corner_%dx%d_%s_b' % (h, w, mode), m, RADII[(n + 2 * k + 3) % 6], mode))
    # one larger picture; the members of the set each job measures to are few, so brute force stays cheap
    big = blob(200, 136, 9)
    out.append(('big_200x136_grow', big, 5, 'grow'))
    out.append(('big_200x136_grow_25', big, 25, 'grow'))
    out.append(('big_200x136_inverse_shrink', 255 - big, 25, 'shrink'))
    wide = np.zeros((130, 200), np.uint8)
    wide[64, 150] = 255                                      # its disc of 64 crosses three tiles each way and the right frame edge
    out.append(('wide_130x200_grow', wide, 64, 'grow'))
    out.append(('wide_130x200_inverse_shrink', 255 - wide, 64, 'shrink'))
    # single pixels at the ends
    last = np.zeros((65, 63), np.uint8)
    last[-1, -1] = 255
    first = np.full((65, 63), 255, np.uint8)
    first[0, 0] = 0
    for mode, r in (('grow', 25), ('shrink', 1), ('border', 5)):
        out.append(('last_pixel_%s' % mode, last, r, mode))
        out.append(('first_unset_%s' % mode, first, r, mode))
    # constant planes, the threshold, a soft plane
    edge = np.where(rng.integers(0, 2, (33, 70)) == 1, 128, 127).astype(np.uint8)
    soft = rng.integers(1, 255, (40, 45)).astype(np.uint8)
    for k, mode in enumerate(MODES):
        out.append(('all_0_%s' % mode, np.zeros((20, 70), np.uint8), RADII[k + 1], mode))
        out.append(('all_255_%s' % mode, np.full((20, 70), 255, np.uint8), RADII[k + 3], mode))
        out.append(('threshold_%s' % mode, edge, (0, 1, 2)[k], mode))
        out.append(('soft_%s' % mode, soft, (2, 1, 0)[k], mode))
    # the discs the definition names
    for r in (25, 5):
        m = np.zeros((57, 59), np.uint8)
        m[28, 29] = 255
        out.append(('disc_%d' % r, m, r, 'grow'))
        out.append(('disc_%d_border' % r, m, r, 'border'))
    # a region that touches the frame, shrunk: the frame edge is no edge of the selection
    sky = np.zeros((40, 70), np.uint8)
    sky[:20, :] = 255
    sky[:, :9] = 255
    for r in (1, 5, 25):
        out.append(('frame_shrink_%d' % r, sky, r, 'shrink'))
    out.append(('frame_border_5', sky, 5, 'border'))
    assert len({c[0] for c in out}) == len(out)
    return out


class Call(object):
    """One morph_u8 call: .src / .out the byte buffers as they are before it (out is src for a call inside one buffer),
    .jobs = [(src_offset, out_offset, h, w, radius, mode)], .want = the destination buffer after it by the oracle."""

    def __init__(self, src, out, jobs):
        self.src, self.out, self.jobs = src, out, jobs
        self.want = out.copy()
        for so, oo, h, w, radius, mode in jobs:
            self.want[oo:oo + h * w] = oracle(src[so:so + h * w].reshape(h, w).copy(), radius, mode).reshape(-1)


def _place(pos, residue):
    while pos % 4 != residue:
        pos += 1
    return pos


def separate_call(group, first=0):
    """The planes of `group` (cases) in a source buffer at ODD offsets, their destinations in another buffer full of GUARD;
    job i's destination starts at residue (first + i) mod 4."""
    jobs, pos_s, pos_o = [], 1, 2
    for i, (_, m, radius, mode) in enumerate(group):
        so, oo = pos_s | 1, _place(pos_o, (first + i) % 4)
        jobs.append((so, oo) + m.shape + (radius, mode))
        pos_s, pos_o = so + m.size + 1, oo + m.size + 1          # one byte at least between two planes
    src = np.full(pos_s + 4, 0xC3, np.uint8)
    for (_, m, _, _), job in zip(group, jobs):
        src[job[0]:job[0] + m.size] = m.reshape(-1)
    return Call(src, np.full(pos_o + 4, GUARD, np.uint8), jobs)


def in_place_call(group, first=1):
    """Every job of `group` in place in ONE buffer: destination = source, GUARD between the planes."""
    jobs, pos = [], 1
    for i, (_, m, radius, mode) in enumerate(group):
        so = _place(pos, (first + i) % 4)
        jobs.append((so, so) + m.shape + (radius, mode))
        pos = so + m.size + 1
    buf = np.full(pos + 4, GUARD, np.uint8)
    for (_, m, _, _), job in zip(group, jobs):
        buf[job[0]:job[0] + m.size] = m.reshape(-1)
    return Call(buf, buf, jobs)


def shared_source_call():
    """Two jobs read the SAME source plane (a grow and a border of it), a third shrinks it in place."""
    m = corners(65, 63)
    n = m.size
    buf = np.full(3 + n + 2 + n + 5 + n + 8, GUARD, np.uint8)
    buf[3:3 + n] = m.reshape(-1)
    a, b = 3 + n + 2, 3 + n + 2 + n + 5
    return Call(buf, buf, [(3, a, 65, 63, 5, 'grow'), (3, b, 65, 63, 2, 'border'), (3, 3, 65, 63, 1, 'shrink')])


def calls():
    """Every case as a call of its own (sources at odd offsets, the destination residues walking through 0..3), then one
    call of 4 jobs with three sizes and three modes, one in place, and one whose jobs share a source: [(name, Call)]."""
    cs = cases()
    by_name = {c[0]: c for c in cs}
    out = [(c[0], separate_call([c], first=n)) for n, c in enumerate(cs)]
    four = [by_name[k] for k in ('corner_129x67_border', 'tiny_5x9_grow', 'disc_25', 'frame_shrink_5')]
    out.append(('four_jobs', separate_call(four, first=3)))
    out.append(('in_place', in_place_call([by_name['corner_65x63_grow'], by_name['big_200x136_inverse_shrink']])))
    out.append(('shared_source', shared_source_call()))
    return out
