"""The cases of the region kernels (t2o_region.hip) and their oracle, shared by tests/test_region_cpu.py and
tests/test_gpu_region.py.  The oracle is a breadth-first flood fill from the seed over Python ints -- it shares nothing
with the kernels' union-find -- and every comparison is byte for byte, guard bytes around every destination included.
The shapes are the smallest at which the labelling can go wrong: no size is a multiple of 4, 32 or 64 unless said."""
from collections import deque

import numpy as np

GUARD = 0xA5
TILE = 64                                                # the kernels' tile, which the shapes are chosen against
A, B = (200, 120, 40), (20, 30, 220)                     # the two colours of a drawn picture: far apart in every channel
TOL = 10                                                 # with a jitter of +-3 on colour A (a difference of 6 at most)


def passing(photo, sx, sy, tol):
    d = np.abs(photo.astype(np.int64) - photo[sy, sx].astype(np.int64)[None, None, :]).max(axis=2)
    return d <= tol


def oracle(photo, sx, sy, tol, conn):
    """(h, w) uint8: 255 where a path of passing pixels (4- or 8-connected steps) joins the pixel to the seed."""
    h, w = photo.shape[:2]
    assert 0 <= sx < w and 0 <= sy < h and 0 <= tol <= 255 and conn in (4, 8)
    ok = passing(photo, sx, sy, tol).reshape(-1).tolist()
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    seen = bytearray(h * w)
    seen[sy * w + sx] = 255
    queue = deque([(sy, sx)])
    while queue:
        y, x = queue.popleft()
        for dy, dx in steps:
            ny, nx = y + dy, x + dx
            if 0 <= ny < h and 0 <= nx < w:
                i = ny * w + nx
                if ok[i] and not seen[i]:
                    seen[i] = 255
                    queue.append((ny, nx))
    return np.frombuffer(bytes(seen), np.uint8).reshape(h, w).copy()


def paint(mask, seed=0):
    """A boolean picture as a photo: colour A (jittered by +-3 per channel) where mask, colour B elsewhere."""
    rng = np.random.default_rng(1000 + seed)
    jitter = rng.integers(-3, 4, mask.shape + (3,))
    return np.where(mask[:, :, None], np.array(A)[None, None, :] + jitter, np.array(B)[None, None, :]).astype(np.uint8)


# ---------------------------------------------------------------- the drawn pictures
def checkerboard(h, w):
    y, x = np.mgrid[:h, :w]
    return (y + x) % 2 == 0


def corner_blobs(anti):
    """Two blobs of 70 x 70 that touch at ONE diagonal corner, which is also the corner of four 64 x 64 tiles."""
    m = np.zeros((70, 70), bool)
    if anti:
        m[57:64, 64:69] = True                           # ends at (63, 64)
        m[64:68, 55:64] = True                           # starts at (64, 63)
    else:
        m[55:64, 58:64] = True                           # ends at (63, 63)
        m[64:69, 64:68] = True                           # starts at (64, 64)
    return m


def small_blobs():
    m = np.zeros((20, 23), bool)
    m[2:9, 2:10] = True
    m[9:16, 10:19] = True                                # (8, 9) and (9, 10) touch diagonally
    return m


def u_shape():
    m = np.zeros((67, 131), bool)
    m[2:, 5:21] = True
    m[2:, 100:121] = True
    m[66, 5:121] = True                                  # the arms meet along the bottom row only
    return m


def comb():
    m = np.zeros((70, 135), bool)
    for k in range(17):
        m[1:69, 2 + 8 * k:5 + 8 * k] = True
    m[68:70, 2:133] = True
    return m


def serpentine(h, w):
    """A one-pixel path through every second row, connectors at alternating ends."""
    m = np.zeros((h, w), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = True
    return m


def spiral(n):
    """A one-pixel square spiral from (0, 0) inward, one pixel of wall between the arms -> (mask, (y, x) of its inner end)."""
    m = np.zeros((n, n), bool)
    y = x = d = turns = 0
    m[0, 0] = True
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    while turns < 2:
        dy, dx = dirs[d]
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= fy < n and 0 <= fx < n and m[fy, fx]):
            y, x, turns = ny, nx, 0
            m[y, x] = True
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m, (y, x)


def ring_depth(h, w):
    y, x = np.mgrid[:h, :w]
    return np.minimum(np.minimum(y, x), np.minimum(h - 1 - y, w - 1 - x))


def rings(h, w):
    return ring_depth(h, w) // 2 % 2 == 0                # rings two pixels wide, two pixels apart


def noise(h, w, share, seed):
    return np.random.default_rng(seed).random((h, w)) < share


def isolated_pixel(m):
    """The first pixel of m (row-major) without a 4-neighbour in m, at least two pixels from the frame."""
    h, w = m.shape
    for y in range(2, h - 2):
        for x in range(2, w - 2):
            if m[y, x] and not (m[y - 1, x] or m[y + 1, x] or m[y, x - 1] or m[y, x + 1]):
                return y, x
    raise AssertionError('no isolated pixel')


NOISE_SEEDS = [(150, 150), (3, 297), (296, 5), (77, 211)]               # (x, y); a fifth one is isolated_pixel's


def tolerance_edges(tol=7):
    """12 x 5: a spine of the seed's colour down column 0; on every second row a pixel that differs by exactly tol in ONE
    channel (passes), then one that differs by tol + 1 (does not), then the seed's colour again (cut off) -> (photo, want)."""
    base = np.array([100, 110, 120])
    photo = np.empty((12, 5, 3), np.int64)
    photo[:] = np.array([250, 5, 250])
    photo[:, 0] = base
    for c, (ch, sign) in enumerate([(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)]):
        for x, d in [(1, tol), (2, tol + 1), (3, 0)]:
            photo[2 * c, x] = base
            photo[2 * c, x, ch] += sign * d
    want = np.zeros((12, 5), np.uint8)
    want[:, 0] = 255
    want[0::2, 1] = 255
    return photo.astype(np.uint8), want


def big_frame():
    """513 x 1027: serpentine above, 65 % noise below (above the threshold of 4 steps too), one pixel between them."""
    h, w = 513, 1027
    m = np.zeros((h, w), bool)
    m[:255] = serpentine(255, w)
    m[255, 700] = True
    m[256:] = noise(h - 256, w, 0.65, 91)
    m[256:261, 698:703] = True                           # a foothold, so that 4 steps get out of the joint too
    return m


# ---------------------------------------------------------------- the list
_cases = []


def cases():
    """[(name, photo (h, w, 3) uint8, seed_x, seed_y, tol, conn)].  Pictures that several cases share are ONE array."""
    if _cases:
        return _cases
    out = _cases

    def both(name, photo, sx, sy, tol=TOL):
        for conn in (4, 8):
            out.append(('%s_c%d' % (name, conn), photo, sx, sy, tol, conn))
    one = paint(np.ones((1, 1), bool))
    both('one_pixel', one, 0, 0)
    row = paint(np.array([[1, 1, 0, 1, 1, 1, 1]], bool), 1)
    out.append(('row_1x7_end', row, 6, 0, TOL, 4))
    out.append(('row_1x7_start', row, 0, 0, TOL, 8))
    col = paint(np.array([[1, 1, 0, 1, 1, 1, 1]], bool).T.copy(), 2)
    out.append(('col_7x1_start', col, 0, 0, TOL, 8))
    out.append(('col_7x1_end', col, 0, 6, TOL, 4))
    both('checker_5x6', paint(checkerboard(5, 6), 3), 0, 0)
    both('checker_65x67', paint(checkerboard(65, 67), 4), 0, 0)
    both('blobs_small', paint(small_blobs(), 5), 3, 3)
    both('blobs_corner', paint(corner_blobs(False), 6), 60, 60)
    both('blobs_anticorner', paint(corner_blobs(True), 7), 66, 60)
    both('u_shape', paint(u_shape(), 8), 10, 2)
    both('comb', paint(comb(), 9), 131, 1)
    serp = paint(serpentine(130, 197), 10)
    both('serpentine_far_end', serp, 196, 128)           # row 128 is entered at x = 0 (the 64th connector): its other end
    both('serpentine_wall', serp, 5, 1)
    sp, (cy, cx) = spiral(129)
    both('spiral', paint(sp, 11), cx, cy)
    both('rings', paint(rings(96, 160), 12), 20, 8)
    both('all_passing', np.random.default_rng(13).integers(0, 256, (257, 263, 3), dtype=np.uint8), 100, 200, 255)
    flat = np.random.default_rng(14).integers(0, 256, (45, 59, 3), dtype=np.uint8)
    flat[10:31, 12:41] = (77, 78, 79)
    both('tol0_patch', flat, 20, 15, 0)
    both('tolerance_edges', tolerance_edges()[0], 0, 0, 7)
    for share, seed in ((0.50, 50), (0.59, 59)):
        m = noise(300, 301, share, seed)
        photo = paint(m, seed)
        iy, ix = isolated_pixel(m)
        for k, (sx, sy) in enumerate(NOISE_SEEDS + [(ix, iy)]):
            both('noise%d_seed%d' % (seed, k), photo, sx, sy)
    big = paint(big_frame(), 15)
    out.append(('big_from_noise_c8', big, 700, 256, TOL, 8))
    out.append(('big_from_path_c4', big, 0, 0, TOL, 4))
    return out


_wants = {}


def want(name):
    """The oracle's plane of a case, computed once."""
    if name not in _wants:
        _, photo, sx, sy, tol, conn = next(c for c in cases() if c[0] == name)
        _wants[name] = oracle(photo, sx, sy, tol, conn)
    return _wants[name]


class Call:
    """One call of the entry point: .photo the buffer that holds the photos (each once, however many jobs read it), .out the
    destination buffer full of GUARD, .jobs = [(photo_offset, out_offset, h, w, seed_x, seed_y, tol, conn)], .names the cases,
    .want = the destination buffer after the call by the oracle."""

    def __init__(self, group, residues):
        photos, where, pos = [], {}, 1
        for (_, photo, *_), (rp, _) in zip(group, residues):
            if id(photo) not in where:
                while pos % 4 != rp:
                    pos += 1
                where[id(photo)] = pos
                photos.append((pos, photo))
                pos += photo.size + 1
        self.photo = np.full(pos + 4, 0x3C, np.uint8)
        for po, photo in photos:
            self.photo[po:po + photo.size] = photo.reshape(-1)
        self.jobs, self.names, pos = [], [], 2
        for (name, photo, sx, sy, tol, conn), (_, ro) in zip(group, residues):
            while pos % 4 != ro:
                pos += 1
            h, w = photo.shape[:2]
            self.jobs.append((where[id(photo)], pos, h, w, sx, sy, tol, conn))
            self.names.append(name)
            pos += h * w + 1                                         # one guard byte at least between two planes
        self.out = np.full(pos + 4, GUARD, np.uint8)
        self.want = self.out.copy()
        for name, (_, oo, h, w, *_) in zip(self.names, self.jobs):
            self.want[oo:oo + h * w] = want(name).reshape(-1)


_calls = []


def calls():
    """The cases four to a call, the residues of the photo and destination offsets rotating through 0..3; then the
    misaligned call (photo offsets 1, 2, 3 and destination offsets 1, 2, 3 modulo 4, odd widths) and the multi-job call
    (four jobs that differ in size, seed, tol and conn, two of them on one photo): [(name, Call)].  Built once."""
    if not _calls:
        cs = cases()
        for n, i in enumerate(range(0, len(cs), 4)):
            group = cs[i:i + 4]
            _calls.append(('call_%d' % n, Call(group, [((n + k) % 4, (n + 3 * k + 1) % 4) for k in range(len(group))])))
        by_name = {c[0]: c for c in cs}
        _calls.append(('misaligned', Call([by_name['checker_65x67_c8'], by_name['u_shape_c4'], by_name['serpentine_far_end_c4']],
                                          [(1, 3), (2, 1), (3, 2)])))
        _calls.append(('multi_job', multi_job()))
    return _calls


def multi_job():
    cs = {c[0]: c for c in cases()}
    name, photo, *_ = cs['noise50_seed0_c4']
    other = (name + '_again', photo, 40, 260, 3, 8)                  # the same photo: another seed, tol and conn
    _wants[other[0]] = oracle(photo, 40, 260, 3, 8)
    return Call([cs['noise50_seed0_c4'], cs['spiral_c8'], other, cs['tol0_patch_c4']], [(0, 1), (3, 0), (0, 2), (2, 3)])
