"""The cases of the fill kernels (t2o_fill.hip) and their oracle, shared by tests/test_fill_cpu.py and
tests/test_gpu_fill.py.  The oracle is int64 numpy over whole levels, written from the text of include/t2onet_hip.h -- it
shares nothing with the kernels' tiles, halos and packed cells -- and every comparison is byte for byte, guard bytes around
every destination included.  The shapes are chosen against the kernels' 64-pixel tile."""
import numpy as np

GUARD = 0xA5
TILE = 64                                                # the kernels' tile, which the shapes are chosen against
SOFT = (1, 97, 254)                                      # scattered soft bytes: not known, hardly / half / almost filled


def pyramid(photo, plane):
    """The pull of the header: ([C_0 .. C_K] int64 (h_k, w_k, 3) in sixteenths, 0 where unknown; [known_0 .. known_K] bool)."""
    P, M = photo.astype(np.int64), plane.astype(np.int64)
    known = [M == 0]
    C = [np.where(known[0][:, :, None], 16 * P, 0)]
    while known[-1].shape != (1, 1):
        hk, wk = known[-1].shape
        hn, wn = (hk + 1) // 2, (wk + 1) // 2
        c = np.zeros((2 * hn, 2 * wn, 3), np.int64)
        k = np.zeros((2 * hn, 2 * wn), np.int64)
        c[:hk, :wk] = C[-1] * known[-1][:, :, None]
        k[:hk, :wk] = known[-1]
        s = c.reshape(hn, 2, wn, 2, 3).sum(axis=(1, 3))
        n = k.reshape(hn, 2, wn, 2).sum(axis=(1, 3))
        nn = np.maximum(n, 1)[:, :, None]
        C.append(np.where(n[:, :, None] > 0, (s + nn // 2) // nn, 0))
        known.append(n > 0)
    return C, known


def oracle(photo, plane):
    """(h, w, 3) uint8: the photo with the pixels under the plane filled, as include/t2onet_hip.h defines it."""
    assert photo.dtype == np.uint8 and plane.dtype == np.uint8 and photo.shape == plane.shape + (3,)
    C, known = pyramid(photo, plane)
    if not known[-1][0, 0]:
        return photo.copy()
    F = C[-1]
    for k in range(len(C) - 2, -1, -1):
        (hk, wk), (hn, wn) = known[k].shape, known[k + 1].shape
        y, x = np.arange(hk), np.arange(wk)
        Y, X = y >> 1, x >> 1
        Yn = np.clip(Y + np.where(y & 1, 1, -1), 0, hn - 1)
        Xn = np.clip(X + np.where(x & 1, 1, -1), 0, wn - 1)
        U = (9 * F[Y][:, X] + 3 * F[Y][:, Xn] + 3 * F[Yn][:, X] + F[Yn][:, Xn] + 8) >> 4
        F = np.where(known[k][:, :, None], C[k], U)
    fill = (F + 8) >> 4
    P, M = photo.astype(np.int64), plane.astype(np.int64)[:, :, None]
    return np.where(M == 0, P, (P * (255 - M) + fill * M + 127) // 255).astype(np.uint8)


def noise(h, w, seed):
    return np.random.default_rng(2000 + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def scattered(h, w, seed, share=0.05):
    """About `share` of the bytes soft (1, 97 or 254), the rest 0."""
    rng = np.random.default_rng(3000 + seed)
    return np.where(rng.random((h, w)) < share, rng.choice(np.array(SOFT, np.uint8), (h, w)), 0).astype(np.uint8)


def corner_hole(h, w, seed):
    """Scattered soft bytes and a hard rectangular hole across the tile corner at (64, 64), as far as the picture reaches."""
    m = scattered(h, w, seed)
    m[52:77, 49:81] = 255
    return m


_cases = []


def cases():
    """[(name, photo (h, w, 3) uint8, plane (h, w) uint8)], built once."""
    if _cases:
        return _cases
    out = _cases
    one = noise(1, 1, 0)
    out.append(('one_pixel_known', one, np.zeros((1, 1), np.uint8)))
    out.append(('one_pixel_unknown', one, np.full((1, 1), 200, np.uint8)))
    out.append(('row_1x7', noise(1, 7, 1), np.array([[0, 255, 255, 97, 0, 255, 1]], np.uint8)))
    out.append(('col_7x1', noise(7, 1, 2), np.array([[255, 255, 0, 254, 255, 255, 255]], np.uint8).T.copy()))
    two = noise(2, 2, 3)
    for y in (0, 1):
        for x in (0, 1):
            m = np.full((2, 2), 255, np.uint8)
            m[y, x] = 0
            m[1 - y, 1 - x] = 128
            out.append(('two_by_two_known_%d%d' % (y, x), two, m))
    for k, (h, w) in enumerate([(63, 65), (64, 64), (65, 63), (129, 67)]):
        out.append(('corner_%dx%d' % (h, w), noise(h, w, 10 + k), corner_hole(h, w, 10 + k)))
    m = scattered(200, 136, 20)
    m[64:128, 64:128] = 255                                          # a whole aligned tile: its cell of level 6 is unknown
    out.append(('tile_200x136', noise(200, 136, 20), m))
    m = scattered(300, 521, 21)
    m[0:256, 0:256] = 255                                            # cells of levels 7 and 8 are unknown
    m[250:300, 440:521] = 255                                        # and a hole on the ragged bottom-right border tiles
    out.append(('big_300x521', noise(300, 521, 21), m))
    m = np.full((130, 70), 255, np.uint8)
    m[40:90, 10:60] = 31
    m[129, 69] = 0
    out.append(('last_pixel_130x70', noise(130, 70, 22), m))
    out.append(('all_255_70x66', noise(70, 66, 23), np.full((70, 66), 255, np.uint8)))
    soft = scattered(70, 66, 24, 0.5)
    soft[soft == 0] = 3
    out.append(('none_known_70x66', noise(70, 66, 24), soft))
    out.append(('all_0_70x66', noise(70, 66, 25), np.zeros((70, 66), np.uint8)))
    return out


_wants = {}


def want(name):
    """The oracle's picture of a case, computed once."""
    if name not in _wants:
        _, photo, plane = next(c for c in cases() if c[0] == name)
        _wants[name] = oracle(photo, plane)
    return _wants[name]


class Call:
    """One call of the entry point: .photo the buffer that holds the photos (each once, however many jobs read it) at odd
    offsets, .planes the buffer of the planes at odd offsets, .out the destination buffer full of GUARD -- or, with `same`,
    None: the destinations are room full of GUARD behind the photos IN .photo, and a job of `in_place` has its own photo as
    its destination.  .jobs = [(photo_offset, plane_offset, out_offset, h, w)], .names the cases, .want = the destination
    buffer after the call by the oracle."""

    def __init__(self, group, residues, same=False, in_place=()):
        photos, where, pos = [], {}, 1
        for _, photo, _ in group:
            if id(photo) not in where:
                where[id(photo)] = pos
                photos.append((pos, photo))
                pos += photo.size + 1
                pos += 1 - pos % 2                                   # odd offsets
        photo_end = pos
        planes, at, ppos = [], {}, 3
        for _, _, plane in group:
            if id(plane) not in at:
                at[id(plane)] = ppos
                planes.append((ppos, plane))
                ppos += plane.size + 2
                ppos += 1 - ppos % 2
        self.planes = np.full(ppos + 4, 0x3C, np.uint8)
        for po, plane in planes:
            self.planes[po:po + plane.size] = plane.reshape(-1)
        self.jobs, self.names, pos = [], [], (photo_end + 2 if same else 2)
        for k, ((name, photo, plane), ro) in enumerate(zip(group, residues)):
            h, w = plane.shape
            if k in in_place:
                assert same
                self.jobs.append((where[id(photo)], at[id(plane)], where[id(photo)], h, w))
            else:
                while pos % 4 != ro:
                    pos += 1
                self.jobs.append((where[id(photo)], at[id(plane)], pos, h, w))
                pos += photo.size + 1                                # one guard byte at least between two destinations
            self.names.append(name)
        self.same = same
        self.photo = np.full((pos if same else photo_end) + 4, GUARD if same else 0x3C, np.uint8)
        for po, photo in photos:
            self.photo[po:po + photo.size] = photo.reshape(-1)
        self.out = None if same else np.full(pos + 4, GUARD, np.uint8)
        self.want = (self.photo if same else self.out).copy()
        for name, (_, _, oo, h, w) in zip(self.names, self.jobs):
            self.want[oo:oo + 3 * h * w] = want(name).reshape(-1)


_calls = []


def calls():
    """Every case as a call of its own, the residue of the destination offset rotating through 0..3; then the multi-job
    call: [(name, Call)].  Built once."""
    if not _calls:
        for n, case in enumerate(cases()):
            _calls.append((case[0], Call([case], [(n + 1) % 4])))
        _calls.append(('multi_job', multi_job()))
    return _calls


def multi_job():
    """Four jobs of different sizes in ONE buffer: two share a photo (under different planes, both written elsewhere), one
    other job runs in place on its photo."""
    cs = {c[0]: c for c in cases()}
    name, photo, plane = cs['corner_129x67']
    other_plane = np.zeros((129, 67), np.uint8)
    other_plane[30:100, 20:50] = 255
    other = (name + '_again', photo, other_plane)
    _wants[other[0]] = oracle(photo, other_plane)
    return Call([cs['corner_129x67'], cs['tile_200x136'], other, cs['row_1x7']], [1, 0, 3, 2], same=True, in_place=(1,))
