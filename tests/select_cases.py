"""Shared cases of the selection tests (tests/test_select_cpu.py on the host emulation, tests/test_gpu_select.py on the
kernel): the numpy int64 oracle of the definition in include/t2onet_hip.h, the host rounding of user units, pictures, and
calls of up to 4 jobs laid out in byte buffers with guard bytes around every destination plane.  Integers throughout:
every comparison is exact."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A
KINDS = ('lum', 'sat', 'hue', 'linear', 'radial', 'plane')
HUE_STEPS = 1536


def tile_px():
    """kSelectTilePx as t2o_select_math.h declares it: the pixels of the stream that one workgroup owns."""
    with open(os.path.join(ROOT, 't2onet_amd', 'csrc', 't2o_select_math.h')) as f:
        text = f.read()
    c = {k: int(v) for k, v in re.findall(r'\b(kSelect(?:Threads|Iter)) = (\d+)', text)}
    return 4 * c['kSelectThreads'] * c['kSelectIter']


TILE = tile_px()
SIZES = [(1, 1), (1, 5), (3, 1), (5, 7), (37, 53), (64, 64), (1, TILE + 1), (TILE + 1, 1)]      # one pixel beyond a tile, both ways


# ---------------------------------------------------------------- the definition, int64
def measures(rgb):
    """rgb: integer array (..., 3) -> (L, S, H) int64; H = -1 where it is undefined."""
    c = np.asarray(rgb).astype(np.int64)
    R, G, B = c[..., 0], c[..., 1], c[..., 2]
    L = (69 * R + 172 * G + 15 * B + 128) >> 8
    mx, mn = c.max(-1), c.min(-1)
    d = mx - mn
    S = np.where(mx == 0, 0, (255 * d + mx // 2) // np.maximum(mx, 1))
    is_r, is_g = mx == R, (mx != R) & (mx == G)
    n = np.where(is_r, G - B, np.where(is_g, B - R, R - G))
    base = np.where(is_r, 0, np.where(is_g, 512, 1024))
    ds = np.maximum(d, 1)
    q = (512 * (n + ds) + ds) // (2 * ds) - 256
    H = np.where(d == 0, -1, (base + q) % HUE_STEPS)
    return L, S, H


def ramp(dist, soft):
    dist = np.asarray(dist, np.int64)
    if soft == 0:
        return np.where(dist == 0, 255, 0).astype(np.int64)
    mid = (255 * (soft - dist) + soft // 2) // soft
    return np.where(dist <= 0, 255, np.where(dist >= soft, 0, mid)).astype(np.int64)


def hue_weight(term, H):
    """The weight of a hue term, inversion left out, for hues H (int64, -1 = undefined)."""
    lo, hi, soft = [int(x) for x in term[2:]] if len(term) == 5 else [int(x) for x in term[2:]] + [0]
    span, rel = (hi - lo) % HUE_STEPS, (H - lo) % HUE_STEPS
    dist = np.where(rel <= span, 0, np.minimum(rel - span, HUE_STEPS - rel))
    return np.where(H < 0, 0, ramp(dist, soft))


def term_weight(term, img, src=None):
    """One integer term (kind, invert, values...) on the uint8 (h, w, 3) picture -> int64 (h, w) in 0..255, inversion
    applied.  src: the byte buffer a 'plane' term's offset counts from."""
    kind, invert, v = term[0], int(term[1]), [int(x) for x in term[2:]]
    kind = KINDS[kind] if not isinstance(kind, str) else kind
    h, w = img.shape[:2]
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    if kind in ('lum', 'sat'):
        lo, hi, soft = v if len(v) == 3 else v + [0]
        val = measures(img)[0 if kind == 'lum' else 1]
        t = ramp(np.where(val < lo, lo - val, np.where(val > hi, val - hi, 0)), soft)
    elif kind == 'hue':
        t = hue_weight((kind, 0) + tuple(v), measures(img)[2])
    elif kind == 'linear':
        X0, Y0, X1, Y1 = v
        DX, DY = X1 - X0, Y1 - Y0
        num, den = (x - X0) * DX + (y - Y0) * DY, DX * DX + DY * DY
        assert den > 0
        t = np.where(num <= 0, 255, np.where(num >= den, 0, (255 * (den - num) + den // 2) // den))
    elif kind == 'radial':
        CX, CY, RI, RO = v
        assert 0 <= RI < RO
        d2, den = (x - CX) ** 2 + (y - CY) ** 2, RO * RO - RI * RI
        t = np.where(d2 <= RI * RI, 255, np.where(d2 >= RO * RO, 0, (255 * (RO * RO - d2) + den // 2) // den))
    else:
        assert kind == 'plane', kind
        t = src[v[0]:v[0] + h * w].reshape(h, w).astype(np.int64)
    t = t.astype(np.int64)
    assert t.min() >= 0 and t.max() <= 255
    return 255 - t if invert else t


def selection(terms, img, src=None):
    """The plane of a selection: uint8 (h, w)."""
    assert 1 <= len(terms) <= 4
    m = term_weight(terms[0], img, src)
    for term in terms[1:]:
        m = (m * term_weight(term, img, src) + 127) // 255
    assert m.min() >= 0 and m.max() <= 255
    return m.astype(np.uint8)


# ---------------------------------------------------------------- user units -> integers
def rnd(v, scale):
    return int(math.floor(float(v) * scale + 0.5))


def round_units(terms, h, w):
    """Terms in user units, ('[!]kind', values...) -> integer terms (kind, invert, values...) for an (h, w) photo:
    floor(v * scale + 0.5) in double; lum / sat fractions * 255; hue degrees * 1536 / 360 modulo 1536 (the softness not
    wrapped); positions fractions of w - 1 and h - 1; radii fractions of min(h, w)."""
    out = []
    for term in terms:
        kind, v = term[0].lstrip('!'), list(term[1:])
        invert = int(term[0].startswith('!'))
        if kind in ('lum', 'sat'):
            v = v if len(v) == 3 else v + [0.0]
            out.append((kind, invert) + tuple(rnd(a, 255.0) for a in v))
        elif kind == 'hue':
            v = v if len(v) == 3 else v + [0.0]
            out.append((kind, invert, rnd(v[0], 1536.0 / 360.0) % HUE_STEPS, rnd(v[1], 1536.0 / 360.0) % HUE_STEPS, rnd(v[2], 1536.0 / 360.0)))
        elif kind == 'linear':
            out.append((kind, invert, rnd(v[0], w - 1), rnd(v[1], h - 1), rnd(v[2], w - 1), rnd(v[3], h - 1)))
        else:
            assert kind == 'radial', kind
            out.append((kind, invert, rnd(v[0], w - 1), rnd(v[1], h - 1), rnd(v[2], min(h, w)), rnd(v[3], min(h, w))))
    return out


# ---------------------------------------------------------------- pictures and selections
def picture(h, w, seed=0):
    """Random bytes with, where they fit, a black pixel (mx = 0), grey and white ones (hue undefined) and the six primaries."""
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    special = [(0, 0, 0), (77, 77, 77), (255, 255, 255), (255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 255, 255), (0, 0, 255),
               (255, 0, 255), (255, 0, 1), (1, 1, 0)]
    flat = img.reshape(-1, 3)
    for k, c in enumerate(special[:max(0, (h * w) // 2)]):
        flat[(7 * k) % (h * w)] = c
    return img


def selections(h, w, plane):
    """[(name, integer terms)] for an (h, w) job whose plane term (random bytes) lies at byte `plane` of the source: every
    kind plain and inverted, a wrapping hue arc, soft = 0, a four-term product, a rule under a painted plane."""
    m = min(h, w)
    lum, sat, hue = ('lum', 0, 128, 255, 32), ('sat', 0, 0, 96, 48), ('hue', 0, 1365, 171, 128)
    lin, rad = ('linear', 0, 0, 0, w - 2, h - 2), ('radial', 0, w // 2, h // 2, m // 8, m // 2 + 1)
    return [('lum', [lum]), ('sat', [sat]), ('hue_wrap', [hue]), ('linear', [lin]), ('radial', [rad]),
            ('not_lum', [('lum', 1, 40, 90, 100)]), ('not_sat', [('sat', 1, 128, 255, 100)]), ('not_hue', [('hue', 1, 300, 900, 768)]),
            ('not_linear', [('linear', 1, w, h // 3, -1, (2 * h) // 3)]), ('not_radial', [('radial', 1, 0, h - 1, 1, max(h, w) // 2 + 2)]),
            ('hue_step', [('hue', 0, 427, 853, 0)]), ('lum_step', [('lum', 0, 64, 191, 0)]), ('sat_point', [('sat', 0, 255, 255, 200)]),
            ('plane', [('plane', 0, plane)]), ('not_plane', [('plane', 1, plane)]),
            ('four', [lum, ('sat', 1, 0, 96, 48), hue, lin]), ('plane_radial', [('plane', 0, plane), rad]),
            ('far', [('linear', 0, -131070, 131070, 131070, -131070), ('radial', 1, 131070, 0, 1000, 131070)])]


NAMES = [n for n, _ in selections(8, 8, 0)]


class Call(object):
    """One select_u8 call: .src the source bytes, .out the destination buffer as it is before the call (GUARD everywhere),
    .jobs = [(src_offset, out_offset, h, w, terms)], .names, .want = the destination buffer after it by the oracle."""

    def __init__(self, src, out, jobs, names):
        self.src, self.out, self.jobs, self.names = src, out, jobs, names
        self.want = out.copy()
        for so, oo, h, w, terms in jobs:
            img = src[so:so + 3 * h * w].reshape(h, w, 3)
            self.want[oo:oo + h * w] = selection(terms, img, src).reshape(-1)


def _place(pos, residue):
    while pos % 4 != residue:
        pos += 1
    return pos


def build_call(group, residues, seed, shared=False):
    """group: [(h, w, selection name)]; residues: [(source offset mod 4, destination offset mod 4)] per job.  Every job gets
    its own photo and its own random plane in the source -- with `shared` all jobs read at the FIRST job's photo offset (a
    smaller job takes the leading bytes as its own h x w picture).  Noise between the source's parts, GUARD around every
    destination plane."""
    rng = np.random.default_rng(1000 + seed)
    parts, jobs, names, pos_s, pos_o = [], [], [], 1, 2
    for i, ((h, w, name), (rs, ro)) in enumerate(zip(group, residues)):
        n = h * w
        if shared and i:
            so = jobs[0][0]
            assert 3 * n <= 3 * jobs[0][2] * jobs[0][3]
        else:
            so = _place(pos_s, rs)
            parts.append((so, picture(h, w, seed * 10 + i).reshape(-1)))
            pos_s = so + 3 * n + 1
        po = _place(pos_s, (rs + ro + i) % 4)
        plane = rng.integers(0, 256, n, dtype=np.uint8)
        plane[:3] = (0, 255, 128)[:n]
        parts.append((po, plane))
        pos_s = po + n + 1
        oo = _place(pos_o, ro)
        pos_o = oo + n + 1                                           # one byte at least between two planes
        jobs.append((so, oo, h, w, dict(selections(h, w, po))[name]))
        names.append(name)
    src = rng.integers(0, 256, pos_s + 4, dtype=np.uint8)
    for at, data in parts:
        src[at:at + data.size] = data
    return Call(src, np.full(pos_o + 4, GUARD, np.uint8), jobs, names)


def specs():
    """Every size with every selection: (h, w, name)."""
    return [(h, w, name) for h, w in SIZES for name in NAMES]


_calls = None


def calls():
    """[(name, Call)]: the specs four to a call (mixed sizes in one call), the residues of both offsets walking along;
    a sweep of all 16 residue pairs on 5 x 7 and 37 x 53 with a four-term selection and with a plane under a rule; and
    one call of 4 jobs of different sizes that share one photo.  Built once."""
    global _calls
    if _calls is None:
        sp = specs()
        assert np.gcd(19, len(sp)) == 1
        order = [sp[(19 * i) % len(sp)] for i in range(len(sp))]     # neighbours in specs() share a size: a call mixes sizes
        out = []
        for n, i in enumerate(range(0, len(order), 4)):
            out.append(('mixed_%d' % n, build_call(order[i:i + 4], [((n + k) % 4, (n // 4 + 2 * k + 1) % 4) for k in range(4)], n)))
        for rs in range(4):
            group = [(5, 7, 'four'), (37, 53, 'plane_radial'), (37, 53, 'four'), (5, 7, 'plane_radial')]
            out.append(('residues_%d' % rs, build_call(group, [(rs, ro) for ro in range(4)], 100 + rs)))
        group = [(37, 53, 'four'), (5, 7, 'hue_wrap'), (3, 1, 'not_sat'), (1, 5, 'plane_radial')]
        out.append(('shared_photo', build_call(group, [(1, 3), (1, 0), (1, 2), (1, 1)], 200, shared=True)))
        _calls = out
    return _calls
