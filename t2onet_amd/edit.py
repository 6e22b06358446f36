"""One photo and one sentence in, the edited photo out (what the reference's demo/seq2seqL1.py does), split the way a
real photo needs it: the DECISION -- which operators, with which parameters -- is taken by the actor on a bounded proxy
(the short-side-600 size the test loader uses, utils/visual_utils.py:34-47), and the decision is then APPLIED to the
original bytes at their native size by the fused 8-bit replay kernel (functional.replay_u8: 6 bytes of memory traffic
per pixel, no fp32 image of the photo ever exists)."""
import numpy as np
import torch

from . import functional as T
from .actor import OP_MASK
from .data import short_side_size, txt2idx


def request_to_idx(text, vocab2id, opt):
    """(1, opt.encoder_max_len) token ids of a request: data.txt2idx (utils/text_utils.py:42-67), unknown words -> id 3."""
    return txt2idx(text, vocab2id, opt.encoder_max_len)


def first_end(ops_vocab, end_id):
    """Number of operators in front of the first END token of one decoded row (all of them when there is none): the
    column train.select_end_images picks, as a count."""
    ops_vocab = list(ops_vocab)
    return ops_vocab.index(end_id) if end_id in ops_vocab else len(ops_vocab)


def nearest_index(src, dst):
    """Source index of each of `dst` destination samples along an axis of `src`: OpenCV's published INTER_NEAREST rule
    sx = min(floor(x * src / dst), src - 1) with the scale src / dst in double -- what the reference's
    resize_and_union_mask applies to a mask (cv2.INTER_NEAREST).  Returns an int64 array of length dst."""
    scale = np.float64(src) / np.float64(dst)
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * scale).astype(np.int64), src - 1)


def _checked_masks(masks, h, w, slots=None):
    """masks {executor operator index or 'all': uint8 (h, w)} -> ([distinct planes], {operator index: plane number}).
    'all' stands for every operator the actor can choose (actor.OP_MASK); an entry for one operator wins over it; planes
    that are the same object are uploaded once.  slots: a dict that receives {id of the mask object: plane number}."""
    planes, slot_of, by_op = [], {}, {}
    for key in sorted(masks, key=lambda k: (k != 'all', str(k))):              # 'all' first, so that named entries overwrite it
        a = masks[key].numpy() if torch.is_tensor(masks[key]) else np.asarray(masks[key])
        if a.dtype != np.uint8 or a.shape != (h, w):
            raise ValueError('edit_image: mask %r must be uint8 (%d, %d), the photo\'s size; got %s %s' % (key, h, w, a.dtype, a.shape))
        if id(masks[key]) not in slot_of:
            slot_of[id(masks[key])] = len(planes)
            planes.append(np.ascontiguousarray(a))
        if key == 'all':
            targets = [i - 3 for i, allowed in enumerate(OP_MASK) if allowed and i >= 3]
        elif isinstance(key, (int, np.integer)) and 0 <= int(key) < len(T.OP_NPARAM):
            targets = [int(key)]
        else:
            raise ValueError('edit_image: mask key %r is neither \'all\' nor an executor operator index 0..7' % (key,))
        for op in targets:
            by_op[op] = slot_of[id(masks[key])]
    if len(planes) > T.REPLAY_MAX_MASKS:
        raise ValueError('edit_image: %d distinct masks, the replay takes %d' % (len(planes), T.REPLAY_MAX_MASKS))
    if slots is not None:
        slots.update(slot_of)
    return planes, by_op


def checked_feather(feather, masks):
    """feather (None, a number, or {key of masks: number}) -> {id of the mask object: sigma > 0}.  Two keys that name one
    plane must agree; a sigma of 0 leaves its plane as it is."""
    if feather is None:
        return {}
    if masks is None:
        raise ValueError('edit_image: feather without masks -- there is no plane to feather')
    if not isinstance(feather, dict):
        feather = {key: feather for key in masks}
    by_plane = {}
    for key, sigma in feather.items():
        if key not in masks:
            raise ValueError('edit_image: feather key %r names no mask (masks: %s)' % (key, ', '.join(repr(k) for k in masks)))
        sigma = float(sigma)
        if not 0.0 <= sigma <= T.FEATHER_MAX_SIGMA:
            raise ValueError('edit_image: feather %r = %r, a sigma must lie in [0, %g]' % (key, sigma, T.FEATHER_MAX_SIGMA))
        if by_plane.setdefault(id(masks[key]), sigma) != sigma:
            raise ValueError('edit_image: feather %r = %g, but another key feathers the same plane by %g'
                             % (key, sigma, by_plane[id(masks[key])]))
    return {plane: sigma for plane, sigma in by_plane.items() if sigma > 0.0}


def refine_eps2(eps):
    """The regulariser of a refinement, a fraction of full scale in (0, 1], in the byte^2 units of functional.refine_u8:
    E = max(1, floor((255 eps)^2 + 0.5)) in double."""
    eps = float(eps)
    if not 0.0 < eps <= 1.0:
        raise ValueError('edit_image: refine eps = %r, a fraction of full scale in (0, 1]' % (eps,))
    return max(1, int(np.floor((np.float64(255.0) * np.float64(eps)) ** 2 + 0.5)))


REFINE_EPS = 0.02


def _refine_value(key, value):
    """A refinement as given -- a radius or (radius, eps) -- -> (radius, E)."""
    pair = tuple(value) if isinstance(value, (tuple, list)) else (value,)
    if not 1 <= len(pair) <= 2:
        raise ValueError('edit_image: refine %r = %r is neither a radius nor (radius, eps)' % (key, value))
    try:
        radius, eps = float(pair[0]), float(pair[1] if len(pair) == 2 else REFINE_EPS)
    except (TypeError, ValueError):
        raise ValueError('edit_image: refine %r = %r has a value that is not a number' % (key, value))
    if not (radius == int(radius) and 0 <= radius <= T.REFINE_MAX_RADIUS):
        raise ValueError('edit_image: refine %r = %r, a radius is a whole number of pixels in 0..%d' % (key, value, T.REFINE_MAX_RADIUS))
    return int(radius), refine_eps2(eps)


def checked_refine(refine, masks):
    """refine (None, a radius, (radius, eps), or {key of masks: either}) -> {id of the mask object: (radius > 0, E)}.  eps is
    a fraction of full scale in (0, 1] (REFINE_EPS when left out; refine_eps2 gives E).  Two keys that name one plane must
    agree; a radius of 0 leaves its plane as it is."""
    if refine is None:
        return {}
    if masks is None:
        raise ValueError('edit_image: refine without masks -- there is no plane to refine')
    if not isinstance(refine, dict):
        refine = {key: refine for key in masks}
    by_plane = {}
    for key, value in refine.items():
        if key not in masks:
            raise ValueError('edit_image: refine key %r names no mask (masks: %s)' % (key, ', '.join(repr(k) for k in masks)))
        pair = _refine_value(key, value)
        if by_plane.setdefault(id(masks[key]), pair) != pair:
            raise ValueError('edit_image: refine %r = %r, but another key refines the same plane by %r'
                             % (key, pair, by_plane[id(masks[key])]))
    return {plane: pair for plane, pair in by_plane.items() if pair[0] > 0}


def _grow_value(key, value):
    """A boundary move as given -- a whole number of pixels (positive grows, negative shrinks) or (mode, radius) with mode one
    of functional.MORPH_MODES -- -> (mode, radius >= 0)."""
    if isinstance(value, (tuple, list)):
        if not (len(value) == 2 and isinstance(value[0], str) and value[0] in T.MORPH_MODES):
            raise ValueError('edit_image: grow %r = %r is neither a number of pixels nor (%s, radius)' % (key, value, ' | '.join(repr(m) for m in T.MORPH_MODES)))
        mode, radius = value
        signed = False
    else:
        mode, radius, signed = None, value, True
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or radius != radius or radius != int(radius):
        raise ValueError('edit_image: grow %r = %r, a radius is a whole number of pixels' % (key, value))
    radius = int(radius)
    if not (-T.MORPH_MAX_RADIUS if signed else 0) <= radius <= T.MORPH_MAX_RADIUS:
        raise ValueError('edit_image: grow %r = %r, a radius lies in %s..%d' % (key, value, '-%d' % T.MORPH_MAX_RADIUS if signed else '0', T.MORPH_MAX_RADIUS))
    return (mode, radius) if mode is not None else ('shrink', -radius) if radius < 0 else ('grow', radius)


def checked_grow(grow, masks):
    """grow (None, a whole number of pixels in -64..64 -- positive grows, negative shrinks --, ('border', R), or {key of masks:
    either}) -> {id of the mask object: (mode, radius)} for functional.morph_u8.  Two keys that name one plane must agree;
    growing or shrinking by 0 leaves its plane exactly as it is (it is not binarised); a border of 0 is the empty plane."""
    if grow is None:
        return {}
    if masks is None:
        raise ValueError('edit_image: grow without masks -- there is no plane to grow')
    if not isinstance(grow, dict):
        grow = {key: grow for key in masks}
    by_plane = {}
    for key, value in grow.items():
        if key not in masks:
            raise ValueError('edit_image: grow key %r names no mask (masks: %s)' % (key, ', '.join(repr(k) for k in masks)))
        pair = _grow_value(key, value)
        if pair[1] == 0 and pair[0] != 'border':
            pair = ('grow', 0)                                       # growing and shrinking by nothing agree
        if by_plane.setdefault(id(masks[key]), pair) != pair:
            raise ValueError('edit_image: grow %r = %r, but another key moves the same plane by %r'
                             % (key, pair, by_plane[id(masks[key])]))
    return {plane: pair for plane, pair in by_plane.items() if pair[1] > 0 or pair[0] == 'border'}


def _round_unit(v, scale):
    """floor(v * scale + 0.5) in double: the host rounding of a selection's user units."""
    return int(np.floor(np.float64(v) * np.float64(scale) + 0.5))


def _select_numbers(term, who):
    if not (isinstance(term, (tuple, list)) and term and isinstance(term[0], str)):
        raise ValueError('%s: select term %r is not (\'[!]kind\', numbers...)' % (who, term))
    try:
        values = [float(v) for v in term[1:]]
    except (TypeError, ValueError):
        raise ValueError('%s: select term %r has a value that is not a number' % (who, term))
    if not all(np.isfinite(values)):
        raise ValueError('%s: select term %r has a value that is not finite' % (who, term))
    return term[0].lstrip('!'), int(term[0].startswith('!')), values


def check_select_terms(terms, who='edit_image'):
    """The checks of a selection in user units that do not need the photo's size; raises ValueError naming the term.
    terms: 1 to 4 of ('[!]lum' | '[!]sat', lo, hi[, soft]) in fractions [0, 1], ('[!]hue', lo, hi[, soft]) in degrees
    [0, 360) with soft <= 180, ('[!]linear', x0, y0, x1, y1) in fractions of w - 1 / h - 1, ('[!]radial', cx, cy, rin, rout)
    with the radii in fractions of min(h, w), ('[!]wand' | '[!]wand8', x, y[, tol]) -- the 4- / 8-connected region around the
    seed at fractions x, y of w - 1 / h - 1, which must lie IN [0, 1] (inside the frame), of the pixels whose bytes differ
    from the seed's by at most the fraction tol in [0, 1] of 255 (WAND_TOL when left out); a leading '!' inverts the term."""
    terms = list(terms) if isinstance(terms, (tuple, list)) else None
    if not terms or len(terms) > T.SELECT_MAX_TERMS:
        raise ValueError('%s: a selection is a list of 1 to %d terms' % (who, T.SELECT_MAX_TERMS))
    for term in terms:
        kind, _, v = _select_numbers(term, who)
        if kind in ('lum', 'sat', 'hue'):
            if len(v) not in (2, 3):
                raise ValueError('%s: select term %r takes lo, hi and an optional softness' % (who, term))
            soft = v[2] if len(v) == 3 else 0.0
            if kind == 'hue':
                if not (0.0 <= v[0] < 360.0 and 0.0 <= v[1] < 360.0 and 0.0 <= soft <= 180.0):
                    raise ValueError('%s: select term %r: hue bounds lie in [0, 360) degrees, the softness in [0, 180]' % (who, term))
            elif not (0.0 <= v[0] <= v[1] <= 1.0 and 0.0 <= soft <= 1.0):
                raise ValueError('%s: select term %r: 0 <= lo <= hi <= 1 and a softness in [0, 1]' % (who, term))
        elif kind in ('linear', 'radial'):
            if len(v) != 4:
                raise ValueError('%s: select term %r takes four numbers' % (who, term))
            if not all(-1.0 <= a <= 2.0 for a in (v if kind == 'linear' else v[:2])):
                raise ValueError('%s: select term %r: positions lie in [-1, 2] (fractions of the frame)' % (who, term))
            if kind == 'linear' and v[:2] == v[2:]:
                raise ValueError('%s: select term %r: the two end points are equal' % (who, term))
            if kind == 'radial' and not 0.0 <= v[2] < v[3] <= 2.0:
                raise ValueError('%s: select term %r: 0 <= rin < rout <= 2 (fractions of the short side)' % (who, term))
        elif kind in WAND_CONN:
            if len(v) not in (2, 3):
                raise ValueError('%s: select term %r takes a seed x, y and an optional tolerance' % (who, term))
            if not (0.0 <= v[0] <= 1.0 and 0.0 <= v[1] <= 1.0):
                raise ValueError('%s: select term %r: the seed lies in [0, 1] (fractions of the frame): it has to be inside it' % (who, term))
            if len(v) == 3 and not 0.0 <= v[2] <= 1.0:
                raise ValueError('%s: select term %r: the tolerance lies in [0, 1] (a fraction of full scale)' % (who, term))
        else:
            raise ValueError('%s: select term %r: the kind is one of lum, sat, hue, linear, radial, wand, wand8' % (who, term))
    return terms


WAND_CONN = {'wand': 4, 'wand8': 8}
WAND_TOL = 0.125                                         # the byte 32


def wand_keys(term_lists):
    """The distinct region jobs of integer term lists (select_terms), in order of appearance: [(sx, sy, tol, conn)]."""
    keys = []
    for terms in term_lists:
        for t in terms:
            if t[0] in WAND_CONN and t[2:5] + (WAND_CONN[t[0]],) not in keys:
                keys.append(t[2:5] + (WAND_CONN[t[0]],))
    return keys


def wand_resolved(terms, offset_of):
    """Integer terms with every wand term replaced by the 'plane' term that reads its region plane: it keeps the invert
    flag.  offset_of: {(sx, sy, tol, conn): byte offset of the plane in the tensor select_u8 takes as src}."""
    return [('plane', t[1], offset_of[t[2:5] + (WAND_CONN[t[0]],)]) if t[0] in WAND_CONN else t for t in terms]


def region_planes(dev_buffer, photo_offset, h, w, keys, offsets):
    """The region planes of one photo, written into dev_buffer itself: functional.region_u8 once per 4 jobs."""
    jobs = [(photo_offset, off, h, w) + key for key, off in zip(keys, offsets)]
    for a in range(0, len(jobs), T.REGION_MAX_JOBS):
        T.region_u8(dev_buffer, jobs[a:a + T.REGION_MAX_JOBS], out=dev_buffer)


def upload_with_room(buffer, descs, room, device):
    """functional.upload_packed with `room` more bytes behind the packed buffer ON THE DEVICE: the device buffer is
    allocated with the room and the packed host buffer copied into its head, so that no byte is uploaded for the room."""
    whole = torch.empty(buffer.numel() + room, dtype=torch.uint8, device=device)
    whole[:buffer.numel()].copy_(buffer, non_blocking=True)
    return T.upload_packed(whole, descs, device)


def select_terms(terms, h, w, who='edit_image'):
    """A selection in user units (check_select_terms) -> the integer terms of functional.select_u8 for an (h, w) photo:
    floor(v * scale + 0.5) in double with scale 255 for lum / sat, 1536 / 360 for hue (bounds modulo 1536), w - 1 and
    h - 1 for positions, min(h, w) for radii.  A gradient that collapses on this size is a ValueError.  A wand term becomes
    ('wand' | 'wand8', invert, sx, sy, tol) with sx, sy the seed pixel and tol a byte: no term of select_u8's, but a job of
    functional.region_u8 whose plane the caller hands to select_u8 (wand_keys, wand_resolved)."""
    if h > 65535 or w > 65535:
        raise ValueError('%s: a selection takes photos up to 65535 pixels a side, got %d x %d' % (who, w, h))
    out = []
    for term in check_select_terms(terms, who):
        kind, invert, v = _select_numbers(term, who)
        if kind in ('lum', 'sat'):
            p = [_round_unit(a, 255.0) for a in (v if len(v) == 3 else v + [0.0])]
        elif kind == 'hue':
            scale = 1536.0 / 360.0
            v = v if len(v) == 3 else v + [0.0]
            p = [_round_unit(v[0], scale) % 1536, _round_unit(v[1], scale) % 1536, _round_unit(v[2], scale)]
        elif kind == 'linear':
            p = [_round_unit(v[0], w - 1), _round_unit(v[1], h - 1), _round_unit(v[2], w - 1), _round_unit(v[3], h - 1)]
            if p[:2] == p[2:]:
                raise ValueError('%s: select term %r: the end points fall on one pixel of a %d x %d photo' % (who, term, w, h))
        elif kind in WAND_CONN:
            p = [_round_unit(v[0], w - 1), _round_unit(v[1], h - 1), _round_unit(v[2] if len(v) == 3 else WAND_TOL, 255.0)]
        else:
            p = [_round_unit(v[0], w - 1), _round_unit(v[1], h - 1), _round_unit(v[2], min(h, w)), _round_unit(v[3], min(h, w))]
            if not p[2] < p[3]:
                raise ValueError('%s: select term %r: the radii fall together on a %d x %d photo' % (who, term, w, h))
        out.append((kind, invert) + tuple(p))
    return out


def _key_targets(key, what):
    if key == 'all':
        return [i - 3 for i, allowed in enumerate(OP_MASK) if allowed and i >= 3]
    if isinstance(key, (int, np.integer)) and not isinstance(key, bool) and 0 <= int(key) < len(T.OP_NPARAM):
        return [int(key)]
    raise ValueError('edit_image: %s key %r is neither \'all\' nor an executor operator index 0..7' % (what, key))


def select_plan(select, masks, feather, h, w, refine=None, keys=None, grow=None):
    """The planes of an edit_image call that gives `select` -- checked without any device use.  select: {executor operator
    index or 'all': selection in user units}, keyed like masks.  Every key of select or masks gets a plane: its selection,
    multiplied by its painted mask when the SAME key has one (a 'plane' term: the intersection); a key with only a painted
    mask is a one-term 'plane' job.  Keys whose rule and painted plane agree share a plane.  Returns (painted, specs, by_op,
    sigma_of): the distinct painted planes to upload, per plane (integer terms, number of its painted plane or None),
    {operator index: plane number} ('all' first, an entry for one operator wins), {plane number: sigma > 0}.  With `refine`
    (keyed like feather; checked_refine) a fifth value follows: {plane number: (radius > 0, E)}.  keys: a dict that receives
    {key of select or masks: plane number}.  With `grow` (keyed like feather; checked_grow) one more value follows behind
    those: {plane number: (mode, radius)}."""
    if not isinstance(select, dict) or not select:
        raise ValueError('edit_image: select is {executor operator index or \'all\': [terms]}')
    masks = masks or {}
    painted, slot_of = [], {}
    for key in masks:
        _key_targets(key, 'mask')
        a = masks[key].numpy() if torch.is_tensor(masks[key]) else np.asarray(masks[key])
        if a.dtype != np.uint8 or a.shape != (h, w):
            raise ValueError('edit_image: mask %r must be uint8 (%d, %d), the photo\'s size; got %s %s' % (key, h, w, a.dtype, a.shape))
        if id(masks[key]) not in slot_of:
            slot_of[id(masks[key])] = len(painted)
            painted.append(np.ascontiguousarray(a))
    specs, by_op, tokens = [], {}, {}
    for key in sorted(set(select) | set(masks), key=lambda k: (k != 'all', str(k))):      # 'all' first, so that named entries overwrite it
        targets = _key_targets(key, 'select' if key in select else 'mask')
        terms = tuple(select_terms(select[key], h, w)) if key in select else ()
        slot = slot_of[id(masks[key])] if key in masks else None
        if len(terms) + (slot is not None) > T.SELECT_MAX_TERMS:
            raise ValueError('edit_image: select %r has %d terms and a painted mask, which counts as one: at most %d'
                             % (key, len(terms), T.SELECT_MAX_TERMS))
        if (terms, slot) not in specs:
            specs.append((terms, slot))
        for op in targets:
            by_op[op] = specs.index((terms, slot))
        tokens[key] = specs.index((terms, slot))
    if len(specs) > T.REPLAY_MAX_MASKS:
        raise ValueError('edit_image: %d distinct planes, the replay takes %d' % (len(specs), T.REPLAY_MAX_MASKS))
    if keys is not None:
        keys.update(tokens)
    handles = [object() for _ in specs]                               # checked_feather tells planes apart by identity
    by_handle = checked_feather(feather, {key: handles[no] for key, no in tokens.items()})
    sigma_of = {no: by_handle[id(hd)] for no, hd in enumerate(handles) if id(hd) in by_handle}
    plan = (painted, specs, by_op, sigma_of)
    if refine is not None:
        by_handle = checked_refine(refine, {key: handles[no] for key, no in tokens.items()})
        plan += ({no: by_handle[id(hd)] for no, hd in enumerate(handles) if id(hd) in by_handle},)
    if grow is not None:
        by_handle = checked_grow(grow, {key: handles[no] for key, no in tokens.items()})
        plan += ({no: by_handle[id(hd)] for no, hd in enumerate(handles) if id(hd) in by_handle},)
    return plan


def _append_planes(buffer, planes):
    """The packed photo with the mask planes behind it, so that ONE upload carries both (a plane is 1 byte per pixel: raw
    bytes outside the descriptor table) -> (buffer, byte offset of each plane)."""
    whole = torch.empty(buffer.numel() + sum(p.size for p in planes), dtype=torch.uint8, pin_memory=buffer.is_pinned())
    whole[:buffer.numel()] = buffer
    flat, pos, offsets = whole.numpy(), buffer.numel(), []
    for p in planes:
        offsets.append(pos)
        flat[pos:pos + p.size] = p.reshape(-1)
        pos += p.size
    return whole, offsets


def _proxy_mask_dict(dev_buffer, mask_offsets, by_op, size, proxy_size):
    """What Actor.get_gt_mask reads, [{str(vocabulary id): [(1, ph, pw) fp32 mask]}], from the native planes on the device:
    nearest_index along both axes (cv2.INTER_NEAREST of resize_and_union_mask), byte / 255."""
    (h, w), (ph, pw) = size, proxy_size
    iy = torch.from_numpy(nearest_index(h, ph)).to(dev_buffer.device)
    ix = torch.from_numpy(nearest_index(w, pw)).to(dev_buffer.device)
    proxies = [(dev_buffer[off:off + h * w].view(h, w)[iy][:, ix].to(torch.float32) / 255.0).unsqueeze(0) for off in mask_offsets]
    return [{str(op + 3): [proxies[slot]] for op, slot in by_op.items()}]


def checked_fill(fill, masks, select):
    """fill (None, or a key that masks or select also carries) -> the key; anything else is a ValueError."""
    if fill is None:
        return None
    _key_targets(fill, 'fill')
    if fill not in (masks or {}) and fill not in (select or {}):
        raise ValueError('edit_image: fill key %r names no plane (masks: %s; select: %s)'
                         % (fill, ', '.join(repr(k) for k in masks or {}) or 'none', ', '.join(repr(k) for k in select or {}) or 'none'))
    return fill


def edit_image(model, img_u8_hwc, x, proxy_short=600, masks=None, feather=None, select=None, refine=None, fill=None, grow=None):
    """img_u8_hwc: the decoded photo, uint8 (h,w,3) RGB (array or CPU tensor); x: (1, L) request token ids.
    Returns (steps_u8, ops, params):
      steps_u8  (max(n,1), h, w, 3) uint8 GPU tensor: picture k is the photo after the first k+1 of the n chosen operators,
                the last one is the result (n = 0, END chosen first: the photo through the two 8-bit conversions);
      ops       the n executor indices in front of the first END (what test() scores: train.select_end_images);
      params    (n, 24) fp32 GPU tensor, their parameter rows.
    The photo is uploaded once; the proxy is made on the device only when the short side exceeds proxy_short (no
    upscaling: a smaller photo is its own proxy); the arg-max episode runs in eval mode under no_grad; pred_ops is read
    back once; ONE replay_u8 launch writes every prefix of the list at native size.  Nothing keeps the actor from
    choosing the sharpness more than once: such a list goes, with or without masks, through ONE replay_u8_stencils launch
    instead (every sharpness reads the neighbours of the image in front of it); lists with at most one sharpness keep
    replay_u8 / replay_u8_masked, the cheaper kernels for them, and their bytes.
    masks: None (a global edit), or {executor operator index or 'all': uint8 (h, w) array at the photo's NATIVE size} for
    a local edit -- 0 leaves a pixel, 255 applies the operator, values between feather the edge; 'all' stands for every
    operator the actor can choose, an entry for one operator wins over it.  The planes travel behind the photo in the same
    upload; the proxy sees each one through nearest_index (indexed on the device, / 255) as the mask_dict of
    Actor.get_gt_mask (one host read of the chosen operator per step, as the reference); ONE replay_u8_masked launch then
    writes every prefix at native size under the native planes.
    feather: None, a standard deviation in pixels of the photo (every plane), or {key of masks: sigma} -- the planes are
    blurred by functional.feather_u8's exact integer Gaussian IN PLACE on the device right after the upload (two launches,
    whatever the number of planes), so that a hard 0/255 selection leaves no seam; the proxy's decision and the native
    replay see the same soft mask.  Keys that share one plane must agree; feather without masks is an error.
    select: None, or {executor operator index or 'all': [terms in user units]} keyed like masks -- the planes are RULES
    (check_select_terms: a luminance, saturation or hue range of the photo itself, a linear or radial gradient over the
    frame) and are written on the device by ONE functional.select_u8 launch into one tensor, which feather, the proxy and
    the replay then read as they read the uploaded planes.  A key that also has a painted mask gets the product of the two
    (the intersection); a key with only a painted mask keeps it; feather may name either.  Nothing but the photo (and the
    painted planes) is uploaded.  Wrong specifications raise ValueError before any device use (select_plan).
    A 'wand' / 'wand8' term is the CONNECTED region around a seed pixel -- "this sky, not the lake of the same blue": the
    pixels joined to the seed by 4- / 8-connected steps over pixels whose three bytes each differ from the seed's by at most
    the tolerance.  The distinct (seed, tolerance, connectivity) of the call each become one job of functional.region_u8
    (three launches per 4 jobs, in front of the select launch; lock-free union-find in which no workgroup waits for another
    and every loop follows strictly falling indices: include/t2onet_hip.h); their hard 0 / 255 planes are written into room
    reserved ON THE DEVICE behind the photo and the painted planes -- no byte is uploaded for it -- and the select launch
    reads each as a 'plane' term with the term's invert flag.  refine and feather soften them like any plane.  The order of
    the stages is region, select, grow, refine, feather, proxy, replay.  Without a wand term the call issues exactly the launches
    and the one upload it issued before there was one.
    refine: None, a radius in pixels of the photo (every plane), (radius, eps), or {key of masks / select: either} -- the
    planes are snapped to the photo's own edges by functional.refine_u8's exact integer guided filter (guide = the photo's
    luminance; eps, a fraction of full scale in (0, 1], default 0.02, is how much contrast counts as an edge) IN PLACE in
    the buffer the later stages read: after select, before feather, the proxy's mask_dict and the replay, so that the
    proxy's decision and the native replay see the same plane.  Four launches, whatever the number of planes.  Keys that
    share one plane must agree; refine without masks or select is an error; None is the path without it, launch for launch.
    fill: None, or a key that masks or select also carries -- the natural one is 4, the inpaint slot; any operator index or
    'all' is allowed, and the plane then also localises those operators as it does without fill.  What lies under that
    plane is REMOVED from the photo: the plane is made exactly as above (region, select, grow, refine, feather), then
    functional.fill_u8 (three launches) replaces every pixel whose plane byte M is > 0, blended by M / 255, with the exact
    integer push-pull fill of include/t2onet_hip.h from the pixels with M = 0 -- IN PLACE in the device buffer, before the proxy
    is made.  The actor therefore decides on the filled picture, the replay edits the filled picture, and every picture of
    steps_u8 carries the fill.  The order of the stages is region, select, grow, refine, feather, fill, proxy, replay: wand seeds
    and select rules read the ORIGINAL bytes.  A soft plane has M > 0 in its soft band, so refine and feather also keep the
    object's anti-aliased rim out of the fill's sources.  The fill plane counts towards the four planes of a call.  It is a
    SMOOTH fill -- sky, walls, blurred backgrounds; it synthesises no texture and is not the reference's inpaint_obj network,
    which stays unexecutable here (operators.InpaintOperator).  A fill key without a plane is a ValueError before any device
    use; None is the path without it, launch for launch and upload for upload.
    grow: None, a whole number of pixels of the photo in -64..64 (every plane; positive GROWS the selection, negative SHRINKS
    it), ('border', R) -- the band of R pixels either side of the selection's edge --, or {key of masks / select: either}.  The
    plane is binarised at 128 and its boundary moved by the EXACT Euclidean distance (functional.morph_u8, two launches,
    whatever the number of planes; the definition is in include/t2onet_hip.h; the frame edge is no edge of the selection) IN
    PLACE in the buffer the later stages read.  The order of the stages is region, select, grow, refine, feather, fill, proxy,
    replay: a wand region grown by a few pixels takes the object's anti-aliased rim, its halo and its contact shadow out of
    the fill's sources, and refine and feather then soften the hard 0 / 255 plane that grow leaves.  Keys that share one plane
    must agree; 0 leaves a plane exactly as it is; grow without masks or select is an error; None is the path without it,
    launch for launch and upload for upload."""
    img = T._u8_hwc(img_u8_hwc)
    h, w = img.shape[:2]
    plane_of = {}
    plan = (select_plan(select, masks, feather, h, w, refine if refine is not None else {}, plane_of, grow if grow is not None else {})
            if select is not None else None)                                                 # before any device use
    sigma_of = checked_feather(feather, masks) if plan is None else {}                       # before any device use
    refine_of = checked_refine(refine, masks) if plan is None else {}                        # before any device use
    grow_of = checked_grow(grow, masks) if plan is None else {}                              # before any device use
    fill = checked_fill(fill, masks, select)                                                 # before any device use
    dev = next(model.parameters()).device
    opt = model.opt
    slot_of = {}
    if plan is not None:
        planes, specs, by_op, plane_sigma, plane_refine, plane_grow = plan
    else:
        planes, by_op = _checked_masks(masks, h, w, slot_of) if masks is not None else ([], {})
    local = masks is not None or plan is not None
    buffer, descs = T.pack_u8([img])
    mask_offsets = []
    if masks is not None:
        buffer, mask_offsets = _append_planes(buffer, planes)
    wands = wand_keys([terms for terms, _ in specs]) if plan is not None else []
    if wands:
        # room for the region planes behind the photo and the painted planes, on the device only: select_u8 reads plane
        # terms from the tensor it takes as src
        wand_offsets = [buffer.numel() + k * h * w for k in range(len(wands))]
        dev_buffer, table_ptr, descs, _keep = upload_with_room(buffer, descs, len(wands) * h * w, dev)
        region_planes(dev_buffer, int(descs[0]['offset']), h, w, wands, wand_offsets)
        specs = [(wand_resolved(terms, dict(zip(wands, wand_offsets))), slot) for terms, slot in specs]
    else:
        dev_buffer, table_ptr, descs, _keep = T.upload_packed(buffer, descs, dev)
    mask_buffer = dev_buffer                                    # where the replay and the proxy read the planes
    if plan is not None:
        # every plane of the call in ONE launch: a rule, a rule times its painted plane, or a painted plane alone
        jobs = [(int(descs[0]['offset']), k * h * w, h, w, list(terms) + ([('plane', 0, mask_offsets[slot])] if slot is not None else []))
                for k, (terms, slot) in enumerate(specs)]
        mask_buffer = T.select_u8(dev_buffer, jobs)
        mask_offsets = [k * h * w for k in range(len(specs))]
        if plane_grow:
            T.morph_u8(mask_buffer, [(mask_offsets[k],) * 2 + (h, w, r, mode) for k, (mode, r) in plane_grow.items()])
        if plane_refine:
            T.refine_u8(dev_buffer, mask_buffer, [(int(descs[0]['offset']),) + (mask_offsets[k],) * 2 + (h, w, r, E) for k, (r, E) in plane_refine.items()])
        if plane_sigma:
            T.feather_u8(mask_buffer, [(mask_offsets[k],) * 2 + (h, w, sigma) for k, sigma in plane_sigma.items()])
    else:
        if grow_of:
            T.morph_u8(dev_buffer, [(mask_offsets[slot_of[p]],) * 2 + (h, w, r, mode) for p, (mode, r) in grow_of.items()])
        if refine_of:
            T.refine_u8(dev_buffer, dev_buffer, [(int(descs[0]['offset']),) + (mask_offsets[slot_of[p]],) * 2 + (h, w, r, E) for p, (r, E) in refine_of.items()])
        if sigma_of:
            T.feather_u8(dev_buffer, [(mask_offsets[slot_of[p]],) * 2 + (h, w, sigma) for p, sigma in sigma_of.items()])
    if fill is not None:
        # the photo filled in place under its finished plane: the proxy and the replay below read the filled bytes
        at = mask_offsets[plane_of[fill] if plan is not None else slot_of[id(masks[fill])]]
        T.fill_u8(dev_buffer, mask_buffer, [(int(descs[0]['offset']), at, int(descs[0]['offset']), h, w)], out=dev_buffer)
    ph, pw = short_side_size(h, w, proxy_short) if min(h, w) > proxy_short else (h, w)
    proxy = T._resize_launch(dev_buffer, table_ptr, 1, ph, pw)
    mask_dict = _proxy_mask_dict(mask_buffer, mask_offsets, by_op, (h, w), (ph, pw)) if local else None
    x = torch.as_tensor(x, dtype=torch.long).view(1, -1)
    lengths = (x != opt.null_id).sum(1)                      # on the host, before the copy
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            _, _, pred_ops, pred_params = model.episode_forward(x.to(dev), proxy, mask_dict, reinforce_sample=False, lengths=lengths)
    finally:
        model.train(was_training)
    ops_vocab = pred_ops[0].cpu().tolist()                   # the one host read: the operator names are wanted anyway
    n = first_end(ops_vocab, opt.end_id)
    ops = [int(o) - 3 for o in ops_vocab[:n]]                # executor index = vocabulary id - 3 (actor.py:100-114)
    if n > T.REPLAY_MAX_STEPS:
        raise NotImplementedError('edit_image: %d operators chosen, the replay takes %d' % (n, T.REPLAY_MAX_STEPS))
    params = torch.cat([p[:1] for p in pred_params[:n]], 0) if n else torch.zeros(0, T.PARAM_PAD, device=dev)
    J = max(n, 1)
    src_offset, nbytes = int(descs[0]['offset']), 3 * h * w
    jobs = [(src_offset, j * nbytes, h, w, ops[:j + 1]) for j in range(J)]       # n = 0: one job with no step
    table = torch.zeros(J, T.REPLAY_MAX_STEPS, T.PARAM_PAD, device=dev)
    table[:, :n] = params
    if local:
        mask_of = [by_op.get(op, -1) for op in ops]
        jobs = [job + (mask_of[:j + 1],) for j, job in enumerate(jobs)]
    out = T.replay_u8_any(dev_buffer, jobs, table, mask_buffer if local else None, mask_offsets)   # the kernel by the list
    return out[:J * nbytes].view(J, h, w, 3), ops, params
