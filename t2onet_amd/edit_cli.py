"""Edit one photo by a request in words (the reference's demo/seq2seqL1.py):

    python -m t2onet_amd.edit_cli --img photo.jpg --request "make it brighter" --checkpoint model.pth --vocab_dir data/language

writes into save_dir/<name>/: <name>_in.<ext> (the photo as decoded), <name>.<ext> (the result), with --multi_img the
pictures after each operator as {k}_inference_<name>.<ext> (k = 1 ..), and <name>.json = [{'input', 'request', 'output',
'operations': [(operator name, its parameters), ...]}] under the reference's operator names and parameter counts
(demo/seq2seqL1.py:121-122,193-196).  Images are written with PIL, the format chosen by the extension.

--mask [NAME=]FILE (repeatable) makes it a LOCAL edit: FILE is decoded as 8-bit grey and must have the photo's size; 0
leaves a pixel as it is, 255 applies the operator, values between feather the edge.  NAME is one of the operator names
above and binds the mask to that operator; without a name the mask applies to every operator (a named mask wins).  At
most 4 distinct files.  The record then also holds 'masks': {name or 'all': file}.

--feather [NAME=]SIGMA (repeatable) blurs a mask on the device before it is used, by an exact 8-bit Gaussian of standard
deviation SIGMA pixels of the photo (at most 64): the soft edge a hard 0/255 selection lacks.  NAME is a name a --mask was
given under; without a name every mask is feathered.  The record then also holds 'feather': {name or 'all': sigma}.

--select [NAME=]TERM[+TERM...] (repeatable) makes it a local edit WITHOUT a mask file: the plane is a rule, computed on
the device from the photo's own bytes (edit.edit_image's `select`).  TERM is one of lum:LO:HI[:SOFT], sat:LO:HI[:SOFT]
(fractions in [0, 1]), hue:LO:HI[:SOFT] (degrees; the arc runs upward from LO to HI and may wrap), linear:X0,Y0:X1,Y1
(full weight at the first point, none at the second; fractions of the frame), radial:CX,CY:RIN:ROUT (radii in fractions
of the short side), wand:X,Y[:TOL] or wand8:X,Y[:TOL] (the magic wand: the 4- / 8-connected region around the seed at
fractions X, Y of the frame, both in [0, 1], of the pixels whose bytes differ from the seed's by at most TOL of full
scale, default 0.125; a hard plane that --refine and --feather soften); a leading '!' inverts a term, '+' multiplies terms (at most 4).  NAME is as for --mask; a --select
and a --mask under the same name are intersected; --feather NAME= may name a --select as well.  The record then also
holds 'select': {name or 'all': the terms as given}, which apply_cli replays on other photos of any size.

--refine [NAME=]RADIUS[:EPS] (repeatable) snaps a plane to the photo's own edges on the device before it is feathered and
used: the exact integer guided filter of edit.edit_image's `refine`, guided by the photo's luminance, over a window of
RADIUS pixels (a whole number, at most 64); EPS, a fraction of full scale in (0, 1] (default 0.02), is how much contrast
counts as an edge.  NAME is a name a --mask or --select was given under; without a name every plane is refined.  The
record then also holds 'refine': {name or 'all': [radius, eps]}, which apply_cli replays under each photo's own luminance.

--grow [NAME=]R, --shrink [NAME=]R and --border [NAME=]R (each repeatable) move a plane's boundary by R pixels of the photo (a
whole number in 0..64) on the device, by the exact Euclidean distance (edit.edit_image's `grow`, functional.morph_u8): the
plane is binarised at 128 and grown, shrunk, or turned into the band of R pixels either side of its edge -- after --select,
before --refine and --feather, which soften the hard plane again.  NAME is a name a --mask or --select was given under;
without a name every plane is moved (a named flag wins); two of these flags on one plane are an error.  The frame edge is no
edge of the selection.  The record then also holds 'grow': {name or 'all': [mode, radius]}, which apply_cli carries to other
photos by the same number of pixels.

--fill [NAME] REMOVES what lies under a plane before anything else is decided: NAME is an operator name a --mask or
--select was given under (default: inpaint, the slot of the operator this project cannot execute).  The plane is made as
above (wand, rule, painted mask, --grow, --refine, --feather); then the pixels under it are replaced on the device, blended by the
plane's byte, with an exact integer push-pull fill from the pixels the plane leaves at 0 (edit.edit_image's `fill`,
functional.fill_u8).  The actor decides on the filled photo and every written picture carries the fill.  It is a SMOOTH
fill: it suits sky, walls and blurred backgrounds, synthesises no texture and is not the reference's inpaint network.  The
record then also holds 'fill': NAME, which apply_cli carries to other photos when the plane is a --select.  For example
    --select 'inpaint=wand:0.5,0.4:0.1' --grow inpaint=4 --feather inpaint=2 --fill

The actor decides on a proxy of the photo (short side --proxy_short, the test loader's 600; a smaller photo is its own
proxy) and the decision is applied to the photo at its native size by the fused 8-bit replay kernel (edit.edit_image).

Deliberate difference from the demo: the result is the image AT THE FIRST END token, which is what test() scores
(experiments/t2onet/test_seq2seqL1.py via train.select_end_images).  The demo saves pred_imgs[:, -1], which also holds
the operators the decoder went on to choose after END; the demo's JSON and step images already stop at END, as here.
"""
import argparse
import json
import os

import torch

from .data import ACT2PN, ACTIONS, decode_image


def load_vocab(vocab_dir, session, dataset='FiveK'):
    """token -> id from <vocab_dir>/<dataset>_vocabs_sess_<session>.json (a list of tokens, utils/text_utils.py:28-38)."""
    with open(os.path.join(vocab_dir, '%s_vocabs_sess_%s.json' % (dataset, session))) as f:
        return {tok: i for i, tok in enumerate(json.load(f))}


def operations_record(ops, params):
    """[(operator name, params[:n])] for executor indices `ops` and their (len(ops), 24) parameter rows."""
    rows = params.tolist() if hasattr(params, 'tolist') else list(params)
    return [(ACTIONS[op], [float(v) for v in row[:ACT2PN[ACTIONS[op]]]]) for op, row in zip(ops, rows)]


def parse_mask_args(specs):
    """--mask values ([NAME=]FILE) -> {operator name or 'all': file}.  NAME must be one of ACTIONS; what stands in front
    of the first '=' counts as a name unless it looks like part of a path (holds a separator or a dot).  At most 4
    distinct files.  Raises ValueError."""
    named = {}
    for spec in specs or []:
        head, sep, tail = spec.partition('=')
        if sep and head in ACTIONS:
            name, path = head, tail
        elif sep and not (os.sep in head or '/' in head or '.' in head):
            raise ValueError('--mask %s: %r is not an operator name (one of %s)' % (spec, head, ', '.join(ACTIONS)))
        else:
            name, path = 'all', spec
        if not path:
            raise ValueError('--mask %s: no file given' % spec)
        named[name] = path
    if len(set(named.values())) > 4:
        raise ValueError('--mask: %d distinct mask files, at most 4 are taken' % len(set(named.values())))
    return named


def parse_feather_args(specs, named):
    """--feather values ([NAME=]SIGMA) -> {name or 'all': sigma}; named: what parse_mask_args returned.  NAME must be a
    name a --mask was given under, SIGMA a number in [0, 64]; no NAME means every mask.  Raises ValueError."""
    import math
    sigmas = {}
    for spec in specs or []:
        head, sep, tail = spec.partition('=')
        name, text = (head, tail) if sep else ('all', spec)
        if not named:
            raise ValueError('--feather %s: there is no --mask to feather' % spec)
        if sep and name not in named:
            raise ValueError('--feather %s: no --mask was given under %r (given: %s)' % (spec, name, ', '.join(sorted(named))))
        try:
            sigma = float(text)
        except ValueError:
            raise ValueError('--feather %s: %r is not a number' % (spec, text))
        if math.isnan(sigma) or not 0.0 <= sigma <= 64.0:
            raise ValueError('--feather %s: SIGMA must lie in [0, 64]' % spec)
        sigmas[name] = sigma
    return sigmas


def parse_refine_args(specs, named):
    """--refine values ([NAME=]RADIUS[:EPS]) -> {name or 'all': (radius, eps)}; named: every name a plane goes by.  NAME
    must be one of them, RADIUS a whole number in 0..64, EPS a number in (0, 1] (0.02 when left out); no NAME means every
    plane.  Raises ValueError naming the spec."""
    import math
    from .edit import REFINE_EPS
    refines = {}
    for spec in specs or []:
        head, sep, tail = spec.partition('=')
        name, text = (head, tail) if sep else ('all', spec)
        if not named:
            raise ValueError('--refine %s: there is no --mask or --select to refine' % spec)
        if sep and name not in named:
            raise ValueError('--refine %s: no --mask or --select was given under %r (given: %s)' % (spec, name, ', '.join(sorted(named))))
        fields = text.split(':')
        if len(fields) not in (1, 2) or not fields[0]:
            raise ValueError('--refine %s: expected RADIUS[:EPS]' % spec)
        try:
            radius = int(fields[0])
        except ValueError:
            raise ValueError('--refine %s: RADIUS %r is not a whole number' % (spec, fields[0]))
        if not 0 <= radius <= 64:
            raise ValueError('--refine %s: RADIUS must lie in 0..64' % spec)
        try:
            eps = float(fields[1]) if len(fields) == 2 else REFINE_EPS
        except ValueError:
            raise ValueError('--refine %s: EPS %r is not a number' % (spec, fields[1]))
        if math.isnan(eps) or not 0.0 < eps <= 1.0:
            raise ValueError('--refine %s: EPS must lie in (0, 1]' % spec)
        refines[name] = (radius, eps)
    return refines


def parse_grow_args(grows, shrinks, borders, named):
    """--grow, --shrink and --border values ([NAME=]R each) -> {name or 'all': (mode, radius)}; named: every name a plane goes
    by.  NAME must be one of them, R a whole number in 0..64; no NAME means every plane.  Two flags on one plane are an
    error.  Raises ValueError naming the flag."""
    moves = {}
    for mode, specs in (('grow', grows), ('shrink', shrinks), ('border', borders)):
        for spec in specs or []:
            head, sep, tail = spec.partition('=')
            name, text = (head, tail) if sep else ('all', spec)
            if not named:
                raise ValueError('--%s %s: there is no --mask or --select to %s' % (mode, spec, mode))
            if sep and name not in named:
                raise ValueError('--%s %s: no --mask or --select was given under %r (given: %s)' % (mode, spec, name, ', '.join(sorted(named))))
            try:
                radius = int(text)
            except ValueError:
                raise ValueError('--%s %s: R %r is not a whole number' % (mode, spec, text))
            if not 0 <= radius <= 64:
                raise ValueError('--%s %s: R must lie in 0..64' % (mode, spec))
            if name in moves:
                raise ValueError('--%s %s: %s already has --%s %d; one of --grow, --shrink and --border to a plane'
                                 % (mode, spec, 'every plane' if name == 'all' else 'the plane %r' % name, moves[name][0], moves[name][1]))
            moves[name] = (mode, radius)
    return moves


def grow_argument(moves, named):
    """{name or 'all': (mode, radius)} of parse_grow_args -> the `grow` argument of edit.edit_image, keyed like the planes of
    `named`.  An unnamed value stands for every plane; a named one wins over it (as feather_argument)."""
    if not moves:
        return None
    grow = {}
    for name in named:
        if name in moves or 'all' in moves:
            grow['all' if name == 'all' else ACTIONS.index(name)] = tuple(moves.get(name, moves.get('all')))
    return grow


def parse_fill_arg(name, named):
    """--fill's value (None when the flag is absent) -> None or the name; named: every name a plane goes by.  Raises
    ValueError when no --mask or --select was given under it."""
    if name is None:
        return None
    if name not in named:
        raise ValueError('--fill %s: no --mask or --select was given under %r (given: %s)' % (name, name, ', '.join(sorted(named)) or 'none'))
    return name


def refine_argument(refines, named):
    """{name or 'all': (radius, eps)} of parse_refine_args -> the `refine` argument of edit.edit_image, keyed like the planes
    of `named`.  An unnamed value stands for every plane; a named one wins over it (as feather_argument)."""
    if not refines:
        return None
    refine = {}
    for name in named:
        if name in refines or 'all' in refines:
            refine['all' if name == 'all' else ACTIONS.index(name)] = tuple(refines.get(name, refines.get('all')))
    return refine


def parse_select_terms(spec):
    """TERM[+TERM...] -> the terms in user units as edit.check_select_terms takes them, [('[!]kind', numbers...)].  Raises
    ValueError naming the spec."""
    terms = []
    for text in spec.split('+'):
        fields = text.split(':')
        kind = fields[0].lstrip('!')
        if kind not in ('lum', 'sat', 'hue', 'linear', 'radial', 'wand', 'wand8') or len(fields[0]) - len(kind) > 1:
            raise ValueError('--select %s: %r is not a term (lum, sat, hue, linear, radial, wand or wand8, with ! in front to invert)' % (spec, text))
        shape = {'linear': (2, 2), 'radial': (2, 1, 1)}.get(kind)
        if kind in ('wand', 'wand8'):
            if len(fields) not in (2, 3):
                raise ValueError('--select %s: %s takes X,Y[:TOL], got %r' % (spec, kind, text))
            shape = (2, 1)[:len(fields) - 1]
        if shape is None and len(fields) not in (3, 4):
            raise ValueError('--select %s: %s takes LO:HI[:SOFT], got %r' % (spec, kind, text))
        if shape is not None and len(fields) != 1 + len(shape):
            raise ValueError('--select %s: %s takes %s, got %r' % (spec, kind, 'X0,Y0:X1,Y1' if kind == 'linear' else 'CX,CY:RIN:ROUT', text))
        values = []
        for k, field in enumerate(fields[1:]):
            parts = field.split(',')
            if len(parts) != (shape[k] if shape else 1):
                raise ValueError('--select %s: %r in %r does not have the numbers %s takes' % (spec, field, text, kind))
            try:
                values += [float(v) for v in parts]
            except ValueError:
                raise ValueError('--select %s: %r in %r is not a number' % (spec, field, text))
        terms.append((fields[0],) + tuple(values))
    return terms


def parse_select_args(specs):
    """--select values ([NAME=]TERM[+TERM...]) -> {operator name or 'all': the terms as given}.  NAME must be one of ACTIONS;
    every selection is parsed and checked (edit.check_select_terms).  Raises ValueError naming the spec."""
    from .edit import check_select_terms
    named = {}
    for spec in specs or []:
        head, sep, tail = spec.partition('=')
        if sep and head not in ACTIONS:
            raise ValueError('--select %s: %r is not an operator name (one of %s)' % (spec, head, ', '.join(ACTIONS)))
        name, text = (head, tail) if sep else ('all', spec)
        if not text:
            raise ValueError('--select %s: no term given' % spec)
        check_select_terms(parse_select_terms(text), '--select %s' % spec)
        named[name] = text
    return named


def select_argument(named):
    """{name or 'all': terms as given} of parse_select_args -> the `select` argument of edit.edit_image."""
    return {('all' if name == 'all' else ACTIONS.index(name)): parse_select_terms(text) for name, text in named.items()} or None


def feather_argument(sigmas, named):
    """{name or 'all': sigma} of parse_feather_args -> the `feather` argument of edit.edit_image, keyed like the masks
    load_masks returns for `named`.  An unnamed sigma stands for every mask; a named one wins over it.  Two names that
    share one file must end up with one sigma (edit.checked_feather)."""
    if not sigmas:
        return None
    feather = {}
    for name in named:
        if name in sigmas or 'all' in sigmas:
            feather['all' if name == 'all' else ACTIONS.index(name)] = sigmas.get(name, sigmas.get('all'))
    return feather


def load_masks(named, h, w):
    """{name: file} -> the `masks` argument of edit.edit_image: every file decoded with PIL as 8-bit grey, one array per
    distinct file; a size other than the photo's (h, w) is an error naming both."""
    from PIL import Image
    import numpy as np
    by_file, masks = {}, {}
    for name, path in named.items():
        if path not in by_file:
            with Image.open(path) as im:
                a = np.ascontiguousarray(np.asarray(im.convert('L'), dtype=np.uint8))
            if a.shape != (h, w):
                raise ValueError('--mask %s is %d x %d (width x height), the photo is %d x %d' % (path, a.shape[1], a.shape[0], w, h))
            by_file[path] = a
        masks['all' if name == 'all' else ACTIONS.index(name)] = by_file[path]
    return masks


def write_outputs(save_dir, img_path, request, img_u8, steps_u8, ops, params, multi_img=False, masks=None, feather=None, select=None,
                  refine=None, fill=None, grow=None):
    """The files of one edit (see the module docstring); steps_u8: (max(n,1), h, w, 3) uint8 array; masks: {name: file}
    of a local edit, feather: {name: sigma}, select: {name: terms as given}, refine: {name: (radius, eps)} and fill: the
    name of the plane whose content was removed, grow: {name: (mode, radius)}, each recorded when given.  Returns the record."""
    from PIL import Image
    name, ext = os.path.splitext(os.path.basename(img_path))
    out_dir = os.path.join(save_dir, name)
    os.makedirs(out_dir, exist_ok=True)
    input_name, output_name = name + '_in' + ext, name + ext
    Image.fromarray(img_u8).save(os.path.join(out_dir, input_name))
    Image.fromarray(steps_u8[-1]).save(os.path.join(out_dir, output_name))
    if multi_img:
        for k in range(len(ops)):
            Image.fromarray(steps_u8[k]).save(os.path.join(out_dir, '%d_inference_%s%s' % (k + 1, name, ext)))
    info = {'input': input_name, 'request': request, 'output': output_name, 'operations': operations_record(ops, params)}
    if masks:
        info['masks'] = dict(masks)
    if feather:
        info['feather'] = dict(feather)
    if select:
        info['select'] = dict(select)
    if refine:
        info['refine'] = {name: [int(v[0]), float(v[1])] for name, v in refine.items()}
    if fill:
        info['fill'] = str(fill)
    if grow:
        info['grow'] = {name: [str(v[0]), int(v[1])] for name, v in grow.items()}
    with open(os.path.join(out_dir, name + '.json'), 'w') as f:
        json.dump([info], f)
    return info


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--img', required=True)
    ap.add_argument('--request', required=True)
    ap.add_argument('--checkpoint', required=True, help='state_dict of the Actor (model.pth)')
    ap.add_argument('--vocab_dir', default='data/language')
    ap.add_argument('--session', type=int, default=1)
    ap.add_argument('--multi_img', action='store_true', help='also write the picture after each operator')
    ap.add_argument('--proxy_short', type=int, default=600, help='short side of the picture the actor decides on')
    ap.add_argument('--save_dir', default='output/demo_output')
    ap.add_argument('--mask', action='append', default=None, metavar='[NAME=]FILE',
                    help='8-bit grey mask of the photo\'s size for a local edit (0 keeps, 255 edits); NAME = an operator name, '
                         'without it the mask applies to every operator; repeatable, at most 4 files')
    ap.add_argument('--feather', action='append', default=None, metavar='[NAME=]SIGMA',
                    help='blur a mask on the device by a Gaussian of SIGMA pixels (at most 64) before it is used; NAME = a name '
                         'a --mask was given under, without it every mask; repeatable')
    ap.add_argument('--select', action='append', default=None, metavar='[NAME=]TERM[+TERM...]',
                    help='a local edit by a rule instead of a mask file: lum:LO:HI[:SOFT], sat:LO:HI[:SOFT], hue:LO:HI[:SOFT], '
                         'linear:X0,Y0:X1,Y1, radial:CX,CY:RIN:ROUT, wand:X,Y[:TOL] / wand8:X,Y[:TOL] (the 4- / 8-connected region '
                         'around the seed at fractions X, Y of the frame, tolerance TOL in [0, 1], default 0.125), ! in front '
                         'inverts, + multiplies; NAME as for --mask; repeatable')
    ap.add_argument('--refine', action='append', default=None, metavar='[NAME=]RADIUS[:EPS]',
                    help='snap a plane to the photo\'s own edges on the device (guided filter, window RADIUS <= 64 pixels, EPS in '
                         '(0, 1], default 0.02) before it is feathered and used; NAME = a name a --mask or --select was given '
                         'under, without it every plane; repeatable')
    for flag, what in (('grow', 'grow a plane'), ('shrink', 'shrink a plane'), ('border', 'turn a plane into the band of R pixels either side of its edge')):
        ap.add_argument('--' + flag, action='append', default=None, metavar='[NAME=]R',
                        help='%s by R pixels (a whole number, at most 64; exact Euclidean distance) on the device, after --select and '
                             'before --refine and --feather; NAME = a name a --mask or --select was given under, without it every '
                             'plane; repeatable, one of --grow, --shrink and --border to a plane' % what)
    ap.add_argument('--fill', nargs='?', const='inpaint', default=None, metavar='NAME',
                    help='remove what lies under a plane before the edit: the pixels under the plane a --mask or --select was given '
                         'under NAME (default inpaint) are replaced on the device by a smooth push-pull fill from the pixels around '
                         'them (sky, walls, blurred backgrounds; no texture is synthesised; not the reference\'s inpaint network)')
    args = ap.parse_args(argv)
    named = parse_mask_args(args.mask)
    rules = parse_select_args(args.select)
    planes = dict(named, **rules)                                                  # every name a plane goes by
    sigmas = parse_feather_args(args.feather, planes)                              # before the model: a wrong value fails early
    refines = parse_refine_args(args.refine, planes)
    moves = parse_grow_args(args.grow, args.shrink, args.border, planes)
    fill_name = parse_fill_arg(args.fill, planes)
    img = decode_image(args.img)
    masks = load_masks(named, img.shape[0], img.shape[1]) if named else None       # before the model: a wrong mask fails early
    feather = feather_argument(sigmas, planes)
    select = select_argument(rules)
    refine = refine_argument(refines, planes)
    grow = grow_argument(moves, planes)
    fill = None if fill_name is None else 'all' if fill_name == 'all' else ACTIONS.index(fill_name)
    if select:
        from .edit import select_plan
        select_plan(select, masks, feather, img.shape[0], img.shape[1], refine, grow=grow)      # a gradient that collapses on this photo, too many planes
    else:
        from .edit import checked_feather, checked_grow, checked_refine
        checked_grow(grow, masks)
        checked_feather(feather, masks)                                            # two names, one file, two sigmas
        checked_refine(refine, masks)

    from . import default_options
    from .actor import Actor
    from .edit import edit_image, request_to_idx
    opt = default_options(vocab_dir=args.vocab_dir, session=args.session)
    vocab2id = load_vocab(args.vocab_dir, args.session, opt.dataset)
    device = torch.device('cuda', torch.cuda.current_device())
    model = Actor(opt)
    model.load_state_dict(torch.load(args.checkpoint, map_location='cpu'), strict=False)      # as the demo (:129)
    model.to(device)
    steps_u8, ops, params = edit_image(model, img, request_to_idx(args.request, vocab2id, opt), args.proxy_short, masks=masks,
                                      feather=feather, select=select, **dict({'refine': refine} if refine else {}, **dict({'fill': fill} if fill is not None else {}, **({'grow': grow} if grow else {}))))
    info = write_outputs(args.save_dir, args.img, args.request, img, steps_u8.cpu().numpy(), ops, params.cpu(), args.multi_img,
                         masks=named or None, feather=sigmas or None, select=rules or None, refine=refines or None, fill=fill_name, grow=moves or None)
    print('%s: %s -> %s' % (args.request, ', '.join(n for n, _ in info['operations']) or '(no operator)',
                            os.path.join(args.save_dir, os.path.splitext(os.path.basename(args.img))[0], info['output'])))
    return info


if __name__ == '__main__':
    main()
