"""Apply the edit of a record that edit_cli wrote to other photos -- the edit decided for one photo on the rest of a
shoot, or a record edited by hand:

    python -m t2onet_amd.apply_cli --record NAME.json --img A.jpg [B.jpg ...] [--save_dir DIR] [--multi_img]

The record is edit_cli's <name>.json = [{'request', 'operations': [[operator name, its parameters], ...], ...}].  No
checkpoint, no vocabulary and no request are needed: applying a record is pure replay.  The operations are parsed with
the reference's operator names and parameter counts (data.ACTIONS / ACT2PN); an unknown name, a wrong number of values,
'inpaint' and more than 8 operations are errors that name the entry.  A list may repeat any operator, sharpness included.

The photos are decoded on the host, packed back to back and uploaded once; each photo is one job of the fused 8-bit
replay at its native size (with --multi_img: one job per prefix of the list), at most 64 jobs per launch.  A list with at
most one sharpness goes through functional.replay_u8, any other through functional.replay_u8_stencils
(functional.replay_u8_any chooses per launch).  The files of each
photo are edit_cli's (write_outputs); the new record takes 'request' from the source record and names it under 'record'.

A record with 'select' (edit_cli --select: {operator name or 'all': TERM[+TERM...]}) and optionally 'feather' ({one of
those names: sigma in pixels}; as in edit_cli, 'all' is the unnamed --feather and softens every plane that has no sigma
of its own) is applied LOCALLY: a selection is a rule in units of the frame, so every photo gets its
own planes at its own size, computed on the device.  The photos are grouped so that a group names at most 4 planes; per
group functional.region_u8 labels the connected regions of its 'wand' terms (each photo from its own seed pixel), ONE
functional.select_u8 launch writes the planes, functional.feather_u8's two launches soften them if asked, and
ONE functional.replay_u8_any launch replays the list under them.  The new records carry 'select' and 'feather' along.
A record that also has 'refine' (edit_cli --refine: {one of those names or 'all': [radius, eps]}) snaps each photo's planes
to that photo's OWN luminance: functional.refine_u8's four launches run between the select launch and feather's two.
A record that also has 'grow' (edit_cli --grow / --shrink / --border: {one of those names or 'all': [mode, radius]}) moves the
boundary of each photo's planes by the same number of pixels at that photo's own size: functional.morph_u8's two launches
run behind the select launch, in front of refine's and feather's.  The sequence is select, grow, refine, feather, fill.
A record that has 'fill' (edit_cli --fill: the name of a plane) and 'select' under that name REMOVES what lies under that
plane from every photo first: the plane is made per photo like the others (its own seed pixel, its own luminance, its own
size), functional.fill_u8 fills the photos of a group in place in ONE call of three launches, and the list is then
replayed on the filled photos.  A smooth fill, not the reference's inpaint network: an 'inpaint' OPERATION stays refused.
Painted masks do not carry from photo to photo: a record with 'masks' and no 'select' is replayed globally, as before,
and a record that has both is refused -- and so is a record whose 'fill' names a painted mask, or nothing.
"""
import argparse
import json
import os

import numpy as np
import torch

from .data import ACT2PN, ACTIONS, decode_image

MAX_STEPS, MAX_JOBS, PARAM_PAD = 8, 64, 24          # functional.REPLAY_MAX_STEPS, REPLAY_MAX_JOBS, PARAM_PAD (checked in apply_record)
MAX_PLANES = 4                                      # functional.REPLAY_MAX_MASKS (checked in apply_record_local)


def parse_record(record):
    """The parsed JSON of a record (or one entry of it) -> (request, ops, params): executor indices and their (n, 24)
    float32 parameter rows.  Raises ValueError naming the entry."""
    info = record[0] if isinstance(record, list) and record else record
    if not (isinstance(info, dict) and isinstance(info.get('operations'), list)):
        raise ValueError('record: expected [{"operations": [[name, values], ...], ...}] as edit_cli writes it')
    operations = info['operations']
    if len(operations) > MAX_STEPS:
        raise ValueError('record: %d operations, the replay takes %d (entry %d: %r)' % (len(operations), MAX_STEPS, MAX_STEPS, operations[MAX_STEPS]))
    ops, params = [], np.zeros((len(operations), PARAM_PAD), np.float32)
    for k, entry in enumerate(operations):
        if not (isinstance(entry, (list, tuple)) and len(entry) == 2 and isinstance(entry[0], str) and isinstance(entry[1], (list, tuple))):
            raise ValueError('record: operation %d is %r, expected [name, [values]]' % (k, entry))
        name, values = entry
        if name not in ACTIONS:
            raise ValueError('record: operation %d: %r is not an operator name (one of %s)' % (k, name, ', '.join(ACTIONS)))
        if name == 'inpaint':
            raise ValueError('record: operation %d: inpaint is not supported by the replay' % k)
        if len(values) != ACT2PN[name]:
            raise ValueError('record: operation %d: %s takes %d values, got %d' % (k, name, ACT2PN[name], len(values)))
        try:
            params[k, :len(values)] = [float(v) for v in values]
        except (TypeError, ValueError):
            raise ValueError('record: operation %d: %s has a value that is not a number: %r' % (k, name, values))
        ops.append(ACTIONS.index(name))
    return str(info.get('request', '')), ops, params


def parse_local(record):
    """The local part of a record -> None (a global edit), or (select, feather): {operator name or 'all': TERM[+TERM...] as
    edit_cli recorded it} and {one of those names: sigma}.  Raises ValueError: a 'select' beside 'masks', a spec that does
    not parse, a feather that names no selection."""
    from .edit_cli import parse_feather_args, parse_select_args
    info = record[0] if isinstance(record, list) and record else record
    select = info.get('select') if isinstance(info, dict) else None
    if select is None:
        return None
    if info.get('masks'):
        raise ValueError('record: it has \'select\' and \'masks\': a rule intersected with a painted plane belongs to one photo '
                         'and is not carried to others (edit_cli --mask stays with its photo)')
    if not (isinstance(select, dict) and select and all(isinstance(k, str) and isinstance(v, str) for k, v in select.items())):
        raise ValueError('record: \'select\' is {operator name or \'all\': TERM[+TERM...]}, got %r' % (select,))
    rules = parse_select_args([text if name == 'all' else '%s=%s' % (name, text) for name, text in select.items()])
    feather = info.get('feather') or {}
    if not isinstance(feather, dict):
        raise ValueError('record: \'feather\' is {name: sigma}, got %r' % (feather,))
    sigmas = parse_feather_args([str(v) if name == 'all' else '%s=%s' % (name, v) for name, v in feather.items()], rules)
    return rules, sigmas


def parse_refine(record):
    """The 'refine' of a record with 'select' -> {one of the selections' names or 'all': (radius, eps)}, {} when it has none.
    A record without 'select' is replayed globally, whatever else it holds.  Raises ValueError: a value that is not
    [radius, eps], a name that no selection goes by."""
    from .edit_cli import parse_refine_args
    info = record[0] if isinstance(record, list) and record else record
    refine = info.get('refine') if isinstance(info, dict) else None
    if not refine or not isinstance(info.get('select'), dict):
        return {}                                                     # (painted planes stay with their photo, and so does their refinement)
    if not (isinstance(refine, dict) and all(isinstance(k, str) and isinstance(v, (list, tuple)) and len(v) == 2 for k, v in refine.items())):
        raise ValueError('record: \'refine\' is {name: [radius, eps]}, got %r' % (refine,))
    return parse_refine_args([('%s:%s' % tuple(v)) if name == 'all' else '%s=%s:%s' % (name, v[0], v[1]) for name, v in refine.items()],
                             info['select'])


def parse_grow(record):
    """The 'grow' of a record with 'select' -> {one of the selections' names or 'all': (mode, radius)}, {} when it has none.  A
    record without 'select' is replayed globally, whatever else it holds.  Raises ValueError naming the entry: a value that
    is not [mode, radius], an unknown mode, a radius that is no whole number in 0..64, a name that no selection goes by."""
    from .edit_cli import parse_grow_args
    info = record[0] if isinstance(record, list) and record else record
    grow = info.get('grow') if isinstance(info, dict) else None
    if not grow or not isinstance(info.get('select'), dict):
        return {}                                                     # (painted planes stay with their photo, and so does what moved them)
    if not isinstance(grow, dict):
        raise ValueError('record: \'grow\' is {name: [mode, radius]}, got %r' % (grow,))
    moves = {}
    for name, value in grow.items():
        if not (isinstance(name, str) and isinstance(value, (list, tuple)) and len(value) == 2 and value[0] in ('grow', 'shrink', 'border')
                and isinstance(value[1], int) and not isinstance(value[1], bool)):
            raise ValueError('record: \'grow\': entry %r: %r is not [\'grow\' | \'shrink\' | \'border\', a whole number of pixels]' % (name, value))
        spec = [str(value[1]) if name == 'all' else '%s=%d' % (name, value[1])]
        try:
            moves.update(parse_grow_args(*[spec if value[0] == m else None for m in ('grow', 'shrink', 'border')], info['select']))
        except ValueError as e:
            raise ValueError('record: \'grow\': entry %r: %s' % (name, e))
    return moves


def parse_fill(record):
    """The 'fill' of a record -> None, or the name of the selection whose content is removed from every photo.  Raises
    ValueError naming the entry: a name whose plane is a painted mask (it stays with its photo), a name without a plane."""
    info = record[0] if isinstance(record, list) and record else record
    fill = info.get('fill') if isinstance(info, dict) else None
    if fill is None:
        return None
    if not isinstance(fill, str):
        raise ValueError('record: \'fill\' is the name a selection goes by, got %r' % (fill,))
    select, masks = info.get('select'), info.get('masks')
    if isinstance(select, dict) and fill in select:
        return fill
    if isinstance(masks, dict) and fill in masks:
        raise ValueError('record: \'fill\': %r names the painted mask %r, which belongs to one photo and is not carried to others '
                         '(edit_cli --mask stays with its photo); only a \'select\' entry can be filled on other photos' % (fill, masks[fill]))
    raise ValueError('record: \'fill\': %r names no entry of \'select\' (given: %s)'
                     % (fill, ', '.join(sorted(select)) if isinstance(select, dict) and select else 'none'))


def local_planes(ops, select, feather, refine=None, fill=None, grow=None):
    """Which planes a photo needs for `ops` under parse_local's (select, feather) -> ([(terms in user units, sigma)],
    mask_of): the distinct planes, and per step the plane's number or -1.  A named entry wins over 'all', in select and in
    feather alike: an 'all' sigma stands for every plane that has none of its own (edit_cli.feather_argument).  With
    parse_refine's `refine` a plane is (terms, sigma, (radius, eps) or None), named entries winning in the same way.  With
    parse_fill's `fill` a third value follows: the number of that name's plane, which is made whether an operation uses it
    or not and counts towards the 4.  With parse_grow's `grow` every plane gains a last value, (mode, radius) or None, named
    entries winning in the same way; growing or shrinking by 0 is None."""
    from .edit_cli import parse_select_terms
    planes, mask_of = [], []

    def plane_of(name):
        plane = (tuple(parse_select_terms(select[name])), float(feather.get(name, feather.get('all', 0.0))))
        if refine is not None:
            pair = refine.get(name, refine.get('all'))
            plane += (tuple(pair) if pair is not None and pair[0] > 0 else None,)
        if grow is not None:
            move = grow.get(name, grow.get('all'))
            plane += (tuple(move) if move is not None and (move[1] > 0 or move[0] == 'border') else None,)
        if plane not in planes:
            planes.append(plane)
        return planes.index(plane)
    for op in ops:
        name = ACTIONS[op] if ACTIONS[op] in select else 'all'
        mask_of.append(plane_of(name) if name in select else -1)
    if fill is not None:
        fill_no = plane_of(fill)
    if len(planes) > MAX_PLANES:
        raise ValueError('record: the operations%s name %d distinct selections, the replay takes %d'
                         % (' and \'fill\'' if fill is not None else '', len(planes), MAX_PLANES))
    return (planes, mask_of) if fill is None else (planes, mask_of, fill_no)


def apply_record_local(images, ops, params, select, feather, multi_img=False, device=None, refine=None, fill=None, grow=None):
    """apply_record under the selections of parse_local: the same result layout.  One upload; per group of photos that
    together name at most 4 planes: one select_u8 launch, refine_u8's four where parse_refine's `refine` gives a radius,
    feather_u8 where a sigma is given, one replay launch.  A 'wand' / 'wand8' term is resolved per photo at that photo's
    size: its seed pixel from the fractions of the rule, one functional.region_u8 job per distinct (seed, tolerance,
    connectivity) of the photo, in calls of at most 4 in front of the group's select launch; the region planes lie in room
    reserved on the device behind the uploaded buffer (no byte is uploaded for it), where the select launch reads them as
    'plane' terms.  With parse_fill's `fill` the photos of a group are filled in place under their own plane of that name by
    one functional.fill_u8 call, behind feather and in front of the replay.  With parse_grow's `grow` one functional.morph_u8
    call per group moves the planes' boundaries in place, behind the select launch and in front of refine."""
    from . import functional as T
    from .edit import refine_eps2, select_terms, upload_with_room, wand_keys, wand_resolved
    assert (MAX_STEPS, MAX_JOBS, PARAM_PAD, MAX_PLANES) == (T.REPLAY_MAX_STEPS, T.REPLAY_MAX_JOBS, T.PARAM_PAD, T.REPLAY_MAX_MASKS)
    if grow:
        planes, mask_of, *fill_no = local_planes(ops, select, feather, refine or {}, fill, grow)
        moves = [p[3] for p in planes]
        planes = [p[:3] for p in planes]
    else:
        planes, mask_of, *fill_no = local_planes(ops, select, feather, refine or None, fill)
        moves = [None] * len(planes)
    snaps = [(p[2][0], refine_eps2(p[2][1])) if len(p) == 3 and p[2] else None for p in planes]      # before any device use
    planes = [p[:2] for p in planes]
    if not planes:                                                    # no operation of the list is selected for
        return apply_record(images, ops, params, multi_img, device)
    shapes = [tuple(int(v) for v in im.shape[:2]) for im in images]
    rules = [[select_terms(terms, h, w, 'record') for terms, _ in planes] for h, w in shapes]      # before any device use
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    buffer, descs = T.pack_u8(images)
    wands = [wand_keys(r) for r in rules]                             # per photo: its own seed pixels
    if any(wands):
        wand_at, pos = [], buffer.numel()
        for (h, w), keys in zip(shapes, wands):
            wand_at.append({key: pos + k * h * w for k, key in enumerate(keys)})
            pos += len(keys) * h * w
        dev_buffer, _, descs, _keep = upload_with_room(buffer, descs, pos - buffer.numel(), device)
        rules = [[wand_resolved(terms, at) for terms in r] for r, at in zip(rules, wand_at)]
    else:
        dev_buffer, _, descs, _keep = T.upload_packed(buffer, descs, device)
    offsets = [int(d['offset']) for d in descs]
    row = torch.zeros(MAX_STEPS, PARAM_PAD)
    row[:len(ops)] = torch.as_tensor(np.asarray(params, np.float32).reshape(len(ops), PARAM_PAD))
    row = row.to(device)
    prefixes = list(range(1, len(ops) + 1)) if multi_img else [len(ops)]
    steps = []
    per = MAX_PLANES // len(planes)                                   # photos of a group
    for a in range(0, len(images), per):
        group = list(range(a, min(a + per, len(images))))
        sel_jobs, move_jobs, snap_jobs, soft_jobs, jobs, where, at, pos = [], [], [], [], [], {}, 0, 0
        for i in group:
            h, w = shapes[i]
            for k, (_, sigma) in enumerate(planes):
                where[i, k] = len(sel_jobs)
                sel_jobs.append((offsets[i], at, h, w, rules[i][k]))
                if moves[k]:
                    move_jobs.append((at, at, h, w, moves[k][1], moves[k][0]))
                if snaps[k]:
                    snap_jobs.append((offsets[i], at, at, h, w) + snaps[k])
                if sigma > 0.0:
                    soft_jobs.append((at, at, h, w, sigma))
                at += h * w
            for n in prefixes:
                jobs.append((offsets[i], pos, h, w, list(ops[:n]), [where[i, k] if k >= 0 else -1 for k in mask_of[:n]]))
                pos += 3 * h * w
        wand_jobs = [(offsets[i], wand_at[i][key]) + shapes[i] + key for i in group for key in wands[i]]
        for k in range(0, len(wand_jobs), T.REGION_MAX_JOBS):
            T.region_u8(dev_buffer, wand_jobs[k:k + T.REGION_MAX_JOBS], out=dev_buffer)
        plane_buffer = T.select_u8(dev_buffer, sel_jobs)
        if move_jobs:                                                 # at most 4 planes to a group: one call
            T.morph_u8(plane_buffer, move_jobs)
        if snap_jobs:
            T.refine_u8(dev_buffer, plane_buffer, snap_jobs)
        if soft_jobs:
            T.feather_u8(plane_buffer, soft_jobs)
        if fill_no:                                                   # at most 4 photos to a group: one call
            T.fill_u8(dev_buffer, plane_buffer, [(offsets[i], sel_jobs[where[i, fill_no[0]]][1], offsets[i]) + shapes[i] for i in group], out=dev_buffer)
        out = T.replay_u8_any(dev_buffer, jobs, row.unsqueeze(0).expand(len(jobs), -1, -1).contiguous(), plane_buffer,
                              [job[1] for job in sel_jobs]).cpu().numpy()
        for i in group:
            h, w = shapes[i]
            mine = [job for job in jobs if job[0] == offsets[i]]
            steps.append(np.stack([out[job[1]:job[1] + 3 * h * w].reshape(h, w, 3) for job in mine]))
    return steps


def pick_wrapper(ops):
    """The name of the functional wrapper that serves `ops`: replay_u8 keeps the lists it takes (it is the cheaper
    kernel), replay_u8_stencils takes those that repeat the sharpness.  The rule itself is functional.replay_u8_pick's."""
    from . import functional as T
    return T.replay_u8_pick([(0, 0, 0, 0, ops)])


def job_lists(shapes, offsets, ops, multi_img=False):
    """shapes: (h, w) per photo, offsets: the photos' first bytes in the uploaded buffer -> the launches, each a list of at
    most 64 (photo index, job) with job = (src_offset, out_offset, h, w, ops prefix).  A photo is one job (the whole
    list), with multi_img one job per prefix; out_offset counts from the launch's own output buffer."""
    flat = []
    for i, ((h, w), off) in enumerate(zip(shapes, offsets)):
        for n in (range(1, len(ops) + 1) if multi_img and ops else [len(ops)]):
            flat.append((i, int(off), int(h), int(w), list(ops[:n])))
    launches = []
    for a in range(0, len(flat), MAX_JOBS):
        pos, launch = 0, []
        for i, off, h, w, prefix in flat[a:a + MAX_JOBS]:
            launch.append((i, (off, pos, h, w, prefix)))
            pos += 3 * h * w
        launches.append(launch)
    return launches


def apply_record(images, ops, params, multi_img=False, device=None):
    """images: decoded photos, uint8 (h, w, 3) arrays -> per photo a (J, h, w, 3) uint8 array, J = 1, or the number of
    operators (at least 1) with multi_img, the last picture being the result.  One upload; ceil(jobs / 64) launches."""
    from . import functional as T
    assert (MAX_STEPS, MAX_JOBS, PARAM_PAD) == (T.REPLAY_MAX_STEPS, T.REPLAY_MAX_JOBS, T.PARAM_PAD)
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    buffer, descs = T.pack_u8(images)
    dev_buffer, _, descs, _keep = T.upload_packed(buffer, descs, device)
    shapes = [(int(d['h']), int(d['w'])) for d in descs]
    row = torch.zeros(MAX_STEPS, PARAM_PAD)
    row[:len(ops)] = torch.as_tensor(np.asarray(params, np.float32).reshape(len(ops), PARAM_PAD))
    row = row.to(device)
    steps = [[] for _ in images]
    for launch in job_lists(shapes, [int(d['offset']) for d in descs], ops, multi_img):
        jobs = [job for _, job in launch]
        out = T.replay_u8_any(dev_buffer, jobs, row.unsqueeze(0).expand(len(jobs), -1, -1).contiguous()).cpu().numpy()
        for i, (_, pos, h, w, _) in launch:
            steps[i].append(out[pos:pos + 3 * h * w].reshape(h, w, 3))
    return [np.stack(s) for s in steps]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--record', required=True, help='NAME.json as edit_cli wrote it (or edited by hand)')
    ap.add_argument('--img', required=True, nargs='+', help='the photos the record is applied to')
    ap.add_argument('--multi_img', action='store_true', help='also write the picture after each operator')
    ap.add_argument('--save_dir', default='output/demo_output')
    args = ap.parse_args(argv)
    with open(args.record) as f:
        record = json.load(f)
    request, ops, params = parse_record(record)                       # before any decode or device use
    local = parse_local(record)
    refine = parse_refine(record)
    fill = parse_fill(record)
    grow = parse_grow(record)
    images = [decode_image(p) for p in args.img]
    from .edit_cli import write_outputs
    infos = []
    if local is None:
        results, carried = apply_record(images, ops, params, args.multi_img), {}
    else:
        results = apply_record_local(images, ops, params, local[0], local[1], args.multi_img, refine=refine, fill=fill, **({'grow': grow} if grow else {}))
        carried = {'select': local[0], 'feather': local[1] or None, 'fill': fill}
        if refine:
            carried['refine'] = refine
        if grow:
            carried['grow'] = grow
    for path, img, steps in zip(args.img, images, results):
        info = write_outputs(args.save_dir, path, request, img, steps, ops, params, args.multi_img, **carried)
        info['record'] = args.record
        name = os.path.splitext(os.path.basename(path))[0]
        with open(os.path.join(args.save_dir, name, name + '.json'), 'w') as f:
            json.dump([info], f)
        infos.append(info)
        print('%s: %s -> %s' % (os.path.basename(args.record), ', '.join(n for n, _ in info['operations']) or '(no operator)',
                                os.path.join(args.save_dir, name, info['output'])))
    return infos


if __name__ == '__main__':
    main()
