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
Global edits only: masks stay with edit_cli --mask.
"""
import argparse
import json
import os

import numpy as np
import torch

from .data import ACT2PN, ACTIONS, decode_image

MAX_STEPS, MAX_JOBS, PARAM_PAD = 8, 64, 24          # functional.REPLAY_MAX_STEPS, REPLAY_MAX_JOBS, PARAM_PAD (checked in apply_record)


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
        request, ops, params = parse_record(json.load(f))             # before any decode or device use
    images = [decode_image(p) for p in args.img]
    from .edit_cli import write_outputs
    infos = []
    for path, img, steps in zip(args.img, images, apply_record(images, ops, params, args.multi_img)):
        info = write_outputs(args.save_dir, path, request, img, steps, ops, params, args.multi_img)
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
