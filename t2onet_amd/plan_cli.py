"""Generate the planned-action set that training reads (preprocess/gen_greedy_seqs_FiveK.py:20-83): for every item of
the FiveK training split a beam search over operator sequences from the input to the expert-retouched image, written as

    save_dir/train{i}/{i:05d}.json    {'request', 'init distance', 'operation sequence': [[(name, params, dist), ...], ...]}
    save_dir/train{i}/input.jpg, target.jpg, edit{k}.jpg (the images of the best sequence)

which is exactly what data.FiveKAct / `train_cli --act_dir` load.  The reference plans one pair at a time with scipy;
here `--pairs_per_batch` pairs are planned in lock-step by planner.beam_search_pairs (optimizer 'batched'), the
multi-parameter fits of all of them sharing launches.

    python -m t2onet_amd.plan_cli --img_dir data/FiveK/images --anno_dir data/FiveK/annotations --save_dir output/actions_set_1

Images are written with PIL as RGB JPEG at the reference's 8-bit rounding (utils/visual_utils.py:50-58: * 255, truncated);
the reference writes them with cv2 (absent here), so byte parity of the JPEG encoding is not claimed.  Items whose record
already exists are skipped: an interrupted run is resumed by running it again.

`--dataset GIER` makes the GIER action set (preprocess/gen_greedy_seqs_GIER.py:40-96), one directory per image pair:

    save_dir/<name>/acts.json         the same three keys, + 'local operators': the names fitted under a mask
    save_dir/<name>/input.jpg, target.jpg, edit{k}.jpg          name = the input file's name up to the first '_'

which is what gier.GIERDatasetAct / `train_cli --dataset GIER --act_dir` load.

    python -m t2onet_amd.plan_cli --dataset GIER --data_dir data/GIER --vocab_dir data/language --save_dir output/GIER_actions_set_1 --local

Without --local it is the global search over [0,1,2,3,5,6].  With --local a candidate of an operator that the pair
annotates a region for is fitted, scored and executed under that region -- the union plane of the annotated masks, a
count, made at --img_size for the whole batch by ONE functional.rle_union_u8 launch from the run lengths (nothing is
decoded on the host) -- and `white` (color_bg) joins the candidates of the pairs that annotate a region for it.  The
reference's own masked search is not in its checkout (its script calls a beam_search that takes no masks); the
semantics are the ones planner.beam_search documents.
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from .data import ACTIONS, FiveK, collate_raw, device_batch

OPERATIONS = [0, 1, 2, 3, 5, 6]                # gen_greedy_seqs_FiveK.py:39
GIER_LOCAL_OPERATIONS = [0, 1, 2, 3, 5, 6, 7]  # + white, for the pairs that annotate a region for it; inpaint (4) never
GIER_OP_VOCAB_BASE = 3                         # executor operator = GIER operator-vocabulary id - 3 (actor.py:165)
JPEG_QUALITY = 95                              # cv2.imwrite's default


def tensor2img(tensor):
    """(1,3,H,W) or (3,H,W) in [0,1] -> (H,W,3) uint8 RGB, rounded as utils/visual_utils.py:50-58 (that one returns BGR
    for cv2.imwrite; PIL takes RGB).  A GPU tensor is converted there (functional.to_u8_hwc: the same product and
    truncation), so the bytes cross the bus, not the floats."""
    if tensor.is_cuda and tensor.dtype == torch.float32:
        from . import functional as T
        return T.to_u8_hwc(tensor.detach().reshape(1, 3, *tensor.shape[-2:]))[0].cpu().numpy()
    out = tensor.detach().reshape(3, *tensor.shape[-2:]).permute(1, 2, 0) * 255
    return out.cpu().numpy().astype(np.uint8)


def record_path(save_dir, phase, i):
    return os.path.join(save_dir, '{}{}'.format(phase, i), '{:05d}.json'.format(i))


def write_record(save_dir, phase, i, request, init_dist, act_seqs, img_seqs, input_img, target_img):
    """Item i's record and images (gen_greedy_seqs_FiveK.py:66-83).  act_seqs / img_seqs: what the beam search returned --
    per surviving sequence its [(name, param list, dist), ...] and its intermediate images; only the best sequence's
    images are written, as edit{k}.jpg.  Needs no GPU.  The record is written last: its presence marks the item done."""
    from PIL import Image
    item_dir = os.path.dirname(record_path(save_dir, phase, i))
    os.makedirs(item_dir, exist_ok=True)
    Image.fromarray(tensor2img(input_img)).save(os.path.join(item_dir, 'input.jpg'), quality=JPEG_QUALITY)
    Image.fromarray(tensor2img(target_img)).save(os.path.join(item_dir, 'target.jpg'), quality=JPEG_QUALITY)
    if len(img_seqs) > 0:
        for k, img in enumerate(img_seqs[0]):
            Image.fromarray(tensor2img(img)).save(os.path.join(item_dir, 'edit{}.jpg'.format(k)), quality=JPEG_QUALITY)
    info = {'request': request, 'init distance': float(init_dist),
            'operation sequence': [[[name, [float(v) for v in params], float(dist)] for name, params, dist in seq] for seq in act_seqs]}
    tmp = record_path(save_dir, phase, i) + '.tmp'
    with open(tmp, 'w') as f:
        json.dump(info, f)
    os.replace(tmp, record_path(save_dir, phase, i))
    return info


def gier_record_path(save_dir, name):
    return os.path.join(save_dir, name, 'acts.json')


def write_gier_record(save_dir, name, request, init_dist, act_seqs, img_seqs, input_img, target_img, local_ops=()):
    """One pair's record and images (gen_greedy_seqs_GIER.py:79-96): the FiveK record's three keys in its exact shape, plus
    'local operators' (the names fitted under a mask; GIERDatasetAct.get_act does not read it).  Needs no GPU.  acts.json
    is written last, through a temporary name: its presence marks the pair done."""
    from PIL import Image
    item_dir = os.path.join(save_dir, name)
    os.makedirs(item_dir, exist_ok=True)
    Image.fromarray(tensor2img(input_img)).save(os.path.join(item_dir, 'input.jpg'), quality=JPEG_QUALITY)
    Image.fromarray(tensor2img(target_img)).save(os.path.join(item_dir, 'target.jpg'), quality=JPEG_QUALITY)
    if len(img_seqs) > 0:
        for k, img in enumerate(img_seqs[0]):
            Image.fromarray(tensor2img(img)).save(os.path.join(item_dir, 'edit{}.jpg'.format(k)), quality=JPEG_QUALITY)
    info = {'request': request, 'init distance': float(init_dist),
            'operation sequence': [[[name_, [float(v) for v in params], float(dist)] for name_, params, dist in seq] for seq in act_seqs],
            'local operators': [str(n) for n in local_ops]}
    tmp = gier_record_path(save_dir, name) + '.tmp'
    with open(tmp, 'w') as f:
        json.dump(info, f)
    os.replace(tmp, gier_record_path(save_dir, name))
    return info


def gier_batch_planes(items, size, device):
    """The union planes of a batch of GIER.get_pair_item items (is_load_mask='rle') at (size, size): ONE rle_union_u8
    launch for all of them, from the run lengths.  Returns, per item, {executor operator: (size,size) uint8 GPU plane}
    for the executor operators the pair annotates a region for."""
    from . import functional as T
    masks, jobs, seen, where = [], [], {}, []
    for b, it in enumerate(items):
        for key, (rles, mask_ids) in it.get('mask_rle', {}).items():
            op = int(key) - GIER_OP_VOCAB_BASE
            if op not in GIER_LOCAL_OPERATIONS:
                continue
            sel = []
            for i in mask_ids:
                at = seen.get(id(rles[i]))
                if at is None:
                    at = seen[id(rles[i])] = len(masks)
                    masks.append(rles[i])
                sel.append(at)
            where.append((b, op))
            jobs.append((sel, len(jobs) * size * size, size, size))
    out = [{} for _ in items]
    if jobs:
        planes = T.rle_union_u8(masks, jobs, device)[:len(jobs) * size * size].view(len(jobs), size, size)
        for k, (b, op) in enumerate(where):
            out[b][op] = planes[k]
    return out


def gier_todo(save_dir, names, overwrite=False):
    """names: {pair id: directory name}.  The pair ids still to plan, in order: those without an acts.json (all of them with
    overwrite) -- an interrupted run is resumed by running it again."""
    return [i for i in sorted(names) if overwrite or not os.path.exists(gier_record_path(save_dir, names[i]))]


def main_gier(args):
    """--dataset GIER: every pair of the training split (gen_greedy_seqs_GIER.py:40-96) -> the number of records written."""
    from . import Executor, default_options, planner
    from .gier import ACTIONS as GIER_ACTIONS, GIER
    device = torch.device('cuda', torch.cuda.current_device())
    executor = Executor(default_options()).to(device)
    index = GIER(args.data_dir, args.vocab_dir, 'train', args.data_mode, 'rle' if args.local else False, args.session, args.img_size)
    operations = GIER_LOCAL_OPERATIONS if args.local else OPERATIONS
    max_step = len(operations) if args.max_step is None else args.max_step
    stop = len(index) if args.limit is None else min(len(index), args.start + args.limit)
    names = {i: index.op_data[i]['input'].split('_')[0] for i in range(args.start, stop)}
    todo = gier_todo(args.save_dir, names, args.overwrite)
    written = 0
    for b0 in range(0, len(todo), args.pairs_per_batch):
        batch = todo[b0:b0 + args.pairs_per_batch]
        tik = time.time()
        items = [index.get_pair_item(i) for i in batch]
        inputs = [it['input'].unsqueeze(0).to(device) for it in items]
        targets = [it['output'].unsqueeze(0).to(device) for it in items]
        planes = gier_batch_planes(items, args.img_size, device) if args.local else None
        results = planner.beam_search_pairs(inputs, targets, None, executor, None, args.beam_size, operations, GIER_ACTIONS,
                                            max_step, args.err, 'L1', replace=False, masks=planes)
        for k, (i, it, img_x, img_y, (act_seqs, img_seqs)) in enumerate(zip(batch, items, inputs, targets, results)):
            init_dist = planner.get_dist(img_x, img_y).item()
            local = [GIER_ACTIONS[op] for op in sorted(planes[k])] if args.local else []
            write_gier_record(args.save_dir, names[i], it['request'], init_dist, act_seqs, img_seqs, img_x, img_y, local)
            written += 1
        print('{}/{} pairs, {:.2f}s per pair'.format(b0 + len(batch), len(todo), (time.time() - tik) / len(batch)), flush=True)
    return written


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--dataset', default='FiveK', choices=['FiveK', 'GIER'])
    ap.add_argument('--data_dir', default='data/GIER', help='GIER: the directory of images/, masks/, splits/')
    ap.add_argument('--vocab_dir', default='data/language', help='GIER: the directory of the two vocabulary files')
    ap.add_argument('--data_mode', default='global', help="GIER: the split families to intersect, e.g. 'global', 'valid', 'shapeAlign+valid'")
    ap.add_argument('--local', action='store_true', help='GIER: fit the operators a pair annotates a region for under that region')
    ap.add_argument('--img_dir', default='data/FiveK/images')
    ap.add_argument('--anno_dir', default='data/FiveK/annotations')
    ap.add_argument('--save_dir', default='output/actions_set_1')
    ap.add_argument('--img_size', type=int, default=None, help='default: 128 (FiveK), 256 (GIER)')
    ap.add_argument('--session', type=int, default=None, help='default: 1 (FiveK), 3 (GIER)')
    ap.add_argument('--beam_size', type=int, default=3)
    ap.add_argument('--max_step', type=int, default=None, help='default: the number of candidate operations')
    ap.add_argument('--err', type=float, default=1e-2)
    ap.add_argument('--pairs_per_batch', type=int, default=8)
    ap.add_argument('--start', type=int, default=0, help='first item')
    ap.add_argument('--limit', type=int, default=None, help='number of items from --start on (default: to the end)')
    ap.add_argument('--overwrite', action='store_true', help='plan items again whose record exists')
    ap.add_argument('--device_resize', action='store_true', help='resize the decoded pairs on the GPU (one launch per batch)')
    args = ap.parse_args(argv)
    gier = args.dataset == 'GIER'
    if args.local and not gier:
        ap.error('--local needs --dataset GIER (FiveK has no masks)')
    if gier and args.device_resize:
        ap.error('--device_resize is the FiveK loader\'s')
    args.img_size = (256 if gier else 128) if args.img_size is None else args.img_size
    args.session = (3 if gier else 1) if args.session is None else args.session
    if not gier and args.max_step is None:
        args.max_step = len(OPERATIONS)
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.dataset == 'GIER':
        return main_gier(args)

    from . import Executor, default_options, planner
    device = torch.device('cuda', torch.cuda.current_device())
    executor = Executor(default_options()).to(device)
    phase = 'train'
    dataset = FiveK(args.img_dir, args.anno_dir, phase, args.session, args.img_size, raw=args.device_resize)
    stop = len(dataset) if args.limit is None else min(len(dataset), args.start + args.limit)
    todo = [i for i in range(args.start, stop) if args.overwrite or not os.path.exists(record_path(args.save_dir, phase, i))]
    written = 0
    for b0 in range(0, len(todo), args.pairs_per_batch):
        batch = todo[b0:b0 + args.pairs_per_batch]
        tik = time.time()
        items = [dataset[i] for i in batch]
        if args.device_resize:
            img_x, img_y = device_batch(collate_raw(items), args.img_size, device)[:2]
            inputs, targets = [img_x[k:k + 1] for k in range(len(items))], [img_y[k:k + 1] for k in range(len(items))]
        else:
            inputs = [it[0].unsqueeze(0).to(device) for it in items]
            targets = [it[1].unsqueeze(0).to(device) for it in items]
        results = planner.beam_search_pairs(inputs, targets, None, executor, None, args.beam_size, OPERATIONS, ACTIONS,
                                            args.max_step, args.err, 'L1', replace=False)
        for i, it, img_x, img_y, (act_seqs, img_seqs) in zip(batch, items, inputs, targets, results):
            init_dist = planner.get_dist(img_x, img_y).item()
            write_record(args.save_dir, phase, i, it[3], init_dist, act_seqs, img_seqs, img_x, img_y)
            written += 1
        print('{}/{} items, {:.2f}s per pair'.format(b0 + len(batch), len(todo), (time.time() - tik) / len(batch)), flush=True)
    return written


if __name__ == '__main__':
    main()
