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
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from .data import ACTIONS, FiveK, collate_raw, device_batch

OPERATIONS = [0, 1, 2, 3, 5, 6]                # gen_greedy_seqs_FiveK.py:39
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--img_dir', default='data/FiveK/images')
    ap.add_argument('--anno_dir', default='data/FiveK/annotations')
    ap.add_argument('--save_dir', default='output/actions_set_1')
    ap.add_argument('--img_size', type=int, default=128)
    ap.add_argument('--session', type=int, default=1)
    ap.add_argument('--beam_size', type=int, default=3)
    ap.add_argument('--max_step', type=int, default=len(OPERATIONS))
    ap.add_argument('--err', type=float, default=1e-2)
    ap.add_argument('--pairs_per_batch', type=int, default=8)
    ap.add_argument('--start', type=int, default=0, help='first item')
    ap.add_argument('--limit', type=int, default=None, help='number of items from --start on (default: to the end)')
    ap.add_argument('--overwrite', action='store_true', help='plan items again whose record exists')
    ap.add_argument('--device_resize', action='store_true', help='resize the decoded pairs on the GPU (one launch per batch)')
    args = ap.parse_args(argv)

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
