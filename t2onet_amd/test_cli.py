"""Score a checkpoint on a split (the reference's experiments/t2onet/test_seq2seqL1.py __main__, :145-160):

    python -m t2onet_amd.test_cli --checkpoint output/.../checkpoint_best/model.pth --img_dir data/FiveK/images \\
        --anno_dir data/FiveK/annotations --vocab_dir data/language [--phase test] [--session 1] [--short_size 600] \\
        [--device_resize] [--requests FILE] [--save_dir DIR] [--save_images] [--max_items N]

walks data.FiveK(phase) at batch size 1 (test_seq2seqL1.py:153-154) with the short side at --short_size, runs
evaluate.test_on_device(is_test=True) -- one fused metrics launch per image, the table read once -- prints the reference's
three lines (input / output L1, input / output SSIM, inference init / L1 dist) and writes <save_dir>/metrics.json:
{'checkpoint', 'phase', 'items', 'in_L1', 'out_L1', 'in_SSIM', 'out_SSIM', 'init_dist', 'dist', 'records': [{'name',
'request', 'operations': [(operator name, its parameters), ...]}, ...]} with the operators in front of the first END as
edit_cli.operations_record names them.  The five means are in_L1, out_L1, in_SSIM, out_SSIM (ImageEvaluator's running
means) and dist (test()'s running mean of the output L1; init_dist is its input counterpart).

--requests FILE (one request per line): also runs evaluate.test_variance_on_device over these requests (the reference's
test_variance, :99-142) and adds 'variance'.  The reference takes its ten sentences from utils/eval.py:11; they are data,
not part of this package.
--save_images: <name>_in.png, <name>_out.png and <name>_gt.png per item under <save_dir>, at the loader's size.

FID (utils/eval.py:20-47) stays out of scope: it needs torchvision's InceptionV3 weights, which are not available here
(evaluate.py).
"""
import argparse
import json
import os

import torch

from . import evaluate
from . import functional as T
from .edit import first_end
from .edit_cli import load_vocab, operations_record


def read_requests(path):
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def save_pictures(save_dir, name, img_x, img_out, img_y):
    """<name>_in / _out / _gt .png from (1,3,H,W) fp32 GPU images: functional.to_u8_hwc (the writers' * 255 truncated), PIL."""
    from PIL import Image
    u8 = T.to_u8_hwc(torch.cat([img_x, img_out, img_y], 0)).cpu().numpy()
    for tag, pic in zip(('in', 'out', 'gt'), u8):
        Image.fromarray(pic).save(os.path.join(save_dir, '%s_%s.png' % (name, tag)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--checkpoint', required=True, help='state_dict of the Actor (model.pth)')
    ap.add_argument('--img_dir', default='data/FiveK/images')
    ap.add_argument('--anno_dir', default='data/FiveK/annotations')
    ap.add_argument('--vocab_dir', default='data/language')
    ap.add_argument('--phase', default='test')
    ap.add_argument('--session', type=int, default=1)
    ap.add_argument('--short_size', type=int, default=600)
    ap.add_argument('--device_resize', action='store_true', help='the loader only decodes; the resize runs on the GPU')
    ap.add_argument('--requests', default=None, help='a file with one request per line: also report the request variance')
    ap.add_argument('--save_dir', default='output/test_output')
    ap.add_argument('--save_images', action='store_true', help='write <name>_in / _out / _gt .png per item')
    ap.add_argument('--max_items', type=int, default=None)
    ap.add_argument('--num_workers', type=int, default=1)
    args = ap.parse_args(argv)

    from torch.utils.data import DataLoader, Subset
    from . import default_options
    from .actor import Actor
    from .data import DeviceBatches, FiveK, collate_raw
    opt = default_options(vocab_dir=args.vocab_dir, session=args.session)
    device = torch.device('cuda', torch.cuda.current_device())
    model = Actor(opt)
    model.load_state_dict(torch.load(args.checkpoint, map_location='cpu'), strict=False)      # as the reference (:150)
    model.to(device)

    def make_loader():
        raw_kw = dict(collate_fn=collate_raw, pin_memory=True) if args.device_resize else {}
        dataset = FiveK(args.img_dir, args.anno_dir, args.phase, args.session, short_size=args.short_size, raw=args.device_resize)
        items = dataset if args.max_items is None else Subset(dataset, range(min(args.max_items, len(dataset))))
        loader = DataLoader(items, batch_size=1, shuffle=False, num_workers=args.num_workers, **raw_kw)
        if args.device_resize:
            loader = DeviceBatches(loader, device=device, short_size=args.short_size, images_only=True)
        return loader, dataset

    loader, dataset = make_loader()
    os.makedirs(args.save_dir, exist_ok=True)
    kept = []                                            # device tensors: read after the loop, not between two images

    def on_batch(itr, data, pred_imgs, first, pred_ops, pred_params):
        kept.append((data[3][0], pred_ops, torch.stack(pred_params, 1)))
        if args.save_images:
            name = os.path.splitext(os.path.basename(dataset.data[itr - 1]['input']))[0]
            name = name[:-3] if name.endswith('_in') else name           # FiveK inputs are <name>_in.jpg
            out = pred_imgs[int(first[0])]                   # (saving reads the pictures back anyway; batch size 1)
            save_pictures(args.save_dir, name, data[0].to(device), out, data[1].to(device))

    init_dist, dist, metrics = evaluate.test_on_device(model, loader, opt, is_test=True, device=device, on_batch=on_batch)
    records = []
    for k, (request, pred_ops, params) in enumerate(kept):
        ops_vocab = pred_ops[0].cpu().tolist()
        n = first_end(ops_vocab, opt.end_id)
        records.append({'name': dataset.data[k]['input'], 'request': request,
                        'operations': operations_record([int(o) - 3 for o in ops_vocab[:n]], params[0, :n].cpu())})
    result = dict(metrics, checkpoint=args.checkpoint, phase=args.phase, items=len(records), init_dist=init_dist, dist=dist,
                  records=records)
    if args.requests:
        requests = read_requests(args.requests)
        vocab2id = load_vocab(args.vocab_dir, args.session, opt.dataset)
        result['variance'] = evaluate.test_variance_on_device(model, make_loader()[0], opt, requests, vocab2id, device=device)
    with open(os.path.join(args.save_dir, 'metrics.json'), 'w') as f:
        json.dump(result, f, indent=1)
    return result


if __name__ == '__main__':
    main()
