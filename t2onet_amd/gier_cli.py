"""Score a checkpoint on a GIER split (the reference's experiments/t2onet/test_GIER_seq2seqL1.py __main__): test_cli's loop
and metrics.json over gier.GIERDataset instead of data.FiveK.

    python -m t2onet_amd.gier_cli --checkpoint output/.../checkpoint_best/model.pth --data_dir data/GIER \\
        --data_mode shapeAlign --vocab_dir data/language [--load_mask] [--phase test] [--session 3] [--requests FILE] \\
        [--save_dir DIR] [--save_images] [--max_items N]

walks gier.GIERDataset(phase) -- one item per request -- at batch size 1 with the short side at 600, runs
evaluate.test_on_device(is_test=True), prints the reference's three lines and writes <save_dir>/metrics.json with the keys
test_cli writes ('dataset' and 'data_mode' added).  Without --load_mask every edit is global, as the reference's script sets
is_load_mask = False.  --load_mask: the annotated COCO run-length masks of each item become a gier.MaskTable at the image's
size (MaskTable.from_rle: the run lengths uploaded, unioned on the GPU, one upload and one launch per item) and the episode
edits locally where the chosen operator has a mask, with no host read per step.
--requests FILE and --save_images: as test_cli (pictures are <input name>_req<k>_in / _out / _gt .png: several requests
share an input).  This is a module of its own so that the FiveK command stays exactly as it is.
"""
import argparse
import json
import os

import torch

from . import evaluate
from .edit import first_end
from .edit_cli import load_vocab, operations_record
from .test_cli import read_requests, save_pictures


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--checkpoint', required=True, help='state_dict of the Actor (model.pth)')
    ap.add_argument('--dataset', default='GIER', choices=['GIER'])
    ap.add_argument('--data_dir', default='data/GIER', help='the directory holding images/, masks/ and splits/')
    ap.add_argument('--data_mode', default='shapeAlign', help='split families joined with +: full, valid, shapeAlign, shapeAlign_nonCrop, global')
    ap.add_argument('--load_mask', action='store_true', help='local edits under the annotated masks (a MaskTable per item, built on the GPU)')
    ap.add_argument('--vocab_dir', default='data/language')
    ap.add_argument('--phase', default='test')
    ap.add_argument('--session', type=int, default=3)
    ap.add_argument('--requests', default=None, help='a file with one request per line: also report the request variance')
    ap.add_argument('--save_dir', default='output/test_output')
    ap.add_argument('--save_images', action='store_true', help='write <name>_req<k>_in / _out / _gt .png per item')
    ap.add_argument('--max_items', type=int, default=None)
    ap.add_argument('--num_workers', type=int, default=1)
    return ap.parse_args(argv)


def _collate_one(items):
    """Batch size 1 over gier._Tuples items: tensors get a batch axis, the request and the run-length dict a list."""
    it = items[0]
    return (it[0].unsqueeze(0), it[1].unsqueeze(0), it[2].unsqueeze(0), [it[3]]) + (([it[4]],) if len(it) > 4 else ())


def main(argv=None):
    args = parse_args(argv)

    from torch.utils.data import DataLoader, Subset
    from . import default_options
    from .actor import Actor
    from .gier import GIERDataset, MaskTable, _Tuples
    opt = default_options(vocab_dir=args.vocab_dir, session=args.session, dataset='GIER')
    device = torch.device('cuda', torch.cuda.current_device())
    model = Actor(opt)
    model.load_state_dict(torch.load(args.checkpoint, map_location='cpu'), strict=False)      # as the reference
    model.to(device)

    def make_loader():
        dataset = GIERDataset(args.data_dir, args.vocab_dir, args.phase, args.data_mode, 'rle' if args.load_mask else False, args.session)
        tuples = _Tuples(dataset, with_masks=args.load_mask)
        items = tuples if args.max_items is None else Subset(tuples, range(min(args.max_items, len(tuples))))
        return DataLoader(items, batch_size=1, shuffle=False, num_workers=args.num_workers, collate_fn=_collate_one), dataset

    loader, dataset = make_loader()
    names = [dataset.GIER.op_data[dataset.GIER.ReqId2PairId[k]]['input'] for k in range(len(dataset))]
    mask_fn = None
    if args.load_mask:
        n_vocab = len(dataset.op_vocab2id)

        def mask_fn(data, img_x):                            # one upload + one launch per item; nothing waits on the host
            return MaskTable.from_rle(data[4], tuple(img_x.shape[-2:]), n_vocab, device)
    os.makedirs(args.save_dir, exist_ok=True)
    kept = []                                                # device tensors: read after the loop, not between two images

    def on_batch(itr, data, pred_imgs, first, pred_ops, pred_params):
        kept.append((data[3][0], pred_ops, torch.stack(pred_params, 1)))
        if args.save_images:
            name = '%s_req%04d' % (os.path.splitext(os.path.basename(names[itr - 1]))[0], itr - 1)
            out = pred_imgs[int(first[0])]                   # (saving reads the pictures back anyway; batch size 1)
            save_pictures(args.save_dir, name, data[0].to(device), out, data[1].to(device))

    init_dist, dist, metrics = evaluate.test_on_device(model, loader, opt, is_test=True, device=device, on_batch=on_batch, mask_fn=mask_fn)
    records = []
    for k, (request, pred_ops, params) in enumerate(kept):
        ops_vocab = pred_ops[0].cpu().tolist()
        n = first_end(ops_vocab, opt.end_id)
        records.append({'name': names[k], 'request': request,
                        'operations': operations_record([int(o) - 3 for o in ops_vocab[:n]], params[0, :n].cpu())})
    result = dict(metrics, checkpoint=args.checkpoint, dataset='GIER', data_mode=args.data_mode, phase=args.phase, items=len(records),
                  init_dist=init_dist, dist=dist, records=records)
    if args.requests:
        requests = read_requests(args.requests)
        vocab2id = load_vocab(args.vocab_dir, args.session, opt.dataset)
        result['variance'] = evaluate.test_variance_on_device(model, make_loader()[0], opt, requests, vocab2id, device=device)
    with open(os.path.join(args.save_dir, 'metrics.json'), 'w') as f:
        json.dump(result, f, indent=1)
    return result


if __name__ == '__main__':
    main()
