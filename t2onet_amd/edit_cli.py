"""Edit one photo by a request in words (the reference's demo/seq2seqL1.py):

    python -m t2onet_amd.edit_cli --img photo.jpg --request "make it brighter" --checkpoint model.pth --vocab_dir data/language

writes into save_dir/<name>/: <name>_in.<ext> (the photo as decoded), <name>.<ext> (the result), with --multi_img the
pictures after each operator as {k}_inference_<name>.<ext> (k = 1 ..), and <name>.json = [{'input', 'request', 'output',
'operations': [(operator name, its parameters), ...]}] under the reference's operator names and parameter counts
(demo/seq2seqL1.py:121-122,193-196).  Images are written with PIL, the format chosen by the extension.

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


def write_outputs(save_dir, img_path, request, img_u8, steps_u8, ops, params, multi_img=False):
    """The files of one edit (see the module docstring); steps_u8: (max(n,1), h, w, 3) uint8 array.  Returns the record."""
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
    args = ap.parse_args(argv)

    from . import default_options
    from .actor import Actor
    from .edit import edit_image, request_to_idx
    opt = default_options(vocab_dir=args.vocab_dir, session=args.session)
    vocab2id = load_vocab(args.vocab_dir, args.session, opt.dataset)
    device = torch.device('cuda', torch.cuda.current_device())
    model = Actor(opt)
    model.load_state_dict(torch.load(args.checkpoint, map_location='cpu'), strict=False)      # as the demo (:129)
    model.to(device)
    img = decode_image(args.img)
    steps_u8, ops, params = edit_image(model, img, request_to_idx(args.request, vocab2id, opt), args.proxy_short)
    info = write_outputs(args.save_dir, args.img, args.request, img, steps_u8.cpu().numpy(), ops, params.cpu(), args.multi_img)
    print('%s: %s -> %s' % (args.request, ', '.join(n for n, _ in info['operations']) or '(no operator)',
                            os.path.join(args.save_dir, os.path.splitext(os.path.basename(args.img))[0], info['output'])))
    return info


if __name__ == '__main__':
    main()
