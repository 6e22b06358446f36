"""One photo and one sentence in, the edited photo out (what the reference's demo/seq2seqL1.py does), split the way a
real photo needs it: the DECISION -- which operators, with which parameters -- is taken by the actor on a bounded proxy
(the short-side-600 size the test loader uses, utils/visual_utils.py:34-47), and the decision is then APPLIED to the
original bytes at their native size by the fused 8-bit replay kernel (functional.replay_u8: 6 bytes of memory traffic
per pixel, no fp32 image of the photo ever exists)."""
import torch

from . import functional as T
from .data import short_side_size, txt2idx


def request_to_idx(text, vocab2id, opt):
    """(1, opt.encoder_max_len) token ids of a request: data.txt2idx (utils/text_utils.py:42-67), unknown words -> id 3."""
    return txt2idx(text, vocab2id, opt.encoder_max_len)


def first_end(ops_vocab, end_id):
    """Number of operators in front of the first END token of one decoded row (all of them when there is none): the
    column train.select_end_images picks, as a count."""
    ops_vocab = list(ops_vocab)
    return ops_vocab.index(end_id) if end_id in ops_vocab else len(ops_vocab)


def edit_image(model, img_u8_hwc, x, proxy_short=600):
    """img_u8_hwc: the decoded photo, uint8 (h,w,3) RGB (array or CPU tensor); x: (1, L) request token ids.
    Returns (steps_u8, ops, params):
      steps_u8  (max(n,1), h, w, 3) uint8 GPU tensor: picture k is the photo after the first k+1 of the n chosen operators,
                the last one is the result (n = 0, END chosen first: the photo through the two 8-bit conversions);
      ops       the n executor indices in front of the first END (what test() scores: train.select_end_images);
      params    (n, 24) fp32 GPU tensor, their parameter rows.
    The photo is uploaded once; the proxy is made on the device only when the short side exceeds proxy_short (no
    upscaling: a smaller photo is its own proxy); the arg-max episode runs in eval mode under no_grad; pred_ops is read
    back once; ONE replay_u8 launch writes every prefix of the list at native size."""
    img = T._u8_hwc(img_u8_hwc)
    h, w = img.shape[:2]
    dev = next(model.parameters()).device
    opt = model.opt
    buffer, descs = T.pack_u8([img])
    dev_buffer, table_ptr, descs, _keep = T.upload_packed(buffer, descs, dev)
    ph, pw = short_side_size(h, w, proxy_short) if min(h, w) > proxy_short else (h, w)
    proxy = T._resize_launch(dev_buffer, table_ptr, 1, ph, pw)
    x = torch.as_tensor(x, dtype=torch.long).view(1, -1)
    lengths = (x != opt.null_id).sum(1)                      # on the host, before the copy
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            _, _, pred_ops, pred_params = model.episode_forward(x.to(dev), proxy, None, reinforce_sample=False, lengths=lengths)
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
    out = T.replay_u8(dev_buffer, jobs, table)
    return out[:J * nbytes].view(J, h, w, 3), ops, params
