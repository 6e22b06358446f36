"""Evaluation loops of experiments/t2onet/test_seq2seqL1.py (test :28-95, test_variance :99-142) and the L1 / SSIM parts of
utils/eval.py:13-60 (FID needs torchvision's InceptionV3: out of scope).
Everything runs on the GPU: argmax episode, END-image select, L1 and SSIM through the HIP kernels.

Two forms of each loop: test / test_variance read every metric back as the reference does (.item() per value);
test_on_device / test_variance_on_device write them into a device table with one fused launch per batch
(functional.eval_metrics / end_select_var_mean) and read the table once at the end, so that the host can enqueue image
k + 1 while the GPU works on image k."""
import time

import torch

from . import functional as T
from .train import first_end_step, select_end_images


class ImageEvaluator(object):
    """Running means of input/output L1 and SSIM against the ground truth (utils/eval.py:13-60)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.itr = 0
        self.avg_out_L1 = self.avg_in_L1 = 0.0
        self.avg_out_SSIM = self.avg_in_SSIM = 0.0

    def update(self, input, output, gt):
        self.itr += 1
        k = 1.0 / self.itr
        self.avg_in_L1 = self.avg_in_L1 * (1 - k) + T.l1_loss(input, gt).item() * k
        self.avg_out_L1 = self.avg_out_L1 * (1 - k) + T.l1_loss(output, gt).item() * k
        self.avg_in_SSIM = self.avg_in_SSIM * (1 - k) + T.ssim(input, gt).item() * k
        self.avg_out_SSIM = self.avg_out_SSIM * (1 - k) + T.ssim(output, gt).item() * k

    def eval(self):
        print('input L1 dist {:.4f}, output L1 dist {:.4f}'.format(self.avg_in_L1, self.avg_out_L1))
        print('input SSIM {:.4f}, output SSIM {:.4f}'.format(self.avg_in_SSIM, self.avg_out_SSIM))
        return dict(in_L1=self.avg_in_L1, out_L1=self.avg_out_L1, in_SSIM=self.avg_in_SSIM, out_SSIM=self.avg_out_SSIM)


def test(model, loader, opt, is_test=False, device=None, verbose=True):
    """loader yields (img_x, img_y, x, req) like datasets/FiveKdataset.py:FiveK.
    Returns (avg_init_dist, avg_dist) = running means of mean|img_x - img_y| and mean|pred - img_y|."""
    model.eval()
    device = device or next(model.parameters()).device
    single = model.module if hasattr(model, 'module') else model
    evaluator = ImageEvaluator() if is_test else None
    itr, avg_time, avg_dist, avg_init_dist = 0, 0.0, 0.0, 0.0
    for data in loader:
        itr += 1
        tik = time.time()
        img_x, img_y, x = data[0], data[1], data[2]
        lengths = (x != opt.null_id).sum(1)                      # on the host, before the copy
        x, img_x, img_y = x.to(device), img_x.to(device), img_y.to(device)
        with torch.no_grad():
            _, pred_imgs, pred_ops, _ = single.episode_forward(x, img_x, None, reinforce_sample=False, lengths=lengths)
            pred_img = select_end_images(pred_imgs, pred_ops, opt.end_id)
            init_dist = T.l1_loss(img_x, img_y).item()
            dist = T.l1_loss(pred_img, img_y).item()
        avg_time += (time.time() - tik - avg_time) / itr
        avg_init_dist += (init_dist - avg_init_dist) / itr
        avg_dist += (dist - avg_dist) / itr
        if evaluator is not None:
            evaluator.update(img_x, pred_img, img_y)
        if verbose and itr % max(1, getattr(opt, 'print_every', 100)) == 0:
            print('iter {:6d}, init dist {:.2f},  L1 dist {:.2f} time {:.2f}'.format(itr, init_dist, dist, avg_time))
    if evaluator is not None:
        evaluator.eval()
    if verbose:
        print('inference init L1 dist {:.4f}; L1 dist {:.4f}'.format(avg_init_dist, avg_dist))
    return avg_init_dist, avg_dist


def test_variance(model, loader, opt, requests, vocab2id=None, device=None, verbose=True):
    """experiments/t2onet/test_seq2seqL1.py:99-142: how much the edit depends on the wording -- for every batch of the
    loader the arg-max episode is run once per test request (the SAME request for every image of the batch), the END
    images of all requests are concatenated and the unbiased variance over that axis is averaged over pixels; returns
    the running mean over batches.

    requests: the reference imports its list from `core.utils.eval.test_txts`, a module that is not part of the
    repository, so the caller supplies it: strings (tokenised with `vocab2id` like utils/text_utils.py:42-67) or
    (1, encoder_max_len) / (encoder_max_len,) token-id tensors.  As in the reference the request row is (1, L) while the
    images are (bs, ...): it is broadcast over the batch here (the reference's encoder does that only for bs = 1)."""
    from .data import txt2idx
    model.eval()
    device = device or next(model.parameters()).device
    single = model.module if hasattr(model, 'module') else model
    rows = []
    for r in requests:
        if isinstance(r, str):
            if vocab2id is None:
                raise ValueError('test_variance: text requests need vocab2id')
            r = txt2idx(r, vocab2id, opt.encoder_max_len)
        rows.append(torch.as_tensor(r, dtype=torch.long).view(1, -1))
    if len(rows) < 2:
        raise ValueError('test_variance: the variance over fewer than two requests is undefined')
    itr, avg_var, avg_time = 0, 0.0, 0.0
    for data in loader:
        itr += 1
        tik = time.time()
        img_x = data[0].to(device)
        ends = []
        for row in rows:
            x = row.expand(img_x.shape[0], -1).contiguous()
            lengths = (x != opt.null_id).sum(1)
            with torch.no_grad():
                _, pred_imgs, pred_ops, _ = single.episode_forward(x.to(device), img_x, None, reinforce_sample=False, lengths=lengths)
                ends.append(select_end_images(pred_imgs, pred_ops, opt.end_id))
        var = torch.var(torch.cat(ends), dim=0).mean().item()
        avg_var += (var - avg_var) / itr
        avg_time += (time.time() - tik - avg_time) / itr
        if verbose and itr % max(1, getattr(opt, 'print_every', 100)) == 0:
            print('iter {:6d}, var {:.6f}, time {:.2f}'.format(itr, avg_var, avg_time))
    if verbose:
        print('avg var: {:.6f}'.format(avg_var))
    return avg_var


class _DeviceTable(object):
    """A (capacity, width) fp32 device table filled row by row: sized by the loader's length when it has one, otherwise
    doubled through a device copy when it runs full (no host read either way)."""

    def __init__(self, width, capacity, device):
        self.rows = torch.zeros(max(int(capacity or 0), 1), width, dtype=torch.float32, device=device)
        self.itr = 0

    def next_row(self):
        if self.itr == self.rows.shape[0]:
            grown = torch.zeros(2 * self.itr, self.rows.shape[1], dtype=torch.float32, device=self.rows.device)
            grown[:self.itr].copy_(self.rows)
            self.rows = grown
        self.itr += 1
        return self.rows[self.itr - 1]

    def read(self):
        """The rows written so far as lists of Python floats: ONE device-to-host copy."""
        return self.rows[:self.itr].cpu().tolist()


def _capacity(loader):
    try:
        return len(loader)
    except TypeError:
        return None


class DeviceEvaluator(object):
    """ImageEvaluator without a host read per image: update() writes [in_L1, out_L1, in_SSIM, out_SSIM] of a batch into row
    `itr` of a (capacity, 4) device table with one functional.eval_metrics call; result() copies the table to the host ONCE
    and replays ImageEvaluator's running-mean updates there, in the same form and order, on the same fp32 values."""

    def __init__(self, capacity=None, device=None, with_ssim=True):
        self.device = device or torch.device('cuda', torch.cuda.current_device())
        self.with_ssim = with_ssim
        self.table = _DeviceTable(4, capacity, self.device)

    @property
    def itr(self):
        return self.table.itr

    def update(self, input, imgs, first, gt=None):
        """update(input, imgs, first, gt): imgs the list of an episode's step images, first (B) int64 -- the output of
        sample b is imgs[first[b]][b]; update(input, output, gt): plain images (the T = 1 form)."""
        if gt is None:
            imgs, gt = [imgs], first
            first = torch.zeros(gt.shape[0], dtype=torch.int64, device=gt.device)
        T.eval_metrics(input, imgs, first, gt, out=self.table.next_row(), with_ssim=self.with_ssim)

    def distances(self, rows=None):
        """(avg_init_dist, avg_dist): the running means of test() over the rows' two L1 values."""
        avg_init_dist, avg_dist = 0.0, 0.0
        for itr, row in enumerate(self.table.read() if rows is None else rows, 1):
            avg_init_dist += (row[0] - avg_init_dist) / itr
            avg_dist += (row[1] - avg_dist) / itr
        return avg_init_dist, avg_dist

    def result(self, rows=None):
        """The keys of ImageEvaluator.eval() from the table (one copy; pass `rows` = table.read() to share it)."""
        avg = [0.0, 0.0, 0.0, 0.0]
        for itr, row in enumerate(self.table.read() if rows is None else rows, 1):
            k = 1.0 / itr
            avg = [a * (1 - k) + v * k for a, v in zip(avg, row)]
        return dict(in_L1=avg[0], out_L1=avg[1], in_SSIM=avg[2], out_SSIM=avg[3])


def test_on_device(model, loader, opt, is_test=False, device=None, verbose=True, on_batch=None, mask_fn=None):
    """The loop of test() with nothing between two images that depends on a device value: the arg-max episode returns its
    step images as a list (stack=False), the END step is an index tensor (train.first_end_step) and ONE eval_metrics call per
    batch writes the two L1 distances -- and with is_test the two SSIM values -- into a DeviceEvaluator's table, read once
    after the loop (the progress line every opt.print_every batches reads the rows written so far).
    on_batch(itr, data, pred_imgs, first, pred_ops, pred_params): called after each batch's launches (test_cli saves pictures
    there).  mask_fn(data, img_x): the batch's `mask_dict` for the episode -- a gier.MaskTable keeps the loop free of host
    reads, a list of dicts costs one per step; None (the default): global edits.  Returns (avg_init_dist, avg_dist, metrics) with metrics = the dict of ImageEvaluator.eval() (None unless
    is_test)."""
    model.eval()
    device = device or next(model.parameters()).device
    single = model.module if hasattr(model, 'module') else model
    evaluator = DeviceEvaluator(_capacity(loader), device, with_ssim=bool(is_test))
    tik = time.time()
    for data in loader:
        img_x, img_y, x = data[0], data[1], data[2]
        lengths = (x != opt.null_id).sum(1)                      # on the host, before the copy
        x, img_x, img_y = (t.to(device, non_blocking=True) for t in (x, img_x, img_y))
        with torch.no_grad():
            mask_dict = None if mask_fn is None else mask_fn(data, img_x)
            _, pred_imgs, pred_ops, pred_params = single.episode_forward(x, img_x, mask_dict, reinforce_sample=False, lengths=lengths,
                                                                         stack=False)
            first = first_end_step(pred_ops, opt.end_id)
            evaluator.update(img_x, pred_imgs, first, img_y)
        itr = evaluator.itr
        if on_batch is not None:
            on_batch(itr, data, pred_imgs, first, pred_ops, pred_params)
        if verbose and itr % max(1, getattr(opt, 'print_every', 100)) == 0:
            row = evaluator.table.rows[itr - 1].tolist()
            print('iter {:6d}, init dist {:.2f},  L1 dist {:.2f} time {:.2f}'.format(itr, row[0], row[1], (time.time() - tik) / itr))
    rows = evaluator.table.read()
    avg_init_dist, avg_dist = evaluator.distances(rows)
    metrics = evaluator.result(rows) if is_test else None
    if verbose:
        if metrics is not None:
            print('input L1 dist {:.4f}, output L1 dist {:.4f}'.format(metrics['in_L1'], metrics['out_L1']))
            print('input SSIM {:.4f}, output SSIM {:.4f}'.format(metrics['in_SSIM'], metrics['out_SSIM']))
        print('inference init L1 dist {:.4f}; L1 dist {:.4f}'.format(avg_init_dist, avg_dist))
    return avg_init_dist, avg_dist, metrics


def request_rows(requests, opt, vocab2id=None):
    """The (1, L) token rows of test_variance's requests: strings are tokenised with vocab2id, tensors taken as they are."""
    from .data import txt2idx
    rows = []
    for r in requests:
        if isinstance(r, str):
            if vocab2id is None:
                raise ValueError('test_variance: text requests need vocab2id')
            r = txt2idx(r, vocab2id, opt.encoder_max_len)
        rows.append(torch.as_tensor(r, dtype=torch.long).view(1, -1))
    if len(rows) < 2:
        raise ValueError('test_variance: the variance over fewer than two requests is undefined')
    return rows


def test_variance_on_device(model, loader, opt, requests, vocab2id=None, device=None, verbose=True):
    """test_variance() (same arguments, same value) without a host read per batch: the R episodes of a batch keep their step
    images as lists, ONE end_select_var_mean launch reads every END image where it lies and writes the batch's variance into
    entry `itr` of a device table; the table is read once after the loop."""
    model.eval()
    device = device or next(model.parameters()).device
    single = model.module if hasattr(model, 'module') else model
    rows = request_rows(requests, opt, vocab2id)
    table = _DeviceTable(1, _capacity(loader), device)
    tik = time.time()
    for data in loader:
        img_x = data[0].to(device, non_blocking=True)
        lists, firsts = [], []
        for row in rows:
            x = row.expand(img_x.shape[0], -1).contiguous()
            lengths = (x != opt.null_id).sum(1)
            with torch.no_grad():
                _, pred_imgs, pred_ops, _ = single.episode_forward(x.to(device, non_blocking=True), img_x, None, reinforce_sample=False,
                                                                   lengths=lengths, stack=False)
                lists.append(pred_imgs)                          # alive until the launch below is enqueued
                firsts.append(first_end_step(pred_ops, opt.end_id))
        T.end_select_var_mean(lists, firsts, out=table.next_row())
        if verbose and table.itr % max(1, getattr(opt, 'print_every', 100)) == 0:
            print('iter {:6d}, time {:.2f}'.format(table.itr, (time.time() - tik) / table.itr))
    avg_var = 0.0
    for itr, (var,) in enumerate(table.read(), 1):
        avg_var += (var - avg_var) / itr
    if verbose:
        print('avg var: {:.6f}'.format(avg_var))
    return avg_var
