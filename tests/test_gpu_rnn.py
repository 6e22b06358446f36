"""The request encoder's LSTM step kernels (t2o_rnn.hip, functional.lstm_layer) against torch.nn.LSTM on packed
sequences in fp64 (models/lang_encoder.py:70-113: pack_padded_sequence -> LSTM -> pad_packed_sequence), forward and
every gradient; and the whole RNNEncoder against the library path.  Beyond the encoder's own configuration: layers
without biases, H = 192, the 8-sample batch-tile boundaries, batches in which no row reaches L, saturated gates, and the
nullable arguments of the C entry points (absent = bit-identical to zeros)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _close(got, ref, tol):
    ref = ref.detach().float().cpu()
    scale = float(ref.abs().max()) or 1.0
    np.testing.assert_allclose(got.detach().float().cpu().numpy(), ref.numpy(), rtol=tol, atol=tol * scale)


def _rel_err(got, ref):
    """max |got - ref| over the largest reference entry: the quantity _close bounds"""
    ref = ref.detach().double()
    return float((got.detach().double() - ref).abs().max()) / (float(ref.abs().max()) or 1.0)


def _packed_lstm(rnn, x, lengths, L, gs, dtype):
    """`rnn` in `dtype` on the CPU over the packed batch, loss = <out, gs[0]> + <h_n, gs[1]> + <c_n, gs[2]>.
    Returns ([out, h_n, c_n], [d x, d parameters in named_parameters() order])."""
    rnn = copy.deepcopy(rnn).to(dtype)
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    po, (h, c) = rnn(pack_padded_sequence(xr, torch.tensor(lengths), batch_first=True, enforce_sorted=False))
    out = pad_packed_sequence(po, batch_first=True, total_length=L)[0]
    ((out * gs[0].to(dtype)).sum() + (h * gs[1].to(dtype)).sum() + (c * gs[2].to(dtype)).sum()).backward()
    return [out.detach(), h.detach(), c.detach()], [xr.grad] + [p.grad for _, p in rnn.named_parameters()]


def _lstm_layer_vs_fp64(case, bias=True, w_scale=1.0, x_scale=1.0, measured=False):
    """functional.lstm_layer against nn.LSTM in fp64: outputs, final states, every gradient.  `measured`: the tolerances
    are the larger of the file's (2e-6 forward, 2e-5 gradients) and 4 x the error of the SAME module run in fp32 on the
    CPU (another, equally valid fp32 summation order), per compared tensor -- for magnitudes the file's numbers were never
    measured at."""
    import t2onet_amd.functional as T
    B, L, E, H, D, lengths = case
    if lengths is None:
        lengths = [int(v) for v in (synth.uniform((B,), 5, 0.0, 1.0) * L).long().clamp(1, L)]
        lengths[0] = L
    torch.manual_seed(3)
    rnn = nn.LSTM(E, H, 1, batch_first=True, bidirectional=D == 2, bias=bias)
    if w_scale != 1.0:
        with torch.no_grad():
            for p in rnn.parameters():
                p.mul_(w_scale)
    x = synth.uniform((B, L, E), 11, -1.0, 1.0) * x_scale
    for b in range(B):
        x[b, lengths[b]:] = 0
    gs = [synth.uniform((B, L, D * H), 12, -1.0, 1.0), synth.uniform((D, B, H), 13, -1.0, 1.0), synth.uniform((D, B, H), 14, -1.0, 1.0)]
    fwd64, bwd64 = _packed_lstm(rnn, x, lengths, L, gs, torch.float64)
    tol_f, tol_b = [2e-6] * 3, [2e-5] * len(bwd64)
    if measured:
        fwd32, bwd32 = _packed_lstm(rnn, x, lengths, L, gs, torch.float32)
        e_f, e_b = [_rel_err(a, r) for a, r in zip(fwd32, fwd64)], [_rel_err(a, r) for a, r in zip(bwd32, bwd64)]
        print('fp32 CPU nn.LSTM vs fp64, relative to the largest entry: out/h_n/c_n %s, gradients %s'
              % (['%.2e' % e for e in e_f], ['%.2e' % e for e in e_b]))
        tol_f, tol_b = [max(2e-6, 4 * e) for e in e_f], [max(2e-5, 4 * e) for e in e_b]
    xg = x.to(DEV).requires_grad_(True)
    ws = [p.detach().to(DEV).requires_grad_(True) for _, p in rnn.named_parameters()]
    per = 4 if bias else 2
    assert len(ws) == per * D
    o, hn, cn = T.lstm_layer(xg, torch.tensor(lengths), [tuple(ws[per * d:per * (d + 1)]) for d in range(D)])
    for got, ref, tol in zip((o, hn, cn), fwd64, tol_f):
        _close(got, ref, tol)
    for b in range(B):
        assert float(o[b, lengths[b]:].abs().sum()) == 0.0
    ((o * gs[0].to(DEV)).sum() + (hn * gs[1].to(DEV)).sum() + (cn * gs[2].to(DEV)).sum()).backward()
    for got, ref, tol in zip([xg] + ws, bwd64, tol_b):
        assert got.grad is not None
        _close(got.grad, ref, tol)


# (B, L, E, H, D, lengths): ragged batch (not a multiple of the 8-sample tile), full / single-token rows, one and two
# directions, the encoder's own shape
CASES = [(5, 7, 30, 64, 2, [7, 3, 5, 1, 7]), (3, 4, 16, 64, 1, [4, 2, 4]), (9, 1, 12, 128, 2, [1] * 9),
         (64, 17, 300, 256, 2, None), (16, 6, 512, 256, 2, [6, 6, 5, 4, 6, 1, 2, 3, 6, 6, 6, 2, 1, 5, 4, 3])]


@pytest.mark.parametrize('case', CASES)
def test_lstm_layer_matches_packed_nn_lstm_fp64(case):
    _lstm_layer_vs_fp64(case)


# nn.LSTM(bias=False): two-tuples in `dirs`, b_ih = b_hh = NULL in k_lstm_fwd_step, no bias column sums in the backward
NO_BIAS_CASES = [(5, 4, 12, 64, 2, [4, 1, 3, 2, 4]), (3, 3, 8, 128, 1, [3, 1, 2])]


@pytest.mark.parametrize('case', NO_BIAS_CASES)
def test_lstm_layer_without_biases(case):
    _lstm_layer_vs_fp64(case, bias=False)


# H = 192 (the one permitted width that is no power of two: 3 unit tiles, 48 k's / 48 column quads per wave); the batch
# tile's boundaries (one full tile, two full tiles, two tiles + one row); a batch in which no row reaches L (the reverse
# direction's first processed steps -- and the forward direction's last -- are masked for every sample)
SHAPE_CASES = [(9, 5, 20, 192, 2, [5, 2, 4, 1, 5, 3, 3, 2, 4]),
               (8, 3, 8, 64, 2, [3, 1, 2, 3, 2, 1, 3, 2]),
               (16, 3, 8, 64, 2, [3, 1, 2, 3, 2, 1, 3, 2, 1, 1, 2, 3, 3, 2, 1, 3]),
               (17, 3, 8, 64, 2, [3, 1, 2, 3, 2, 1, 3, 2, 1, 1, 2, 3, 3, 2, 1, 3, 2]),
               (4, 6, 12, 64, 2, [3, 1, 2, 3])]


@pytest.mark.parametrize('case', SHAPE_CASES, ids=['H192', 'B8', 'B16', 'B17', 'no-row-reaches-L'])
def test_lstm_layer_widths_batch_tiles_and_short_batches(case):
    _lstm_layer_vs_fp64(case)


@pytest.mark.parametrize('case', NO_BIAS_CASES)
def test_lstm_layer_saturated_gates(case):
    """Weights x 8, inputs x 4: pre-activations of several units, sigmoids at 0 / 1 and tanh at +-1 in fp32."""
    _lstm_layer_vs_fp64(case, bias=False, w_scale=8.0, x_scale=4.0, measured=True)


def _encoder_own_vs_library(monkeypatch, enc, x):
    """RNNEncoder on the GPU, own kernels vs the packed library call: outputs and all gradients; each pass must take
    its own path."""
    import t2onet_amd.functional as T
    import t2onet_amd.lang_encoder as LE
    lengths = (x != 0).sum(1).cpu()
    res = {}
    for own in (True, False):
        with monkeypatch.context() as m:
            m.setattr(LE, '_OWN_LSTM', own)
            if own:
                m.setattr(LE, 'pack_padded_sequence', lambda *a, **k: pytest.fail('the library path ran'))
            else:
                m.setattr(T, 'lstm_layer', lambda *a, **k: pytest.fail('the own kernels ran'))
            enc.zero_grad(set_to_none=True)
            out, (h, c), emb = enc(x, lengths)
            (out.square().sum() + h.sum() + 2 * c.sum()).backward()
        res[own] = (out.detach().clone(), h.detach().clone(), c.detach().clone(),
                    {n: p.grad.detach().clone() for n, p in enc.named_parameters() if p.grad is not None})
    for a, b in zip(res[True][:3], res[False][:3]):
        _close(a, b, 1e-5)
    assert res[True][3].keys() == res[False][3].keys()
    for n in res[True][3]:
        _close(res[True][3][n], res[False][3][n], 1e-4)
    return res


def test_request_encoder_own_kernels_match_the_library_path(monkeypatch):
    """RNNEncoder on the GPU: own LSTM kernels vs the packed library call (dropout off), outputs and all gradients."""
    import t2onet_amd
    import t2onet_amd.lang_encoder as LE
    from t2onet_amd.actor import Actor
    opt = t2onet_amd.default_options(input_dropout_p=0.0, dropout_p=0.0)
    torch.manual_seed(5)
    model = Actor(opt).to(DEV).train()
    x = synth.requests(16, 17, 21).to(DEV)
    lengths = (x != 0).sum(1).cpu()
    res = _encoder_own_vs_library(monkeypatch, model.lang_encoder, x)
    # without host lengths (one device->host copy for the truncation length) and with `longest` given (none at all)
    monkeypatch.setattr(LE, '_OWN_LSTM', True)
    with torch.no_grad():
        o2 = model.lang_encoder(x)[0]
        o3 = model.lang_encoder(x, (x != 0).sum(1), int(lengths.max()))[0]
    assert torch.equal(o2, res[True][0]) and torch.equal(o3, res[True][0])


def test_request_encoder_without_biases(monkeypatch):
    """The same comparison with the encoder's LSTM rebuilt as nn.LSTM(bias=False): lang_encoder hands lstm_layer
    (w_ih, w_hh) pairs for both layers and directions."""
    from t2onet_amd.lang_encoder import RNNEncoder
    torch.manual_seed(6)
    enc = RNNEncoder(918, 300, 256, 4, bidirectional=True, n_layers=2)
    enc.rnn = nn.LSTM(300, 256, 2, batch_first=True, bidirectional=True, bias=False)
    enc = enc.to(DEV).train()
    assert not enc.rnn.bias and len(list(enc.rnn.parameters())) == 8
    res = _encoder_own_vs_library(monkeypatch, enc, synth.requests(11, 9, 23).to(DEV))
    assert sorted(n for n in res[True][3] if n.startswith('rnn.')) == sorted('rnn.' + n for n, _ in enc.rnn.named_parameters())


def test_absent_biases_and_gradients_equal_zero_tensors_bitwise():
    """What autograd cannot reach (it materialises zeros): t2o_lstm_layer_fwd with b_ih / b_hh = NULL and
    t2o_lstm_layer_bwd with dout / dhn / dcn = NULL, each alone and all together, against the same call with a zero
    tensor in place of the absent argument -- bit for bit."""
    from t2onet_amd import _lib
    from t2onet_amd.functional import _stream
    lib = _lib.load()
    B, L, H, D = 11, 4, 64, 2                                       # two batch tiles, the second one partial
    G = 4 * H
    lengths = torch.tensor([4, 2, 3, 1, 4, 3, 2, 3, 1, 2, 3], device=DEV)
    gi = synth.uniform((B, L, D * G), 41, -2.0, 2.0).to(DEV)
    w_hh = [synth.uniform((G, H), 42 + d, -0.3, 0.3).to(DEV) for d in range(D)]
    whh_t = torch.stack([t.view(4, H, H).permute(2, 1, 0) for t in w_hh], 0).contiguous()     # as functional._LstmLayerFn packs them
    whh = torch.stack([t.view(H, 4, H).permute(0, 2, 1) for t in w_hh], 0).contiguous()
    st = _stream(torch.device(DEV))
    ptr = lambda t: None if t is None else t.data_ptr()           # noqa: E731

    def forward(b_ih, b_hh):
        o = [torch.zeros(s, device=DEV) for s in ((B, L, D * H), (L, D, B, H), (L, D, B, H), (L, D, B, G))]
        assert lib.t2o_lstm_layer_fwd(gi.data_ptr(), whh_t.data_ptr(), ptr(b_ih), ptr(b_hh), lengths.data_ptr(), o[0].data_ptr(),
                                      o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), B, L, H, D, st) == 0, lib.t2o_last_error()
        return o

    zb = torch.zeros(D, G, device=DEV)
    full = forward(zb, zb)
    assert float(full[0].abs().max()) > 0.1
    for b_ih, b_hh in ((None, zb), (zb, None), (None, None)):
        for a, b in zip(forward(b_ih, b_hh), full):
            assert torch.equal(a, b)
    _, _, cnew, gates = full

    def backward(dout, dhn, dcn):
        dgates, carry, dc = torch.zeros(L, D, B, G, device=DEV), torch.zeros(D, B, H, device=DEV), torch.zeros(D, B, H, device=DEV)
        assert lib.t2o_lstm_layer_bwd(whh.data_ptr(), lengths.data_ptr(), cnew.data_ptr(), gates.data_ptr(), ptr(dout), ptr(dhn), ptr(dcn),
                                      dgates.data_ptr(), carry.data_ptr(), dc.data_ptr(), B, L, H, D, st) == 0, lib.t2o_last_error()
        return dgates

    g = [synth.uniform((B, L, D * H), 51, -1.0, 1.0).to(DEV), synth.uniform((D, B, H), 52, -1.0, 1.0).to(DEV),
         synth.uniform((D, B, H), 53, -1.0, 1.0).to(DEV)]
    z = [torch.zeros_like(t) for t in g]
    everything = backward(*g)
    for k in range(3):                                             # one absent, the other two real
        zeros = backward(*[z[i] if i == k else g[i] for i in range(3)])
        absent = backward(*[None if i == k else g[i] for i in range(3)])
        assert torch.equal(absent, zeros)
        assert not torch.equal(zeros, everything)                   # (the argument matters: the check is not vacuous)
    assert torch.equal(backward(None, None, None), backward(*z))
    assert float(backward(None, None, None).abs().max()) == 0.0
