"""functional.replay_u8_any on the GPU: for each of its routes the bytes EQUAL those of the wrapper it should have chosen,
called directly.  A 33 x 35 picture (two tiles each way, the last ones ragged), two jobs per launch: the list and its first
step, so that a launch in which one job repeats the sharpness goes to the stencils kernel as a whole."""
import numpy as np
import pytest
import torch

from tests import replay_cases as RC
from tests import replay_mask_cases as MC

pytestmark = pytest.mark.gpu
H, W = 33, 35
ROUTES = {                                   # name -> (ops, with the mask plane, the wrapper that serves it)
    'plain': ([0, 6], False, 'replay_u8'),
    'masked': ([0, 6], True, 'replay_u8_masked'),
    'stencils': ([6, 5, 6], False, 'replay_u8_stencils'),
    'stencils_masked': ([6, 5, 6], True, 'replay_u8_stencils'),
}


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_the_dispatcher_gives_the_chosen_wrappers_bytes(route, monkeypatch):
    import t2onet_amd.functional as T
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    dev = torch.device('cuda:0')
    ops, local, want = ROUTES[route]
    src = torch.from_numpy(RC.picture(H, W, 21).reshape(-1).copy()).to(dev)
    nbytes = 3 * H * W
    jobs = [(0, 0, H, W, ops), (0, nbytes, H, W, ops[:1])]
    masks, offsets = None, []
    if local:
        buf, offsets = MC.pack_masks([MC.mask('soft', H, W)])
        masks = torch.from_numpy(np.ascontiguousarray(buf)).to(dev)
        jobs = [job + ([0] * len(job[4]),) for job in jobs]
    params = torch.from_numpy(np.stack([RC.params_for(ops, 5)] * 2)).to(dev)
    direct = getattr(T, want)
    ref = direct(src, jobs, params) if want == 'replay_u8' else direct(src, jobs, params, masks, offsets)
    taken = []
    for name in ('replay_u8', 'replay_u8_masked', 'replay_u8_stencils'):
        monkeypatch.setattr(T, name, (lambda f, n: lambda *a, **k: (taken.append(n), f(*a, **k))[1])(getattr(T, name), name))
    got = T.replay_u8_any(src, jobs, params, masks, offsets)
    assert taken == [want]
    assert got.dtype == torch.uint8 and got.numel() == 2 * nbytes and torch.equal(got, ref)
    assert not torch.equal(got[:nbytes], src) and not torch.equal(got[:nbytes], got[nbytes:])      # both jobs did something, and not the same
