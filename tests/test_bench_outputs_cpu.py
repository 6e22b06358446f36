"""bench.py --dump-outputs: step_outputs() samples the same elements in every run and stays within its size bound; the
--full-only options are refused without --full (no GPU needed)."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _model_and_trainer():
    from t2onet_amd.train import FlatGradients
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(300, 100), torch.nn.BatchNorm1d(100), torch.nn.Linear(100, 7))
    model(torch.rand(16, 300)).sum().backward()

    class Trainer:
        pass
    tr = Trainer()
    grads = {id(p): p.grad.clone() for p in model.parameters()}
    tr.grads = FlatGradients(model.parameters())                  # (on the host: no kernels, .grad become views of one buffer)
    for p in model.parameters():
        p.grad.copy_(grads[id(p)])
    return model, tr


def test_step_outputs_sample_is_fixed_and_bounded():
    import bench
    model, tr = _model_and_trainer()
    loss = torch.tensor(0.25)
    a = bench.step_outputs(model, tr, loss)
    b = bench.step_outputs(model, tr, loss)
    assert sorted(a) == ['bn_stats', 'grads', 'loss', 'params']
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
    assert a['loss'].tolist() == [0.25]
    params = list(model.parameters())
    sizes = [min(p.numel(), bench.DUMP_PER_TENSOR) for p in params]
    assert a['params'].size == a['grads'].size == sum(sizes)
    assert params[0].numel() > bench.DUMP_PER_TENSOR                 # the 300 x 100 weight is sampled at the seeded positions,
    idx = np.sort(np.random.default_rng([bench.DUMP_SEED, 0]).choice(params[0].numel(), bench.DUMP_PER_TENSOR, replace=False))
    assert np.array_equal(a['params'][:sizes[0]], params[0].detach().reshape(-1).numpy()[idx])       # the same ones for the
    assert np.array_equal(a['grads'][:sizes[0]], params[0].grad.reshape(-1).numpy()[idx])            # weight and its gradient
    off = sizes[0]                                                # ... the rest goes in whole, in order
    for p, n in zip(params[1:], sizes[1:]):
        assert np.array_equal(a['params'][off:off + n], p.detach().reshape(-1).numpy())
        assert np.array_equal(a['grads'][off:off + n], p.grad.reshape(-1).numpy())
        off += n
    bn = model[1]
    assert np.array_equal(a['bn_stats'], torch.cat([bn.running_mean, bn.running_var]).numpy())


def test_write_outputs(tmp_path):
    import bench
    model, tr = _model_and_trainer()
    out = bench.step_outputs(model, tr, torch.tensor(1.5))
    bench.write_outputs(str(tmp_path / 'd'), out)
    for k, v in out.items():
        assert np.array_equal(np.load(str(tmp_path / 'd' / (k + '.npy'))), v)


def test_no_train_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--no-train'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and '--full' in r.stderr
