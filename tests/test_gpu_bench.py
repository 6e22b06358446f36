"""bench.py on the GPU box, as one rank of a data-parallel job (N = 8 readiness without a node): started the way
torch.distributed.run starts a rank -- RANK / WORLD_SIZE / MASTER_* in the environment -- with T2O_OWN_COMM=1, so that the step's
one collective is the C ABI's t2o_allreduce_mean (include/t2onet_hip.h) on a communicator built through
t2o_comm_*, INSIDE the timed region; the line must carry the keys a scaling run is checked by."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_one_rank_job_with_the_c_abi_allreduce_on_the_timed_path(tmp_path):
    env = dict(os.environ, RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()),
               T2O_OWN_COMM='1', T2O_BENCH_DETAIL_DIR=str(tmp_path), HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--full', '--quick',
                        '--no-cpu-baseline', '--exec-steps', '5', '--exec-warmup', '2'], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1]
    d = json.loads(line)
    assert d['n_gpus'] == 1 and d['value'] > 0 and d['config']['backend'].startswith('nccl')
    ts = d['train_step']
    assert ts['own_communicator'] is True                   # the C ABI's all-reduce ran in every timed step
    assert ts['allreduce_ms'] is not None and ts['allreduce_ms'] > 0 and ts['allreduce_bytes'] == 22165917 * 4 + (ts['allreduce_bytes'] - 22165917 * 4)
    assert ts['allreduce_bytes'] >= 22165917 * 4            # the flat buffer: every parameter on a 256-byte boundary
    assert 0 < ts['ms_per_step_over_ranks']['min'] <= ts['ms_per_step_over_ranks']['max']
    with open(os.path.join(str(tmp_path), 'bench_detail.json')) as f:
        detail = json.load(f)
    assert detail['train_step']['parameters_finite'] is True


def test_plain_run_times_the_headline_only_and_dumps_its_last_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` runs the train step alone (no --full legs in the line), times exactly K steps,
    and --dump-outputs writes the last timed step's loss and a sample of the model it updated as float32 .npy files -- the same
    files in a second run with the same arguments."""
    import numpy as np
    env = dict(os.environ, T2O_BENCH_DETAIL_DIR=str(tmp_path))
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    out = tmp_path / 'outputs'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                        '--dump-outputs', str(out)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d['steps'] == 2 and d['warmup'] == 1
    with open(os.path.join(str(tmp_path), 'bench_detail.json')) as f:
        assert json.load(f)['train_step']['steps'] == 2
    assert d['value'] > 0 and d['ms_per_step'] > 0 and d['unit'] == 'images/sec' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert abs(d['value'] - 64 * 1e3 / d['ms_per_step']) < 0.01 * d['value']
    for k in ('executor', 'roofline', 'cpu_baseline', 'train_step_128', 'parity'):
        assert k not in d, k
    assert 'supervised_ms' not in d['train_step']
    total = 0
    for name in ('loss', 'params', 'grads', 'bn_stats'):
        a = np.load(str(out / (name + '.npy')))
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), name
        total += a.nbytes
    assert total < 64 << 20
    assert abs(float(np.load(str(out / 'loss.npy'))[0]) - d['train_step']['loss']) < 1e-6
    # the same arguments: the same inputs, and (the train legs run on the framework's deterministic implementations) the same
    # outputs -- the same files, shapes and dtypes, finite, equal
    again = tmp_path / 'again'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                        '--dump-outputs', str(again)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(str(again))) == sorted(os.listdir(str(out)))
    for name in ('loss', 'params', 'grads', 'bn_stats'):
        a, b = np.load(str(out / (name + '.npy'))), np.load(str(again / (name + '.npy')))
        assert a.shape == b.shape and a.dtype == b.dtype and np.isfinite(b).all(), name
        assert np.array_equal(a, b), (name, float(np.abs(a - b).max()))


_TWO_RANK_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import torch
import torch.distributed as dist
rank = int(os.environ['RANK'])
torch.cuda.set_device(rank)
dev = torch.device('cuda', rank)
dist.init_process_group('nccl', rank=rank, world_size=2, device_id=dev)
from t2onet_amd.train import Communicator
comm = Communicator(dev)                                     # id by an object broadcast on the group, t2o_comm_init_rank on both
t = torch.full((1 << 20,), float(rank + 1), device=dev)
comm.all_reduce_(t)                                          # 1 + 2
ok = bool((t == 3.0).all())
comm.all_reduce_(t, mean=True)                               # (3 + 3) / 2
ok = ok and bool((t == 3.0).all())
u = torch.full((5,), float(rank), device=dev)
dist.all_reduce(u)                                           # torch's own communicator beside it still works
ok = ok and bool((u == 1.0).all())
comm.close()
dist.destroy_process_group()
print('RANK%%d %%s' %% (rank, 'OK' if ok else 'WRONG'), flush=True)
'''


def test_two_ranks_through_the_c_abi_communicator(tmp_path):
    """t2o_comm_unique_id / t2o_comm_init_rank / t2o_allreduce(_mean) with TWO ranks over RCCL, next to torch's own communicator
    (the N > 1 path of Communicator had only ever run with one rank).  Needs two GPUs: skipped on the 1-GPU pool."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip('needs 2 GPUs (the pool leases one)')
    script = tmp_path / 'worker.py'
    script.write_text(_TWO_RANK_WORKER % {'root': ROOT})
    port = str(_free_port())
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', LOCAL_RANK=str(r), MASTER_ADDR='127.0.0.1', MASTER_PORT=port,
                   HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert 'RANK0 OK' in outs[0] and 'RANK1 OK' in outs[1], outs
