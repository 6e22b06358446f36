"""The stencils replay kernel (t2o_replay_stencils.hip) on the GPU: operator lists with any number of sharpness steps, with
and without masks.  The kernel's bytes must EQUAL those of the materialised path -- resize_u8 at the picture's own size,
operator_apply per step (with the mask as (1,1,h,w) fp32 = byte / 255 where the step names one) and every image
materialised, to_u8_hwc -- with no tolerance: both sides run the same device functions.  Lists, sizes and mask rules are
shared with tests/test_replay_stencils_cpu.py (tests/replay_stencils_cases.py).

A call's jobs share at most 4 mask planes, and a plane is bytes at an offset read with the JOB's own (h, w): every call
here carries one table of four planes at the largest size, and a smaller job reads a prefix of the plane it names."""
import json
import types

import numpy as np
import pytest
import torch

from tests import replay_cases as RC
from tests import replay_mask_cases as MC
from tests import replay_stencils_cases as SC

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A
BIG = (40, 70)
assert all(h * w <= BIG[0] * BIG[1] for h, w in SC.SIZES)
TABLE = ['soft', 'blocks', 'zeros', 'full']
PLANES = [MC.mask(p, BIG[0], BIG[1]) for p in TABLE]
MASK_BUF, MASK_OFFSETS = MC.pack_masks(PLANES)
RULES = [SC._all0, SC._sharp_only, SC._front_of_sharp, SC._two]
_reference = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def plane_of(slot, h, w):
    """What a job of size (h, w) reads when it names table entry `slot`."""
    return MASK_BUF[MASK_OFFSETS[slot]:MASK_OFFSETS[slot] + h * w].reshape(h, w)


def case(i, masked):
    """Job i of a call: list i mod 10 on a size that walks along, so that 64 jobs meet every list and every size; with
    masks, the rule (which steps name a mask) and the table entries walk along too ->
    (key, img, ops, params, mask_of as table slots or None)."""
    name, s = SC.NAMES[i % len(SC.NAMES)], (i + i // len(SC.NAMES)) % len(SC.SIZES)
    ops = SC.LISTS[name]
    h, w = SC.SIZES[s]
    slots = None
    if masked:
        first = (i + i // 4) % 4
        slots = [-1 if m < 0 else (first + m) % 4 for m in RULES[(i // 2) % len(RULES)](ops)]
    return (name, s, None if slots is None else tuple(slots)), RC.picture(h, w, 200 + s), ops, SC.params_for(name, 11 + i % 7), slots


def materialised(dev, img, ops, params, slots):
    """The path the kernel replaces: / 255 on the device, one t2o_op_fwd per step (with its mask), * 255 truncated."""
    import t2onet_amd.functional as T
    h, w = img.shape[:2]
    x = T.resize_u8([img], (h, w), device=dev)
    for k, op in enumerate(ops):
        if op >= 0:
            m = None if slots is None or slots[k] < 0 else MC.mask_f32(plane_of(slots[k], h, w)).to(dev)
            x = T.operator_apply(op, x, torch.from_numpy(params[k:k + 1]).to(dev), m)
    return T.to_u8_hwc(x)[0].cpu().numpy()


def reference(dev, i, masked):
    key, img, ops, params, slots = case(i, masked)
    if key + (i % 7,) not in _reference:
        _reference[key + (i % 7,)] = materialised(dev, img, ops, params, slots)
    return _reference[key + (i % 7,)]


def run_jobs(dev, cases, share_first_source=False, graph=False, fn=None):
    """One replay_u8_stencils call over `cases` = [(img, ops, params, slots or None)], sources and destinations packed at
    odd byte offsets with gaps; returns the per-job pictures after checking that every byte outside them still holds the
    sentinel.  Jobs without masks are 5-tuples, the others 6-tuples; the mask table is passed when any job names one."""
    import t2onet_amd.functional as T
    src_parts, jobs, pos_s, pos_o = [], [], 1, 3
    for i, (img, ops, params, slots) in enumerate(cases):
        h, w = img.shape[:2]
        if share_first_source and i == 1:
            assert img.shape == cases[0][0].shape and np.array_equal(img, cases[0][0])
            so = jobs[0][0]
        else:
            so = pos_s
            src_parts.append((so, img))
            pos_s += img.size + 1 + 2 * (i % 2)                # the next source starts at another residue modulo 4
        jobs.append((so, pos_o, h, w, list(ops)) + (() if slots is None else (list(slots),)))
        pos_o += img.size + 1 + 2 * ((i + 1) % 2)
    src = np.full(pos_s + 4, 0xC3, np.uint8)
    for so, img in src_parts:
        src[so:so + img.size] = img.reshape(-1)
    src_d = torch.from_numpy(src).to(dev)
    any_mask = any(c[3] is not None for c in cases)
    msk_d = torch.from_numpy(MASK_BUF).to(dev) if any_mask else None
    out_d = torch.full((pos_o + 4,), SENTINEL, dtype=torch.uint8, device=dev)
    par_d = torch.from_numpy(np.stack([c[2] for c in cases])).to(dev)

    def call():
        if fn is not None:
            return fn(src_d, jobs, par_d, msk_d, out_d)
        return T.replay_u8_stencils(src_d, jobs, par_d, msk_d, MASK_OFFSETS if any_mask else (), out=out_d)
    if graph:
        eager = call().clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()                                               # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        out_d.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_d, eager)
    else:
        assert call() is out_d
    out = out_d.cpu().numpy()
    untouched = np.ones(out.size, bool)
    pictures = []
    for job in jobs:
        oo, h, w = job[1:4]
        untouched[oo:oo + 3 * h * w] = False
        pictures.append(out[oo:oo + 3 * h * w].reshape(h, w, 3))
    assert (out[untouched] == SENTINEL).all(), 'a byte outside every job was written'
    return pictures


def _assert_equal(got, want, what):
    assert np.array_equal(got, want), '%s: %d bytes differ, first at %s' % (what, int((got != want).sum()), tuple(np.argwhere(got != want)[0]))


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('J', [1, 7, 64])
def test_bytes_equal_the_materialised_path(dev, J, masked):
    one = next(i for i in range(90) if case(i, masked)[0][:2] == ('five', SC.SIZES.index((33, 65))))      # J = 1: five sharpness steps on 33 x 65
    idx = [5 + i for i in range(J)] if J > 1 else [one]
    cases = [case(i, masked) for i in idx]
    if J == 64:
        assert {c[0][0] for c in cases} == set(SC.NAMES) and {c[0][1] for c in cases} == set(range(len(SC.SIZES)))
        if masked:
            assert {s for c in cases for s in c[4]} == {-1, 0, 1, 2, 3}
    if J == 7:                                                   # two jobs on one source: another list on job 0's picture
        cases[1] = (None, cases[0][1], cases[1][2], cases[1][3], cases[1][4])
        refs = [materialised(dev, *c[1:]) for c in cases]
    else:
        refs = [reference(dev, i, masked) for i in idx]
    got = run_jobs(dev, [c[1:] for c in cases], share_first_source=J == 7)
    for c, g, r in zip(cases, got, refs):
        _assert_equal(g, r, '%s %s' % (c[0], c[1].shape))


@pytest.mark.parametrize('masked', [False, True])
def test_launch_without_a_long_ring_equals_the_materialised_path(dev, masked):
    """A launch whose jobs all apply at most two sharpness steps takes the kernel's small instance (the 64- and 7-job
    calls above hold a list with more and take the large one for every job)."""
    idx = [i for i in range(40) if sum(op == 6 for op in case(i, masked)[2]) <= 2][:14]
    assert {case(i, masked)[0][0] for i in idx} == {n for n in SC.NAMES if sum(op == 6 for op in SC.LISTS[n]) <= 2}
    got = run_jobs(dev, [case(i, masked)[1:] for i in idx])
    for i, g in zip(idx, got):
        _assert_equal(g, reference(dev, i, masked), str(case(i, masked)[0]))


def _emul():
    from tests.test_replay_stencils_cpu import _compile
    return _compile('emul_replay_stencils')


def test_kernel_bytes_equal_the_host_program(dev):
    """The same phase functions, compiled by hipcc for the device and by g++ for the host."""
    from tests.test_replay_stencils_cpu import run
    lib = _emul()
    img = RC.picture(33, 65, 77)
    ops, params = SC.LISTS['five'], SC.params_for('five', 5)
    _assert_equal(run_jobs(dev, [(img, ops, params, None)])[0], run(lib.emul_replay_u8_stencils, img, ops, params), 'five 33x65')
    img = RC.picture(40, 70, 78)
    ops, params = SC.LISTS['c_ss_b'], SC.params_for('c_ss_b', 6)
    slots = [1, 0, 1, -1]
    planes = [plane_of(0, 40, 70), plane_of(1, 40, 70)]
    _assert_equal(run_jobs(dev, [(img, ops, params, slots)])[0], run(lib.emul_replay_u8_stencils, img, ops, params, slots, planes),
                  'masked c_ss_b 40x70')


def test_lists_of_the_existing_wrappers_give_their_bytes(dev):
    import t2onet_amd.functional as T
    names = ['sharp_first', 'sharp_middle', 'sharp_last', 'with_end', 'steps0', 'steps8', 'clamp_chain', 'tone']
    cases = [(RC.picture(*RC.SIZES[(2 + i) % 6], 40 + i), RC.LISTS[n][0], RC.params_for(RC.LISTS[n][0], i, RC.LISTS[n][1]), None)
             for i, n in enumerate(names)]
    old = run_jobs(dev, cases, fn=lambda src, jobs, par, msk, out: T.replay_u8(src, jobs, par, out=out))
    for n, a, b in zip(names, run_jobs(dev, cases), old):
        _assert_equal(a, b, n)
    mnames = ['sharp_first_self', 'sharp_middle_front', 'sharp_last_self', 'two_masks', 'steps8_masked', 'with_end_masked']
    cases = [(RC.picture(*RC.SIZES[(3 + i) % 6], 50 + i), MC.LISTS[n][0], RC.params_for(MC.LISTS[n][0], i),
              [-1 if m < 0 else (i + m) % 4 for m in MC.LISTS[n][1]]) for i, n in enumerate(mnames)]
    old = run_jobs(dev, cases, fn=lambda src, jobs, par, msk, out: T.replay_u8_masked(src, jobs, par, msk, MASK_OFFSETS, out=out))
    for n, a, b in zip(mnames, run_jobs(dev, cases), old):
        _assert_equal(a, b, n)


@pytest.mark.parametrize('masked', [False, True])
def test_call_is_graph_capturable(dev, masked):
    idx = [5 + i for i in range(7)]
    got = run_jobs(dev, [case(i, masked)[1:] for i in idx], graph=True)
    for i, g in zip(idx, got):
        _assert_equal(g, reference(dev, i, masked), str(case(i, masked)[0]))


def test_wrapper_refuses_what_the_library_refuses(dev):
    import t2onet_amd.functional as T
    src = torch.zeros(3 * 16 + 8, dtype=torch.uint8, device=dev)
    msk = torch.zeros(32, dtype=torch.uint8, device=dev)
    par = torch.zeros(1, 8, 24, device=dev)
    ok = (0, 0, 4, 4, [6, 6])
    assert T.replay_u8_stencils(src, [ok], par).numel() == 48
    with pytest.raises(NotImplementedError, match='inpaint'):
        T.replay_u8_stencils(src, [(0, 0, 4, 4, [6, 4, 6])], par)
    with pytest.raises(ValueError, match='steps'):
        T.replay_u8_stencils(src, [(0, 0, 4, 4, [6] * 9)], par)
    with pytest.raises(ValueError, match='64'):
        T.replay_u8_stencils(src, [ok] * 65, torch.zeros(65, 8, 24, device=dev))
    with pytest.raises(ValueError, match='reads outside'):
        T.replay_u8_stencils(src, [(12, 0, 4, 4, [6, 6])], par)
    with pytest.raises(ValueError, match='writes outside'):
        T.replay_u8_stencils(src, [ok], par, out=torch.zeros(47, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='out must be'):
        T.replay_u8_stencils(src, [ok], par, out=torch.zeros(48, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r'\(J, 8, 24\)'):
        T.replay_u8_stencils(src, [ok], torch.zeros(2, 8, 24, device=dev))
    with pytest.raises(ValueError, match='mask index'):
        T.replay_u8_stencils(src, [ok + ([0, 1],)], par, msk, [0])
    with pytest.raises(ValueError, match='mask index'):
        T.replay_u8_stencils(src, [ok + ([0, 0],)], par)                                   # no mask table at all
    with pytest.raises(ValueError, match='outside the 32-byte mask buffer'):
        T.replay_u8_stencils(src, [ok + ([0, 0],)], par, msk, [17])
    with pytest.raises(ValueError, match='at most 4 masks'):
        T.replay_u8_stencils(src, [ok + ([0, 0],)], par, msk, [0] * 5)
    with pytest.raises(ValueError, match='names 3 masks for 2 steps'):
        T.replay_u8_stencils(src, [ok + ([0, 0, 0],)], par, msk, [0])
    with pytest.raises(ValueError, match='masks must be'):
        T.replay_u8_stencils(src, [ok + ([0, 0],)], par, msk.cpu(), [0])
    # the two older wrappers refuse a second sharpness as before
    with pytest.raises(NotImplementedError, match='sharpness'):
        T.replay_u8(src, [ok], par)
    with pytest.raises(NotImplementedError, match='sharpness'):
        T.replay_u8_masked(src, [ok + ([0, 0],)], par, msk, [0])


class StubActor(torch.nn.Module):
    """What edit_image needs of the actor: a parameter (the device), `opt`, and an episode_forward that returns a fixed
    decision: pred_ops (1, n) vocabulary ids (executor index + 3, END = opt.end_id), pred_params a list of (1, 24) rows."""

    def __init__(self, ops, params):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.opt = types.SimpleNamespace(null_id=0, end_id=2)
        self.ops, self.params = ops, params

    def episode_forward(self, x, img, mask_dict, reinforce_sample=False, lengths=None):
        dev = self.anchor.device
        vocab = [self.opt.end_id if op is None else op + 3 for op in self.ops]
        return None, None, torch.tensor([vocab], device=dev), [torch.from_numpy(p[None]).to(dev) for p in self.params]


@pytest.mark.parametrize('local', [False, True])
def test_edit_image_finishes_on_a_decision_with_two_sharpness_steps(dev, local, monkeypatch):
    """[sharpness, brightness, sharpness, END]: three prefix pictures, each the materialised path's, through ONE
    replay_u8_stencils launch.  (Before the stencils kernel this decision ended in NotImplementedError.)"""
    import t2onet_amd.functional as T
    from t2onet_amd.edit import edit_image
    h, w = 37, 50
    img = RC.picture(h, w, 9)
    ops = [6, 0, 6]
    params = RC.params_for(ops + [-1], 4)
    model = StubActor(ops + [None], params[:4]).to(dev)
    plane = MC.mask('soft', h, w)
    taken = []
    for name in [n for n in ('replay_u8', 'replay_u8_masked', 'replay_u8_stencils') if hasattr(T, n)]:
        monkeypatch.setattr(T, name, (lambda f, n: lambda *a, **k: (taken.append(n), f(*a, **k))[1])(getattr(T, name), name))
    steps, got_ops, got_params = edit_image(model, img, torch.ones(1, 4, dtype=torch.long), masks={'all': plane} if local else None)
    assert taken == ['replay_u8_stencils'] and got_ops == ops and tuple(steps.shape) == (3, h, w, 3)
    assert torch.equal(got_params.cpu(), torch.from_numpy(params[:3]))
    x = T.resize_u8([img], (h, w), device=dev)
    m = MC.mask_f32(plane).to(dev) if local else None
    for k, op in enumerate(ops):
        x = T.operator_apply(op, x, torch.from_numpy(params[k:k + 1]).to(dev), m)
        _assert_equal(steps[k].cpu().numpy(), T.to_u8_hwc(x)[0].cpu().numpy(), 'prefix %d' % (k + 1))


def test_edit_image_keeps_replay_u8_for_one_sharpness(dev, monkeypatch):
    import t2onet_amd.functional as T
    from t2onet_amd.edit import edit_image
    img = RC.picture(37, 50, 9)
    ops = [0, 6]
    params = RC.params_for(ops + [-1], 4)
    model = StubActor(ops + [None], params[:3]).to(dev)
    taken = []
    for name in [n for n in ('replay_u8', 'replay_u8_masked', 'replay_u8_stencils') if hasattr(T, n)]:
        monkeypatch.setattr(T, name, (lambda f, n: lambda *a, **k: (taken.append(n), f(*a, **k))[1])(getattr(T, name), name))
    steps, got_ops, _ = edit_image(model, img, torch.ones(1, 4, dtype=torch.long))
    assert taken == ['replay_u8'] and got_ops == ops
    src = torch.from_numpy(img.reshape(-1).copy()).to(dev)
    table = torch.zeros(2, 8, 24, device=dev)
    table[:, :2] = torch.from_numpy(params[:2]).to(dev)
    want = T.replay_u8(src, [(0, 0, 37, 50, [0]), (0, 3 * 37 * 50, 37, 50, [0, 6])], table)
    assert torch.equal(steps.reshape(-1), want)


def test_apply_cli_end_to_end(dev, tmp_path):
    from PIL import Image
    import t2onet_amd.functional as T
    from t2onet_amd import apply_cli
    tone = [1.0, 1.1, 0.9, 1.2, 0.8, 1.0, 1.3, 0.7]
    record = [{'input': 'a_in.png', 'request': 'crisper', 'output': 'a.png',
               'operations': [['sharpness', [0.4]], ['tone', tone], ['sharpness', [0.3]]]}]
    with open(str(tmp_path / 'a.json'), 'w') as f:
        json.dump(record, f)
    photos = {'p.png': RC.picture(37, 50, 1), 'q.png': RC.picture(33, 65, 2)}
    for name, a in photos.items():
        Image.fromarray(a).save(str(tmp_path / name))
    infos = apply_cli.main(['--record', str(tmp_path / 'a.json'), '--img'] + [str(tmp_path / n) for n in photos]
                           + ['--save_dir', str(tmp_path / 'out'), '--multi_img'])
    ops = [6, 5, 6]
    params = np.zeros((8, 24), np.float32)
    params[0, 0], params[1, :8], params[2, 0] = 0.4, tone, 0.3
    for info, (name, a) in zip(infos, photos.items()):
        stem = name[:-4]
        h, w = a.shape[:2]
        want = T.replay_u8_stencils(torch.from_numpy(a.reshape(-1).copy()).to(dev), [(0, k * a.size, h, w, ops[:k + 1]) for k in range(3)],
                                    torch.from_numpy(params).to(dev)[None].repeat(3, 1, 1)).cpu().numpy().reshape(3, h, w, 3)
        d = tmp_path / 'out' / stem
        assert np.array_equal(np.asarray(Image.open(str(d / name))), want[2])
        assert np.array_equal(np.asarray(Image.open(str(d / (stem + '_in.png')))), a)
        for k in range(3):
            assert np.array_equal(np.asarray(Image.open(str(d / ('%d_inference_%s' % (k + 1, name))))), want[k])
        with open(str(d / (stem + '.json'))) as f:
            saved = json.load(f)
        assert saved == [json.loads(json.dumps(info))]
        assert saved[0]['request'] == 'crisper' and saved[0]['record'] == str(tmp_path / 'a.json')
        assert [n for n, _ in saved[0]['operations']] == ['sharpness', 'tone', 'sharpness']
        assert apply_cli.parse_record(saved)[1] == ops                      # a written record can be applied again
