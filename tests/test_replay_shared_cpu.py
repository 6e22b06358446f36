"""No-GPU checks of what the three 8-bit replay entry points share on the host: one table of refused inputs through
t2o_replay_u8, t2o_replay_u8_masked and t2o_replay_u8_stencils (the same status from each, each message under the name
that entry point has always printed for that input), and the rule table of functional.replay_u8_any with the three
wrappers replaced by recorders.  Every input of the first table is refused before any launch."""
import ctypes

import pytest
import torch

ENTRIES = ('replay_u8', 'replay_u8_masked', 'replay_u8_stencils')
JOB = (0, 0, 4, 4, [0, 6], [0, -1])          # (src_offset, out_offset, h, w, ops, mask_of): a list every entry point takes

# name -> (what differs from a good call, status, who names the refusal: the entry point called ('entry'), or for a
# refusal inside a job 'job': replay_u8_masked has always printed those as "replay_u8: ...")
REFUSED = {
    'null src': (dict(src=None), 1, 'entry'),
    'J = 0': (dict(J=0), 1, 'entry'),
    'J = 65': (dict(jobs=[JOB] * 65), 1, 'entry'),
    'h = 0': (dict(jobs=[(0, 0, 0, 4) + JOB[4:]]), 1, 'job'),
    'negative src_offset': (dict(jobs=[(-1,) + JOB[1:]]), 1, 'job'),
    'steps = 9': (dict(jobs=[JOB[:4] + ([0] * 9, [0] * 8)]), 1, 'job'),
    'operator 8': (dict(jobs=[JOB[:4] + ([0, 8], [0, -1])]), 1, 'job'),
    'operator 4': (dict(jobs=[JOB[:4] + ([0, 4], [0, -1])]), 2, 'job'),
    'params = NULL with an applied step': (dict(params=None), 1, 'entry'),
    # the two entry points that take masks
    'n_masks = 5': (dict(n_masks=5), 1, 'entry'),
    'negative mask offset': (dict(offsets=[-4]), 1, 'entry'),
    'mask index = n_masks': (dict(jobs=[JOB[:5] + ([1, -1],)]), 1, 'entry'),
}
MASK_CASES = ('n_masks = 5', 'negative mask offset', 'mask index = n_masks')


@pytest.fixture(scope='module')
def lib():
    from t2onet_amd import build, _lib
    build.build()
    return _lib.load()


def call(lib, entry, jobs=(JOB,), J=None, src=True, params=True, offsets=(0,), n_masks=None):
    """One call of `entry` with host pointers (every input here is refused before anything is read through them) ->
    (status, message)."""
    import t2onet_amd.functional as T
    p = torch.zeros(64).data_ptr()
    jobs = list(jobs)
    head = (p if src else None, p, T.replay_jobs([j[:5] for j in jobs]))
    J = len(jobs) if J is None else J
    if entry == 'replay_u8':
        rc = lib.t2o_replay_u8(*head, J, p if params else None, None)
    else:
        offs = (ctypes.c_longlong * 8)(*offsets)
        rc = getattr(lib, 't2o_' + entry)(*head, T.replay_mask_table(jobs), J, p if params else None, p, offs,
                                          len(offsets) if n_masks is None else n_masks, None)
    return rc, lib.t2o_last_error().decode()


@pytest.mark.parametrize('name', sorted(REFUSED))
def test_refused_inputs_get_one_status_and_each_entry_points_own_prefix(lib, name):
    change, status, level = REFUSED[name]
    entries = [e for e in ENTRIES if e != 'replay_u8' or name not in MASK_CASES]
    got = {e: call(lib, e, **change) for e in entries}
    assert {rc for rc, _ in got.values()} == {status}, got
    for e, (_, msg) in got.items():
        who = 'replay_u8' if level == 'job' and e == 'replay_u8_masked' else e
        assert msg.startswith(who + ': '), (e, msg)


# ---------------------------------------------------------------- the dispatcher's rule
def five(ops):
    return (0, 0, 3, 5, list(ops))


def six(ops):
    return five(ops) + ([0] * len(ops),)


RULE = [
    ([five([])], 'replay_u8'), ([five([0, 5])], 'replay_u8'), ([five([0, 6, 5])], 'replay_u8'),
    ([six([0, 6])], 'replay_u8_masked'),
    ([five([6, 5, 6])], 'replay_u8_stencils'), ([five([6] * 8)], 'replay_u8_stencils'),
    ([six([6, 5, 6])], 'replay_u8_stencils'), ([six([6] * 8)], 'replay_u8_stencils'),
    # one job of several repeats the sharpness: the launch goes to the stencils kernel as a whole
    ([five([0, 6]), five([6, 0, 6]), five([])], 'replay_u8_stencils'),
    ([six([0, 6]), six([6, 6]), six([5])], 'replay_u8_stencils'),
]


@pytest.mark.parametrize('row', range(len(RULE)))
def test_the_dispatcher_holds_the_rule(monkeypatch, row):
    import t2onet_amd.functional as T
    from t2onet_amd import apply_cli
    from t2onet_amd.data import ACTIONS
    assert T.REPLAY_SHARPNESS == ACTIONS.index('sharpness') == 6          # the rows below spell the sharpness 6
    jobs, want = RULE[row]
    calls = []

    def recorder(name):
        def fn(*args):
            calls.append((name, args))
            return name
        return fn
    for name in ENTRIES:
        monkeypatch.setattr(T, name, recorder(name))
    src, params, masks, out = (torch.zeros(1) for _ in range(4))
    masked = len(jobs[0]) == 6
    got = T.replay_u8_any(src, jobs, params, masks if masked else None, [0] if masked else (), out)
    assert got == want and [name for name, _ in calls] == [want]
    args = calls[0][1]
    assert args[0] is src and [tuple(j) for j in args[1]] == [tuple(j) for j in jobs] and args[2] is params and args[-1] is out
    if want != 'replay_u8':
        assert len(args) == 6 and args[3] is (masks if masked else None) and list(args[4]) == ([0] if masked else [])
    assert T.replay_u8_pick(jobs) == want
    if not masked:
        for job in jobs:                                              # apply_cli's name of the same rule
            assert apply_cli.pick_wrapper(job[4]) == T.replay_u8_pick([job])
        assert want == ('replay_u8_stencils' if any(apply_cli.pick_wrapper(job[4]) == 'replay_u8_stencils' for job in jobs) else 'replay_u8')
