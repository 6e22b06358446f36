"""The cases of the resident-item gather, shared by the no-GPU emulation (test_resident_gier_cpu.py) and the kernel
(test_gpu_resident_gier.py): N = 6 items of K pictures of random bytes in a store with guard bytes between the slots.
Items SHARE slots the way GIER items do -- item 1 has item 0's input and planned steps but its own target (two pairs on one
input picture), item 2 is item 1 again (two requests of one pair), item 5 uses one picture in two of its columns -- and
items 3 and 4 lack some of their middle columns.  A row table (N, V) of plane numbers and -1, and four index vectors: one
item, repeats, an index outside [0, N) on either side, and a batch whose rows need more than one workgroup.  The
expectation is numpy's: store[...].astype(float32).transpose(2,0,1) / float32(255), zeros for an absent picture or a bad
index; rows[index], -1 for a bad index."""
import functools

import numpy as np

from tests.resident_cases import GUARD, aligned_bytes

# the sizes the gather must serve: one pixel, h w % 4 != 0, h w % 4 == 0, one full workgroup less a pixel; (40, 30) adds a
# picture of two workgroups
SIZES = [(1, 1), (5, 7), (4, 4), (33, 31), (40, 30)]
KS = [1, 7, 10, 16]
VS = [0, 1, 11]
N = 6


def index_vectors():
    rng = np.random.default_rng(12)
    return {'one': np.array([4], np.int64), 'repeat': np.array([2, 5, 2, 1], np.int64),
            'bad': np.array([3, N, -1, 0, 1 << 40], np.int64), 'batch37': rng.integers(0, N, 37).astype(np.int64)}


@functools.lru_cache(maxsize=None)
def case(h, w, K):
    """(store, slots (N,K) int64) -- computed once per shape and not to be modified.  Slots start on 16-byte boundaries, in
    shuffled order, with 16 .. 48 guard bytes in front of each and behind the last."""
    rng = np.random.default_rng(100000 * K + 1000 * h + w)
    name = np.full((N, K), -1, np.int64)                             # picture numbers first, offsets below
    count = 0
    for i in range(N):
        for k in range(K):
            name[i, k] = count
            count += 1
    if K > 1:
        name[1, :K - 1] = name[0, :K - 1]                             # another pair on the same input and action directory
        name[5, K - 1] = name[5, 0]                                   # one picture in two columns of an item
    name[2] = name[1]                                                 # another request of the same pair
    for i, gone in ((3, range(2, K - 1)), (4, range(1, K - 1, 2))):  # absent middle columns
        name[i, list(gone)] = -1
    used = np.unique(name[name >= 0])
    size = 3 * h * w
    pos, where = 0, {}
    for j in rng.permutation(len(used)):
        pos += 16 * int(rng.integers(1, 4))
        where[int(used[j])] = pos
        pos = (pos + size + 15) // 16 * 16
    store = aligned_bytes(pos + 16, GUARD)
    for off in where.values():
        store[off:off + size] = rng.integers(0, 256, size).astype(np.uint8)
    slots = np.array([[where[int(p)] if p >= 0 else -1 for p in row] for row in name], np.int64).reshape(N, K)
    if K > 1:
        assert slots[1, 0] == slots[0, 0] and slots[1, K - 1] != slots[0, K - 1] and (slots[2] == slots[1]).all()
    if K > 2:
        assert (slots[4] < 0).any()
    store.flags.writeable = False
    slots.flags.writeable = False
    return store, slots


@functools.lru_cache(maxsize=None)
def rows(V):
    """(N, V) int32: plane numbers in [0, 50) and -1, every item's row distinct."""
    rng = np.random.default_rng(77 + V)
    table = rng.integers(-1, 50, (N, V)).astype(np.int32)
    if V:
        table[:, 0] = 10 * np.arange(N) - 1                           # item 0: -1 ("no entry")
    table.flags.writeable = False
    return table


@functools.lru_cache(maxsize=None)
def expected(h, w, K, which):
    """(img_x (B,3,h,w), img_ys (B,K-1,3,h,w)) fp32 for index vector `which`: the numpy statement."""
    store, slots = case(h, w, K)
    index = index_vectors()[which]
    out = np.zeros((len(index), K, 3, h, w), np.float32)
    for b, i in enumerate(index):
        for k in range(K):
            if 0 <= i < N and slots[i, k] >= 0:
                off = int(slots[i, k])
                out[b, k] = store[off:off + 3 * h * w].reshape(h, w, 3).astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    out.flags.writeable = False
    return out[:, 0], out[:, 1:]


def expected_rows(V, which):
    index = index_vectors()[which]
    ok = (index >= 0) & (index < N)
    return np.where(ok[:, None], rows(V)[np.where(ok, index, 0)], -1).astype(np.int32)
