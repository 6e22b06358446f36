"""The cases of the resident-set gather, shared by the no-GPU emulation (test_resident_cpu.py) and the kernel
(test_gpu_resident.py): N = 6 items of K = 7 pictures of random bytes in a store with guard bytes between the slots, a
slot table in which every item lacks between 1 and 5 of its middle columns, and three index vectors.  The expectation
is numpy's: store[...].astype(float32).transpose(2,0,1) / float32(255), zeros for an absent picture."""
import functools

import numpy as np

SIZES = [(1, 1), (5, 7), (16, 16), (33, 31), (128, 128)]
N, K = 6, 7
GUARD = 0xA5


def aligned_bytes(n, fill):
    """n bytes whose first one lies at a 16-byte boundary (so that a slot's offset IS its alignment)."""
    raw = np.full(n + 16, fill, np.uint8)
    at = (-raw.ctypes.data) % 16
    return raw[at:at + n]


def index_vectors():
    rng = np.random.default_rng(11)
    return {'one': np.array([4], np.int64), 'repeat': np.array([2, 5, 2], np.int64),
            'batch64': rng.integers(0, N, 64).astype(np.int64)}


@functools.lru_cache(maxsize=None)
def case(h, w):
    """(store, slots (N,K) int64, pictures {(i, k): (h,w,3) uint8}) -- computed once per size and not to be modified.
    Slots start on 16-byte boundaries, in shuffled order, with 16 .. 48 guard bytes in front of each and behind the last."""
    rng = np.random.default_rng(1000 * h + w)
    slots = np.full((N, K), -1, np.int64)
    present = []
    for i in range(N):
        n_absent = 1 + i % 5                                        # 1 .. 5 of the middle columns 1 .. 5
        gone = set((rng.permutation(5)[:n_absent] + 1).tolist())
        present += [(i, k) for k in range(K) if k not in gone]
    assert {sum(1 for i, _ in present if i == j) for j in range(N)} == {2, 3, 4, 5, 6}
    size = 3 * h * w
    pos, where = 0, {}
    for j in rng.permutation(len(present)):
        pos += 16 * int(rng.integers(1, 4))
        where[present[j]] = pos
        pos = (pos + size + 15) // 16 * 16
    store = aligned_bytes(pos + 16, GUARD)
    pictures = {}
    for (i, k), off in where.items():
        pictures[(i, k)] = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        store[off:off + size] = pictures[(i, k)].reshape(-1)
        slots[i, k] = off
    store.flags.writeable = False
    slots.flags.writeable = False
    return store, slots, pictures


@functools.lru_cache(maxsize=None)
def expected(h, w, which):
    """(img_x (B,3,h,w), img_ys (B,K-1,3,h,w)) fp32 for index vector `which`: the numpy statement."""
    store, slots, pictures = case(h, w)
    index = index_vectors()[which]
    out = np.zeros((len(index), K, 3, h, w), np.float32)
    for b, i in enumerate(index):
        for k in range(K):
            if slots[i, k] >= 0:
                off = int(slots[i, k])
                out[b, k] = store[off:off + 3 * h * w].reshape(h, w, 3).astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    out.flags.writeable = False
    return out[:, 0], out[:, 1:]
