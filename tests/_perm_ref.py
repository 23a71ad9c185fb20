"""Reference of the keyed pixel permutation (ssdnerf_amd/csrc/keyed_perm.h), restated in numpy FROM THE HEADER'S COMMENT, not from its code: the even
domain width, the balanced Feistel network, the two-multiply round function, the Philox round keys (tests/_philox_ref.py) and the cycle walk.  Both test
modules draw from here: tests/test_ray_perm_cpu.py (the gcc build equals this bit for bit; bijection; statistics; key separation) and
tests/test_ray_perm_gpu.py (the kernels equal it bit for bit).  ``rounds`` is a parameter only so that the statistical tests can show that a weakened
network fails them.

Nothing here needs a GPU."""
import numpy as np

import _philox_ref as PR

ROUNDS = 12
TAG = 0x5045524D                                                               # "PERM": c3 of the round keys' counter (the noise uses c3 = 0)
U32 = np.uint32


def half_bits(P):
    """h = b / 2: b the smallest even number >= 2 with 2^b >= P"""
    P = int(P)
    assert 1 <= P < 1 << 32
    h = 1
    while (1 << (2 * h)) < P:
        h += 1
    return h


def round_keys(seed, scene, draw, rounds=ROUNDS):
    """uint32 [..., rounds]: k[4 q + e] = word e of Philox4x32-10(key = seed, counter = {scene, draw, q, TAG}); ``scene`` / ``draw`` may be arrays"""
    seed = int(seed) & ((1 << 64) - 1)
    scene, draw = np.broadcast_arrays(np.asarray(scene, np.uint64), np.asarray(draw, np.uint64))
    words = []
    for q in range((rounds + 3) // 4):
        words += PR.philox4x32_10(scene, draw, np.uint64(q), np.uint64(TAG), seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(words[:rounds], axis=-1)


def mix(t):
    """t ^= t >> 16; t *= 0x7FEB352D; t ^= t >> 15; t *= 0x846CA68B; t ^= t >> 16 on uint32 arrays (numpy's uint32 product wraps modulo 2^32)"""
    t = t ^ (t >> U32(16))
    t = t * U32(0x7FEB352D)
    t = t ^ (t >> U32(15))
    t = t * U32(0x846CA68B)
    return t ^ (t >> U32(16))


def feistel(keys, h, v):
    """pihat on a uint32 array ``v`` of values below 4^h; ``keys`` [..., rounds] broadcasts against v[..., None]"""
    h, m = U32(h), U32((1 << h) - 1)
    L, R = v >> h, v & m
    with np.errstate(over="ignore"):
        for i in range(keys.shape[-1]):
            L, R = R, L ^ (mix(R + keys[..., i]) & m)
    return (L << h) | R


def walk(keys, P, j):
    """(pi(j), evaluations) for a uint32 array ``j`` of positions below P"""
    h = half_bits(P)
    keys = np.asarray(keys, U32)
    v = np.array(np.broadcast_to(np.asarray(j, U32), np.broadcast_shapes(np.shape(j), keys.shape[:-1])))
    keys = np.broadcast_to(keys, v.shape + keys.shape[-1:])
    evals = np.zeros(v.shape, np.int64)
    todo = np.ones(v.shape, bool)
    while todo.any():
        v[todo] = feistel(keys[todo], h, v[todo])
        evals[todo] += 1
        todo &= v >= U32(int(P))
    return v.astype(np.int64), evals


def perm_range(seed, scene, draw, P, start=0, count=None, rounds=ROUNDS):
    """int64 [count]: pi(seed, scene, draw, P)(start + r)"""
    count = int(P) - int(start) if count is None else count
    assert int(start) + count <= int(P)
    j = (np.uint64(int(start)) + np.arange(count, dtype=np.uint64)).astype(U32)
    return walk(round_keys(seed, scene, draw, rounds), P, j)[0]


def perm_draws(seed, scene, first_draw, draws, P, n, rounds=ROUNDS):
    """int64 [draws, n]: pi(seed, scene, first_draw + d, P)(r), r < n"""
    keys = round_keys(seed, scene, int(first_draw) + np.arange(draws), rounds)            # [draws, rounds]
    return walk(keys[:, None, :], P, np.arange(n, dtype=U32)[None, :])[0]


def perm_indices(seed, S, draw, P, start, R):
    """int64 [S, R]: what ssdnerf_perm_indices writes"""
    return np.stack([perm_range(seed, s, draw, P, start, R) for s in range(S)])
