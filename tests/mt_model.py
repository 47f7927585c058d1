"""A plain MT19937 model in numpy uint32, independent of the oracle and of every kernel (Matsumoto & Nishimura 1998,
the reference implementation's genrand_int32): what tests/test_mt_model.py holds CPython's `random`, numpy's
`RandomState` and the oracle to, and what tests/test_gpu_rng_blocks.py compares end states with.

A state is 625 words, the layout of random.getstate()[1]: the 624-word block, then the index 0..624 of the next word."""

import numpy as np

N, M = 624, 397
_UPPER, _LOWER, _MATRIX_A = np.uint32(0x80000000), np.uint32(0x7FFFFFFF), np.uint32(0x9908B0DF)


def twist(block):
    """The block after `block`: word i from the old words i, i + 1 and word (i + 397) % 624, which for i >= 227 is a NEW
    word -- and word 623's `i + 1` is the NEW word 0."""
    mt = np.array(block, dtype=np.uint32).reshape(N).copy()
    for i in range(N):
        y = (mt[i] & _UPPER) | (mt[(i + 1) % N] & _LOWER)
        mt[i] = mt[(i + M) % N] ^ (y >> np.uint32(1)) ^ (_MATRIX_A if y & np.uint32(1) else np.uint32(0))
    return mt


def temper(word):
    y = np.uint32(word)
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def state(block, index):
    s = np.empty(N + 1, dtype=np.uint32)
    s[:N] = np.asarray(block, dtype=np.uint32).reshape(N)
    s[N] = index
    return s


def _next_word(st):
    """the next tempered 32-bit output; `st` (625 words) is advanced in place"""
    if st[N] >= N:
        st[:N] = twist(st[:N])
        st[N] = 0
    y = temper(st[int(st[N])])
    st[N] += 1
    return y


def draw_py(st):
    """random.getrandbits(8): the top 8 bits of the next output (video.py:178,291)"""
    return int(_next_word(st) >> np.uint32(24))


def draw_np(st):
    """np.random.randint(0, 256): the low 8 bits of the next output (video.py:265)"""
    return int(_next_word(st) & np.uint32(0xFF))


def canonical(words625):
    """(B, 624) -> (twist(B), 0); every other index as it is.  Both name the same stream -- the next draw is word 0 of
    twist(B) either way -- so two states are the same stream exactly when their canonical forms are equal, word for word."""
    st = np.array(words625, dtype=np.uint32).reshape(N + 1).copy()
    assert st[N] <= N, "index %d" % st[N]
    if st[N] == N:
        st[:N] = twist(st[:N])
        st[N] = 0
    return st
