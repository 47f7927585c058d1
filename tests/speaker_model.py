"""numpy restatement of include/iivision.h section f13: the PCM a stream's ticks play.  The slow way, on purpose: the signal is
built cycle by cycle as an int array, the filter by repeated np.convolve, and the samples are picked from the full convolution --
no running sums, no period arithmetic beyond the header's own q(k), nothing csrc/iiv_speaker.hip could share a mistake with.
tests/test_speaker_model.py holds it to things that are not the model; the GPU tests hold the kernel to it."""

import numpy as np

PERIOD = 73
ACK_WIDTH = 34
ODD_WIDTHS = {22: 21, 40: 41}      # the two opcodes whose pulse is a cycle off
MAX_DECIM, MAX_ORDER, MAX_GAIN = 73, 4, 32767


def width(tick):
    """cycles the speaker is high in the period of a tick opcode; 0 for a byte that is no tick"""
    t = int(tick)
    if t % 2 or t < 4 or t > 66:
        return 0
    return ODD_WIDTHS.get(t, t)


def acks_before(k):
    """A(k): ACKs in front of opcode k"""
    return 0 if k < 291 else 1 + (k - 291) // 292


def q(k):
    """the period of opcode k"""
    return k + 2 * acks_before(k)


def periods(n_ops):
    """Q(n): periods of a stream of n opcodes"""
    n = max(int(n_ops), 0)
    return n + 2 * acks_before(n)


def sample_count(n_ops, decim):
    """M: samples of a stream of n opcodes"""
    return -(-PERIOD * periods(n_ops) // decim)


def widths(ticks):
    """W[p] for every period of the stream, and whether a tick byte was illegal"""
    ticks = np.asarray(ticks, dtype=np.uint8).reshape(-1)
    n = len(ticks)
    W = np.full(periods(n), ACK_WIDTH, dtype=np.int64)   # what no opcode claims is an ACK period
    bad = False
    for k in range(n):
        t = int(ticks[k])
        W[q(k)] = width(t)
        bad = bad or (t % 2 == 1 or t < 4 or t > 66)
    return W, bad


def signal(ticks):
    """x(c) for 0 <= c < 73 Q, as +1 / -1"""
    W, _ = widths(ticks)
    x = -np.ones(PERIOD * len(W), dtype=np.int64)
    for p, w in enumerate(W):
        x[PERIOD * p:PERIOD * p + w] = 1
    return x


def taps(decim, order):
    """h_order"""
    h1 = np.ones(decim, dtype=np.int64)
    h = h1
    for _ in range(order - 1):
        h = np.convolve(h, h1)
    return h


def accumulate(ticks, decim, order):
    """acc[m] for 0 <= m < M"""
    n = len(np.asarray(ticks).reshape(-1))
    M = sample_count(n, decim) if n else 0
    if M == 0:
        return np.zeros(0, dtype=np.int64)
    h = taps(decim, order)
    x = signal(ticks)
    # x rests at -1 on both sides: pad far enough that every window of every sample lies inside the array
    pad = len(h) + decim
    xx = np.concatenate([-np.ones(pad, dtype=np.int64), x, -np.ones(pad, dtype=np.int64)])
    y = np.convolve(xx, h)              # y[j] = sum_i h[i] xx[j - i]
    m = np.arange(M)
    return y[pad + m * decim + decim - 1]


def pcm(ticks, decim=23, order=3, gain=16384):
    """-> (int16 (M,), bad): the samples, and whether *d_err would be set"""
    assert 1 <= decim <= MAX_DECIM and 1 <= order <= MAX_ORDER and 0 <= gain <= MAX_GAIN
    acc = accumulate(ticks, decim, order)
    v = (acc * gain) // (decim ** order)     # numpy's // floors towards minus infinity
    _, bad = widths(ticks)
    return np.clip(v, -32768, 32767).astype(np.int16), bad
