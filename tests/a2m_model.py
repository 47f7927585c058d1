"""numpy restatement of include/iivision.h section f9: reading an .a2m stream -- its layout, the status of a stream as
written (scan), its opcodes (decode) and the screen memory a player holds after k of them (replay).  Written from the
prose of that section, one byte at a time where the device works in parallel; tests/test_a2m_model.py holds it to the
reference's own recordings, the GPU tests hold the kernels to it."""

import numpy as np

OK, BAD_LENGTH, BAD_HEADER, BAD_ACK, BAD_ADDRESS, NO_TERMINATE, BAD_PADDING = range(7)
STATUS_NAMES = ("OK", "BAD_LENGTH", "BAD_HEADER", "BAD_ACK", "BAD_ADDRESS", "NO_TERMINATE", "BAD_PADDING")


def P(k):
    """byte position of slot k"""
    if k < 291:
        return 7 + 7 * k
    g, r = divmod(k - 291, 292)
    return 2048 * (1 + g) + 7 * r


def max_ops(length):
    """whole slots in a stream of that length, by counting"""
    k = 0
    while P(k) + 7 <= length:
        k += 1
    return k


def _inverse(tick_addr):
    t = np.asarray(tick_addr, dtype=np.uint16).reshape(1024)
    return {int(a): i for i, a in enumerate(t)}


def _addr(b, p):
    return (int(b[p]) << 8) | int(b[p + 1])


def _acks_before(n_ops):
    """byte positions of the ACKs that follow a tick slot k < n_ops"""
    return [P(k) + 7 for k in range(n_ops) if (P(k) + 7) % 2048 == 2044]


def scan(stream, tick_addr, ack_addr, terminate_addr):
    """-> (status, mode, n_ops, position)"""
    b = np.asarray(stream, dtype=np.uint8).reshape(-1)
    L = len(b)
    if L == 0 or L % 2048:
        return BAD_LENGTH, 0, 0, 0
    inv = _inverse(tick_addr)
    slots = max_ops(L)
    n_ops = slots
    for k in range(slots):
        if _addr(b, P(k)) not in inv:
            n_ops = k
            break
    mode = int(b[6])
    offences = []   # (position, status)
    for i in range(6):
        if b[i] != 0xff:
            offences.append((i, BAD_HEADER))
    if mode not in (0, 1):
        offences.append((6, BAD_HEADER))
    for p in _acks_before(n_ops):
        if b[p] != ack_addr >> 8:
            offences.append((p, BAD_ACK))
        elif b[p + 1] != ack_addr & 0xff:
            offences.append((p + 1, BAD_ACK))
        elif b[p + 2] not in (0x54, 0x55):
            offences.append((p + 2, BAD_ACK))
        elif b[p + 3] != 0xff:
            offences.append((p + 3, BAD_ACK))
    pt = P(n_ops)
    if n_ops == slots:
        offences.append((pt, NO_TERMINATE))
    else:
        if _addr(b, pt) != terminate_addr:
            offences.append((pt, BAD_ADDRESS))
        nz = np.flatnonzero(b[pt + 2:])
        if len(nz):
            offences.append((pt + 2 + int(nz[0]), BAD_PADDING))
        end = (pt + 2 + 2047) // 2048 * 2048
        if L != end:
            offences.append((end, BAD_PADDING))
    if not offences:
        return OK, mode, n_ops, 0
    pos, status = min(offences)
    return status, mode, n_ops, pos


def decode(stream, tick_addr, ack_addr, terminate_addr):
    """-> (mode, ops (n_ops, 6), ticks (n_ops,), banks (n_ops,)) of the first n_ops opcodes, whatever the status"""
    b = np.asarray(stream, dtype=np.uint8).reshape(-1)
    _, mode, n_ops, _ = scan(b, tick_addr, ack_addr, terminate_addr)
    inv = _inverse(tick_addr)
    ops = np.zeros((n_ops, 6), np.uint8)
    ticks = np.zeros(n_ops, np.uint8)
    banks = np.zeros(n_ops, np.uint8)
    bank = 0
    for k in range(n_ops):
        p = P(k)
        ti, pi = divmod(inv[_addr(b, p)], 32)
        ops[k, 0] = 32 + pi
        ops[k, 1:] = b[p + 2:p + 7]
        ticks[k] = 4 + 2 * ti
        banks[k] = bank
        if (p + 7) % 2048 == 2044:
            bank = int(b[p + 9]) & 1
    return mode, ops, ticks, banks


def replay(stream, tick_addr, ack_addr, terminate_addr, first, every, n, init=None):
    """-> (main, aux) uint8 (n, 32, 256): snapshot j is the screen memory after the first min(first + j * every, n_ops)
    opcodes, each storing its content byte at its four offsets of its page in its bank, in stream order.
    init: (main, aux) (32, 256) starting state, None = zeros."""
    _, ops, _, banks = decode(stream, tick_addr, ack_addr, terminate_addr)
    mem = np.zeros((2, 32, 256), np.uint8)
    if init is not None:
        mem[0], mem[1] = init
    out = np.zeros((n, 2, 32, 256), np.uint8)
    k = 0
    for j in range(n):
        target = min(first + j * every, len(ops))
        while k < target:
            page, content = int(ops[k, 0]) - 32, ops[k, 1]
            for off in ops[k, 2:6]:
                mem[banks[k], page, off] = content
            k += 1
        out[j] = mem
    return out[:, 0].copy(), out[:, 1].copy()


def random_ops(rng, n, pages=(32, 64), offsets=None):
    """n opcodes of random bytes on pages[0] .. pages[1] - 1 (offsets: drawn from these only), and their tick bytes"""
    ops = rng.integers(0, 256, (n, 6), dtype=np.uint8)
    ops[:, 0] = rng.integers(pages[0], pages[1], n)
    if offsets is not None:
        ops[:, 2:] = rng.choice(np.asarray(offsets, dtype=np.uint8), (n, 4))
    ticks = (rng.integers(0, 32, n) * 2 + 4).astype(np.uint8)
    return ops, ticks
