"""Streams broken in one place each (and one in two), with the status include/iivision.h section f9 gives them, worked out
by hand from that section -- not by running anything.  Shared by tests/test_a2m_model.py (the numpy model) and
tests/test_gpu_a2m_reader.py (the kernels)."""

import numpy as np

import a2m_model as M


def addresses(g6):
    """(tick_addr, ack, terminate) of the g6 recording"""
    return g6["tick_addr"], int(g6["special_addr"][0]), int(g6["special_addr"][1])


def broken_streams(g6):
    """[(name, bytes, (status, mode, n_ops, position))] from g6's DHGR_a: 1000 opcodes, 8192 bytes, Terminate at P(1000) = 7019,
    ACKs at 2044, 4092 and 6140; an intact copy between the broken ones."""
    base = g6["DHGR_a/stream"].copy()
    assert len(base) == 8192 and M.P(1000) == 7019
    intact = ("intact", base, (M.OK, 1, 1000, 0))
    out = []

    def case(name, b, want):
        out.append((name, b, want))
        out.append(intact)

    out.append(intact)
    case("length 4095", base[:4095].copy(), (M.BAD_LENGTH, 0, 0, 0))
    b = base.copy(); b[3] = 0
    case("header byte 3 zero", b, (M.BAD_HEADER, 1, 1000, 3))
    b = base.copy(); b[6] = 2
    case("mode byte 2", b, (M.BAD_HEADER, 2, 1000, 6))
    b = base.copy(); b[M.P(100)] = 0; b[M.P(100) + 1] = 1            # address 0x0001: no opcode of the recording's player
    case("slot 100 unknown", b, (M.BAD_ADDRESS, 1, 100, M.P(100)))
    b = base.copy(); b[2046] = 0x56
    case("bank byte 0x56", b, (M.BAD_ACK, 1, 1000, 2046))
    b = base.copy(); b[2047] = 0
    case("ack fourth byte 0", b, (M.BAD_ACK, 1, 1000, 2047))
    case("no terminate", base[:2048].copy(), (M.NO_TERMINATE, 1, 291, 2048))
    b = base.copy(); b[8000] = 1
    case("padding byte", b, (M.BAD_PADDING, 1, 1000, 8000))
    case("2048 extra zeros", np.concatenate([base, np.zeros(2048, np.uint8)]), (M.BAD_PADDING, 1, 1000, 8192))
    b = base.copy(); b[8191] = 9; b[4094] = 0x53
    case("two offences", b, (M.BAD_ACK, 1, 1000, 4094))
    return out
