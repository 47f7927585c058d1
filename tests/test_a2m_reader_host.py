"""CPU: the host side of the .a2m reader (include/iivision.h section f9) -- the closed-form slot count, the refusals of
iiv_a2m_reader_create that come before the device is touched, and the placeholder addresses the tools share."""

import numpy as np
import pytest

import a2m_model as M


def test_max_ops_equals_the_model(native):
    for L in range(0, 64 * 1024 + 1, 2048):
        assert native.a2m_max_ops(L) == M.max_ops(L), L
    for L in (1, 13, 14, 20, 21, 2043, 2044, 2047, 2049, 2054, 2055, 4091, 4095, 4097, 4102, 4103, 104448 - 1):
        assert native.a2m_max_ops(L) == M.max_ops(L), L
    assert native.a2m_max_ops(104448) == 291 + 292 * 50


def test_reader_refuses_addresses_that_are_not_distinct(native, golden):
    g = golden.g6_a2m
    tick, ack, term = g["tick_addr"], int(g["special_addr"][0]), int(g["special_addr"][1])
    twice = tick.copy()
    twice[31, 31] = twice[0, 0]
    for args in ((twice, ack, term), (tick, ack, ack), (tick, int(tick[3, 4]), term), (tick, ack, int(tick[30, 1]))):
        with pytest.raises(native.IIVError) as e:
            native.A2mReaderHandle(*args)
        assert e.value.code == native.ERR_INVALID


def test_placeholder_addresses_are_the_ones_transcode_clip_has_always_written(native):
    import a2m
    p = a2m.OpcodeAddresses.placeholder()
    assert p.tick.dtype == np.uint16 and p.tick.shape == (32, 32)
    assert np.array_equal(p.tick.reshape(-1), 0x8000 + 16 * np.arange(1024))
    assert (p.ack, p.terminate) == (0xc000, 0xc100)
    assert len(set(p.tick.reshape(-1).tolist()) | {p.ack, p.terminate}) == 1026
