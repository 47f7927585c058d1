"""CPU: tests/a2m_model.py (the numpy restatement of include/iivision.h section f9) against the reference's own recordings:
the opcodes and ticks its emitter was given (g6), the screen memory its Movie held when the stream ended (g7), and every
status on streams broken in one place each."""

import numpy as np
import pytest

import a2m_cases
import a2m_model as M

G6 = ("HGR_a", "DHGR_a", "DHGR_b", "DHGR_c", "HGR_limit", "DHGR_empty")
G7 = ("DHGR_n1", "DHGR_n2", "HGR_n1", "HGR_n2", "DHGR_n2_audio_end")


def test_slot_positions_and_counts():
    assert [M.P(k) for k in (0, 1, 290, 291, 292, 582, 583)] == [7, 14, 2037, 2048, 2055, 4085, 4096]
    assert [M.max_ops(L) for L in (0, 13, 14, 2047, 2048, 2054, 2055, 4096)] == [0, 0, 1, 291, 291, 291, 292, 583]


@pytest.mark.parametrize("tag", G6)
def test_model_reads_back_what_the_reference_emitter_was_given(golden, tag):
    g = golden.g6_a2m
    addr = a2m_cases.addresses(g)
    stream, ops, ticks = g[tag + "/stream"], g[tag + "/ops"], g[tag + "/ticks"]
    n = {"HGR_limit": 427, "DHGR_empty": 0}.get(tag, len(ops))
    assert M.scan(stream, *addr) == (M.OK, int(g[tag + "/meta"][0]), n, 0)
    mode, got_ops, got_ticks, banks = M.decode(stream, *addr)
    assert mode == int(g[tag + "/meta"][0])
    assert np.array_equal(got_ops, ops[:n]) and np.array_equal(got_ticks, ticks[:n])
    want_banks = {"DHGR_b": {0}, "DHGR_c": {0, 1}, "DHGR_a": {0, 1}, "HGR_a": {0}, "HGR_limit": {0}, "DHGR_empty": set()}[tag]
    assert set(banks.tolist()) == want_banks
    if tag == "DHGR_c":
        assert banks[:291].max() == 0 and banks[291] == 1
    if tag == "DHGR_a":   # the bank after ACK i is the parity of i + 1
        assert np.array_equal(banks, ((np.arange(1000) + 1) // 292 & 1).astype(np.uint8))


@pytest.mark.parametrize("tag", G7)
def test_model_replays_the_reference_movie_to_its_own_screen_memory(golden, tag):
    g = golden.g7_movie
    addr = a2m_cases.addresses(golden.g6_a2m)
    stream = g[tag + "/stream"]
    status, mode, n_ops, _ = M.scan(stream, *addr)
    assert (status, mode) == (M.OK, int(g[tag + "/meta"][0]))
    assert n_ops == (2527 if tag == "DHGR_n2_audio_end" else 14699)
    main, aux = M.replay(stream, *addr, first=1 << 40, every=1, n=1)
    assert np.array_equal(main[0], g[tag + "/mem_main"])
    if mode == 1:
        assert np.array_equal(aux[0], g[tag + "/mem_aux"])
    else:
        assert not aux.any()


def test_model_status_of_every_broken_stream(golden):
    g = golden.g6_a2m
    addr = a2m_cases.addresses(g)
    cases = a2m_cases.broken_streams(g)
    assert {c[2][0] for c in cases} == set(range(7))
    for name, b, want in cases:
        assert M.scan(b, *addr) == want, name


def test_model_snapshots_are_prefixes(golden):
    """snapshot j of a sampled replay is the final snapshot of a replay cut at that many opcodes; an offset named twice and
    the starting state are honoured"""
    g = golden.g6_a2m
    addr = a2m_cases.addresses(g)
    stream = g["DHGR_a/stream"]
    rng = np.random.default_rng(5)
    init = rng.integers(0, 256, (2, 32, 256), dtype=np.uint8)
    main, aux = M.replay(stream, *addr, first=3, every=250, n=6, init=(init[0], init[1]))
    for j in range(6):
        m1, a1 = M.replay(stream, *addr, first=min(3 + 250 * j, 1000), every=1, n=1, init=(init[0], init[1]))
        assert np.array_equal(main[j], m1[0]) and np.array_equal(aux[j], a1[0])
    assert np.array_equal(main[5], main[4]) and not np.array_equal(main[4], main[3])
    m0, a0 = M.replay(stream, *addr, first=0, every=1, n=1, init=(init[0], init[1]))
    assert np.array_equal(m0[0], init[0]) and np.array_equal(a0[0], init[1])
