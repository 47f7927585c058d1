"""CPU: tests/speaker_model.py (include/iivision.h section f13) held to things that are not the model -- the DAC value a boxcar
of one period reads back, the plain sum of the signal, f9's byte layout, the literal table of the two odd widths -- and the host
closed forms of the library held to the model."""
import os
import re

import numpy as np
import pytest

import a2m_model
import speaker_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [0, 1, 2, 289, 290, 291, 292, 293, 581, 582, 583, 584, 585, 874, 875, 900]
DECIMS = [1, 2, 23, 72, 73]


def _ticks(rng, n):
    return (rng.integers(0, 32, n) * 2 + 4).astype(np.uint8)


def test_a_boxcar_of_one_period_reads_the_dac_value_back():
    """order 1, decim 73, gain 73: sample p is the sum of x over period p = 2 W[p] - 73.  Every tick value once, then enough of
    them to pass the first ACK."""
    every = np.arange(4, 68, 2, dtype=np.uint8)
    ticks = np.concatenate([every, _ticks(np.random.default_rng(1), 300)])
    pcm, bad = M.pcm(ticks, decim=73, order=1, gain=73)
    assert not bad and len(pcm) == M.periods(len(ticks)) == len(ticks) + 2
    for k, t in enumerate(ticks):
        want = {22: -31, 40: 9}.get(int(t), 2 * int(t) - 73)
        assert pcm[M.q(k)] == want, (k, t)
    assert M.q(290) == 290 and M.q(291) == 293
    assert pcm[291] == pcm[292] == 2 * 34 - 73 == -5          # the ACK behind opcode 290


def test_the_odd_widths_are_the_two_the_player_has():
    assert M.ODD_WIDTHS == {22: 21, 40: 41}
    for t in range(256):
        legal = t % 2 == 0 and 4 <= t <= 66
        assert M.width(t) == ({22: 21, 40: 41}.get(t, t) if legal else 0), t
    W, bad = M.widths(np.array([4, 22, 40, 66, 5, 68, 2, 0], np.uint8))
    assert list(W) == [4, 21, 41, 66, 0, 0, 0, 0] and bad
    assert not M.widths(np.array([4, 22, 40, 66], np.uint8))[1]


@pytest.mark.parametrize("decim", [1, 2, 7, 23, 64, 72, 73])
def test_a_boxcar_loses_nothing(decim):
    """order 1: the samples' windows tile [0, M decim), so sum(acc) is the sum of x over it (x = -1 past the stream's end)"""
    ticks = _ticks(np.random.default_rng(decim), 600)
    acc = M.accumulate(ticks, decim, 1)
    x = M.signal(ticks)
    m = M.sample_count(len(ticks), decim)
    assert len(acc) == m and m * decim >= len(x) > (m - 1) * decim
    assert int(acc.sum()) == int(x.sum()) - (m * decim - len(x))


def test_periods_follow_the_byte_layout_of_f9():
    """an ACK sits in front of every 2 KiB boundary but the first: opcode k has passed P(k) // 2048 of them"""
    for k in range(2001):
        assert M.q(k) == k + 2 * (a2m_model.P(k) // 2048), k
        assert M.acks_before(k) == a2m_model.P(k) // 2048
    for n in COUNTS:
        assert M.periods(n) == (M.q(n - 1) + 1 + (2 if n in (291, 583, 875) else 0) if n else 0), n
    assert [M.periods(n) for n in (290, 291, 292, 582, 583, 584)] == [290, 293, 294, 584, 587, 588]
    assert M.periods(-5) == 0


def test_filter_taps():
    for decim in DECIMS:
        for order in (1, 2, 3, 4):
            h = M.taps(decim, order)
            assert len(h) == order * (decim - 1) + 1 and int(h.sum()) == decim ** order
            assert (h == h[::-1]).all() and h[0] == 1
    assert 73 ** 4 * 32767 > 2 ** 32      # the product the header asks 64 bits for


def test_silence_before_and_after_and_the_scaling():
    """a stream of one opcode: the samples whose window lies wholly outside the pulse read -gain"""
    pcm, _ = M.pcm(np.array([66], np.uint8), decim=1, order=1, gain=32767)
    assert len(pcm) == 73 and (pcm[:66] == 32767).all() and (pcm[66:] == -32767).all()
    pcm, _ = M.pcm(np.array([4], np.uint8), decim=7, order=3, gain=1000)
    assert pcm[-1] == -1000 and pcm.max() < 1000
    assert len(M.pcm(np.zeros(0, np.uint8))[0]) == 0
    # the floor is towards minus infinity: acc = -1 of 2 at gain 1 is -1, not 0
    assert (np.array([-1]) * 1) // 2 == -1


# ---- the library's host closed forms (no GPU) -----------------------------------------------------------------------------------

def test_the_header_has_the_section():
    hdr = open(os.path.join(ROOT, "include", "iivision.h")).read()
    assert re.search(r"==== f13: speaker preview =+", hdr)
    for name in ("iiv_speaker_periods", "iiv_speaker_sample_count", "iiv_speaker_pcm"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def test_host_closed_forms_equal_the_model(native):
    L = native.lib()
    for n in COUNTS + [2000, 14700 * 60, 10 ** 9]:
        assert L.iiv_speaker_periods(n) == M.periods(n) == native.speaker_periods(n), n
        for decim in DECIMS:
            assert L.iiv_speaker_sample_count(n, decim) == M.sample_count(n, decim) == native.speaker_sample_count(n, decim), (n, decim)
    assert L.iiv_speaker_periods(-3) == 0 and L.iiv_speaker_sample_count(-3, 23) == 0
    for decim in (0, 74, -1):
        assert L.iiv_speaker_sample_count(100, decim) == native.ERR_INVALID
        with pytest.raises(native.IIVError):
            native.speaker_sample_count(100, decim)


def test_speaker_rate():
    import audio
    assert audio.speaker_rate() == audio.speaker_rate(23) == 44369
    assert audio.speaker_rate(1) == 1020484 and audio.speaker_rate(73, 1020484) == 13979
    assert audio.speaker_rate(23, 1000000) == 43478
