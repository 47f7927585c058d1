"""GPU: the speaker preview (include/iivision.h section f13; csrc/iiv_speaker.hip) against the numpy model
(tests/speaker_model.py), sample for sample: nine streams of nine counts in one batch over every decimation, order and gain of the
grid and three kinds of ticks, the error flag, the recorded .a2m streams through A2mReader.speaker_pcm, a scan's own counts, the
refusals, and one call on a busy side stream."""
import ctypes as C

import numpy as np
import pytest

import a2m_model
import speaker_cases as SC
import speaker_model as M
from device_guards import guarded, ok
from stream_cases import dp as _dp, g6_addresses
from stream_probe import Probe
from test_gpu_a2m_reader import G6, G7

pytestmark = pytest.mark.gpu

S = len(SC.COUNTS)
GUARD = 0xA5
LEAD, TRAIL = 64 + 2, 64     # the output starts 2 bytes past a 64-byte boundary: no row is 16-byte aligned unless its stride makes it so


def _counts_tensor(counts=SC.COUNTS):
    import torch
    return torch.tensor(list(counts), dtype=torch.int64, device="cuda")


def _check_batch(got, kind, decim, order, gain, label):
    """got: int16 numpy (S, stride) that held SENTINEL everywhere before the call"""
    for s in range(S):
        want = SC.want(kind, s, decim, order, gain)
        m = M.sample_count(SC.COUNTS[s], decim)
        assert len(want) == m
        bad = np.flatnonzero(got[s, :m] != want)
        assert len(bad) == 0, "%s: stream %d (%d opcodes): %d of %d samples differ, the first at %s: kernel %s, model %s" % (
            label, s, SC.COUNTS[s], len(bad), m, bad[:5], got[s, bad[:5]], want[bad[:5]])
        assert (got[s, m:] == SC.SENTINEL).all(), "%s: stream %d wrote behind its %d samples" % (label, s, m)


@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("order", SC.ORDERS)
@pytest.mark.parametrize("decim", SC.DECIMS)
def test_batch_of_nine_counts_equals_the_model(native, decim, order, kind):
    """Every gain; rows at an odd stride from an address that is 2 (mod 16) -- the 2-byte stores and, where a row happens to fall
    on 16 bytes, the 16-byte ones -- and rows the binding lays out 16-byte aligned.  The flag stays 0: no byte behind a count is
    read."""
    import torch
    L = native.lib()
    ticks = torch.from_numpy(SC.ticks(kind).copy()).cuda()
    counts = _counts_tensor()
    width = M.sample_count(SC.STRIDE, decim)
    stride = width + 3
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    for gain in SC.GAINS:
        buf, view = guarded(S * stride * 2, LEAD, TRAIL, GUARD)
        out = view.view(torch.int16).view(S, stride)
        out.fill_(SC.SENTINEL)
        ok(native, L.iiv_speaker_pcm(S, _dp(ticks), SC.STRIDE, _dp(counts), 1, decim, order, gain, _dp(out), stride, _dp(err),
                                     native.stream_ptr()))
        _check_batch(out.cpu().numpy(), kind, decim, order, gain, "odd stride, gain %d" % gain)
        host = buf.cpu().numpy()
        assert (host[:LEAD] == GUARD).all() and (host[LEAD + S * stride * 2:] == GUARD).all()
        aligned = torch.full((S, -(-width // 8) * 8), SC.SENTINEL, dtype=torch.int16, device="cuda")
        got, m = native.speaker_pcm(ticks, counts, decim, order, gain, out=aligned, d_err=err)
        assert got.data_ptr() == aligned.data_ptr() and got.data_ptr() % 16 == 0 and got.stride(0) % 8 == 0
        assert list(m) == [M.sample_count(n, decim) for n in SC.COUNTS]
        _check_batch(got.cpu().numpy(), kind, decim, order, gain, "aligned rows, gain %d" % gain)
    assert int(err.item()) == 0


def test_the_extremes_reach_full_scale():
    """what the all-4 and all-66 rows are for, on the model: at gain 32767 and one sample a cycle the level is +-32767"""
    hi, lo = SC.want("extremes", 8, 1, 1, 32767), SC.want("extremes", 7, 1, 1, 32767)
    assert hi.max() == 32767 and hi.min() == -32767 and lo.max() == 32767 and lo.min() == -32767
    assert (SC.ticks("extremes")[8, :900] == 66).all() and (SC.ticks("extremes")[7, :584] == 4).all()


def test_a_bad_tick_raises_the_flag_and_counts_as_silence(native):
    """an odd tick and a 68: width 0, *d_err = 1; the same batch without them leaves the flag alone"""
    import torch
    clean = SC.ticks("random").copy()
    dirty = clean.copy()
    dirty[8, 100], dirty[6, 400] = 35, 68
    counts = _counts_tensor()
    for t, flag in ((clean, 0), (dirty, 1)):
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        got, m = native.speaker_pcm(torch.from_numpy(t).cuda(), counts, 23, 3, 16384, d_err=err)
        assert int(err.item()) == flag
        got = got.cpu().numpy()
        for s in range(S):
            want, bad = M.pcm(t[s, :SC.COUNTS[s]], 23, 3, 16384)
            assert bad == (flag == 1 and s in (6, 8))
            assert np.array_equal(got[s, :m[s]], want), s
    # the model of the dirty rows is the model of the rows with a width-0 pulse there, and that differs from the clean rows
    assert not np.array_equal(M.pcm(dirty[8, :900])[0], M.pcm(clean[8, :900])[0])
    # d_err may be NULL
    got, _ = native.speaker_pcm(torch.from_numpy(dirty).cuda(), counts)
    assert np.array_equal(got.cpu().numpy()[8, :M.sample_count(900, 23)], M.pcm(dirty[8, :900])[0])


@pytest.fixture(scope="module")
def addr(golden):
    import a2m
    g = golden.g6_a2m
    return a2m.OpcodeAddresses(g["tick_addr"], g["special_addr"][0], g["special_addr"][1], g["special_addr"][2])


def test_recorded_streams_through_the_reader(native, addr, golden):
    """A2mReader.speaker_pcm of the recordings tests/test_gpu_a2m_reader.py reads -- 0 to 14 699 opcodes, fifty ACKs -- against
    the model on the model's own decoding of their ticks"""
    import a2m
    streams = [golden.g6_a2m[t + "/stream"] for t in G6] + [golden.g7_movie[t + "/stream"] for t in G7]
    reader = a2m.A2mReader(addr)
    try:
        got = reader.speaker_pcm(streams)
        other = reader.speaker_pcm(streams[:6], decim=64, order=4, gain=32767)
    finally:
        reader.close()
    assert len(got) == len(streams)
    counts = []
    for i, b in enumerate(streams):
        _, _, ticks, _ = a2m_model.decode(b, addr.tick, addr.ack, addr.terminate)
        counts.append(len(ticks))
        want, bad = M.pcm(ticks)
        assert not bad and got[i].dtype.is_signed and tuple(got[i].shape) == (M.sample_count(len(ticks), 23),)
        assert np.array_equal(got[i].cpu().numpy(), want), i
        if i < 6:
            assert np.array_equal(other[i].cpu().numpy(), M.pcm(ticks, 64, 4, 32767)[0]), i
    assert min(counts) == 0 and max(counts) == 14699


def test_counts_straight_from_a_scan(native, golden):
    """d_info + 2 with stride 4 as d_counts: scan, decode and the speaker kernel enqueued one behind the other"""
    import torch
    L = native.lib()
    tick, ack, term = g6_addresses(golden)
    streams = [golden.g6_a2m[t + "/stream"] for t in G6]
    n_s, stride = len(streams), max(len(b) for b in streams)
    data = torch.zeros((n_s, stride), dtype=torch.uint8, device="cuda")
    for i, b in enumerate(streams):
        data[i, :len(b)] = torch.from_numpy(b.copy()).cuda()
    lengths = torch.tensor([len(b) for b in streams], dtype=torch.int64, device="cuda")
    h = native.A2mReaderHandle(tick, ack, term)
    max_ops = native.a2m_max_ops(stride)
    width = native.speaker_sample_count(max_ops, 23)
    info = torch.empty((n_s, 4), dtype=torch.int64, device="cuda")
    ops = torch.zeros((n_s, max_ops, 6), dtype=torch.uint8, device="cuda")
    ticks = torch.full((n_s, max_ops), SC.FILL_TICK, dtype=torch.uint8, device="cuda")
    banks = torch.zeros((n_s, max_ops), dtype=torch.uint8, device="cuda")
    out = torch.full((n_s, width), SC.SENTINEL, dtype=torch.int16, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = native.stream_ptr()
    ok(native, L.iiv_a2m_scan(h._h, n_s, _dp(data), stride, _dp(lengths), _dp(info), st))
    ok(native, L.iiv_a2m_decode(h._h, n_s, _dp(data), stride, _dp(info), _dp(ops), max_ops * 6, _dp(ticks), _dp(banks), max_ops, st))
    ok(native, L.iiv_speaker_pcm(n_s, _dp(ticks), max_ops, C.c_void_p(info.data_ptr() + 16), 4, 23, 3, 16384, _dp(out), width, _dp(err), st))
    got = out.cpu().numpy()
    assert int(err.item()) == 0
    for i, b in enumerate(streams):
        _, _, m_ticks, _ = a2m_model.decode(b, tick, ack, term)
        want, _ = M.pcm(m_ticks)
        assert np.array_equal(got[i, :len(want)], want) and (got[i, len(want):] == SC.SENTINEL).all(), i
    h.close()


def test_counts_are_clamped_to_the_row(native):
    """a negative count is 0, one above ticks_stride is ticks_stride"""
    import torch
    t = SC.ticks("random")[8:9, :900].copy()
    ticks = torch.from_numpy(np.repeat(t, 3, axis=0)).cuda()
    counts = torch.tensor([-5, 900, 1 << 40], dtype=torch.int64, device="cuda")
    out = torch.full((3, M.sample_count(900, 23) + 8), SC.SENTINEL, dtype=torch.int16, device="cuda")
    got, m = native.speaker_pcm(ticks, counts, out=out)
    want = M.pcm(t[0])[0]
    assert list(m) == [0, len(want), len(want)]
    got = got.cpu().numpy()
    assert (got[0] == SC.SENTINEL).all()
    for s in (1, 2):
        assert np.array_equal(got[s, :len(want)], want) and (got[s, len(want):] == SC.SENTINEL).all()


def test_refusals_write_nothing(native):
    import torch
    L = native.lib()
    ticks = torch.from_numpy(SC.ticks("random").copy()).cuda()
    counts = _counts_tensor()
    width = M.sample_count(SC.STRIDE, 23)
    out = torch.full((S, width), SC.SENTINEL, dtype=torch.int16, device="cuda")
    err = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    st, null = native.stream_ptr(), C.c_void_p(0)

    def call(n=S, t=_dp(ticks), ts=SC.STRIDE, c=_dp(counts), cs=1, decim=23, order=3, gain=16384, o=_dp(out), os_=width, e=_dp(err)):
        return L.iiv_speaker_pcm(n, t, ts, c, cs, decim, order, gain, o, os_, e, st)
    refused = [call(decim=0), call(decim=74), call(order=0), call(order=5), call(gain=-1), call(gain=32768),
               call(t=null), call(c=null), call(o=null), call(n=-1), call(os_=width - 1),
               call(os_=M.sample_count(SC.STRIDE, 7) - 1, decim=7),
               call(c=C.c_void_p(counts.data_ptr() + 4)), call(o=C.c_void_p(out.data_ptr() + 1))]
    assert refused == [native.ERR_INVALID] * len(refused)
    assert call(n=0) == 0                                      # no streams: succeeds, writes nothing
    torch.cuda.synchronize()
    assert bool((out == SC.SENTINEL).all()) and int(err.item()) == 7
    assert call() == 0 and call(e=null) == 0
    torch.cuda.synchronize()
    assert int(err.item()) == 7                                 # (a clean batch leaves the flag as it was)
    _check_batch(out.cpu().numpy(), "random", 23, 3, 16384, "after the refusals")
    with pytest.raises(ValueError):
        native.speaker_pcm(ticks, counts, decim=74)
    with pytest.raises(ValueError):
        native.speaker_pcm(ticks, counts, out=out[:, :width - 1])


def test_array_audio_previews_its_own_ticks(native):
    """audio.ArrayAudio.speaker_pcm is the kernel on the ticks of ticks()"""
    import audio
    rng = np.random.default_rng(5)
    t = np.arange(6000) / 44100.0
    pcm = np.clip(np.round(9000 * np.sin(2 * np.pi * 440.0 * t) + rng.normal(0, 1500, 6000)), -32768, 32767).astype(np.int16)
    au = audio.ArrayAudio(np.stack([pcm, pcm[::-1]])[:, :, None], 44100, block_frames=2048)
    n = au.tick_count()
    ticks = au.ticks().cpu().numpy()[:, :n]
    got = au.speaker_pcm(decim=64, order=1, gain=20000)
    assert tuple(got.shape) == (2, M.sample_count(n, 64))
    for s in range(2):
        assert np.array_equal(got[s].cpu().numpy(), M.pcm(ticks[s], 64, 1, 20000)[0]), s


def test_on_a_busy_side_stream(native):
    """One call under the probe of tests/stream_probe.py: the ticks and the counts are decoys until the side stream reaches the
    call, the outputs hold a sentinel; the real batch has one bad tick, the decoy none, so the flag must be the real batch's."""
    import torch
    L = native.lib()
    decim, order, gain = 7, 4, 32767
    real = SC.ticks("random").copy()
    real[5, 17] = 9
    decoy = SC.ticks("odd")
    counts_real = np.array(SC.COUNTS, np.int64)
    counts_decoy = np.array(SC.COUNTS[::-1], np.int64)
    width = M.sample_count(SC.STRIDE, decim) + 5
    p = Probe()
    ticks = p.input(real, decoy)
    counts = p.input(counts_real, counts_decoy)
    out = p.output((S, width), torch.int16)
    err = p.output((1,), torch.int32)

    def call(st):
        ok(native, L.iiv_speaker_pcm(S, _dp(ticks), SC.STRIDE, _dp(counts), 1, decim, order, gain, _dp(out), width, _dp(err), st))
    call(native.stream_ptr())
    p.run(call)
    got = out.cpu().numpy()
    assert int(err.item()) == 1
    for s in range(S):
        want, bad = M.pcm(real[s, :SC.COUNTS[s]], decim, order, gain)
        assert bad == (s == 5)
        assert np.array_equal(got[s, :len(want)], want), s
        assert (got[s, len(want):] == SC.SENTINEL).all(), s
