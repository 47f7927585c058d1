"""GPU: an encoder owns its device and pinned memory -- creating one, switching on every lazily built resource, encoding
and closing it leaves nothing behind -- and an option it refuses leaves it as it was."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODE = 1   # DHGR: every lazily built table exists in it


def _free(torch):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def _full_encoder(native, device_tables):
    """A one-stream encoder from dm with every lazily built resource switched on: the split diff-weight table, both forms
    of the joint content choice's tables, both snapshot slots, both live queues."""
    t, s = device_tables.get(MODE, 5)
    enc = native.Encoder(MODE, t, s, 1, dm=device_tables.dm[(MODE, 5)])
    enc.set_diff_weights_mode("split")
    enc.set_content_choice(True)
    enc.set_content_choice("split")
    enc.snapshot(0)
    enc.snapshot(1)
    for slot in (0, 1):
        assert enc.live_queue(slot).shape == (4096,)
    return enc


def _cycle(native, device_tables, fm, fa):
    enc = _full_encoder(native, device_tables)
    ops = enc.encode(fm, fa, [(0, 0, 1, 40), (0, 1, 1, 24)])
    enc.check()
    assert ops.shape == (1, 64, 6)
    enc.close()


def test_encoder_cycles_leave_no_memory_behind(native, device_tables):
    """H = what one encoder holds (free memory before / after creating one).  Sixteen further create / use / close cycles
    must leave less than H behind: less than one encoder's worth in sixteen."""
    import torch
    import stream_batch
    fm, fa = stream_batch.synth_frames_torch(1, 1, True, seed=21)
    device_tables.get(MODE, 5)
    before = _free(torch)
    enc = _full_encoder(native, device_tables)
    held = before - _free(torch)
    enc.close()
    print("one encoder holds %d KiB" % (held >> 10))
    assert held > 0
    _cycle(native, device_tables, fm, fa)
    first = _free(torch)
    for _ in range(16):
        _cycle(native, device_tables, fm, fa)
    last = _free(torch)
    print("free after the first cycle %d KiB, after sixteen more %d KiB: %d KiB left behind" % (first >> 10, last >> 10, (first - last) >> 10))
    assert first - last < held, "%d KiB left behind by sixteen encoders, one holds %d KiB" % ((first - last) >> 10, held >> 10)


def _invalid(native, call):
    with pytest.raises(native.IIVError) as e:
        call()
    assert e.value.code == native.ERR_INVALID


@pytest.mark.parametrize("with_dm", [False, True])
def test_refused_option_leaves_the_encoder_as_it_was(native, device_tables, with_dm):
    """A bad option value -- and, without dm, the options that need the tables built from it -- are refused with
    ERR_INVALID, and the encoder then emits the bytes a fresh one emits."""
    import stream_batch
    fm, fa = stream_batch.synth_frames_torch(1, 1, True, seed=22)
    t, s = device_tables.get(MODE, 5)
    dm = device_tables.dm[(MODE, 5)] if with_dm else None
    segs = [(0, 0, 1, 60), (0, 1, 1, 30)]

    def set_option(enc, option, value):
        native.check(native.lib().iiv_encoder_set_option(enc._h, option, value))

    enc = native.Encoder(MODE, t, s, 1, dm=dm)
    for option in (native.OPT_DIFF_WEIGHTS, native.OPT_GREEDY_KERNEL, native.OPT_CONTENT_CHOICE, native.OPT_FOURTH_OFFSET,
                   native.OPT_STREAM_ORDER):
        _invalid(native, lambda: set_option(enc, option, 99))
    _invalid(native, lambda: set_option(enc, native.OPT_GREEDY_LDS_PAD, -1))
    _invalid(native, lambda: set_option(enc, 99, 0))
    if not with_dm:
        _invalid(native, lambda: enc.set_content_choice(True))
        _invalid(native, lambda: enc.set_content_choice("split"))
        _invalid(native, lambda: enc.set_diff_weights_mode("split"))
    got = enc.encode(fm, fa, segs).cpu().numpy()
    enc.check()
    enc.close()
    fresh = native.Encoder(MODE, t, s, 1, dm=dm)
    exp = fresh.encode(fm, fa, segs).cpu().numpy()
    fresh.check()
    fresh.close()
    assert got.shape == (1, 90, 6) and np.array_equal(got, exp)
