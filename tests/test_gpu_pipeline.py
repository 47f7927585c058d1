"""GPU: the overlapped pipeline, byte-checked.  (a) bench.py's `e2e` arrangement built from the library's own pieces at a small
size -- conversion on an ingest stream, encode, slice emission, a non-blocking copy to pinned memory on a copy stream, the four
events used as the bench uses them -- with a sleep in front of every conversion and every copy, so that a dependency the
library loses shows instead of being won by luck; every step's frames differ.  (b) two encoders on two streams, interleaved
from the host ("Different encoders are independent of each other", include/iivision.h).  Expected bytes: the oracle's."""
import numpy as np
import pytest

from stream_cases import Enc as _Enc, dp as _dp, frames as _frames, g6_addresses
from stream_probe import SLEEP_CYCLES, independent_stream

pytestmark = pytest.mark.gpu

HGR, DHGR = 0, 1


@pytest.fixture(scope="module")
def addresses(golden):
    return g6_addresses(golden)


S, F, STEPS = 3, 2, 6                    # 3 streams, 2 frames per step, the first step and 5 more
PIPELINE_SLEEP = SLEEP_CYCLES // 8       # in front of each of the 6 conversions and 6 copies of a run


@pytest.mark.parametrize("own_stream", [False, True], ids=["encode-on-default-stream", "encode-on-its-own-stream"])
@pytest.mark.parametrize("dither", [32, 256], ids=["ordered", "diffusion"])
@pytest.mark.parametrize("mode", [DHGR, HGR], ids=["DHGR", "HGR"])
def test_e2e_arrangement(native, O, device_tables, oracle_tables, addresses, mode, dither, own_stream):
    import torch
    import stream_batch
    tick, ack, term = addresses
    pal = np.asarray(O.PALETTE_RGB[5], np.uint8)
    rgb = stream_batch.synth_rgb_torch(S, STEPS * F, seed=900 + mode)                      # (S, STEPS F, 192, 280, 3)
    rgb = rgb.view(S, STEPS, F, 192, 280, 3).transpose(0, 1).contiguous()                  # a step's source is contiguous
    rgb_host = rgb.cpu().numpy()
    assert len({rgb_host[k].tobytes() for k in range(STEPS)}) == STEPS
    nb = 2 if mode == DHGR else 1
    bufs = [[torch.zeros((S, F, 32, 256), dtype=torch.uint8, device="cuda") for _ in range(nb)] for _ in range(2)]
    t, s = device_tables.get(mode, 5)
    seeds = [(i + 1, i + 11) for i in range(S)]
    b = stream_batch.StreamBatch(mode, t, s, S, seeds=seeds, dm=device_tables.dm[(mode, 5)])
    ops = torch.zeros((S, 1200, 6), dtype=torch.uint8, device="cuda")
    d_tick = torch.from_numpy(tick.view(np.int16).copy()).cuda()
    width = native.emit_chunk_range(mode, 0, 1200)[1] + 16
    dev = [torch.zeros(S * width, dtype=torch.uint8, device="cuda") for _ in range(2)]
    host = [torch.zeros(S * width, dtype=torch.uint8).pin_memory() for _ in range(2)]
    copy_stream, ingest_stream = independent_stream(), independent_stream()      # (streams the null stream runs beside)
    main = independent_stream() if own_stream else torch.cuda.default_stream()
    done, ready, converted, encoded = ([torch.cuda.Event(), torch.cuda.Event()] for _ in range(4))
    state = {"first_op": 0}
    in_flight, chunks, all_segs = {}, [], []
    torch.cuda.synchronize()

    def ingest(k):
        j = k & 1
        with torch.cuda.stream(ingest_stream):
            ingest_stream.wait_event(encoded[j])
            torch.cuda._sleep(PIPELINE_SLEEP)
            native.frames_to_memory_maps(mode, pal, rgb[k].view(S * F, 192, 280, 3), dither,
                                         out=(bufs[j][0], bufs[j][1] if mode == DHGR else None))
            converted[j].record()

    def harvest(j):
        """the consumer: waits for the copy that last filled host[j] (an event of the copy stream, nothing else)"""
        if j in in_flight:
            nbytes = in_flight.pop(j)
            done[j].synchronize()
            chunks.append(host[j][: S * nbytes].view(S, nbytes).numpy().copy())

    def step(k):
        j = k & 1
        harvest(j)
        main.wait_event(converted[j])
        if k + 1 < STEPS:
            ingest(k + 1)                                             # the next step's frames, beside this step's encode
        view, segs = b.encode_frames(bufs[j][0], bufs[j][1] if mode == DHGR else None, F, ops, loop=True)
        encoded[j].record()
        all_segs.extend(segs)
        n = sum(g[3] for g in segs)
        main.wait_event(done[j])
        nbytes = native.emit_chunk_range(mode, state["first_op"], n)[1]
        o = dev[j][: S * nbytes].view(S, nbytes)
        native.emit_chunk(mode, view, state["first_op"], d_tick, ack, o)
        ready[j].record()
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(ready[j])
            torch.cuda._sleep(PIPELINE_SLEEP)
            host[j][: S * nbytes].copy_(dev[j][: S * nbytes], non_blocking=True)
            done[j].record()
        in_flight[j] = nbytes
        state["first_op"] += n

    with torch.cuda.stream(main):
        for ev in done + encoded:
            ev.record()
        ingest(0)
        for k in range(STEPS):
            step(k)
        harvest(STEPS & 1)
        harvest((STEPS + 1) & 1)
    torch.cuda.synchronize()
    with torch.cuda.stream(main):
        b.enc.check()
    b.close()
    got = np.concatenate(chunks, axis=1)
    total = state["first_op"]
    assert got.shape[1] == sum(native.emit_chunk_range(mode, 0, total)) and total == sum(g[3] for g in all_segs)
    for i in range(S):
        v = O.Video(mode, oracle_tables.get(mode, 5), seed_py=seeds[i][0], seed_np=seeds[i][1])
        exp = []
        for (f, a, r, n) in all_segs:
            if r:
                fm, fa = O.frame_to_memory_map(mode, pal, rgb_host[f // F, i, f % F], dither)
                v.encode_frame(fm, fa, a)
            exp.append(v.next(n))
        whole = O.emit_stream(mode, np.concatenate(exp), np.full(total, 34, np.uint8), tick, ack, term)
        bad = np.nonzero(got[i] != whole[:got.shape[1]])[0]
        assert len(bad) == 0, "stream %d: first wrong byte %d of %d" % (i, bad[0], got.shape[1])


def test_two_encoders_on_two_streams(native, O, device_tables, oracle_tables):
    """a DHGR encoder on the LDS-shared one-wave kernel and an HGR encoder on the eight-wave kernel, each on a non-blocking stream
    of its own, three encode calls each, interleaved from the host with no synchronisation until the end"""
    import ctypes as C
    import torch
    L = native.lib()
    n = 3
    runs = []
    for mode, kernel, seed in ((DHGR, "shared", 81), (HGR, "team", 91)):
        bank = 1 if mode == DHGR else 0
        e = _Enc(native, O, device_tables, oracle_tables, mode, n, seed, kernel=kernel)
        fm, fa = _frames(mode, n, 2, 2000 + mode)
        calls = [[(0, 0, 1, 150)], [(0, bank, 1, 100), (1, 0, 1, 60)], [(1, 0, 0, 45), (1, bank, 1, 80)]]
        runs.append(dict(e=e, mode=mode, fm=fm, fa=fa, calls=calls, stream=independent_stream(),
                         d_main=torch.from_numpy(fm).cuda(), d_aux=torch.from_numpy(fa).cuda() if mode == DHGR else None,
                         segs=[native.segment_array(c) for c in calls],
                         ops=[torch.zeros((n, sum(g[3] for g in c), 6), dtype=torch.uint8, device="cuda") for c in calls]))
    torch.cuda.synchronize()
    for c in range(3):
        for r in runs:
            native.check(L.iiv_encode(r["e"].enc._h, _dp(r["d_main"]), _dp(r["d_aux"]), 2, r["segs"][c], len(r["calls"][c]),
                                      _dp(r["ops"][c]), C.c_void_p(r["stream"].cuda_stream)))
    torch.cuda.synchronize()
    for r in runs:
        e = r["e"]
        e.enc.check()
        flat = [g for c in r["calls"] for g in c]
        got = np.concatenate([o.cpu().numpy() for o in r["ops"]], axis=1)
        for i in range(n):
            assert np.array_equal(got[i], e.oracle(i, r["fm"], r["fa"], flat)), (r["mode"], i)
        e.check_state()
        e.close()
