"""What the stream-order tests (tests/test_gpu_stream_order.py, tests/test_gpu_pipeline.py) share besides the probe itself
(tests/stream_probe.py): random memory maps and target frames, an encoder of seeded streams with its oracle twins, the g6
recording's opcode addresses."""
import ctypes as C

import numpy as np

import encode_harness
from encode_harness import next_draws

HGR, DHGR = 0, 1


def g6_addresses(golden):
    """(tick_addr uint16 [1024], ack, terminate) of the g6 recording"""
    g = golden.g6_a2m
    return np.ascontiguousarray(g["tick_addr"], np.uint16).reshape(1024), int(g["special_addr"][0]), int(g["special_addr"][1])


def dp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def maps(rng, n, mode):
    """n random memory maps (screen holes zero; DHGR: bit 7 clear)"""
    m = rng.integers(0, 128 if mode == DHGR else 256, (n, 32, 256), dtype=np.uint8)
    m[..., (np.arange(256) & 127) >= 120] = 0
    return m


def frames(mode, n_streams, nframes, seed):
    """(main, aux) (n_streams, nframes, 32, 256), coherent from frame to frame"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        m = maps(rng, n_streams * nframes, mode).reshape(n_streams, nframes, 32, 256)
        for f in range(1, nframes):
            keep = rng.random((n_streams, 32, 256)) < 0.9
            m[:, f] = np.where(keep, m[:, f - 1], m[:, f])
        out.append(m)
    return out[0], out[1]


class Enc:
    """An encoder of n seeded streams with its oracle twins, and the probe's pieces around it."""

    def __init__(self, native, O, device_tables, oracle_tables, mode, n, seed0, kernel=None, joint=False, fourth=False, lds_pad=0):
        self.native, self.O, self.mode, self.n = native, O, mode, n
        self.seeds = [(seed0 + i, seed0 + 100 + i) for i in range(n)]
        named = {k: v for k, v in (("kernel", kernel), ("joint", joint or None), ("fourth", fourth or None)) if v is not None}
        self.enc = encode_harness.make_encoder(native, device_tables, mode, 5, n, rng=self.seeds, O=O, **named)
        if lds_pad:
            self.enc.set_greedy_lds_pad(lds_pad)
        self.videos = [O.Video(mode, oracle_tables.get(mode, 5), seed_py=a, seed_np=b) for a, b in self.seeds]
        for v in self.videos:
            v.set_joint(joint)
            v.set_fourth_offset(fourth)

    def oracle(self, i, fm, fa, segments):
        """stream i's oracle through `segments` -> (k, 6) opcodes"""
        v, out = self.videos[i], [np.zeros((0, 6), np.uint8)]
        for (f, a, r, k) in segments:
            if r:
                v.encode_frame(fm[i, f], fa[i, f] if self.mode == DHGR else None, a)
            if k:
                out.append(v.next(k))
        return np.concatenate(out)

    def warm(self, call):
        """the call once on the default stream, then everything it did to the encoder undone (slot 1 of the snapshots)"""
        import torch
        self.enc.snapshot(1)
        call(self.native.stream_ptr())
        self.enc.rollback(1)
        torch.cuda.synchronize()

    def check_state(self, counters=True):
        """screen memory and both RNG positions of every stream against its oracle twin: the draw counters (exact positions; not
        where the test itself re-seeded a stream half way) and the next four draws of each generator"""
        for i, v in enumerate(self.videos):
            if counters:
                cnt = self.enc.get_state(self.native.STATE_COUNTERS, i)
                assert (int(cnt[0]), int(cnt[1])) == v.draws(), ("draws", i)
            assert np.array_equal(self.enc.get_state(self.native.STATE_MEM_MAIN, i), v.memory(0)), ("main", i)
            if self.mode == DHGR:
                assert np.array_equal(self.enc.get_state(self.native.STATE_MEM_AUX, i), v.memory(1)), ("aux", i)
            for what, words, high in ((self.native.STATE_RNG_PY, v.rng_py().state_words(), True),
                                      (self.native.STATE_RNG_NP, v.rng_np().state_words(), False)):
                assert next_draws(self.O, self.enc.get_state(what, i), 4, high) == next_draws(self.O, words, 4, high), (what, i)

    def close(self):
        self.enc.close()
