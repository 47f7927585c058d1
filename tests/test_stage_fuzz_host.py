"""The generator of tests/stage_fuzz.py, without a device: a fuzz that draws the same case every round, or asks the library for
a refusal by accident, proves nothing.  For the committed seed and round counts: every category the stages force occurs, every
drawn case lies inside its entry point's documented preconditions (include/iivision.h), and no audio stream sits on the level
boundaries often enough for check_ticks' 0.5 % allowance to matter."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import a2m_model
import audio_model
import bitmap_model
import colour_cases
import diffusion_model
import ingest_model
import resize_model
import stage_fuzz as F
import yuv_model


def _cases(stage, rounds=None):
    return [F.DRAW[stage](F.stage_rng(F.SEED, r, stage), r) for r in range(rounds or F.ROUNDS[stage])]


@pytest.fixture(scope="module")
def cases():
    return {stage: _cases(stage) for stage in F.STAGES}


def test_round_counts():
    assert F.ROUNDS == {"resize": 12, "ingest": 12, "mono": 12, "render": 12, "a2m": 12, "audio": 12, "chain": 4, "bitmap": 12, "yuv": 12,
                        "direct": 12, "chain_yuv": 4, "colour": 12}
    assert set(F.ROUNDS) == set(F.STAGES) == set(F.DRAW) == set(F.CHECK) == set(F.FUZZ)


# round 0 of every stage that existed before yuv, direct and chain_yuv were appended, as the commit before them drew it: the
# description and every array of the case, sha256.  A stage's generator is seeded by its index in STAGES, so a stage put in
# front of these, or a draw added to a helper they share, would change every committed case without a test noticing.
OLD_ROUND_0 = {
    "resize": "95c8f9cd0b2c86c4",
    "ingest": "6f820248f98c1a4b",
    "mono": "d6bbb82721132994",
    "render": "6abc0449870117a8",
    "a2m": "8dcec69b530656d6",
    "audio": "be48debc581a363e",
    "chain": "1ab8fb20a47e11f3",
    "bitmap": "d9ad8c802bccc95d",
}


def _digest(case):
    h = hashlib.sha256(F.describe(case).encode())
    for k in sorted(case):
        if isinstance(case[k], np.ndarray):
            h.update(k.encode())
            h.update(np.ascontiguousarray(case[k]).tobytes())
    return h.hexdigest()[:16]


def test_the_old_stages_draw_what_they_drew(cases):
    assert F.STAGES[:8] == tuple(OLD_ROUND_0) and [F.STAGE_ID[s] for s in OLD_ROUND_0] == list(range(8))
    assert {s: _digest(cases[s][0]) for s in OLD_ROUND_0} == OLD_ROUND_0


def test_a_case_is_a_function_of_seed_round_and_stage(cases):
    for stage in F.STAGES:
        lines = [F.describe(c) for c in cases[stage]]
        assert lines == [F.describe(c) for c in _cases(stage)], stage
        assert len(set(lines)) == len(lines), stage                                   # no two rounds alike
        other = F.DRAW[stage](F.stage_rng(F.SEED + 1, 0, stage), 0)
        assert F.describe(other) != lines[0], stage
    a, b = F.stage_rng(F.SEED, 3, "resize"), F.stage_rng(F.SEED, 3, "mono")
    assert a.integers(1 << 30) != b.integers(1 << 30)


def test_a_failure_names_seed_round_and_parameters():
    case = F.draw_resize(F.stage_rng(F.SEED, 5, "resize"), 5)
    case["seed"], case["round"] = F.SEED, 5
    with pytest.raises(AssertionError) as e:
        F._same(case, "resize_frames", np.zeros((1, 2)), np.ones((1, 2)))
    msg = str(e.value)
    assert "seed=%d round=5" % F.SEED in msg and "h=%d" % case["params"]["h"] in msg and "--stage resize --round 5" in msg


def test_resize_draws(cases):
    seen = set()
    for c in cases["resize"]:
        p = c["params"]
        n, h, w, H, W = (p[k] for k in ("n", "h", "w", "H", "W"))
        assert 1 <= n <= 5 and 1 <= h <= 8192 and 1 <= w <= 8192 and 1 <= H <= 1024 and 1 <= W <= 1024      # iiv_resize_frames
        assert c["frames"].shape == (n, h, w, 3) and c["frames"].dtype == np.uint8
        big = c["big"]
        if p["view"] is None:
            assert big is c["frames"]
            seen.add("contiguous")
        else:
            f0, step, ro, co = p["view"]
            v = big[f0:f0 + n * step:step, ro:ro + h, co:co + w]
            assert v.shape == c["frames"].shape and np.array_equal(v, c["frames"])      # inside the allocation, rows do not overlap
            assert p["align"] == (v.__array_interface__["data"][0] - big.__array_interface__["data"][0]) % 4
            seen.add("view")
            seen.add("step %d" % step)
            if p["align"]:
                seen.add("misaligned view")
        seen.add(p["content"])
        if H == h and W == w:
            seen.add("copy")
        elif H == h:
            seen.add("horizontal pass only")
        elif W == w:
            seen.add("vertical pass only")
        elif resize_model.vertical_first(h, w):
            seen.add("vertical first")
        else:
            seen.add("horizontal first")
        if (H, W) == (192, 280):
            seen.add("192x280")
    assert seen >= {"contiguous", "view", "step 1", "step 2", "misaligned view", "noise", "checker", "ramp", "copy", "horizontal pass only",
                    "vertical pass only", "vertical first", "horizontal first", "192x280"}, seen
    for first in (0, 8, 16):      # every 8 rounds, wherever they start
        kinds = [(c["params"]["H"] == c["params"]["h"], c["params"]["W"] == c["params"]["w"],
                  resize_model.vertical_first(c["params"]["h"], c["params"]["w"])) for c in _cases("resize", first + 8)[first:]]
        assert (True, False, False) in kinds and (False, True, False) in kinds and any(k[:2] == (True, True) for k in kinds)
        assert any(k[2] for k in kinds)


def test_ingest_draws(cases):
    import frame_grabber
    families = set()
    for c in cases["ingest"]:
        p = c["params"]
        assert p["mode"] in (0, 1) and p["palette"] in ingest_model.NAMES and 1 <= p["n"] <= 70
        assert p["lead_main"] % 8 == 0 and p["lead_aux"] % 8 == 0 and (p["frame_offset"] * F.FRAME_BYTES) % 4 == 0
        assert len(c["idx"]) == p["n"] and set(c["idx"].tolist()) == set(range(len(p["pool"]))) and len(p["pool"]) <= 3
        families.add(c["family"])
        if c["weights"] is None:
            assert 0 <= c["divisor"] <= 255 or c["divisor"] == F.DIFFUSION
        else:
            w = diffusion_model.check_arguments(c["weights"], c["divisor"])        # the contract's refusals, as a ValueError
            assert not w[0, :3].any() and w.sum() <= c["divisor"] <= 64
            if c["family"] == "named":
                assert (tuple(tuple(int(v) for v in r) for r in w), c["divisor"]) in [
                    (tuple(tuple(r) for r in k), d) for k, d in frame_grabber.DIFFUSION_KERNELS.values()]
    assert families == set(F.DITHER_FAMILIES)
    # the random kernels stay inside the contract wherever they are drawn, and do not all look alike
    rng = np.random.default_rng(5)
    drawn = [F._random_kernel(rng) for _ in range(300)]
    for w, d in drawn:
        diffusion_model.check_arguments(w, d)
    assert len(set(drawn)) > 250 and any(sum(w) == d for w, d in drawn) and any(np.count_nonzero(w) >= 6 for w, d in drawn)
    frames = F.ingest_pool_frames([(k, 7) for k in range(7)], "ntsc")
    assert frames.shape == (7, 192, 280, 3) and len({f.tobytes() for f in frames}) == 7
    assert F.HOLES.sum() == 8192 - 192 * 40


def test_mono_draws(cases):
    families, modes = set(), set()
    for c in cases["mono"]:
        p = c["params"]
        assert p["mode"] in (0, 1) and 1 <= p["n"] <= 70 and (0 <= p["dither"] <= 255 or p["dither"] == F.DIFFUSION)
        assert p["lead_main"] % 8 == 0 and p["lead_aux"] % 8 == 0 and len(c["idx"]) == p["n"] and c["idx"].max() < 16
        assert (p["frame_offset"] * 192 * (560 if p["mode"] else 280) * 3) % 4 == 0
        families.add(c["family"])
        modes.add(p["mode"])
    assert families == {"ordered", "fs"} and modes == {0, 1}
    for mode in (0, 1):
        assert F.mono_pool_frames(mode, 3).shape == (16, 192, 560 if mode else 280, 3)


def test_render_draws(cases):
    seen = set()
    for c in cases["render"]:
        p = c["params"]
        assert p["n"] in (1, 2, 3, 5, 17) and p["palette"] in F.RENDER_PALETTES and p["ref_width"] in (280, 560)
        assert p["lead_main"] % 8 == 0 and p["lead_aux"] % 8 == 0 and p["lead_rgb"] % 16 == 0 and p["lead_ref"] % 16 == 0
        assert min(p["lead_main"], p["lead_aux"]) >= 8 and min(p["lead_rgb"], p["lead_ref"]) >= 16 and p["lead_sums"] >= 1
        assert p["ref"] == "noise" or p["ref_width"] == 560
        seen |= {("mode", p["mode"]), p["ref"], p["ref_width"]}
        if p["lead_main"] % 16 == 8 or p["lead_aux"] % 16 == 8:
            seen.add("maps at 8 and no more")
        if p["lead_rgb"] % 32 == 16:
            seen.add("output at 16 and no more")
    assert seen >= {("mode", 0), ("mode", 1), "own", "noise", 280, 560, "maps at 8 and no more", "output at 16 and no more"}, seen


def test_a2m_draws(cases, O):
    seen = set()
    for c in cases["a2m"]:
        p = c["params"]
        S, n, kept, length = p["S"], p["n_ops"], p["kept"], p["length"]
        assert 1 <= S <= 4 and c["ops"].shape == (S, n, 6) and c["ticks"].shape == (S, n)
        assert ((c["ops"][:, :, 0] >= 32) & (c["ops"][:, :, 0] <= 63)).all()                         # iiv_emit_stream's refusals
        assert ((c["ticks"] >= 4) & (c["ticks"] <= 66) & (c["ticks"] % 2 == 0)).all()
        assert p["stride"] >= length >= 2048 and length % 2048 == 0
        assert p["first"] >= 0 and p["every"] >= 1 and 1 <= p["n"] <= 5 and p["first"] + p["n"] * p["every"] < 1 << 62
        # the prefix max_bytes_out keeps and the stream's length, as the oracle's emitter has them
        addr = O.PALETTE_RGB and (0x8000 + 16 * np.arange(1024, dtype=np.uint16), 0xc000, 0xc100)
        want = O.emit_stream(p["mode"], c["ops"][0], c["ticks"][0], addr[0], addr[1], addr[2], p["max_bytes_out"])
        assert len(want) == length and a2m_model.scan(want, *addr) == (a2m_model.OK, p["mode"], kept, 0)
        if p["corrupt"] is not None:
            s, pos, x = p["corrupt"]
            assert 0 <= s < S and 0 <= pos < length and 1 <= x <= 255
            seen.add("corrupted")
            bad = want.copy()
            bad[pos] ^= x
            seen.add(a2m_model.STATUS_NAMES[a2m_model.scan(bad, *addr)[0]])
        seen.add("cut" if kept < n else "whole")
        if p["first"] == kept:
            seen.add("first == n_ops")
        if p["every"] > kept:
            seen.add("every > n_ops")
        if p["stride"] > length:
            seen.add("stride > length")
        if kept > 291:
            seen.add("an ACK")
        seen.add(("init", p["init"]))
        seen.add(p["addresses"])
    assert seen >= {"corrupted", "cut", "whole", "first == n_ops", "every > n_ops", "stride > length", "an ACK", ("init", True),
                    ("init", False), "placeholder", "golden"}, seen
    assert len(seen & set(a2m_model.STATUS_NAMES[1:])) >= 1, seen                                      # a change the scan rejects
    assert [F.a2m_kept(5, m) for m in (None, 1, 7, 8, 14, 15, 35, 36)] == [5, 0, 0, 1, 1, 2, 4, 5]


def test_audio_draws_and_their_boundary_share(cases):
    seen, worst = set(), 0.0
    for c in cases["audio"]:
        p = c["params"]
        assert 1 <= p["S"] <= 4 and p["rate"] in F.AUDIO_RATES and p["block_frames"] in F.AUDIO_BLOCKS
        seen.add("identity" if p["rate"] == audio_model.BITRATE else "resampled")
        for s, (nf, ch, kind, seed, _) in enumerate(p["streams"]):
            assert 1 <= nf <= 40000 and ch in (1, 2) and kind in audio_model.SIGNAL_KINDS
            norm, own = c["norms"][s]
            assert np.isfinite(norm) and norm != 0 and np.isfinite(own) and own != 0                  # iiv_audio_ticks refuses those
            pcm = audio_model.signal(kind, nf, ch, seed)
            assert np.array_equal(pcm, c["pcms"][s])
            want, v = audio_model.ticks(pcm.reshape(-1), ch, p["rate"], norm, block_frames=p["block_frames"])
            assert np.array_equal(want, c["wants"][s][0]) and len(want) == audio_model.tick_count(nf, p["rate"], block_frames=p["block_frames"])
            share = float((np.abs(v - np.round(v)) < 1e-3).sum()) / len(v)
            assert share < 0.0025, (p, s, share)        # half of what check_ticks allows: the model alone, before any device error
            worst = max(worst, share)
            seen.add("few frames" if nf < 100 else "many frames")
            seen.add(ch)
            if nf > p["block_frames"]:
                seen.add("several blocks")
    assert seen >= {"identity", "resampled", "few frames", "many frames", 1, 2, "several blocks"}, seen
    assert worst <= 0.002457, worst                     # the figure tests/stage_fuzz.py's docstring states


def test_chain_draws(cases):
    for c in cases["chain"]:
        p = c["params"]
        assert p["n"] in (2, 3) and c["frames"].shape == (p["n"], p["h"], p["w"], 3) and 1 <= p["h"] <= 400 and 1 <= p["w"] <= 400
        assert p["palette"] in ingest_model.NAMES
        if c["weights"] is not None:
            diffusion_model.check_arguments(c["weights"], c["divisor"])


def test_bitmap_draws(cases):
    seen = set()
    for c in cases["bitmap"]:
        p = c["params"]
        mode, n, k = p["mode"], p["n"], p["queries"]
        assert mode in (0, 1) and p["is_aux"] in ((0, 1) if mode == 1 else (0,)) and 1 <= n <= 6 and 1 <= k <= 64      # HGR has no aux bank
        assert c["screens"].shape == (2, 2, n, 32, 256) and c["screens"].dtype == np.uint8
        assert 0 <= p["which"] < n and 0 <= p["lead_main"] <= 3 and 0 <= p["lead_aux"] <= 3 and p["lead_out"] >= 1
        # include/iivision.h: pages in 0..31 (the host cannot check them); a content's byte is its low 8 bits
        assert c["pages"].shape == c["contents"].shape == c["junk"].shape == (k,) and c["pages"].dtype == np.int32
        assert ((c["pages"] >= 0) & (c["pages"] <= 31)).all() and ((c["contents"] >= 0) & (c["contents"] <= 255)).all()
        assert not (c["junk"] & 0xff).any() and (c["junk"] >= 0).all() and ((c["contents"] | c["junk"]) & 0xff == c["contents"]).all()
        assert c["rows"].shape == (k, 256) and c["rows"].dtype == np.int32 and np.abs(c["rows"]).max() <= F.BITMAP_ROW_RANGE
        seen |= {("mode", mode), ("bank", mode, p["is_aux"]), "n = 1" if n == 1 else "n > 1"}
        if len(set(zip(c["pages"].tolist(), c["contents"].tolist()))) < k:
            seen.add("a duplicate query")
        if (np.diff(c["pages"]) < 0).any():
            seen.add("unsorted pages")
        seen |= {("page", int(v)) for v in c["pages"] if v in (0, 31)}
        for bank in c["screens"].reshape(-1, n, 32, 256):
            assert (bank >= 128).mean() > 0.25 and len({s.tobytes() for s in bank}) == n       # bit 7, every screen different
        if (c["screens"] >= 128).any():
            seen.add(("bit 7", mode))
        if c["junk"].any():
            seen.add("junk above bit 7")
        if p["lead_main"] % 2 or p["lead_aux"] % 2:
            seen.add("an odd first byte")
        if (c["rows"] < 0).any() and (c["rows"] > 65535).any():
            seen.add("rows no table holds")
    assert seen >= {("mode", 0), ("mode", 1), ("bank", 1, 0), ("bank", 1, 1), "n = 1", "n > 1", "a duplicate query", "unsorted pages",
                    ("page", 0), ("page", 31), ("bit 7", 0), ("bit 7", 1), "junk above bit 7", "an odd first byte", "rows no table holds"}, seen
    # the first four rounds alone hold both modes, both DHGR banks, n = 1 and n > 1
    first = [c["params"] for c in cases["bitmap"][:4]]
    assert [(q["mode"], q["is_aux"]) for q in first] == [(0, 0), (1, 0), (0, 0), (1, 1)] and first[0]["n"] == 1 and first[1]["n"] > 1
    assert bitmap_model.HGR == F.HGR and bitmap_model.DHGR == F.DHGR


def test_yuv_draws(cases):
    import test_gpu_yuv
    assert F.YUV_LAYOUTS == tuple(test_gpu_yuv.LAYOUTS) and set(F.YUV_PRESETS) == set(yuv_model.MATRICES)
    seen = set()
    for r, c in enumerate(cases["yuv"]):
        p = c["params"]
        n, h, w, H, W = (p[k] for k in ("n", "h", "w", "H", "W"))
        assert 1 <= n <= 5 and 1 <= h <= 8192 and 1 <= w <= 8192 and 1 <= H <= 1024 and 1 <= W <= 1024      # iiv_resize_frames_yuv420
        y, u, v = c["planes"]
        assert y.shape == (n, h, w) and u.shape == v.shape == (n, (h + 1) // 2, (w + 1) // 2) and {y.dtype, u.dtype, v.dtype} == {np.dtype(np.uint8)}
        assert p["layout"] in F.YUV_LAYOUTS and 0 <= p["fill"] <= 255 and c["forced"] == F.YUV_FORCED[r % 8]
        m = p["matrix"]
        if isinstance(m, str):
            assert m in yuv_model.MATRICES
            seen.add("preset")
        else:
            assert len(m) == 6 and 0 <= m[0] <= 255 and all(-1023 <= k <= 1023 for k in m[1:])            # the header's bounds
            seen.add("at the bounds" if m[0] in (0, 255) and all(abs(k) == 1023 for k in m[1:]) else "inside the bounds")
        tall, unfused = h > 100 * w, W == w or (H != h and h > 100 * w)
        # the path the host code takes, and the forced category really is that path
        kind = ("same size" if (H, W) == (h, w) else "vertical only" if W == w else "horizontal only" if H == h else
                "vertical first" if tall else "two passes")
        seen |= {kind, p["content"], p["layout"], "unfused" if unfused else "fused"}
        if tall:
            seen.add("tall, W == w" if W == w else "tall, W != w")
        if (w + 3) & ~3 > 4096:
            assert h <= 4
            seen.add("one row per workgroup")
        want = {"horizontal only": "horizontal only", "vertical only": "vertical only", "same size": "same size", "tall": "vertical only",
                "tall and the width changes": "vertical first", "two passes": ("two passes", "vertical first")}.get(c["forced"])
        assert want is None or kind == want or kind in want, (c["forced"], kind)
        assert c["forced"] not in ("tall", "tall and the width changes") or tall
        assert c["forced"] != "wide" or ((w + 3) & ~3 > 4096 and W != w)
        if p["content"] == "extremes":
            assert set(np.unique(y)) <= {0, 255} and set(np.unique(u)) <= {0, 255}
        if p["content"] == "checker" and u.shape[2] > 1:
            assert (u[:, :, 1:] != u[:, :, :-1]).all() and (u.astype(int) + v == 255).all()
    assert seen >= {"preset", "at the bounds", "inside the bounds", "same size", "vertical only", "horizontal only", "vertical first", "two passes",
                    "tall, W == w", "tall, W != w", "one row per workgroup", "noise", "extremes", "checker", "fused", "unfused"}, seen
    assert len(seen & set(F.YUV_LAYOUTS)) >= 4 and seen & {"nv12", "nv21", "nv12_rows", "nv12_cut"} and seen & {"i420", "rows", "frames", "cut"}, seen
    assert sum(c["forced"] == "wide" for c in cases["yuv"]) == 1


def test_direct_draws(cases):
    seen = set()
    for c in cases["direct"]:
        p = c["params"]
        assert p["mode"] in (0, 1) and p["width"] in (280, 560) and p["palette"] in ingest_model.NAMES and 1 <= p["n"] <= 70
        assert p["dither"] in F.AMPLITUDES and 0 <= p["dither"] <= 255                                        # no diffusion: refused
        # include/iivision.h f10: d_rgb 4-byte aligned, the maps and d_cost 8-byte aligned -- and here no more than that, sometimes
        assert p["lead_rgb"] % 4 == 0 and p["lead_main"] % 8 == 0 and p["lead_aux"] % 8 == 0 and p["lead_cost"] % 8 == 0
        assert min(p["lead_rgb"], p["lead_main"], p["lead_aux"], p["lead_cost"]) >= 4 and (p["frame_offset"] * 192 * p["width"] * 3) % 4 == 0
        assert len(c["idx"]) == p["n"] and set(c["idx"].tolist()) == set(range(len(p["pool"]))) and len(p["pool"]) <= 3
        assert all(0 <= k < F.DIRECT_KINDS for k, _ in p["pool"])
        seen |= {("mode", p["mode"]), p["width"], ("cost", p["cost"]), "dither 0" if p["dither"] == 0 else "dithered"}
        seen |= {("kind", max(k, 5)) for k, _ in p["pool"]}                  # (5: any of ingest_model.frame_set's)
        if p["dither"] == 0 and p["cost"]:
            seen.add("cost against the screen error")
        if p["lead_rgb"] % 8 == 4:
            seen.add("source at 4 and no more")
        if p["lead_main"] % 16 == 8 or p["lead_aux"] % 16 == 8:
            seen.add("maps at 8 and no more")
        if p["cost"] and p["lead_cost"] % 16 == 8:
            seen.add("cost at 8 and no more")
        if p["frame_offset"]:
            seen.add("a frame offset")
    assert seen >= {("mode", 0), ("mode", 1), 280, 560, ("cost", True), ("cost", False), "dither 0", "dithered", ("kind", 5), ("kind", 6),
                    ("kind", 7), ("kind", 8), "cost against the screen error", "source at 4 and no more", "maps at 8 and no more",
                    "cost at 8 and no more", "a frame offset"}, seen
    # the pool's frames: the right shape at both widths, all different, a flat frame flat, and rows that do tie in the tie frame
    import direct_model
    for width in (280, 560):
        frames = F.direct_pool_frames([(k, 11) for k in range(F.DIRECT_KINDS)], "ntsc", width)
        assert frames.shape == (F.DIRECT_KINDS, 192, width, 3) and len({f.tobytes() for f in frames}) == F.DIRECT_KINDS
        assert (frames[7] == frames[7][0, 0]).all() and (frames[8] == frames[8][:, :1]).all() and len(np.unique(frames[8][:, 0], axis=0)) > 16
    pal = F._palette("pairs")
    tie = F.direct_pool_frames([(8, 5)], "pairs", 280)[0]
    C = direct_model.window_costs(pal, direct_model.target(tie[None], 0)[0, :, :1])            # (192, 1, 16): the first dot of every row
    assert ((C == C.min(axis=-1, keepdims=True)).sum(axis=-1) > 1).mean() > 0.5                # most rows: several windows of least cost


def test_chain_yuv_draws(cases):
    seen = set()
    for c in cases["chain_yuv"]:
        p = c["params"]
        y, u, v = c["planes"]
        assert p["n"] in (2, 3) and y.shape == (p["n"], p["h"], p["w"]) and 1 <= p["h"] <= 400 and 1 <= p["w"] <= 400
        assert u.shape == v.shape == (p["n"], (p["h"] + 1) // 2, (p["w"] + 1) // 2)
        assert p["palette"] in ingest_model.NAMES and p["matrix"] in yuv_model.MATRICES and p["layout"] in F.YUV_LAYOUTS
        assert p["width"] in (280, 560) and 0 <= p["dither"] <= 255
        seen |= {p["width"], (p["width"], p["dither"] == 0)}
    assert seen >= {280, 560, (280, True), (560, True)}, seen


def test_colour_draws(cases):
    seen = set()
    for r, case in enumerate(cases["colour"]):
        p = case["params"]
        assert case["rgb"].shape == (16, 3) and case["rgb"].dtype == np.uint8                       # any 48 bytes are a palette
        assert case["lab1"].shape == case["lab2"].shape == (p["n"], 3) and case["lab1"].dtype == case["lab2"].dtype == np.float64
        assert case["lab1"].flags.c_contiguous and case["lab2"].flags.c_contiguous
        assert p["n"] in F.COUNTS or 100 <= p["n"] <= 700
        # the two conditions of tests/colour_cases.py hold for what was kept, whatever was drawn again
        assert colour_cases.knife_edges_kept(colour_cases.matrix_of(case["rgb"].tobytes())[0]), r
        for a, b in zip(case["lab1"], case["lab2"]):
            assert colour_cases.pair_allowed(tuple(a.tolist()), tuple(b.tolist())), r
        assert p["palette"] == F.COLOUR_KINDS[r % 4] and p["different"] == len(np.unique(case["rgb"], axis=0))
        if p["palette"] == "dark":
            assert case["rgb"].max() <= 27
        if p["palette"] == "greyish":
            assert (case["rgb"].max(axis=1).astype(int) - case["rgb"].min(axis=1) <= 4).all()
        if p["palette"] == "duplicates":
            assert p["different"] < 16
        seen |= {p["palette"], "one workgroup" if p["n"] <= 64 else "several workgroups", "own pairs" if p["own_pairs"] else "no own pairs"}
        if p["n"] % 64:
            seen.add("a last workgroup that is not full")
    assert seen >= set(F.COLOUR_KINDS) | {"one workgroup", "several workgroups", "own pairs", "a last workgroup that is not full"}, seen
    dark = np.concatenate([c["rgb"].reshape(-1) for c in cases["colour"] if c["params"]["palette"] == "dark"])
    assert {10, 11, 23, 24} <= set(dark.tolist())                                                    # both segments' ends, both sides


@pytest.mark.parametrize("stage", ["yuv", "direct", "chain_yuv", "colour"])
def test_the_new_stages_reproduce_one_case_from_the_command_line(stage, monkeypatch):
    """python tests/stage_fuzz.py 1 SEED --stage STAGE --round R and IIV_STAGE_FUZZ_SIDE_STREAM=1 reach the new stages as the old
    ones: main() hands run() that one stage, that one round and the side-stream switch (run() itself needs a device)."""
    calls = []
    monkeypatch.setattr(F, "run", lambda rounds, seed, stages, side, first, log=None: calls.append((rounds, seed, stages, side, first)) or [])
    monkeypatch.setenv("IIV_STAGE_FUZZ_SIDE_STREAM", "1")
    F.main(["1", str(F.SEED), "--stage", stage, "--round", "3"])
    monkeypatch.delenv("IIV_STAGE_FUZZ_SIDE_STREAM")
    F.main(["1", str(F.SEED), "--stage", stage, "--round", "3"])
    assert calls == [(1, F.SEED, [stage], True, 3), (1, F.SEED, [stage], False, 3)]
    case = F.DRAW[stage](F.stage_rng(F.SEED, 3, stage), 3)
    case["seed"], case["round"] = F.SEED, 3
    with pytest.raises(AssertionError, match=r"python tests/stage_fuzz.py 1 %d --stage %s --round 3" % (F.SEED, stage)):
        F._same(case, "a comparison", np.zeros(2), np.ones(2))
    assert F.describe(case) == F.describe(F.DRAW[stage](F.stage_rng(F.SEED, 3, stage), 3))
    # the stand-alone program knows the stage (its own argument parser, in a process of its own, no device touched)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(F.__file__)), "stage_fuzz.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and stage in r.stdout
