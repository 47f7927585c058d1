"""Seeded differential fuzz of the kernels around the encoder against their numpy models: the generator that draws cases for
resize_model, ingest_model / diffusion_model, mono_model, render_model / render_error_model, a2m_model, audio_model,
bitmap_model, yuv_model, direct_model and colour_model (tests/fuzz_parity.py does the same for the encoder against the oracle).

    python tests/stage_fuzz.py [rounds] [seed] [--stage NAME] [--round K]     (on an MI355X; 200 rounds is the long run)

Every stage comes in two halves:
    draw_<stage>(rng, round_index) -> case     pure numpy, no device (tests/test_stage_fuzz_host.py checks the draws themselves)
    check_<stage>(native, case)                runs the kernels through the wrappers of _iiv_native / a2m that the tools use and
                                               compares with the model
and fuzz_<stage>(native, rng, round_index) does both and returns a one-line description of the case.  The generator of stage
`s` in round `r` is np.random.default_rng([seed, r, STAGE_ID[s]]): a case does not depend on which other stages or rounds ran.
A failing assertion names the stage, the seed, the round and the drawn parameters, and the command that runs that one case
again:  python tests/stage_fuzz.py 1 SEED --stage STAGE --round ROUND.

What a stage draws (sizes are the smallest at which each kernel can still go wrong, not the workload's):
    resize   n 1..5 frames, h, w, H, W from the sizes around the tile and clamp edges or uniform 1..400 (192x280 half the time);
             every 8 rounds: H == h, W == w, both, and h > 100 w (the vertical pass first); a contiguous input or a view (row
             offset, column offset -- any alignment mod 4 --, frame step 1 or 2); noise, a 0/255 checkerboard or a steep ramp
    ingest   mode, a palette of ingest_model.NAMES, n frames, a dither family by turns -- an ordered amplitude, Floyd-Steinberg
             through iiv_frames_to_memory_maps, a named kernel or a random legal kernel through .._diffused --, frames of
             ingest_model.frame_set and noise, a view at a frame offset into a larger batch, out= views in guarded buffers.  The
             batch repeats at most three different frames (the models walk the picture pixel by pixel in Python; a frame's
             bytes depend on nothing but the frame): every frame of the batch is compared, the model runs three times at most
    mono     mode, n, ordered amplitude or Floyd-Steinberg, frames of mono_model's sets and noise, a view at a frame offset
    render   mode, palette (NTSC, IIGS, MONO, ingest_model.PALETTES), n in {1, 2, 3, 5, 17}, random screen bytes (bit 7 set in
             DHGR, non-zero holes), every pointer at its least alignment plus a random multiple of it inside a sentinel-filled
             buffer; render_error against noise (560 or 280 wide) or the screen's own rendering (all nine sums zero)
    a2m      S 1..4 streams of n_ops opcodes (around 291 + 292 i, or 1..6000), random opcodes and ticks, max_bytes_out as
             test_emit_kernel_random_sizes_and_cuts draws it: emit == the oracle's bytes; the device bytes at a row stride >=
             the length (junk behind it) to scan, decode and replay with random first / every / n against a2m_model; one round
             in four one byte of one stream is changed.  decode takes any scan's output (the header says so) and runs on every
             stream; the header does not say it of replay, which runs on the streams the model's scan accepts
    audio    S 1..4 streams (n_frames at the small-transform edges or 1..40000, 1 or 2 channels, a signal of
             audio_model.signal), one rate and one block size per call: ticks by audio_model.check_ticks, the resample within
             1e-5 max|y|, the normalisation within 1e-5 relative
    bitmap   mode and bank, n 1..6 all-bit screens as source and as target (bit 7 set in DHGR too), the memory maps 0..3 bytes
             into sentinel-filled buffers, pack / diff_weights / compute_delta_pages into guarded slices through the C ABI;
             1..64 (page, content) queries with duplicates (pages 0 and 31 by turns), contents with junk above bit 7, random
             rows to subtract in [-70000, 70000]; the table is the NTSC one, on the host from the oracle
    chain    2..3 frames of a random source size through resize -> ingest -> render_rgb -> render_error (against the resized
             frames), each stage handed the very tensor the one before returned; every arrow against the models' composition
    yuv      n 1..5 frames of 4:2:0 planes, h, w, H, W as resize draws them; every 8 rounds: same size, each one-pass form,
             h > 100 w with W == w and with W != w (the unfused path, the vertical pass first), w > 4096 with a small h (one
             row per workgroup); one of tests/test_gpu_yuv.py's eight plane layouts with a random fill byte around the planes;
             a preset matrix, a random one inside the argument bounds or one at them; noise, planes of 0 and 255, or a
             one-sample chroma checkerboard: resize_model.resize(yuv_model.to_rgb(...))
    direct   mode, a source width of 280 or 560, a palette of ingest_model.NAMES, an ordered amplitude, n frames over a pool
             of at most three (a frame's bytes depend on that frame alone): ingest_model.frame_set, noise, a flat frame, or a
             frame of flat rows half-way between two palette colours, where many byte rows tie; a view at a frame offset into
             a larger batch; d_rgb 4 bytes, the maps and d_cost 8 bytes off their buffers' alignment, in guarded buffers, through
             the C ABI; d_cost NULL or given: bytes and costs against direct_model, and with dither 0 the cost against
             render_error_model's level 0 of the model's maps
    chain_yuv  2..3 frames of random 4:2:0 planes through resize_frames_yuv420 -> frames_to_memory_maps_direct -> render_rgb ->
             render_error (against the resized frames), each handed the very tensor the one before returned; every arrow
             against the models' composition
    colour   a palette by turns uniform, dark (bytes 0..27: both linear segments' ends), grey-ish (a grey and -2..2 a channel)
             or with k rows repeated, through iiv_cie2000_matrix: floats within colour_model.T of colour_model, ints equal;
             n of COUNTS or 100..700 Lab pairs, uniform over [0, 100] x [-128, 128]^2 mixed with the palette's own, through
             iiv_delta_e_cie2000 within T.  Conditions on the case, as on the committed set of tests/colour_cases.py: no
             delta-E of the palette within 1e-6 of an integer, no pair within 1e-6 degrees of a discontinuity of the formula

check_ticks lets ticks differ within 1e-3 of a level boundary if fewer than 0.5 % of a stream's samples do.  That cap is a
condition on the case: draw_audio draws again (from the same generator, so still a function of the seed) while a stream of
the model alone has 0.25 % or more of its samples that close to a boundary.  The largest share of any stream of the
committed audio cases (SEED, ROUNDS["audio"] rounds) is 0.2457 % (tests/test_stage_fuzz_host.py asserts it stays below 0.25 %).
"""
import argparse
import contextlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "ii-vision_amd", "transcoder"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import a2m_model  # noqa: E402
import audio_model  # noqa: E402
import bitmap_model  # noqa: E402
import colour_cases  # noqa: E402
import colour_model  # noqa: E402
import device_guards  # noqa: E402
import diffusion_model  # noqa: E402
import direct_model  # noqa: E402
import ingest_model  # noqa: E402
import mono_model  # noqa: E402
import render_error_model  # noqa: E402
import render_model  # noqa: E402
import resize_model  # noqa: E402
import yuv_model  # noqa: E402

SEED = 2027
STAGES = ("resize", "ingest", "mono", "render", "a2m", "audio", "chain", "bitmap", "yuv", "direct", "chain_yuv",
          "colour")   # (appended to: the index seeds the stage)
STAGE_ID = {name: i for i, name in enumerate(STAGES)}
# rounds of tests/test_gpu_stage_fuzz.py (the chain, four stages a round, runs 4)
ROUNDS = {"resize": 12, "ingest": 12, "mono": 12, "render": 12, "a2m": 12, "audio": 12, "chain": 4, "bitmap": 12, "yuv": 12, "direct": 12,
          "chain_yuv": 4, "colour": 12}

HGR, DHGR = 0, 1
DIFFUSION = 256
GUARD = 0xA5
GUARD64 = 0x5A5A5A5A5A5A5A5A
EDGE_SIZES = (1, 2, 3, 4, 5, 7, 63, 64, 65, 191, 192, 193, 279, 280, 281)
COUNTS = (1, 2, 3, 31, 32, 33, 64, 65)
AMPLITUDES = (0, 1, 16, 32, 255)
FRAME_BYTES = 192 * 280 * 3
BOUNDARY_SHARE = 0.0025       # the most a stream of the model alone may have within 1e-3 of a level boundary (check_ticks allows 0.5 %)


def stage_rng(seed, round_index, stage):
    return np.random.default_rng([int(seed), int(round_index), STAGE_ID[stage]])


def describe(case):
    return "%s %s" % (case["stage"], " ".join("%s=%s" % kv for kv in case["params"].items()))


def _fail(case, what):
    seed, rnd = case.get("seed", "?"), case.get("round", "?")
    raise AssertionError("stage_fuzz seed=%s round=%s: %s: %s [python tests/stage_fuzz.py 1 %s --stage %s --round %s]"
                         % (seed, rnd, describe(case), what, seed, case["stage"], rnd))


def _require(ok, case, what):
    if not ok:
        _fail(case, what() if callable(what) else what)


def _first_difference(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s, model %s" % (got.shape, want.shape)
    bad = np.argwhere(got != want)
    return "%d values differ, the first at %s: %s, model %s" % (len(bad), tuple(int(v) for v in bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _same(case, what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    _require(got.shape == want.shape and bool((got == want).all()), case, lambda: "%s: %s" % (what, _first_difference(got, want)))


def _sync():
    import torch
    torch.cuda.current_stream().synchronize()


def _guarded(n_bytes, lead, trail):
    return device_guards.guarded(n_bytes, lead, trail, GUARD)


def _guards_kept(case, what, buf, lead, n_bytes):
    _require(device_guards.guards_kept(buf, lead, n_bytes, GUARD), case, "%s: bytes outside the slice were written" % what)


def _palette(name):
    """a palette by the name a case carries: ingest_model's adversarial ones, the two real ones, the mono screen's"""
    if name in ingest_model.PALETTES:
        return ingest_model.PALETTES[name]
    if name.lower() in ("ntsc", "iigs"):
        import oracle
        return oracle.PALETTE_RGB[{"ntsc": 5, "iigs": 0}[name.lower()]]
    if name == "MONO":
        import palette
        return palette.MonoPalette.rgb_array()
    raise ValueError(name)


def _size(rng):
    return int(rng.choice(EDGE_SIZES)) if rng.random() < 0.5 else int(rng.integers(1, 401))


def _count(rng):
    return int(rng.choice(COUNTS)) if rng.random() < 0.5 else int(rng.integers(1, 71))


# ---- resize -----------------------------------------------------------------------------------------------------------

def _content(kind, n, h, w, rng):
    """(n, h, w, 3) uint8: noise, a 0/255 one-pixel checkerboard (both clamps, through the negative lobes) or a steep ramp"""
    f, y, x, c = np.ogrid[0:n, 0:h, 0:w, 0:3]
    if kind == "noise":
        return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if kind == "checker":
        return np.broadcast_to((((x + y + f) & 1) * 255).astype(np.uint8), (n, h, w, 3)).copy()
    return np.clip(((x + 2 * y + f + c) % 8) * 64 - 128, 0, 255).astype(np.uint8)


def draw_resize(rng, round_index=0):
    n = int(rng.integers(1, 6))
    h, w = _size(rng), _size(rng)
    H, W = (192, 280) if rng.random() < 0.5 else (_size(rng), _size(rng))
    force = round_index % 8
    if force == 5:                                    # the vertical pass first: h > 100 w
        w = int(rng.integers(1, 4))
        h = int(rng.integers(100 * w + 1, 401))
        H, W = 192, 280
    while force in (1, 4) and W == w:                 # (one pass means one: the other axis does change)
        W = _size(rng)
    while force in (2, 6) and H == h:
        H = _size(rng)
    if force in (1, 3, 4):
        H = h
    if force in (2, 3, 6):
        W = w
    kind = ("noise", "checker", "ramp")[int(rng.integers(0, 3))]
    frames = _content(kind, n, h, w, rng)
    if rng.random() < 0.3 and force != 7:
        view = None
        big = frames
        align = 0
    else:
        f0, step = int(rng.integers(0, 2)), int(rng.integers(1, 3))
        ro, co, rb, cr = int(rng.integers(0, 6)), int(rng.integers(0, 5)), int(rng.integers(0, 4)), int(rng.integers(0, 5))
        if force == 7:                                # a first byte off the 4-byte grid
            ro, co = next((r_, c_) for r_ in range(ro, ro + 4) for c_ in range(co, co + 4)
                          if (((f0 * (r_ + h + rb) + r_) * (c_ + w + cr) + c_) * 3) % 4)
        big = rng.integers(0, 256, (f0 + n * step, ro + h + rb, co + w + cr, 3), dtype=np.uint8)
        big[f0:f0 + n * step:step, ro:ro + h, co:co + w] = frames
        view = (f0, step, ro, co)
        align = int((((f0 * big.shape[1] + ro) * big.shape[2] + co) * 3) % 4)
    params = dict(n=n, h=h, w=w, H=H, W=W, content=kind, view=view, big=tuple(big.shape[:3]), align=align)
    return dict(stage="resize", params=params, frames=frames, big=big)


def _resize_view(case, dev):
    p = case["params"]
    if p["view"] is None:
        return dev
    f0, step, ro, co = p["view"]
    return dev[f0:f0 + p["n"] * step:step, ro:ro + p["h"], co:co + p["w"]]


def check_resize(native, case):
    import torch
    p = case["params"]
    v = _resize_view(case, torch.from_numpy(case["big"]).cuda())
    _require(tuple(v.shape) == case["frames"].shape, case, "the view has shape %s" % (tuple(v.shape),))
    got = native.resize_frames(v, (p["H"], p["W"]))
    _sync()
    _same(case, "resize_frames", got.cpu().numpy(), resize_model.resize(case["frames"], (p["H"], p["W"])))


# ---- colour ingest ----------------------------------------------------------------------------------------------------

DITHER_FAMILIES = ("ordered", "fs", "named", "random")


def _random_kernel(rng):
    """15 weights and a divisor inside iiv_frames_to_memory_maps_diffused's contract: divisor 1..64, weights[0..2] (the pixel
    itself and what lies left of it on its row) zero, every weight 0..255, their sum at most the divisor"""
    divisor = int(rng.integers(1, 65))
    total = int(rng.integers(0, divisor + 1))
    w = np.zeros(15, dtype=np.int64)
    w[3:] = rng.multinomial(total, rng.dirichlet(np.full(12, 0.5)))
    return tuple(int(v) for v in w), divisor


def _draw_dither(rng, family):
    """-> (what the case prints, weights | None, divisor | amplitude)"""
    if family == "ordered":
        a = int(rng.choice(AMPLITUDES))
        return "ordered:%d" % a, None, a
    if family == "fs":
        return "diffusion", None, DIFFUSION
    if family == "named":
        import frame_grabber
        name = sorted(frame_grabber.DIFFUSION_KERNELS)[int(rng.integers(0, len(frame_grabber.DIFFUSION_KERNELS)))]
        w, d = frame_grabber.DIFFUSION_KERNELS[name]
        return name, tuple(int(v) for row in w for v in row), int(d)
    w, d = _random_kernel(rng)
    return "kernel:%s/%d" % (",".join(str(v) for v in w), d), w, d


def _draw_pool(rng, n, most=3, kinds=7):
    """the different frames of a batch, as (kind 0..5 of ingest_model.frame_set | 6 = more noise, seed), and which one each of
    the n frames is (every one of the pool occurs)"""
    k = min(n, int(rng.integers(1, most + 1)))
    pool = [(int(rng.integers(0, kinds)), int(rng.integers(1 << 30))) for _ in range(k)]
    idx = rng.integers(0, k, n)
    idx[rng.permutation(n)[:k]] = np.arange(k)
    return pool, idx


def ingest_pool_frames(pool, palette_name):
    out = np.empty((len(pool), 192, 280, 3), np.uint8)
    for i, (kind, seed) in enumerate(pool):
        if kind == 6:
            out[i] = np.random.default_rng([seed, 6]).integers(0, 256, (192, 280, 3))
        else:
            out[i] = ingest_model.frame_set(_palette(palette_name), seed)[kind]
    return out


def draw_ingest(rng, round_index=0):
    mode = int(rng.integers(0, 2))
    pal = ingest_model.NAMES[int(rng.integers(0, len(ingest_model.NAMES)))]
    n = _count(rng)
    family = DITHER_FAMILIES[round_index % 4]
    name, weights, divisor = _draw_dither(rng, family)
    pool, idx = _draw_pool(rng, n)
    params = dict(mode=mode, palette=pal, n=n, dither=name, frame_offset=int(rng.integers(0, 4)), tail=int(rng.integers(0, 3)),
                  lead_main=8 * int(rng.integers(0, 5)), lead_aux=8 * int(rng.integers(0, 5)), pool=pool,
                  junk=int(rng.integers(1 << 30)))
    return dict(stage="ingest", params=params, family=family, weights=weights, divisor=divisor, idx=idx)


def _ingest_device(native, case, mode, pal, src, out):
    if case["weights"] is None:
        return native.frames_to_memory_maps(mode, pal, src, case["divisor"], out=out)
    return native.frames_to_memory_maps_diffused(mode, pal, src, np.array(case["weights"]).reshape(3, 5), case["divisor"], out=out)


def _ingest_model(case, mode, pal, frames):
    if case["weights"] is None:
        return ingest_model.frames_to_memory_maps(mode, pal, frames, case["divisor"])
    return diffusion_model.frames_to_memory_maps(mode, pal, frames, case["weights"], case["divisor"])


HOLES = np.ones(8192, dtype=bool)
for _y in range(192):
    HOLES[ingest_model.y_to_offset(_y):ingest_model.y_to_offset(_y) + 40] = False


def _offset_batch(frames, frame_offset, tail, junk_seed):
    """the frames as a view `frame_offset` frames into a larger batch of junk on the device"""
    import torch
    n = len(frames)
    big = np.random.default_rng(junk_seed).integers(0, 256, (frame_offset + n + tail,) + frames.shape[1:], dtype=np.uint8)
    big[frame_offset:frame_offset + n] = frames
    return torch.from_numpy(big).cuda()[frame_offset:frame_offset + n]


def _check_maps(case, what, mode, n, bufs, leads, want):
    for bank, (buf, view), lead, exp in zip(("main", "aux"), bufs, leads, want):
        if exp is None:
            _require(bool((buf.cpu().numpy() == GUARD).all()), case, "%s: HGR wrote into the aux buffer" % what)
            continue
        got = view.cpu().numpy().reshape(n, 32, 256)
        _same(case, "%s %s" % (what, bank), got, exp)
        _require(not got.reshape(n, 8192)[:, HOLES].any(), case, "%s %s: a screen hole is not zero" % (what, bank))
        _guards_kept(case, "%s %s" % (what, bank), buf, lead, n * 8192)


def check_ingest(native, case):
    p = case["params"]
    mode, n, pal = p["mode"], p["n"], _palette(p["palette"])
    pool = ingest_pool_frames(p["pool"], p["palette"])
    src = _offset_batch(pool[case["idx"]], p["frame_offset"], p["tail"], p["junk"])
    bufs = [_guarded(n * 8192, p["lead_main"], 40), _guarded(n * 8192, p["lead_aux"], 40)]
    main, aux = _ingest_device(native, case, mode, pal, src, (bufs[0][1], bufs[1][1]))
    _sync()
    _require(main.data_ptr() == bufs[0][1].data_ptr() and (aux is None) == (mode == HGR), case, "the out= tensors were not used")
    m, a = _ingest_model(case, mode, pal, pool)
    _check_maps(case, "ingest", mode, n, bufs, (p["lead_main"], p["lead_aux"]), (m[case["idx"]], a[case["idx"]] if a is not None else None))


# ---- mono ingest ------------------------------------------------------------------------------------------------------

def mono_pool_frames(mode, seed):
    """sixteen frames: four of mono_model's structured ones, its nine corner frames, three of noise"""
    return np.concatenate([mono_model.structured_frames(mode, 4, seed), mono_model.corner_frames(mode), mono_model.noise_frames(mode, 3, seed + 1)])


def draw_mono(rng, round_index=0):
    mode = int(rng.integers(0, 2))
    n = _count(rng)
    family = ("fs", "ordered", ("ordered", "fs")[int(rng.integers(0, 2))])[round_index % 3]
    dither = DIFFUSION if family == "fs" else int(rng.choice(AMPLITUDES))
    params = dict(mode=mode, n=n, dither=dither, frame_offset=int(rng.integers(0, 4)), tail=int(rng.integers(0, 3)),
                  lead_main=8 * int(rng.integers(0, 5)), lead_aux=8 * int(rng.integers(0, 5)), frames_seed=int(rng.integers(1 << 30)),
                  junk=int(rng.integers(1 << 30)))
    return dict(stage="mono", params=params, family=family, idx=rng.integers(0, 16, n))


def check_mono(native, case):
    p = case["params"]
    mode, n = p["mode"], p["n"]
    pool = mono_pool_frames(mode, p["frames_seed"])
    used, inverse = np.unique(case["idx"], return_inverse=True)
    src = _offset_batch(pool[case["idx"]], p["frame_offset"], p["tail"], p["junk"])
    bufs = [_guarded(n * 8192, p["lead_main"], 40), _guarded(n * 8192, p["lead_aux"], 40)]
    native.frames_to_memory_maps_mono(mode, src, p["dither"], out=(bufs[0][1], bufs[1][1]))
    _sync()
    m, a = mono_model.frames_to_memory_maps(mode, pool[used], p["dither"])
    _check_maps(case, "mono ingest", mode, n, bufs, (p["lead_main"], p["lead_aux"]), (m[inverse], a[inverse] if a is not None else None))


# ---- render and render_error ------------------------------------------------------------------------------------------

RENDER_PALETTES = ("NTSC", "IIGS", "MONO") + tuple(ingest_model.PALETTES)
RENDER_FRAME = 192 * 560 * 3


def _lead(rng, alignment):
    """the contract's least alignment plus a random multiple of it"""
    return alignment * (1 + int(rng.integers(0, 8)))


def draw_render(rng, round_index=0):
    mode = int(rng.integers(0, 2))
    pal = RENDER_PALETTES[int(rng.integers(0, len(RENDER_PALETTES)))]
    n = int(rng.choice((1, 2, 3, 5, 17)))
    own = round_index % 3 == 0 or rng.random() < 0.2
    ref_width = 560 if own or rng.random() < 0.5 else 280       # (only a 560-wide reference can be the screen's own rendering)
    params = dict(mode=mode, palette=pal, n=n, ref="own" if own else "noise", ref_width=ref_width, lead_main=_lead(rng, 8),
                  lead_aux=_lead(rng, 8), lead_rgb=_lead(rng, 16), lead_ref=_lead(rng, 16), lead_sums=1 + int(rng.integers(0, 8)),
                  seed=int(rng.integers(1 << 30)))
    return dict(stage="render", params=params)


def check_render(native, case):
    import torch
    p = case["params"]
    mode, n, pal = p["mode"], p["n"], _palette(p["palette"])
    rng = np.random.default_rng(p["seed"])
    main, aux = rng.integers(0, 256, (n, 32, 256), dtype=np.uint8), rng.integers(0, 256, (n, 32, 256), dtype=np.uint8)
    mbuf, mview = _guarded(n * 8192, p["lead_main"], 8)
    abuf, aview = _guarded(n * 8192, p["lead_aux"], 8)
    mview.copy_(torch.from_numpy(main).reshape(-1))
    aview.copy_(torch.from_numpy(aux).reshape(-1))
    obuf, oview = _guarded(n * RENDER_FRAME, p["lead_rgb"], 64)
    dev_aux = aview if mode == DHGR else None
    got = native.render_rgb(mode, pal, mview, dev_aux, out=oview)
    _sync()
    want = render_model.render_rgb(mode, main, aux if mode == DHGR else None, pal)
    _same(case, "render_rgb", got.cpu().numpy(), want)
    _guards_kept(case, "render_rgb", obuf, p["lead_rgb"], n * RENDER_FRAME)
    ref = want if p["ref"] == "own" else rng.integers(0, 256, (n, 192, p["ref_width"], 3), dtype=np.uint8)
    rbuf, rview = _guarded(ref.size, p["lead_ref"], 16)
    rview.copy_(torch.from_numpy(np.ascontiguousarray(ref)).reshape(-1))
    sbuf = torch.full((p["lead_sums"] + 9 * n + 3,), GUARD64, dtype=torch.int64, device="cuda")
    sview = sbuf[p["lead_sums"]:p["lead_sums"] + 9 * n]
    sums = native.render_error(mode, pal, mview, dev_aux, rview.view(ref.shape), out=sview)
    _sync()
    want_sums = render_error_model.render_error(mode, main, aux if mode == DHGR else None, pal, ref)
    _same(case, "render_error", sums.cpu().numpy().view(np.uint64).reshape(n, 3, 3), want_sums)
    if p["ref"] == "own":
        _require(not sview.cpu().numpy().any(), case, "render_error against the screen's own rendering is not zero")
    whole = sbuf.cpu().numpy()
    _require((whole[:p["lead_sums"]] == GUARD64).all() and (whole[p["lead_sums"] + 9 * n:] == GUARD64).all(), case,
             "render_error: sums outside the slice were written")
    _same(case, "the main bank after the calls", mview.cpu().numpy(), main.reshape(-1))
    _same(case, "the aux bank after the calls", aview.cpu().numpy(), aux.reshape(-1))
    _guards_kept(case, "the reference", rbuf, p["lead_ref"], ref.size)


# ---- emit -> scan -> decode -> replay -----------------------------------------------------------------------------------

A2M_COUNTS = (0, 1, 2, 290, 291, 292, 293, 582, 583, 584)
FAR = 1 << 40


def a2m_kept(n_ops, max_bytes_out):
    """opcodes Movie.emit_stream writes before max_bytes_out stops it (movie.py:132-134): opcode k goes out while the stream
    is shorter than the limit, and it begins at a2m_model.P(k)"""
    if not max_bytes_out:
        return n_ops
    k = 0
    while k < n_ops and a2m_model.P(k) < max_bytes_out:
        k += 1
    return k


def a2m_length(kept):
    return ((a2m_model.P(kept) + 2) // 2048 + 1) * 2048


def draw_a2m(rng, round_index=0):
    force = round_index % 4
    mode = int(rng.integers(0, 2))
    S = int(rng.integers(1, 5))
    n = int(rng.choice(A2M_COUNTS)) if rng.random() < 0.5 else int(rng.integers(1, 6001))
    if force == 0 and n < 2:
        n = int(rng.integers(2, 6001))
    ops = rng.integers(0, 256, (S, n, 6), dtype=np.uint8)
    ops[:, :, 0] = rng.integers(32, 64, (S, n))
    ticks = (rng.integers(2, 34, (S, n)) * 2).astype(np.uint8)
    mx = None if rng.random() < 0.5 else int(rng.choice([1, 7, 8, 14, 2043, 2044, 2048, 2049, int(rng.integers(1, 7 * n + 64))]))
    if force == 0:                                    # a cut stream: opcode n - 1 begins at 7 n or later
        mx = int(rng.integers(1, 7 * n + 1))
    kept = a2m_kept(n, mx)
    length = a2m_length(kept)
    extra = int(rng.choice([0, 1, 7, 2048, int(rng.integers(0, 5000))]))
    corrupt = None
    if force == 3 or rng.random() < 0.1:
        acks = a2m_model._acks_before(kept)
        where = [int(rng.integers(0, length)), int(rng.integers(0, 7)), a2m_model.P(kept) + int(rng.integers(0, 2))]
        if kept:
            where.append(a2m_model.P(int(rng.integers(0, kept))) + int(rng.integers(0, 2)))
        if acks:
            where.append(acks[int(rng.integers(0, len(acks)))] + int(rng.integers(0, 4)))
        if a2m_model.P(kept) + 2 < length:
            where.append(int(rng.integers(a2m_model.P(kept) + 2, length)))
        corrupt = (int(rng.integers(0, S)), where[int(rng.integers(0, len(where)))], int(rng.integers(1, 256)))
    first = int(rng.choice([0, kept, int(rng.integers(0, kept + 4)), FAR]))
    every = int(rng.choice([1, int(rng.integers(1, kept + 3)), 2 * kept + 7, FAR]))
    if force == 1:
        first = kept                                  # first == n_ops
    if force == 2:
        every = 2 * kept + 7                          # every larger than the stream
    params = dict(mode=mode, S=S, n_ops=n, max_bytes_out=mx, kept=kept, length=length, stride=length + extra, corrupt=corrupt,
                  first=first, every=every, n=int(rng.integers(1, 6)), init=bool(rng.random() < 0.5),
                  addresses=("placeholder", "golden")[int(rng.integers(0, 2))], seed=int(rng.integers(1 << 30)))
    return dict(stage="a2m", params=params, ops=ops, ticks=ticks)


def _addresses(kind):
    import a2m
    if kind == "placeholder":
        return a2m.OpcodeAddresses.placeholder()
    g = np.load(os.path.join(ROOT, "tests", "golden", "g6_a2m.npz"))
    return a2m.OpcodeAddresses(g["tick_addr"], g["special_addr"][0], g["special_addr"][1], g["special_addr"][2])


def check_a2m(native, case):
    import torch
    import a2m
    import oracle as O
    p = case["params"]
    mode, S, kept, length, stride = p["mode"], p["S"], p["kept"], p["length"], p["stride"]
    addr = _addresses(p["addresses"])
    margs = (addr.tick, addr.ack, addr.terminate)
    rng = np.random.default_rng(p["seed"])
    emitted = a2m.emit_stream(mode, torch.from_numpy(case["ops"]).cuda(), torch.from_numpy(case["ticks"]).cuda(), addr, p["max_bytes_out"])
    _sync()
    host = [O.emit_stream(mode, case["ops"][s], case["ticks"][s], addr.tick, addr.ack, addr.terminate, p["max_bytes_out"]) for s in range(S)]
    _require(tuple(emitted.shape) == (S, length) and all(len(h) == length for h in host), case,
             lambda: "emit_stream: %s bytes, the oracle %s, expected %d" % (tuple(emitted.shape), [len(h) for h in host], length))
    _same(case, "emit_stream", emitted.cpu().numpy(), np.stack(host))
    # the device's bytes, junk behind them, to the reader
    data = torch.from_numpy(rng.integers(0, 256, (S, stride), dtype=np.uint8)).cuda()
    data[:, :length] = emitted
    if p["corrupt"] is not None:
        c, pos, x = p["corrupt"]
        data[c, pos] = data[c, pos] ^ x
        host[c][pos] ^= x
    lengths = [length] * S
    reader = a2m.A2mReader(addr)
    try:
        info = reader.scan(data, lengths)
        model = [a2m_model.scan(h, *margs) for h in host]
        _same(case, "scan {status, mode, n_ops, position}", info, np.array(model, dtype=np.int64))
        for s in range(S):
            if p["corrupt"] is None or p["corrupt"][0] != s:
                _require(model[s] == (a2m_model.OK, mode, kept, 0), case, "the model's scan of untouched stream %d is %s" % (s, model[s]))
        decoded = reader.decode(data, lengths, strict=False)
        _sync()
        for s, (d_mode, d_ops, d_ticks, d_banks) in enumerate(decoded):
            m_mode, m_ops, m_ticks, m_banks = a2m_model.decode(host[s], *margs)
            _require(d_mode == m_mode, case, "decode: mode of stream %d" % s)
            _same(case, "decode: opcodes of stream %d" % s, d_ops.cpu().numpy(), m_ops)
            _same(case, "decode: ticks of stream %d" % s, d_ticks.cpu().numpy(), m_ticks)
            _same(case, "decode: banks of stream %d" % s, d_banks.cpu().numpy(), m_banks)
            if p["corrupt"] is None or p["corrupt"][0] != s:    # what was emitted, or the prefix the cut kept
                _same(case, "decoded opcodes against the emitted ones, stream %d" % s, m_ops, case["ops"][s, :kept])
                _same(case, "decoded ticks against the emitted ones, stream %d" % s, m_ticks, case["ticks"][s, :kept])
        good = [s for s in range(S) if model[s][0] == a2m_model.OK]
        if good:
            init = rng.integers(0, 256, (2, S, 32, 256), dtype=np.uint8) if p["init"] else None
            sub = data[good] if len(good) < S else data
            dev_init = tuple(torch.from_numpy(np.ascontiguousarray(init[b][good])).cuda() for b in (0, 1)) if init is not None else None
            main, aux = reader.replay(sub, first=p["first"], every=p["every"], n=p["n"], init=dev_init, lengths=[length] * len(good))
            _sync()
            main, aux = main.cpu().numpy(), aux.cpu().numpy()
            for i, s in enumerate(good):
                m_main, m_aux = a2m_model.replay(host[s], *margs, first=p["first"], every=p["every"], n=p["n"],
                                                 init=(init[0, s], init[1, s]) if init is not None else None)
                _same(case, "replay: main of stream %d" % s, main[i], m_main)
                _same(case, "replay: aux of stream %d" % s, aux[i], m_aux)
    finally:
        reader.close()


# ---- audio ------------------------------------------------------------------------------------------------------------

AUDIO_FRAMES = (1, 2, 3, 97, 2047, 2048, 2049)
AUDIO_RATES = (8000, 11025, 14700, 22050, 44100, 48000)
AUDIO_BLOCKS = (1024, 2048, 3001, 4096)


def boundary_share(v):
    """the share of the model's own a * 16 within 1e-3 of an integer: where check_ticks lets a tick differ by a level"""
    v = np.asarray(v)
    return float((np.abs(v - np.round(v)) < 1e-3).sum()) / max(len(v), 1)


def draw_audio(rng, round_index=0):
    redraws = 0
    while True:
        S = int(rng.integers(1, 5))
        rate = 14700 if round_index % 4 == 3 else int(rng.choice(AUDIO_RATES))
        block = int(rng.choice(AUDIO_BLOCKS))
        streams, pcms, norms, wants, shares = [], [], [], [], []
        for s in range(S):
            nf = int(rng.choice(AUDIO_FRAMES)) if rng.random() < 0.5 else int(rng.integers(1, 40001))
            ch = int(rng.integers(1, 3))
            kind = audio_model.SIGNAL_KINDS[int(rng.integers(0, len(audio_model.SIGNAL_KINDS)))]
            seed = int(rng.integers(1 << 30))
            pcm = audio_model.signal(kind, nf, ch, seed)
            own = audio_model.normalization(pcm.reshape(-1), ch, rate) if pcm.any() else np.inf
            # the clip's own normalisation, or any other: a stream of a few samples normalises its largest one onto a level
            norm = float(own) if nf >= 200 and np.isfinite(own) and rng.random() < 0.5 else float(rng.uniform(0.5, 4.0))
            want, v = audio_model.ticks(pcm.reshape(-1), ch, rate, norm, block_frames=block)
            streams.append((nf, ch, kind, seed, round(norm, 6)))
            pcms.append(pcm)
            norms.append((norm, float(own)))
            wants.append((want, v))
            shares.append(boundary_share(v))
        if max(shares) < BOUNDARY_SHARE and all(np.isfinite(o) for _, o in norms):
            break
        redraws += 1
    params = dict(S=S, rate=rate, block_frames=block, streams=streams, pad=int(rng.integers(0, 100)), redraws=redraws,
                  junk=int(rng.integers(1 << 30)))
    return dict(stage="audio", params=params, pcms=pcms, norms=norms, wants=wants, shares=shares)


def check_audio(native, case):
    import torch
    p = case["params"]
    S, rate, block = p["S"], p["rate"], p["block_frames"]
    pcms = case["pcms"]
    width = max(q.size for q in pcms) + p["pad"]
    host = np.random.default_rng(p["junk"]).integers(-32768, 32768, (S, width)).astype(np.int16)   # (junk behind every stream's frames)
    for s, q in enumerate(pcms):
        host[s, :q.size] = q.reshape(-1)
    pcm = torch.from_numpy(host).cuda()
    nf, ch = [q.shape[0] for q in pcms], [q.shape[1] for q in pcms]
    norms = [n for n, _ in case["norms"]]
    counts = [audio_model.tick_count(n, rate, block_frames=block) for n in nf]
    out = torch.full((S, max(counts) + 64), 0xAB, dtype=torch.uint8, device="cuda")
    t, got_counts = native.audio_ticks(pcm, nf, ch, rate, norms, block_frames=block, out=out)
    _sync()
    _require(t is out and list(got_counts) == counts, case, lambda: "audio_ticks: counts %s, model %s" % (list(got_counts), counts))
    ticks = out.cpu().numpy()
    for s in range(S):
        want, v = case["wants"][s]
        _require(len(want) == counts[s], case, "the model's tick count of stream %d" % s)
        try:
            audio_model.check_ticks(ticks[s, :counts[s]], want, v)
        except AssertionError as e:
            _fail(case, "audio_ticks stream %d: %s" % (s, e))
        _require((ticks[s, counts[s]:] == 0xAB).all(), case, "audio_ticks stream %d: bytes past the tick count were written" % s)
        _require(set(np.unique(ticks[s, :counts[s]])) <= set(range(4, 67, 2)), case, "audio_ticks stream %d: a tick outside 4..66" % s)
    y, lens = native.audio_resample(pcm, nf, ch, rate)
    _sync()
    y = y.cpu().numpy()
    for s, q in enumerate(pcms):
        want = audio_model.decode(q.reshape(-1), q.shape[1], rate)
        _require(lens[s] == len(want) == audio_model.n_out(q.shape[0], rate), case, "audio_resample stream %d: length %d, model %d" % (s, lens[s], len(want)))
        err = np.abs(y[s, :lens[s]] - want).max()
        _require(err <= 1e-5 * np.abs(want).max(), case, "audio_resample stream %d: max error %g of max |y| %g" % (s, err, np.abs(want).max()))
    got = native.audio_normalization(pcm, nf, ch, rate)
    for s in range(S):
        want = case["norms"][s][1]
        _require(abs(got[s] - want) <= 1e-5 * abs(want), case, "audio_normalization stream %d: %r, model %r" % (s, got[s], want))


# ---- the chain --------------------------------------------------------------------------------------------------------

def draw_chain(rng, round_index=0):
    mode = int(rng.integers(0, 2))
    pal = ingest_model.NAMES[int(rng.integers(0, len(ingest_model.NAMES)))]
    n = int(rng.integers(2, 4))
    h, w = _size(rng), _size(rng)
    kind = ("noise", "checker", "ramp")[int(rng.integers(0, 3))]
    family = DITHER_FAMILIES[int(rng.integers(0, 4))]
    name, weights, divisor = _draw_dither(rng, family)
    frames = _content(kind, n, h, w, rng)
    if kind != "noise":                               # (a pattern alone resizes to little more than grey: some colour under it)
        frames = (frames // 2 + rng.integers(0, 128, (n, 1, 1, 3)).astype(np.uint8)).astype(np.uint8)
    params = dict(mode=mode, palette=pal, n=n, h=h, w=w, content=kind, dither=name)
    return dict(stage="chain", params=params, family=family, weights=weights, divisor=divisor, frames=frames)


def check_chain(native, case):
    import torch
    p = case["params"]
    mode, n, pal = p["mode"], p["n"], _palette(p["palette"])
    small = native.resize_frames(torch.from_numpy(case["frames"]).cuda())
    main, aux = _ingest_device(native, case, mode, pal, small, None)          # each stage takes the tensor the last one returned
    rgb = native.render_rgb(mode, pal, main, aux)
    sums = native.render_error(mode, pal, main, aux, small)
    _sync()
    m_small = resize_model.resize(case["frames"], (192, 280))
    _same(case, "chain: resize", small.cpu().numpy(), m_small)
    m_main, m_aux = _ingest_model(case, mode, pal, m_small)
    _same(case, "chain: ingest main", main.cpu().numpy(), m_main)
    _require((aux is None) == (m_aux is None), case, "chain: ingest aux")
    if aux is not None:
        _same(case, "chain: ingest aux", aux.cpu().numpy(), m_aux)
    m_rgb = render_model.render_rgb(mode, m_main, m_aux, pal)
    _same(case, "chain: render_rgb", rgb.cpu().numpy(), m_rgb)
    _same(case, "chain: render_error", sums.cpu().numpy().view(np.uint64).reshape(n, 3, 3),
          render_error_model.error_sums_of_screens(m_rgb, m_small))


# ---- the stand-alone Bitmap kernels ----------------------------------------------------------------------------------------

BITMAP_ROW_RANGE = 70000
_ntsc_tables = {}


def ntsc_table(mode):
    """the NTSC edit-distance table on the host, from the oracle (tests/test_gpu_tables.py holds the device's to it entry by
    entry); the device's own copy is built from the same matrix"""
    if mode not in _ntsc_tables:
        import oracle
        oracle.build()
        _ntsc_tables[mode] = oracle.build_table(mode, oracle.cie2000_matrix(oracle.PALETTE_RGB[5])[1], symmetric=True)
    return _ntsc_tables[mode]


def draw_bitmap(rng, round_index=0):
    mode = (round_index + int(rng.integers(0, 2)) * (round_index >= 4)) % 2            # rounds 0..3: HGR, DHGR, HGR, DHGR
    is_aux = 0 if mode == HGR else (round_index // 2 + (int(rng.integers(0, 2)) if round_index >= 4 else 0)) % 2
    n = 1 if round_index % 4 == 0 else int(rng.integers(2, 7)) if round_index % 4 == 1 else int(rng.integers(1, 7))
    screens = rng.integers(0, 256, (2, 2, n, 32, 256), dtype=np.uint8)                  # [source | target][main | aux]
    k = int(rng.integers(1, 65))
    pages = rng.integers(0, 32, k).astype(np.int32)
    pages[int(rng.integers(0, k))] = (0, 31)[round_index % 2]
    contents = rng.integers(0, 256, k).astype(np.int32)
    if k > 1:                                                                           # a duplicate query, elsewhere in the list
        a, b = rng.permutation(k)[:2]
        pages[a], contents[a] = pages[b], contents[b]
    junk = rng.integers(0, 1 << 23, k).astype(np.int32) << 8                            # bits 8..30 of a content: ignored
    rows = rng.integers(-BITMAP_ROW_RANGE, BITMAP_ROW_RANGE + 1, (k, 256)).astype(np.int32)
    params = dict(mode=mode, is_aux=is_aux, n=n, queries=k, which=int(rng.integers(0, n)), lead_main=int(rng.integers(0, 4)),
                  lead_aux=int(rng.integers(0, 4)), lead_out=1 + int(rng.integers(0, 8)))
    return dict(stage="bitmap", params=params, screens=screens, pages=pages, contents=contents, junk=junk, rows=rows)


def _words(n, dtype, lead, trail=5):
    import torch
    fill = GUARD64 if dtype == torch.int64 else GUARD64 & 0xffffffff
    buf = torch.full((lead + n + trail,), fill, dtype=dtype, device="cuda")
    return buf, buf[lead:lead + n], fill


def _words_kept(case, what, buf, lead, n, fill):
    b = buf.cpu().numpy()
    _require((b[:lead] == fill).all() and (b[lead + n:] == fill).all(), case, "%s: words outside the slice were written" % what)


def check_bitmap(native, case):
    import torch
    p = case["params"]
    mode, ia, n, k = p["mode"], p["is_aux"], p["n"], p["queries"]
    L, dp, M = native.lib(), native.dptr, bitmap_model
    otab = ntsc_table(mode)
    import oracle
    table = native.build_table(mode, oracle.cie2000_matrix(oracle.PALETTE_RGB[5])[1], True)      # (milliseconds; on this round's stream)
    want_packed = []
    dev_packed = []
    for side in (0, 1):                                            # source, target
        main, aux = case["screens"][side]
        mbuf, mview = _guarded(n * 8192, p["lead_main"], 3)
        abuf, aview = _guarded(n * 8192, p["lead_aux"], 3)
        mview.copy_(torch.from_numpy(main).reshape(-1))
        aview.copy_(torch.from_numpy(aux).reshape(-1))
        obuf, oview, fill = _words(n * 4096, torch.int64, p["lead_out"])
        native.check(L.iiv_pack(mode, n, dp(mview), dp(aview) if mode == DHGR or side else dp(None), dp(oview), native.stream_ptr()))
        _sync()
        want = M.pack(mode, main, aux)
        _same(case, "pack (%s)" % ("source", "target")[side], oview.cpu().numpy().view(np.uint64).reshape(n, 32, 128), want)
        _words_kept(case, "pack", obuf, p["lead_out"], n * 4096, fill)
        _guards_kept(case, "pack: the main bank", mbuf, p["lead_main"], n * 8192)
        _same(case, "the main bank after pack", mview.cpu().numpy(), main.reshape(-1))
        want_packed.append(want)
        dev_packed.append(oview)                                   # the device's own output goes on to the next kernel
    wbuf, wview, fill = _words(n * 8192, torch.int32, p["lead_out"])
    native.check(L.iiv_diff_weights(mode, dp(table), n, dp(dev_packed[0]), dp(dev_packed[1]), ia, dp(wview), native.stream_ptr()))
    _sync()
    want_dw = M.diff_weights(mode, otab, want_packed[0], want_packed[1], ia)
    _same(case, "diff_weights", wview.cpu().numpy().reshape(n, 32, 256), want_dw)
    _words_kept(case, "diff_weights", wbuf, p["lead_out"], n * 8192, fill)
    tgt = dev_packed[1][p["which"] * 4096:(p["which"] + 1) * 4096]   # one screen of the batch is the queries' bitmap
    pages, contents, rows = (torch.from_numpy(a).cuda() for a in (case["pages"], case["contents"] | case["junk"], case["rows"]))
    dbuf, dview, fill = _words(k * 256, torch.int32, p["lead_out"])
    native.check(L.iiv_compute_delta_pages(mode, dp(table), k, dp(tgt), dp(pages), dp(contents), dp(rows), ia, dp(dview), native.stream_ptr()))
    _sync()
    want_d = M.compute_delta_pages(mode, otab, want_packed[1][p["which"]], case["pages"], case["contents"], case["rows"], ia)
    _same(case, "compute_delta_pages", dview.cpu().numpy().reshape(k, 256), want_d)
    _words_kept(case, "compute_delta_pages", dbuf, p["lead_out"], k * 256, fill)
    _same(case, "the rows after the call", rows.cpu().numpy(), case["rows"])


# ---- 4:2:0 planes into the resize ------------------------------------------------------------------------------------------

YUV_LAYOUTS = ("i420", "nv12", "nv21", "rows", "nv12_rows", "frames", "cut", "nv12_cut")      # tests/test_gpu_yuv.py: LAYOUTS
YUV_PRESETS = ("bt601", "bt709", "jpeg")
YUV_FORCED = ("free", "horizontal only", "vertical only", "same size", "tall", "tall and the width changes", "wide", "two passes")


def _yuv_planes(kind, n, h, w, rng):
    """(y, u, v): noise, planes of 0 and 255, or noise under a one-sample chroma checkerboard of 0 and 255"""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if kind == "noise":
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, h, w), (n, ch, cw), (n, ch, cw)))
    if kind == "extremes":
        return tuple((rng.integers(0, 2, s) * 255).astype(np.uint8) for s in ((n, h, w), (n, ch, cw), (n, ch, cw)))
    f, y, x = np.ogrid[0:n, 0:ch, 0:cw]
    u = (((x + y + f) & 1) * 255).astype(np.uint8)
    return rng.integers(0, 256, (n, h, w), dtype=np.uint8), u, (255 - u).astype(np.uint8)


def _draw_yuv_matrix(rng):
    kind = ("preset", "inside", "bounds")[int(rng.integers(0, 3))]
    if kind == "preset":
        return YUV_PRESETS[int(rng.integers(0, 3))]
    if kind == "inside":
        return (int(rng.integers(0, 256)),) + tuple(int(k) for k in rng.integers(-1023, 1024, 5))
    return (int(rng.choice((0, 255))),) + tuple(int(k) for k in rng.choice((-1023, 1023), 5))


def draw_yuv(rng, round_index=0):
    n = int(rng.integers(1, 6))
    h, w = _size(rng), _size(rng)
    H, W = (192, 280) if rng.random() < 0.5 else (_size(rng), _size(rng))
    forced = YUV_FORCED[round_index % 8]
    if forced in ("tall", "tall and the width changes"):       # h > 100 w: the conversion alone, then the RGB path
        w = int(rng.integers(1, 4))
        h = int(rng.integers(100 * w + 1, 401))
    if forced == "wide":                                        # w_pad > 4096: one row per workgroup
        w, h = int(rng.integers(4097, 4200)), int(rng.integers(1, 5))
        H = h if rng.random() < 0.5 else int(rng.integers(1, 9))
    while forced in ("horizontal only", "tall and the width changes", "wide", "two passes") and W == w:
        W = _size(rng)
    while forced in ("vertical only", "tall", "tall and the width changes", "two passes") and H == h:
        H = _size(rng)
    if forced in ("horizontal only", "same size"):
        H = h
    if forced in ("vertical only", "same size", "tall"):
        W = w
    kind = ("noise", "extremes", "checker")[int(rng.integers(0, 3))]
    planes = _yuv_planes(kind, n, h, w, rng)
    params = dict(n=n, h=h, w=w, H=H, W=W, content=kind, layout=YUV_LAYOUTS[int(rng.integers(0, len(YUV_LAYOUTS)))],
                  fill=int(rng.integers(0, 256)), matrix=_draw_yuv_matrix(rng))
    return dict(stage="yuv", params=params, forced=forced, planes=planes)


def _yuv_views(p, planes):
    """the planes on the device in the case's layout (the layouts are tests/test_gpu_yuv.py's own)"""
    import test_gpu_yuv
    return test_gpu_yuv._layout(p["layout"], *planes, fill=p["fill"])


def check_yuv(native, case):
    p = case["params"]
    y, u, v = case["planes"]
    got = native.resize_frames_yuv420(*_yuv_views(p, (y, u, v)), (p["H"], p["W"]), matrix=p["matrix"])
    _sync()
    _same(case, "resize_frames_yuv420", got.cpu().numpy(), resize_model.resize(yuv_model.to_rgb(y, u, v, p["matrix"]), (p["H"], p["W"])))


# ---- direct ingest ----------------------------------------------------------------------------------------------------

DIRECT_WIDTHS = (280, 560)
DIRECT_KINDS = 9          # 0..5 of ingest_model.frame_set, 6 noise, 7 a flat frame, 8 flat rows between two palette colours
DIRECT_FORCED = (6, 7, 8, None)


def direct_pool_frames(pool, palette_name, width):
    pal = _palette(palette_name)
    out = np.empty((len(pool), 192, width, 3), np.uint8)
    for i, (kind, seed) in enumerate(pool):
        rng = np.random.default_rng([seed, kind])
        if kind < 6:
            out[i] = np.repeat(ingest_model.frame_set(pal, seed)[kind], width // 280, axis=1)
        elif kind == 6:
            out[i] = rng.integers(0, 256, (192, width, 3))
        elif kind == 7:
            out[i] = rng.integers(0, 256, 3)
        else:       # every row flat and half-way between two palette colours: both colours' rows cost the same where the sum is even
            a, b = np.asarray(pal, np.int64)[rng.integers(0, 16, (2, 192))]
            out[i] = ((a + b) // 2)[:, None, :]
    return out


def draw_direct(rng, round_index=0):
    mode = int(rng.integers(0, 2))
    width = DIRECT_WIDTHS[int(rng.integers(0, 2))]
    pal = ingest_model.NAMES[int(rng.integers(0, len(ingest_model.NAMES)))]
    dither = int(rng.choice(AMPLITUDES))
    cost = bool(rng.integers(0, 2))
    if round_index % 3 == 0:                              # the cost against the screen error: only without dither
        dither, cost = 0, True
    n = _count(rng)
    pool, idx = _draw_pool(rng, n, kinds=DIRECT_KINDS)
    forced = DIRECT_FORCED[round_index % 4]
    if forced is not None:
        pool[0] = (forced, pool[0][1])
    params = dict(mode=mode, width=width, palette=pal, n=n, dither=dither, cost=cost, frame_offset=int(rng.integers(0, 4)),
                  tail=int(rng.integers(0, 3)), lead_rgb=_lead(rng, 4), lead_main=_lead(rng, 8), lead_aux=_lead(rng, 8),
                  lead_cost=_lead(rng, 8), pool=pool, junk=int(rng.integers(1 << 30)))
    return dict(stage="direct", params=params, idx=idx)


def check_direct(native, case):
    import torch
    p = case["params"]
    mode, n, width, pal = p["mode"], p["n"], p["width"], np.ascontiguousarray(_palette(p["palette"]), dtype=np.uint8).reshape(16, 3)
    frame_bytes = 192 * width * 3
    pool = direct_pool_frames(p["pool"], p["palette"], width)
    frames = pool[case["idx"]]
    total = p["frame_offset"] + n + p["tail"]
    big = np.random.default_rng(p["junk"]).integers(0, 256, (total, 192, width, 3), dtype=np.uint8)   # the batch the frames lie in
    big[p["frame_offset"]:p["frame_offset"] + n] = frames
    sbuf, sview = _guarded(total * frame_bytes, p["lead_rgb"], 16)
    sview.copy_(torch.from_numpy(big.reshape(-1)))
    src = sview[p["frame_offset"] * frame_bytes:(p["frame_offset"] + n) * frame_bytes]
    bufs = [_guarded(n * 8192, p["lead_main"], 40), _guarded(n * 8192, p["lead_aux"], 40)]
    cbuf, cview = _guarded(n * 8, p["lead_cost"], 24)
    _require(src.data_ptr() % 4 == 0 and all(b[1].data_ptr() % 8 == 0 for b in bufs) and cview.data_ptr() % 8 == 0, case,
             "the buffers are not at the contract's alignments")
    hp = pal.reshape(48)
    native.check(native.lib().iiv_frames_to_memory_maps_direct(mode, native.hptr(hp), n, native.dptr(src), width, p["dither"],
                                                               native.dptr(bufs[0][1]), native.dptr(bufs[1][1]),
                                                               native.dptr(cview) if p["cost"] else None, native.stream_ptr()))
    _sync()
    m, a, c = direct_model.frames_to_memory_maps_direct(mode, pal, pool, p["dither"])
    idx = case["idx"]
    _check_maps(case, "direct ingest", mode, n, bufs, (p["lead_main"], p["lead_aux"]), (m[idx], a[idx] if a is not None else None))
    if p["cost"]:
        _same(case, "direct ingest: d_cost", cview.cpu().numpy().view(np.uint64), c[idx])
        _guards_kept(case, "direct ingest: d_cost", cbuf, p["lead_cost"], n * 8)
        if p["dither"] == 0:
            level0 = render_error_model.render_error(mode, m, a, pal, pool)[:, 0, :].sum(axis=1)
            _same(case, "the model's cost against render_error_model's level 0", c, level0)
    else:
        _require(bool((cbuf.cpu().numpy() == GUARD).all()), case, "direct ingest: d_cost is NULL and the buffer was written")
    _guards_kept(case, "direct ingest: the source", sbuf, p["lead_rgb"], total * frame_bytes)
    _same(case, "the source after the call", sview.cpu().numpy(), big.reshape(-1))


# ---- the chain from 4:2:0 planes --------------------------------------------------------------------------------------------

def draw_chain_yuv(rng, round_index=0):
    mode = int(rng.integers(0, 2))
    pal = ingest_model.NAMES[int(rng.integers(0, len(ingest_model.NAMES)))]
    n = int(rng.integers(2, 4))
    h, w = _size(rng), _size(rng)
    kind = ("noise", "extremes", "checker")[int(rng.integers(0, 3))]
    planes = _yuv_planes(kind, n, h, w, rng)
    dither = int(rng.choice(AMPLITUDES))
    # both source widths of the direct ingest, and dither 0 (where its cost is the screen error) with each, every four rounds
    params = dict(mode=mode, palette=pal, n=n, h=h, w=w, width=DIRECT_WIDTHS[round_index % 2], content=kind,
                  layout=YUV_LAYOUTS[int(rng.integers(0, len(YUV_LAYOUTS)))], fill=int(rng.integers(0, 256)),
                  matrix=YUV_PRESETS[int(rng.integers(0, 3))], dither=0 if round_index % 4 < 2 else dither)
    return dict(stage="chain_yuv", params=params, planes=planes)


def check_chain_yuv(native, case):
    p = case["params"]
    mode, n, pal, size = p["mode"], p["n"], _palette(p["palette"]), (192, p["width"])
    small = native.resize_frames_yuv420(*_yuv_views(p, case["planes"]), size, matrix=p["matrix"])
    main, aux, cost = native.frames_to_memory_maps_direct(mode, pal, small, p["dither"], cost=True)   # each stage takes the last one's tensor
    rgb = native.render_rgb(mode, pal, main, aux)
    sums = native.render_error(mode, pal, main, aux, small)
    _sync()
    m_small = resize_model.resize(yuv_model.to_rgb(*case["planes"], p["matrix"]), size)
    _same(case, "chain_yuv: resize", small.cpu().numpy(), m_small)
    m_main, m_aux, m_cost = direct_model.frames_to_memory_maps_direct(mode, pal, m_small, p["dither"])
    _same(case, "chain_yuv: direct ingest main", main.cpu().numpy(), m_main)
    _require((aux is None) == (m_aux is None), case, "chain_yuv: direct ingest aux")
    if aux is not None:
        _same(case, "chain_yuv: direct ingest aux", aux.cpu().numpy(), m_aux)
    _same(case, "chain_yuv: direct ingest cost", cost.cpu().numpy().view(np.uint64), m_cost)
    m_rgb = render_model.render_rgb(mode, m_main, m_aux, pal)
    _same(case, "chain_yuv: render_rgb", rgb.cpu().numpy(), m_rgb)
    m_sums = render_error_model.error_sums_of_screens(m_rgb, m_small)
    _same(case, "chain_yuv: render_error", sums.cpu().numpy().view(np.uint64).reshape(n, 3, 3), m_sums)
    if p["dither"] == 0:
        _same(case, "chain_yuv: the cost against render_error's level 0", m_cost, m_sums[:, 0, :].sum(axis=1))


# ---- palette bytes -> delta-E matrix, Lab pairs -> delta-E ------------------------------------------------------------------

COLOUR_KINDS = ("uniform", "dark", "greyish", "duplicates")


def _colour_palette(rng, kind):
    if kind == "dark":
        return rng.integers(0, 28, (16, 3))
    if kind == "greyish":
        return np.clip(rng.integers(0, 256, (16, 1)) + rng.integers(-2, 3, (16, 3)), 0, 255)
    pal = rng.integers(0, 256, (16, 3))
    if kind == "duplicates":
        k = int(rng.integers(1, 16))
        rows = rng.permutation(16)
        pal[rows[:k]] = pal[rows[k:]][rng.integers(0, 16 - k, k)]
    return pal


def draw_colour(rng, round_index=0):
    kind = COLOUR_KINDS[round_index % 4]
    pal, redraws = colour_cases.draw_palette(rng, lambda g: _colour_palette(g, kind))
    n = int(rng.choice(COUNTS)) if rng.random() < 0.5 else int(rng.integers(100, 701))
    own = [colour_model.lab_double(row) for row in pal]
    pairs, own_pairs = [], 0
    while len(pairs) < n:
        if rng.random() < 0.3:
            i, j = (int(v) for v in rng.integers(0, 16, 2))
            a, b, mine = own[i], own[j], 1
        else:
            a, b = (tuple(float(v) for v in rng.uniform((0, -128, -128), (100, 128, 128))) for _ in range(2))
            mine = 0
        if colour_cases.pair_allowed(a, b):
            pairs.append((a, b))
            own_pairs += mine
        else:
            redraws += 1
    lab = np.array(pairs, dtype=np.float64).reshape(n, 2, 3)
    params = dict(palette=kind, n=n, own_pairs=own_pairs, different=len(np.unique(pal, axis=0)), redraws=redraws,
                  first="%02x%02x%02x" % tuple(pal[0]))
    return dict(stage="colour", params=params, rgb=pal, lab1=np.ascontiguousarray(lab[:, 0]), lab2=np.ascontiguousarray(lab[:, 1]))


def colour_wants(case):
    """colour_model's values of a case: (the matrix as doubles, its floor, the pairs' delta-E as doubles)"""
    f, i = colour_cases.matrix_of(case["rgb"].tobytes())
    pairs = np.array([float(colour_model.delta_e(tuple(a.tolist()), tuple(b.tolist()))) for a, b in zip(case["lab1"], case["lab2"])])
    return f, i, pairs


def check_colour(native, case):
    T = colour_model.T
    want_f, want_i, want_pairs = colour_wants(case)
    f, i = native.cie2000_matrix(case["rgb"])
    _require(not np.isnan(f).any(), case, "cie2000_matrix: a NaN")
    err = np.abs(f - want_f)
    _require(err.max() <= T, case, lambda: "cie2000_matrix: %g from the model at %s (T = %g)" % (err.max(), divmod(int(err.argmax()), 16), T))
    _same(case, "cie2000_matrix, the ints", i, want_i)
    same = (case["rgb"][:, None, :] == case["rgb"][None, :, :]).all(axis=2)
    _require(not f[same].any() and not np.signbit(f[same]).any(), case, "cie2000_matrix: a colour against itself is not 0.0")
    got = native.delta_e_cie2000(case["lab1"], case["lab2"])
    _require(got.shape == want_pairs.shape and not np.isnan(got).any(), case, "delta_e_cie2000: shape %s or a NaN" % (got.shape,))
    err = np.abs(got - want_pairs)
    _require(err.max() <= T, case, lambda: "delta_e_cie2000: %g from the model at pair %d (T = %g)" % (err.max(), int(err.argmax()), T))


# ---- the loop ---------------------------------------------------------------------------------------------------------

DRAW = {"resize": draw_resize, "ingest": draw_ingest, "mono": draw_mono, "render": draw_render, "a2m": draw_a2m, "audio": draw_audio,
        "chain": draw_chain, "bitmap": draw_bitmap, "yuv": draw_yuv, "direct": draw_direct, "chain_yuv": draw_chain_yuv, "colour": draw_colour}
CHECK = {"resize": check_resize, "ingest": check_ingest, "mono": check_mono, "render": check_render, "a2m": check_a2m,
         "audio": check_audio, "chain": check_chain, "bitmap": check_bitmap, "yuv": check_yuv, "direct": check_direct,
         "chain_yuv": check_chain_yuv, "colour": check_colour}


def _fuzz(stage, native, rng, round_index, seed=None):
    case = DRAW[stage](rng, round_index)
    case["seed"], case["round"] = seed, round_index
    CHECK[stage](native, case)
    return describe(case)


def fuzz_resize(native, rng, round_index, seed=None):
    return _fuzz("resize", native, rng, round_index, seed)


def fuzz_ingest(native, rng, round_index, seed=None):
    return _fuzz("ingest", native, rng, round_index, seed)


def fuzz_mono(native, rng, round_index, seed=None):
    return _fuzz("mono", native, rng, round_index, seed)


def fuzz_render(native, rng, round_index, seed=None):
    return _fuzz("render", native, rng, round_index, seed)


def fuzz_a2m(native, rng, round_index, seed=None):
    return _fuzz("a2m", native, rng, round_index, seed)


def fuzz_audio(native, rng, round_index, seed=None):
    return _fuzz("audio", native, rng, round_index, seed)


def fuzz_chain(native, rng, round_index, seed=None):
    return _fuzz("chain", native, rng, round_index, seed)


def fuzz_bitmap(native, rng, round_index, seed=None):
    return _fuzz("bitmap", native, rng, round_index, seed)


def fuzz_yuv(native, rng, round_index, seed=None):
    return _fuzz("yuv", native, rng, round_index, seed)


def fuzz_direct(native, rng, round_index, seed=None):
    return _fuzz("direct", native, rng, round_index, seed)


def fuzz_chain_yuv(native, rng, round_index, seed=None):
    return _fuzz("chain_yuv", native, rng, round_index, seed)


def fuzz_colour(native, rng, round_index, seed=None):
    return _fuzz("colour", native, rng, round_index, seed)


FUZZ = {"resize": fuzz_resize, "ingest": fuzz_ingest, "mono": fuzz_mono, "render": fuzz_render, "a2m": fuzz_a2m, "audio": fuzz_audio,
        "chain": fuzz_chain, "bitmap": fuzz_bitmap, "yuv": fuzz_yuv, "direct": fuzz_direct, "chain_yuv": fuzz_chain_yuv,
        "colour": fuzz_colour}


def run(rounds, seed=SEED, stages=None, side_stream=False, first_round=0, log=None):
    """`rounds` rounds (a number, or a number per stage as ROUNDS) of every stage of `stages` (all by default) at `seed`,
    from round first_round on.  side_stream: all device work of a round on one non-blocking stream instead of the default
    (null) stream, which orders itself against everything and so hides a launch or copy issued on the wrong stream; every
    check synchronises that stream before it compares.  -> the descriptions of the cases that ran."""
    import torch
    import _iiv_native as native
    native.lib()
    side = torch.cuda.Stream() if side_stream else None
    done = []
    for stage in (stages or STAGES):
        n = rounds[stage] if isinstance(rounds, dict) else int(rounds)
        for r in range(first_round, first_round + n):
            with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
                line = FUZZ[stage](native, stage_rng(seed, r, stage), r, seed)
            done.append(line)
            if log:
                log("round %3d ok: %s" % (r, line))
    return done


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rounds", nargs="?", type=int, default=12)
    ap.add_argument("seed", nargs="?", type=int, default=SEED)
    ap.add_argument("--stage", action="append", choices=STAGES, help="only this stage (may be given more than once)")
    ap.add_argument("--round", type=int, default=0, help="the first round to run (with rounds = 1: that case alone)")
    args = ap.parse_args(argv)
    side = os.environ.get("IIV_STAGE_FUZZ_SIDE_STREAM") == "1"
    t0 = time.time()
    done = run(args.rounds, args.seed, args.stage, side, args.round, log=lambda s: print(s[:300], flush=True))
    print("stage fuzz: %d cases at seed %d%s, all equal to their models (%.0f s)" % (len(done), args.seed, " on a side stream" if side else "",
                                                                                    time.time() - t0))


if __name__ == "__main__":
    main(sys.argv[1:])
