"""GPU: the mono error diffusion (csrc/iiv_mono.hip) past its first chunk.  mono_frames cuts a call with IIV_DITHER_DIFFUSION
into chunks of CHUNK = 2048 frames; each chunk moves d_rgb, d_main and d_aux on by f0 frames and reuses one stream-ordered luma
scratch.  n = 2051 is one chunk of 2048 and one of 3.

Frame i of the source is item i % 7 of a pool of seven, gathered on the device with index_select (331 MB of source in HGR, 661 MB
in DHGR); tests/mono_model.py runs on the seven and EVERY frame's memory maps are compared on the device.  2048 % 7 = 4: the second
chunk starts on item 4, not on item 0 as the first did, so a chunk that reads d_rgb at frame 0 again, or writes its maps where
the first chunk's lie, shows in the bytes.  The maps are written into a larger batch at a frame offset, d_main and d_aux at
different ones, every other frame of it a fill byte: a chunk that writes outside frames 0 .. n - 1 of either bank shows too, and
in DHGR the two banks are checked one after the other, so the report names the bank.

The ordered dither at the same n does not go through the loop (one launch over all frames): it holds the loop's neighbour.
IIV_EXP_MONO_CHUNK is not used: it is read once per process and is a timing knob, not a contract.
tests/test_render_batches_host.py holds CHUNK to the source's text and the seven items' maps pairwise different, on the CPU."""
import functools

import numpy as np
import pytest

import mono_model as M

pytestmark = pytest.mark.gpu

CHUNK = 2048                # csrc/iiv_mono.hip:259   int chunk = chunk_env > 0 ? chunk_env : 2048
P = 7                       # items in the pool
N = CHUNK + 3
MODES = [M.HGR, M.DHGR]
ORDERED = 32                # the ordered-dither amplitude of the neighbour case
FILL = 0xEE                 # (bit 7 set: no byte a mono map holds)
MAIN_AT, AUX_AT, SPARE = 3, 5, 9     # the frame offsets of the maps in their batches of N + SPARE frames


def assert_chunks(n):
    """the arithmetic the cases rely on"""
    assert n > CHUNK and n - CHUNK < CHUNK          # two chunks, the second a short one
    assert CHUNK % P == 4                           # the second chunk starts on another item than the first
    assert MAIN_AT != AUX_AT and max(MAIN_AT, AUX_AT) < SPARE


@functools.lru_cache(maxsize=None)
def pool(mode):
    """seven source frames, one pixel per dot: four picture-like ones and three of uniform noise"""
    rgb = np.ascontiguousarray(np.concatenate([M.structured_frames(mode, 4, seed=25), M.noise_frames(mode, 3, seed=26)]))
    assert len(rgb) == P
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(maxsize=None)
def want_maps(mode, dither):
    """the model's memory maps of the seven: computed once, shared, never written to"""
    main, aux = M.frames_to_memory_maps(mode, pool(mode), dither)
    main.setflags(write=False)
    if aux is not None:
        aux.setflags(write=False)
    return main, aux


def _bad_frames(got, exp):
    """got: CUDA (n, 32, 256); exp: numpy (P, 32, 256) -> the frames i that differ from exp[i % P]"""
    import torch
    n = got.shape[0]
    e = torch.from_numpy(np.array(exp)).to(got.device)
    bad = torch.zeros(n, dtype=torch.bool, device=got.device)
    for r in range(P):
        bad[r::P] = (got[r::P] != e[r]).flatten(1).any(1)
    return torch.nonzero(bad).flatten().cpu().numpy()


def _run(native, mode, dither):
    import torch
    n = N
    assert_chunks(n)
    src = torch.from_numpy(np.array(pool(mode))).cuda()
    rgb = src.index_select(0, torch.arange(n, device="cuda") % P)
    assert tuple(rgb.shape) == (n, 192, M.width(mode), 3) and rgb.is_contiguous()
    main_batch = torch.full((n + SPARE, 32, 256), FILL, dtype=torch.uint8, device="cuda")
    aux_batch = torch.full((n + SPARE, 32, 256), FILL, dtype=torch.uint8, device="cuda") if mode == M.DHGR else None
    main = main_batch[MAIN_AT:MAIN_AT + n]
    aux = aux_batch[AUX_AT:AUX_AT + n] if mode == M.DHGR else None
    got_main, got_aux = native.frames_to_memory_maps_mono(mode, rgb, dither, out=(main, aux))
    assert got_main.data_ptr() == main.data_ptr() and (got_aux is None) == (mode == M.HGR)
    em, ea = want_maps(mode, dither)
    bad = _bad_frames(main, em)
    assert len(bad) == 0, "main: %d of %d frames differ from the model, the first at %s" % (len(bad), n, bad[:10])
    assert bool((main_batch[:MAIN_AT] == FILL).all()) and bool((main_batch[MAIN_AT + n:] == FILL).all()), "main: written outside the n frames"
    if mode == M.DHGR:
        bad = _bad_frames(aux, ea)
        assert len(bad) == 0, "aux: %d of %d frames differ from the model, the first at %s" % (len(bad), n, bad[:10])
        assert bool((aux_batch[:AUX_AT] == FILL).all()) and bool((aux_batch[AUX_AT + n:] == FILL).all()), "aux: written outside the n frames"
    del rgb, main, aux, main_batch, aux_batch, got_main, got_aux
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", MODES)
def test_diffusion_every_frame_past_the_first_chunk(native, mode):
    _run(native, mode, M.DITHER_DIFFUSION)


@pytest.mark.parametrize("mode", MODES)
def test_ordered_dither_at_the_same_batch(native, mode):
    _run(native, mode, ORDERED)
