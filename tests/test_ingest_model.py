"""CPU: the oracle's colour RGB -> memory-map conversion (orc_frame_to_memory_map, the yardstick of csrc/iiv_ingest.hip)
against tests/ingest_model.py, an independent restatement of the contract in include/iivision.h -- byte for byte, for
every adversarial palette of the model file and the two real ones, both modes, no dither / ordered dither at its
smallest, a middle and its largest amplitude / error diffusion, on the frames of ingest_model.frame_set.  And the
palettes built to tie do tie, the way the contract resolves it."""

import numpy as np
import pytest

import ingest_model as M
from ingest_model import NAMES, frames_of, palette

MODES = [M.DHGR, M.HGR]


def _assert_equal(O, mode, pal, frames, dither, model_main, model_aux, what):
    for i in range(len(frames)):
        om, oa = O.frame_to_memory_map(mode, pal, frames[i], dither)
        assert (om == model_main[i]).all(), what + (M.FRAME_KINDS[i], "main", int((om != model_main[i]).sum()))
        if mode == M.DHGR:
            assert (oa == model_aux[i]).all(), what + (M.FRAME_KINDS[i], "aux", int((oa != model_aux[i]).sum()))
        else:
            assert oa is None and model_aux is None


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_model_ordered(O, name, mode):
    pal, frames = palette(O, name), frames_of(O, name)
    for dither in M.DITHERS_CPU:
        if dither == M.DITHER_DIFFUSION:
            continue
        mm, ma = M.frames_to_memory_maps(mode, pal, frames, dither)
        _assert_equal(O, mode, pal, frames, dither, mm, ma, (name, mode, dither))


@pytest.fixture(scope="module")
def diffusion_model(O):
    """The model's error diffusion of every palette's whole frame set, one raster loop per mode for all of them."""
    pals = np.concatenate([np.broadcast_to(palette(O, n), (len(M.FRAME_KINDS), 16, 3)) for n in NAMES])
    frames = np.concatenate([frames_of(O, n) for n in NAMES])
    return {mode: M.frames_to_memory_maps(mode, pals, frames, M.DITHER_DIFFUSION) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_model_diffusion(O, diffusion_model, name, mode):
    pal, frames = palette(O, name), frames_of(O, name)
    at = NAMES.index(name) * len(M.FRAME_KINDS)
    mm, ma = diffusion_model[mode]
    _assert_equal(O, mode, pal, frames, M.DITHER_DIFFUSION, mm[at:at + len(frames)],
                  ma[at:at + len(frames)] if ma is not None else None, (name, mode, "diffusion"))


def test_model_single_frame_entry_point(O):
    """frame_to_memory_map (one frame, one palette) is the batch of one."""
    pal, frames = palette(O, "random_a"), frames_of(O, "random_a")
    for mode in MODES:
        for dither in (32, M.DITHER_DIFFUSION):
            m, a = M.frame_to_memory_map(mode, pal, frames[3], dither)
            om, oa = O.frame_to_memory_map(mode, pal, frames[3], dither)
            assert m.shape == (32, 256) and m.dtype == np.uint8 and (m == om).all()
            assert (a is None and oa is None) if mode == M.HGR else (a == oa).all()
            assert (m[O.screen_holes()] == 0).all()


# ---- the palettes built to tie: they do, and the contract's rule decides ------------------------

def _quads(main, aux):
    return (M.unpack(M.DHGR, main, aux).reshape(192, 140, 4).astype(np.int64) << np.arange(4)).sum(axis=-1)


def _patterns(main):
    return (M.unpack(M.HGR, main).reshape(192, 140, 2).astype(np.int64) << np.arange(2)).sum(axis=-1)


@pytest.mark.parametrize("dither", M.DITHERS_CPU)
def test_all_equal_palette_ties_to_value_0_pattern_0_palette_bit_0(O, dither):
    pal, frames = palette(O, "all_equal"), frames_of(O, "all_equal")
    for f in frames:
        main, aux = O.frame_to_memory_map(M.DHGR, pal, f, dither)
        assert not main.any() and not aux.any()                  # every dot quad is colour value 0
        main, _ = O.frame_to_memory_map(M.HGR, pal, f, dither)
        assert not (main & 0x80).any() and not main.any()        # palette bit 0 everywhere, and pattern 0


@pytest.mark.parametrize("dither", M.DITHERS_CPU)
def test_pairs_palette_never_picks_the_upper_twin(O, dither):
    pal, frames = palette(O, "pairs"), frames_of(O, "pairs")
    seen = set()
    for f in frames:
        q = _quads(*O.frame_to_memory_map(M.DHGR, pal, f, dither))
        assert (q < 8).all()
        seen |= set(np.unique(q).tolist())
    assert seen == set(range(8))                                  # (and every lower twin is picked somewhere)


@pytest.mark.parametrize("dither", M.DITHERS_CPU)
@pytest.mark.parametrize("name", ["hgr_ties", "hgr_ties_bw"])
def test_hgr_ties_palettes_keep_palette_bit_0(O, name, dither):
    pal, frames = palette(O, name), frames_of(O, name)
    seen = set()
    for f in frames:
        main, _ = O.frame_to_memory_map(M.HGR, pal, f, dither)
        assert not (main & 0x80).any()
        seen |= set(np.unique(_patterns(main)).tolist())
    # (not by leaving the screen black; and with white == black the lower pattern stands for both)
    assert seen == ({0, 1, 2} if name == "hgr_ties_bw" else {0, 1, 2, 3})


def test_odd_grey_between_two_even_greys_takes_the_lower(O):
    """even_greys on its frame of odd greys, no dither: grey 2 j + 1 is as far from entry j as from entry j + 1."""
    pal, frames = palette(O, "even_greys"), frames_of(O, "even_greys")
    grey = frames[1][:, 0::2, 0].astype(np.int64)
    assert (grey % 2 == 1).all() and grey.max() < 30 and (frames[1][:, 0::2] == frames[1][:, 1::2]).all()
    q = _quads(*O.frame_to_memory_map(M.DHGR, pal, frames[1], 0))
    assert (q == (grey - 1) // 2).all()


def test_real_palettes_use_what_the_tie_palettes_must_not(O):
    """The assertions above are not vacuous: with sixteen distinct colours the same frames do set palette bits and do
    pick colour values of 8 and above."""
    pal, frames = palette(O, "ntsc"), frames_of(O, "ntsc")
    for dither in M.DITHERS_CPU:
        main, _ = O.frame_to_memory_map(M.HGR, pal, frames[0], dither)
        bits = M.rows_of(main) >> 7
        assert 0.1 < bits.mean() < 0.9
        assert (_quads(*O.frame_to_memory_map(M.DHGR, pal, frames[0], dither)) >= 8).any()
