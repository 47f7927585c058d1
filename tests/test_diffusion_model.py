"""CPU: tests/diffusion_model.py, the contract of iiv_frames_to_memory_maps_diffused in numpy.
  - with Floyd-Steinberg's weights it gives the bytes of ingest_model's IIV_DITHER_DIFFUSION and of the oracle, in both modes,
    for every adversarial palette of ingest_model and the two real ones: the new contract has reproduced the old one's
    wording, HGR's palette-bit look-ahead included;
  - every named kernel -- the model's table and frame_grabber.DIFFUSION_KERNELS, which must be the same table -- obeys the
    contract's constraints;
  - the multiply-and-shift the kernel divides with is floor(acc / divisor) over the whole range |acc| <= 255 * 64, for every
    divisor 1..64, within the widths the kernel computes in;
  - DHGR with all-zero weights is the conversion without dither.  (HGR is left out of that: the ordered path gives a straddling
    pixel's dots per byte, the diffusion path per pixel -- the note at the top of ingest_model.py.)"""

import numpy as np
import pytest

import diffusion_model as D
import ingest_model as M
from ingest_model import NAMES, frames_of, palette

MODES = [M.DHGR, M.HGR]


@pytest.fixture(scope="module")
def sweep(O):
    pals = np.concatenate([np.broadcast_to(palette(O, n), (len(M.FRAME_KINDS), 16, 3)) for n in NAMES])
    frames = np.concatenate([frames_of(O, n) for n in NAMES])
    return pals, frames


@pytest.fixture(scope="module")
def floyd_steinberg(sweep):
    """one raster loop per mode and model for every palette's whole frame set"""
    pals, frames = sweep
    w, d = D.KERNELS["floyd-steinberg"]
    return {mode: (D.frames_to_memory_maps(mode, pals, frames, w, d), M.frames_to_memory_maps(mode, pals, frames, M.DITHER_DIFFUSION))
            for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_floyd_steinberg_weights_give_the_old_contracts_bytes(O, floyd_steinberg, name, mode):
    (nm, na), (om, oa) = floyd_steinberg[mode]
    pal, frames = palette(O, name), frames_of(O, name)
    at = NAMES.index(name) * len(M.FRAME_KINDS)
    for i in range(len(frames)):
        assert (nm[at + i] == om[at + i]).all(), (name, mode, M.FRAME_KINDS[i], "ingest_model", int((nm[at + i] != om[at + i]).sum()))
        xm, xa = O.frame_to_memory_map(mode, pal, frames[i], O.DITHER_DIFFUSION)
        assert (nm[at + i] == xm).all(), (name, mode, M.FRAME_KINDS[i], "oracle", int((nm[at + i] != xm).sum()))
        if mode == M.DHGR:
            assert (na[at + i] == oa[at + i]).all() and (na[at + i] == xa).all(), (name, mode, M.FRAME_KINDS[i], "aux")
        else:
            assert na is None and oa is None and xa is None


def test_the_look_ahead_is_exercised(O, floyd_steinberg):
    """the equality above is not vacuous for HGR: under the real palette the diffusion sets palette bits, and differently
    from the conversion without dither"""
    at = NAMES.index("ntsc") * len(M.FRAME_KINDS)
    (nm, _), _ = floyd_steinberg[M.HGR]
    bits = M.rows_of(nm[at]) >> 7
    assert 0.1 < bits.mean() < 0.9
    plain, _ = M.frame_to_memory_map(M.HGR, palette(O, "ntsc"), frames_of(O, "ntsc")[0], 0)
    assert (M.rows_of(plain) >> 7 != bits).any()


def test_every_named_kernel_obeys_the_constraints():
    import frame_grabber
    assert set(frame_grabber.DIFFUSION_KERNELS) == set(D.KERNELS) and len(D.KERNELS) == 9
    for name, (w, d) in D.KERNELS.items():
        pw, pd = frame_grabber.DIFFUSION_KERNELS[name]
        assert np.array_equal(np.asarray(pw), w) and pd == d, name
        assert np.array_equal(D.check_arguments(pw, pd), w)
        assert 1 <= d <= 64 and not w[0, :3].any() and (w >= 0).all() and 0 < w.sum() <= d, name
    # all of the error, except Atkinson's 6/8
    assert {n for n, (w, d) in D.KERNELS.items() if w.sum() != d} == {"atkinson"} and D.KERNELS["atkinson"][0].sum() == 6
    for w, d in D.MADE_UP:
        D.check_arguments(w, d)
    assert np.array_equal(D.check_arguments(np.zeros(15, int), 1), np.zeros((3, 5), int))     # no diffusion is legal


@pytest.mark.parametrize("weights,divisor", [
    (D.KERNELS["jarvis"][0], 0), (D.KERNELS["jarvis"][0], 65), (D.KERNELS["jarvis"][0], 47),
    ([1, 0, 0, 7, 0, 0, 3, 5, 0, 0, 0, 0, 0, 0, 0], 16), ([0, 1, 0, 7, 0, 0, 3, 5, 0, 0, 0, 0, 0, 0, 0], 16),
    ([0, 0, 1, 7, 0, 0, 3, 5, 0, 0, 0, 0, 0, 0, 0], 16)])
def test_the_model_refuses_what_the_contract_refuses(weights, divisor):
    with pytest.raises(ValueError):
        D.check_arguments(weights, divisor)


def test_multiply_and_shift_is_floor_division_over_the_whole_range():
    acc = np.arange(-D.ACC_MAX, D.ACC_MAX + 1, dtype=np.int64)
    for d in range(1, 65):
        bias, mul, shift, bias_q = D.floor_div_constants(d)
        assert bias == bias_q * d and bias >= D.ACC_MAX
        biased = acc + bias
        # the widths the kernel computes in: a 24-bit by 24-bit multiply whose product fits 32 bits unsigned
        assert biased.min() >= 0 and biased.max() < 1 << 15 and 0 < mul < 1 << 24 and int(biased.max()) * mul < 1 << 32, d
        assert np.array_equal(((biased * mul) >> shift) - bias_q, np.floor_divide(acc, d)), d
        assert np.array_equal(D.floor_div(acc, d), np.floor_divide(acc, d)), d


def test_dhgr_without_weights_is_the_conversion_without_dither(O):
    pal, frames = palette(O, "ntsc"), frames_of(O, "ntsc")
    for divisor in (1, 64):
        main, aux = D.frames_to_memory_maps(M.DHGR, pal, frames, np.zeros((3, 5), int), divisor)
        em, ea = M.frames_to_memory_maps(M.DHGR, pal, frames, 0)
        assert (main == em).all() and (aux == ea).all()


def test_the_kernels_differ_from_one_another(O):
    """nine names, nine pictures: no two kernels of the table give the same bytes on the gradient"""
    pal, frame = palette(O, "ntsc"), frames_of(O, "ntsc")[3:4]
    seen = {}
    for name, (w, d) in D.KERNELS.items():
        main, aux = D.frames_to_memory_maps(M.DHGR, pal, frame, w, d)
        key = main.tobytes() + aux.tobytes()
        assert key not in seen, (name, seen[key])
        seen[key] = name
