"""CPU: the host arithmetic the four frame converters share (ii-vision_amd/csrc/iiv_frontend.h): the screen's row offsets,
the ordered-dither offsets and the palette's linear forms.  That part of the header is plain C++ (no HIP type), so a
stand-alone program built by the host compiler prints it; what it prints is held to tests/ingest_model.py and to the
formulas of the contract comment in include/iivision.h (colour distance = 2 dr^2 + 4 dg^2 + 3 db^2, ties to the lower value)."""
import os
import subprocess

import numpy as np
import pytest

import ingest_model as M
from test_launch_choice_host import CSRC, _compiler

AMPLITUDES = (0, 1, 15, 16, 17, 128, 255)

PROGRAM = r"""
#include "iiv_frontend.h"
#include <stdio.h>
using namespace iiv;
int main()
{
    for (int y = 0; y < 192; y++) printf("%%d ", y_to_offset(y));
    printf("\n");
    const int amplitudes[] = {%(amplitudes)s};
    for (int a : amplitudes) {
        int32_t d[16];
        dither_offsets(a, d);
        for (int c = 0; c < 16; c++) printf("%%d ", (int)d[c]);
        printf("\n");
    }
    const uint8_t palettes[][48] = {%(palettes)s};
    for (auto &pal : palettes) {
        const PaletteForms p = make_palette_forms(pal);
        const void *rows[] = {p.k, p.a, p.b, p.c, p.bc, p.rgb};
        for (int r = 0; r < 6; r++) {
            for (int c = 0; c < 16; c++) {
                const uint32_t x = ((const uint32_t *)rows[r])[c];
                if (r < 4) printf("%%d ", (int)x);
                else printf("%%u ", (unsigned)x);
            }
            printf("\n");
        }
    }
    return 0;
}
"""


def _palettes():
    import palette
    return [palette.NTSCPalette.rgb_array(), palette.IIGSPalette.rgb_array(), np.full((16, 3), 255, dtype=np.uint8)]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("frontend_host")
    src = tmp / "frontend.cpp"
    pals = ", ".join("{%s}" % ", ".join(str(int(v)) for v in p.reshape(-1)) for p in _palettes())
    src.write_text(PROGRAM % dict(amplitudes=", ".join(map(str, AMPLITUDES)), palettes=pals))
    exe = tmp / "frontend"
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    rows = [np.array(line.split(), dtype=np.int64) for line in lines]
    assert len(rows) == 1 + len(AMPLITUDES) + 6 * 3
    return rows


def test_row_offsets_are_the_models_and_stay_out_of_the_holes(printed):
    off = printed[0]
    assert off.tolist() == [M.y_to_offset(y) for y in range(192)]
    assert len(set(off.tolist())) == 192
    assert off.min() >= 0 and (off + 39).max() < 8192
    for end in (off, off + 39):                       # a row's 40 bytes lie inside one 128-byte half page, below its hole
        assert ((end & 127) < 120).all()
    assert ((off >> 7) == ((off + 39) >> 7)).all()


def test_dither_offsets_are_the_models(printed):
    for amplitude, got in zip(AMPLITUDES, printed[1:1 + len(AMPLITUDES)]):
        want = M.bayer_offset(amplitude)[:4, :4].reshape(-1)          # index (y & 3) * 4 + (k & 3)
        assert got.tolist() == want.tolist(), amplitude
    assert not printed[1].any()                                       # amplitude 0: no dither


def test_palette_forms_are_the_contracts_formulas(printed):
    for n, pal in enumerate(_palettes()):
        k, a, b, c, bc, rgb = printed[1 + len(AMPLITUDES) + 6 * n:][:6]
        R, G, B = (pal[:, j].astype(np.int64) for j in range(3))
        v = np.arange(16)
        # key_v = 16 (2 (r - R)^2 + 4 (g - G)^2 + 3 (b - B)^2 - (2 r^2 + 4 g^2 + 3 b^2)) + v = k + a r + b g + c b
        assert k.tolist() == (16 * (2 * R * R + 4 * G * G + 3 * B * B) + v).tolist()
        assert a.tolist() == (-16 * 4 * R).tolist()
        assert b.tolist() == (-16 * 8 * G).tolist()
        assert c.tolist() == (-16 * 6 * B).tolist()
        assert rgb.tolist() == (R | G << 8 | B << 16).tolist()
        # the two halves of a bc word, as int16: -128 G and -96 B, without wrap (at the limit palette -32640 and -24480)
        lo = (bc & 0xffff).astype(np.uint16).view(np.int16).astype(np.int64)
        hi = (bc >> 16).astype(np.uint16).view(np.int16).astype(np.int64)
        assert lo.tolist() == (-128 * G).tolist() and hi.tolist() == (-96 * B).tolist()
        # and the forms order the colours as the distance does, ties to the lower value: spot pixels, every colour
        px = np.array([[0, 0, 0], [255, 255, 255], [1, 254, 127], [200, 13, 77]], dtype=np.int64)
        for r, g, bl in px:
            key = k + a * r + b * g + c * bl
            dist = 2 * (r - R) ** 2 + 4 * (g - G) ** 2 + 3 * (bl - B) ** 2
            assert int(np.argmin(key)) == int(np.argmin(dist))
            assert ((key - v) // 16 + (2 * r * r + 4 * g * g + 3 * bl * bl) == dist).all()
    assert (_palettes()[2] == 255).all()
