"""RGB palettes for rendering NominalColour pixels (mirrors transcoder/palette.py).

The reference stores colormath sRGBColor objects; colormath is not a dependency
here (the CIE2000 arithmetic runs on the GPU, csrc/iiv_tables.hip), so RGB is a
small value class with the attributes the reference's users touch.
"""

import enum
from typing import Dict, Type

import numpy as np

from colours import HGRColours


class RGB:
    """8-bit sRGB triple; rgb_r/g/b are the 0..1 floats colormath would hold."""

    __slots__ = ("r", "g", "b")

    def __init__(self, r, g, b):
        self.r, self.g, self.b = int(r), int(g), int(b)

    rgb_r = property(lambda self: self.r / 255.0)
    rgb_g = property(lambda self: self.g / 255.0)
    rgb_b = property(lambda self: self.b / 255.0)

    def get_upscaled_value_tuple(self):
        return (self.r, self.g, self.b)

    def __repr__(self):
        return "RGB(%d, %d, %d)" % (self.r, self.g, self.b)


def rgb(r, g, b):
    return RGB(r, g, b)


class Palette(enum.Enum):
    """BMP2DHR palette numbers (palette.py:18-23)."""
    UNKNOWN = -1
    IIGS = 0
    NTSC = 5
    MONO = 100   # a monochrome monitor: not a BMP2DHR palette number (MonoPalette below)


class BasePalette:
    ID = Palette.UNKNOWN  # type: Palette
    RGB = {}  # type: Dict[HGRColours, RGB]

    @classmethod
    def rgb_array(cls) -> np.ndarray:
        """(16, 3) uint8, row i = colour whose HGRColours value is i."""
        out = np.zeros((16, 3), dtype=np.uint8)
        for colour, v in cls.RGB.items():
            out[colour.value] = v.get_upscaled_value_tuple()
        return out


def _table(rows):
    names = ("BLACK", "MAGENTA", "BROWN", "ORANGE", "DARK_GREEN", "GREY1", "GREEN", "YELLOW",
             "DARK_BLUE", "VIOLET", "GREY2", "PINK", "MED_BLUE", "LIGHT_BLUE", "AQUA", "WHITE")
    return {HGRColours[n]: rgb(*v) for n, v in zip(names, rows)}


class NTSCPalette(BasePalette):
    """BMP2DHGR's default NTSC palette (palette.py:33-54)."""
    ID = Palette.NTSC
    RGB = _table(((0, 0, 0), (148, 12, 125), (99, 77, 0), (249, 86, 29), (51, 111, 0), (126, 126, 126),
                  (67, 200, 0), (221, 206, 23), (32, 54, 212), (188, 55, 255), (126, 126, 126),
                  (255, 129, 236), (7, 168, 225), (158, 172, 255), (93, 248, 133), (255, 255, 255)))


class IIGSPalette(BasePalette):
    """BMP2DHGR's KEGS32 palette (palette.py:57-78)."""
    ID = Palette.IIGS
    RGB = _table(((0, 0, 0), (221, 0, 51), (136, 85, 34), (255, 102, 0), (0, 119, 0), (85, 85, 85),
                  (0, 221, 0), (255, 255, 0), (0, 0, 153), (221, 0, 221), (170, 170, 170),
                  (255, 153, 136), (34, 34, 255), (102, 170, 255), (0, 255, 153), (255, 255, 255)))


def _popcount4(v):
    return (v & 1) + ((v >> 1) & 1) + ((v >> 2) & 1) + ((v >> 3) & 1)


class MonoPalette(BasePalette):
    """A monochrome monitor (the reference README's "mono playback mode").  A colour value of the sliding-window model
    is four dots, bit k the dot at screen position = k mod 4 (colours.py:100-134); a mono screen shows the dots
    themselves, so what a change of colour value costs is the dots it changes -- diff_matrix() -- and no RGB
    distance.  RGB is the grey of the lit share of the four dots, for display only."""
    ID = Palette.MONO
    RGB = {c: rgb(*(3 * ((255 * _popcount4(c.value) + 2) // 4,))) for c in HGRColours}

    @classmethod
    def diff_matrix(cls) -> np.ndarray:
        """(16, 16) int32: dm[a][b] = 16 |popcount(a) - popcount(b)| + 8 popcount(a ^ b): how many dots are lit, and
        which.  A metric; the smallest off-diagonal entry is 16, which keeps the reference's regime "a transpose (cost 1)
        is always cheaper than a substitution" (make_data_tables.py:38-41); the largest is 96, and 96 x MASKED_DOTS
        stays inside the 2047 iiv_encoder_create demands."""
        a = np.arange(16)[:, None]
        b = np.arange(16)[None, :]
        return (16 * np.abs(_popcount4(a) - _popcount4(b)) + 8 * _popcount4(a ^ b)).astype(np.int32)


# (exactly the reference's two: make_data_tables.main() writes one pair of files per entry)
PALETTES = {
    Palette.IIGS: IIGSPalette,
    Palette.NTSC: NTSCPalette
}  # type: Dict[Palette, Type[BasePalette]]


def palette_class(palette_id: Palette) -> Type[BasePalette]:
    """The palette class of an id, MONO included (PALETTES holds only the reference's colour palettes)."""
    if palette_id == Palette.MONO:
        return MonoPalette
    return PALETTES[palette_id]


def diff_matrix(palette_id: Palette) -> np.ndarray:
    """The (16, 16) int32 substitution-cost matrix of a palette: CIE2000 between its colours (on the device), or the
    mono dot distance."""
    if palette_id == Palette.MONO:
        return MonoPalette.diff_matrix()
    import make_data_tables
    return make_data_tables.compute_diff_matrix(PALETTES[palette_id])
