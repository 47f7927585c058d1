"""Writes tests/golden/g12_fit.npz: what the installed Pillow makes of a few tiny noise frames with
Image.resize((rw, rh), LANCZOS, box=box) pasted at (rx, ry) onto a canvas of the fill colour (include/iivision.h f12), so
that the tests can hold model and device to Pillow itself on a machine without Pillow.  The cases are fit_cases.GOLDEN; noise
does not compress, so of a source only its CRC-32 is kept (fit_cases.source regenerates it from its seed).

    python tests/golden/make_fit_golden.py
"""
import os
import sys
import zlib

import numpy as np
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import fit_cases as FC   # noqa: E402
import fit_model as FM   # noqa: E402


def main():
    out = {"pillow_version": np.array(PIL.__version__), "names": np.array(FC.GOLDEN), "fill": np.array(FC.FILL, np.uint8)}
    for name in FC.GOLDEN:
        _, h, w, box, size, rect = FC.case(name)
        src = FC.source(name)
        out["crc_" + name] = np.array(zlib.crc32(src.tobytes()), np.uint32)
        out["geo_" + name] = np.array(tuple(box) + tuple(size) + tuple(rect), np.float64)
        out["dst_" + name] = FM.pillow_fit(src, tuple(float(np.float32(v)) for v in box), size, rect, FC.FILL)
    np.savez_compressed(os.path.join(HERE, "g12_fit.npz"), **out)


if __name__ == "__main__":
    main()
