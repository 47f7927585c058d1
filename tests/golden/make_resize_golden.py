"""Writes tests/golden/g9_resize.npz: a few small frames and what the installed Pillow's Image.resize(..., LANCZOS) makes
of them (frame_grabber.py:75,100), so that the GPU tests can hold the device to Pillow itself on a machine without Pillow.

    python tests/golden/make_resize_golden.py
"""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(120, 160, 192, 280), (37, 53, 24, 35), (401, 4, 17, 9), (400, 4, 17, 9), (5, 7, 3, 2), (90, 300, 192, 280)]


def frame(h, w, seed):
    """a gradient with noise and hard edges: ringing, clamping at 0 and 255, and incompressible enough to matter"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x // 7 + y // 5) % 2) * 255], -1)
    return np.clip(base + rng.randint(-40, 41, size=(h, w, 3)), 0, 255).astype(np.uint8)


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for i, (h, w, H, W) in enumerate(CASES):
        src = frame(h, w, i)
        out["src_%d" % i] = src
        out["dst_%d" % i] = np.asarray(Image.fromarray(src).resize((W, H), resample=Image.LANCZOS))
    np.savez_compressed(os.path.join(HERE, "g9_resize.npz"), **out)


if __name__ == "__main__":
    main()
