"""Frames of a video as Apple II memory maps -- converted on the GPU.

Mirrors the interface of the reference's transcoder/frame_grabber.py: FrameGrabber carries
`video_mode` and `input_frame_rate` (video.Video reads the latter, video.py:31-33) and
`frames()` yields (main, aux) screen.MemoryMap pairs exactly as FileFrameGrabber.frames() does
(frame_grabber.py:56-147), aux being None for HGR.

What differs, and why: the reference decodes with ffmpeg, resizes each frame to 280x192 with
PIL (frame_grabber.py:75,100) and shells out to the external tool /usr/local/bin/bmp2dhr for
the image -> memory-map conversion (frame_grabber.py:78-82,103-108).  Decoding stays out of
scope; the resize runs on the device, byte-exact with Pillow's LANCZOS (csrc/iiv_resize.hip,
ArrayFrameGrabber(..., resize=True)); the conversion itself is row f3 of SURVEY 8f and runs
here as a HIP kernel (csrc/iiv_ingest.hip).  bmp2dhr is not part of the
reference's source, so its output cannot be matched: the conversion is specified in
include/iivision.h (iiv_frames_to_memory_maps) and the tests hold the kernel to it.
"""

from fractions import Fraction
from typing import Iterator, Tuple

import numpy as np

import _iiv_native as native
import palette as palette_mod
import screen
from palette import Palette
from video_mode import VideoMode


# Error-diffusion kernels by name: (3 x 5 weights, divisor) -- weights[dy][dx + 2] is the share, in divisor-ths, of pixel
# (y + dy, k + dx) (include/iivision.h: iiv_frames_to_memory_maps_diffused).  ArrayFrameGrabber(dither=<name>) runs
# csrc/iiv_diffuse.hip with them; dither="diffusion" stays iiv_frames_to_memory_maps' own Floyd-Steinberg kernel.
DIFFUSION_KERNELS = {
    "floyd-steinberg": (((0, 0, 0, 7, 0), (0, 3, 5, 1, 0), (0, 0, 0, 0, 0)), 16),
    "jarvis": (((0, 0, 0, 7, 5), (3, 5, 7, 5, 3), (1, 3, 5, 3, 1)), 48),
    "stucki": (((0, 0, 0, 8, 4), (2, 4, 8, 4, 2), (1, 2, 4, 2, 1)), 42),
    "atkinson": (((0, 0, 0, 1, 1), (0, 1, 1, 1, 0), (0, 0, 1, 0, 0)), 8),       # 6/8 of the error: flat areas stay flat
    "burkes": (((0, 0, 0, 8, 4), (2, 4, 8, 4, 2), (0, 0, 0, 0, 0)), 32),
    "sierra": (((0, 0, 0, 5, 3), (2, 4, 5, 4, 2), (0, 2, 3, 2, 0)), 32),
    "sierra-2": (((0, 0, 0, 4, 3), (1, 2, 3, 2, 1), (0, 0, 0, 0, 0)), 16),
    "sierra-lite": (((0, 0, 0, 2, 0), (0, 1, 1, 0, 0), (0, 0, 0, 0, 0)), 4),
    # bmp2dhr's D9, the dither the reference asks it for (frame_grabber.py:80-82,106-108): its weights AS REMEMBERED from
    # bmp2dhr's source, which is not here to check -- an assumption; no equality with bmp2dhr is claimed
    "buckels": (((0, 0, 0, 2, 1), (0, 1, 2, 1, 0), (0, 0, 1, 0, 0)), 8),
}

# 4:2:0 YCbCr -> RGB by name: (y_off, ky, rv, gu, gv, bu) of include/iivision.h f11 (the one table; native holds it because
# native.resize_frames_yuv420 takes the names too).  ArrayFrameGrabber((y, u, v), ..., resize=True, yuv_matrix=<name or tuple>).
YUV_MATRICES = native.YUV_MATRICES


FITS = ("stretch", "letterbox", "crop")


def _float32(q):
    """the float32 nearest the rational q (ties to even), as a Python float: from q itself, not from its float64 rounding"""
    near = np.float32(float(q))
    best = min((near, np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))),
               key=lambda c: (abs(Fraction(float(c)) - q), c != near))
    return float(best)


def fit_geometry(h, w, H, W, fit, sar=(1, 1)):
    """How an h x w source with pixel aspect ratio sar = (num, den) goes onto the H x W screen -> (box, rect) for
    native.resize_frames(box=, rect=) (include/iivision.h f12).  The full screen is a 4:3 picture whatever H
    and W are (280 and 560 dots across show the same picture), so only the source's display aspect w sar / h against 4:3
    counts.  Rationals throughout; the box is rounded to float32, as Pillow holds it, at the very end.
      "stretch"    the whole frame over the whole screen: the reference's resize((280, 192))
      "letterbox"  the whole frame into a centred rectangle of its own display aspect, as large as fits: the side that does not
                   fill the screen is rounded half up -- a width to the nearest even number, so that no colour pixel (two dots)
                   is split --, at least 1 (a width: 2), and centred with the odd pixel, if any, on the far side
      "crop"       the centred box of display aspect 4:3, as large as fits, over the whole screen
    A source that is 4:3 on display gets the whole frame and the whole screen whatever `fit` is."""
    h, w, H, W = int(h), int(w), int(H), int(W)
    sn, sd = (int(v) for v in sar)
    if fit not in FITS:
        raise ValueError("fit must be one of %s, got %r" % (", ".join(FITS), fit))
    if min(h, w, H, W) < 1 or sn < 1 or sd < 1:
        raise ValueError("sizes and both terms of sar must be positive")
    display = Fraction(w * sn, h * sd)
    screen_aspect = Fraction(4, 3)
    box = (Fraction(0), Fraction(0), Fraction(w), Fraction(h))
    rect = (0, 0, W, H)
    if fit == "letterbox" and display > screen_aspect:     # bars above and below
        rh = max(int(Fraction(H) * screen_aspect / display + Fraction(1, 2)), 1)
        rect = (0, (H - rh) // 2, W, rh)
    elif fit == "letterbox" and display < screen_aspect:   # bars left and right
        rw = min(max(2 * int(Fraction(W) * display / screen_aspect / 2 + Fraction(1, 2)), 2), W)
        rect = ((W - rw) // 2, 0, rw, H)
    elif fit == "crop" and display > screen_aspect:        # the sides go
        bw = Fraction(w) * screen_aspect / display
        box = ((w - bw) / 2, Fraction(0), (w + bw) / 2, Fraction(h))
    elif fit == "crop" and display < screen_aspect:        # top and bottom go
        bh = Fraction(h) * display / screen_aspect
        box = (Fraction(0), (h - bh) / 2, Fraction(w), (h + bh) / 2)
    return tuple(_float32(q) for q in box), rect


LUMA_WEIGHTS = (77, 150, 29)   # Y = (77 R + 150 G + 29 B + 128) >> 8 (include/iivision.h f15)


def levels_lut(black=0, white=255, gamma=1.0, brightness=0, contrast=1.0):
    """uint8 (256,): the table of one channel for native.levels_apply (include/iivision.h f15).
    The linear part, in integers: with D = white - black >= 1, L[v] = clamp(floor((510 (v - black) + D) / (2 D)), 0, 255) --
    255 (v - black) / D rounded half up --, so (0, 255) is the identity, L[black] = 0 and L[white] = 255.
    The result is C[L[v]], C the float64 curve  C[u] = clamp(floor(255 (((u / 255) ** (1 / gamma) - 0.5) contrast + 0.5) +
    brightness + 0.5), 0, 255): gamma (above 1 lifts the mid-tones), contrast about mid-grey, brightness in levels, rounded half
    up.  At gamma = 1, brightness = 0, contrast = 1 the curve is skipped, not evaluated.  Monotone for contrast >= 0.  The curve
    lives here alone: the C ABI takes tables."""
    black, white = int(black), int(white)
    if not 0 <= black < white <= 255:
        raise ValueError("levels need 0 <= black < white <= 255, got (%d, %d)" % (black, white))
    gamma, brightness, contrast = float(gamma), float(brightness), float(contrast)
    if not (gamma > 0 and np.isfinite(gamma) and contrast >= 0 and np.isfinite(contrast) and -255 <= brightness <= 255):
        raise ValueError("levels need gamma > 0, contrast >= 0 and brightness in -255..255")
    d = white - black
    linear = np.clip((510 * (np.arange(256, dtype=np.int64) - black) + d) // (2 * d), 0, 255)
    if gamma == 1.0 and brightness == 0.0 and contrast == 1.0:
        return linear.astype(np.uint8)
    u = np.arange(256, dtype=np.float64) / 255.0
    curve = np.clip(np.floor(255.0 * ((u ** (1.0 / gamma) - 0.5) * contrast + 0.5) + brightness + 0.5), 0, 255).astype(np.uint8)
    return curve[linear]


def saturation_matrix(s256):
    """int16 (3, 3), Q8: the matrix of native.levels_apply that keeps a pixel's luma and scales its distance from grey by
    s256 / 256 (0..1024).  With w = LUMA_WEIGHTS: o_R and o_B = ((256 - s256) w_k + 128) >> 8, o_G = (256 - s256) - o_R - o_B, and
    m[c][k] = o_k + (c == k) s256.  Every row sums to 256, so greys are fixed points; 256 is the identity, 0 is grey."""
    if int(s256) != s256 or not 0 <= int(s256) <= 1024:
        raise ValueError("s256 is an integer in 0..1024, got %r" % (s256,))
    s256 = int(s256)
    o_r, o_b = ((256 - s256) * LUMA_WEIGHTS[0] + 128) >> 8, ((256 - s256) * LUMA_WEIGHTS[2] + 128) >> 8
    o = np.array([o_r, (256 - s256) - o_r - o_b, o_b], np.int64)
    return (o[None, :] + s256 * np.eye(3, dtype=np.int64)).astype(np.int16)


class Levels:
    """What ArrayFrameGrabber(levels=) does to a frame behind the resize and in front of the temporal hold.
    black, white: the points pulled to 0 and 255; gamma, brightness, contrast: levels_lut's curve; saturation: 1.0 leaves the
    colours, 0.0 is grey, up to 4.0 (saturation_matrix(round(256 saturation))).  auto=(lo_ppm, hi_ppm), or True for (5000, 5000):
    black and white come from the clip's own histogram instead -- of Y, or with per_channel=True of R, G and B, one table each --
    summed over frames 0 .. auto_frames - 1 (None: the whole clip)."""

    def __init__(self, black=0, white=255, gamma=1.0, brightness=0, contrast=1.0, saturation=1.0, auto=None, per_channel=False,
                 auto_frames=None):
        levels_lut(black, white, gamma, brightness, contrast)   # (refuses bad values now)
        self.black, self.white = int(black), int(white)
        self.gamma, self.brightness, self.contrast, self.saturation = float(gamma), float(brightness), float(contrast), float(saturation)
        if not 0 <= self.saturation <= 4:
            raise ValueError("saturation is 0..4, got %r" % (saturation,))
        self.s256 = int(np.floor(self.saturation * 256 + 0.5))
        if auto is True:
            auto = native.LEVELS_PPM
        if auto is not None:
            try:
                lo, hi = auto
                if int(lo) != lo or int(hi) != hi or not (0 <= lo <= 500000 and 0 <= hi <= 500000):
                    raise ValueError
                auto = (int(lo), int(hi))
            except (TypeError, ValueError):
                raise ValueError("auto is None or (lo_ppm, hi_ppm), integers in 0..500000, got %r" % (auto,)) from None
            if (self.black, self.white) != (0, 255):
                raise ValueError("auto finds black and white itself: give one or the other")
        elif per_channel or auto_frames is not None:
            raise ValueError("per_channel and auto_frames go with auto")
        if auto_frames is not None and (int(auto_frames) != auto_frames or auto_frames < 1):
            raise ValueError("auto_frames is None or a positive integer")
        self.auto, self.per_channel = auto, bool(per_channel)
        self.auto_frames = None if auto_frames is None else int(auto_frames)


BINOMIAL_TAPS = (16, 64, 96, 64, 16)   # (1, 4, 6, 4, 1) / 16 scaled to 256 (include/iivision.h f16)


def filter_taps(sigma):
    """Five taps of one axis for native.filter_frames (include/iivision.h f16): the Gaussian exp(-k^2 / (2 sigma^2)),
    k = -2..2, scaled to 256 and rounded half up, the centre taking the remainder so that the sum is exactly 256.  sigma == 0 gives
    the identity (0, 0, 256, 0, 0).  The curve lives here alone: the C ABI takes taps."""
    sigma = float(sigma)
    if not (sigma >= 0 and np.isfinite(sigma)):
        raise ValueError("a blur's sigma is a finite number >= 0, got %r" % (sigma,))
    if sigma == 0:
        return (0, 0, 256, 0, 0)
    w = np.exp(-np.arange(-2, 3, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    side = [int(np.floor(256.0 * w[k] / w.sum() + 0.5)) for k in (0, 1)]
    return (side[0], side[1], 256 - 2 * (side[0] + side[1]), side[1], side[0])


def _int_pair(what, pair, hi_a, hi_b):
    try:
        a, b = pair
        if int(a) != a or int(b) != b:
            raise ValueError
        a, b = int(a), int(b)
    except (TypeError, ValueError):
        raise ValueError("%s is two integers, got %r" % (what, pair)) from None
    if not (0 <= a <= hi_a and 0 <= b <= hi_b):
        raise ValueError("%s needs 0..%d and 0..%d, got (%d, %d)" % (what, hi_a, hi_b, a, b))
    return a, b


def filter_gain(denoise=None, sharpen=None):
    """int16 (256,), Q8: the gain table of native.filter_frames over m, the largest channel difference between a pixel and its
    blur (include/iivision.h f16).  denoise=(lo, hi), 0 <= lo <= hi <= 255: -256 for m <= lo (the pixel becomes the blur), -256 +
    floor(256 (m - lo) / (hi - lo + 1)) for lo < m <= hi, 0 above (an edge is left alone).  sharpen=(amount256, threshold),
    amount256 0..1024, threshold 0..255 and at least hi: amount256 for m > threshold (an unsharp mask that stays off the noise).
    Neither: all zero, the identity."""
    g = np.zeros(256, np.int64)
    m = np.arange(256, dtype=np.int64)
    hi = 0
    if denoise is not None:
        lo, hi = _int_pair("denoise=(lo, hi)", denoise, 255, 255)
        if lo > hi:
            raise ValueError("denoise needs lo <= hi, got (%d, %d)" % (lo, hi))
        g = np.where(m <= lo, -256, np.where(m <= hi, -256 + (256 * (m - lo)) // (hi - lo + 1), 0))
    if sharpen is not None:
        amount, threshold = _int_pair("sharpen=(amount256, threshold)", sharpen, 1024, 255)
        if denoise is not None and threshold < hi:
            raise ValueError("sharpen's threshold %d lies below denoise's hi %d" % (threshold, hi))
        g = np.where(m > threshold, amount, g)
    return g.astype(np.int16)


class Spatial:
    """What ArrayFrameGrabber(spatial=) does to a frame behind the levels and in front of the temporal hold.
    blur=(sx, sy): the Gaussian sigmas of the two axes in pixels (filter_taps); None is BINOMIAL_TAPS on both.  denoise, sharpen:
    filter_gain's.  taps_x, taps_y and gain are what native.filter_frames takes."""

    def __init__(self, blur=None, denoise=None, sharpen=None):
        if blur is None:
            self.taps_x = self.taps_y = BINOMIAL_TAPS
        else:
            try:
                sx, sy = blur
            except (TypeError, ValueError):
                raise ValueError("blur is None or (sx, sy), got %r" % (blur,)) from None
            self.taps_x, self.taps_y = filter_taps(sx), filter_taps(sy)
        self.blur, self.denoise, self.sharpen = blur, denoise, sharpen
        self.gain = filter_gain(denoise, sharpen)


class FrameGrabber:
    """frame_grabber.py:18-24."""

    def __init__(self, mode: VideoMode):
        self.video_mode = mode
        self.input_frame_rate = 30

    def frames(self) -> Iterator[Tuple[screen.MemoryMap, screen.MemoryMap]]:
        raise NotImplementedError


def _upload_chroma(torch, u, v):
    """The two chroma planes on the device.  Views of one interleaved array (NV12: v one byte behind u; NV21: in front) go up
    as that array, once, and come back as its two views; anything else as two planar tensors."""
    au, av = u.__array_interface__["data"][0], v.__array_interface__["data"][0]
    if u.size and u.strides == v.strides and u.strides[2] == 2 and abs(au - av) == 1:
        first = u if au < av else v
        uv = np.lib.stride_tricks.as_strided(first, shape=first.shape + (2,), strides=first.strides + (1,))
        d = torch.from_numpy(np.ascontiguousarray(uv)).cuda()
        return (d[..., 0], d[..., 1]) if first is u else (d[..., 1], d[..., 0])
    return torch.from_numpy(np.ascontiguousarray(u)).cuda(), torch.from_numpy(np.ascontiguousarray(v)).cuda()


class ArrayFrameGrabber(FrameGrabber):
    """Frames given as an array (n, 192, 280, 3) uint8 -- what FileFrameGrabber holds after its
    resize -- converted `batch` frames at a time by iiv_frames_to_memory_maps.  With resize=True the
    frames may be any size (n, h, w, 3) (1 <= h, w <= 8192): each is resized to 280x192 on the device
    first, byte for byte as the reference's Image.resize((280, 192), LANCZOS) (frame_grabber.py:75,100).
    palette=Palette.MONO (a monochrome monitor): a frame is one pixel per DOT -- (192, 560) for DHGR,
    (192, 280) for HGR --, resize=True resizes to that size, and the conversion is iiv_frames_to_memory_maps_mono.
    dither: 0..255 = amplitude of the ordered dither; "diffusion" = Floyd-Steinberg (iiv_frames_to_memory_maps); a name of
    DIFFUSION_KERNELS or (3 x 5 weights, divisor) = error diffusion with that kernel (iiv_frames_to_memory_maps_diffused;
    colour palettes only); "direct" = per screen row the bytes whose rendered dots are nearest the frame
    (iiv_frames_to_memory_maps_direct; colour palettes only), `amplitude` 0..255 the ordered dither added to its
    target -- `amplitude` is legal with "direct" alone.
    Frames as a decoder delivers them: a (y, u, v) triple of uint8 arrays, y (n, h, w) and u, v (n, (h + 1) // 2, (w + 1) // 2) --
    planar I420, or uv[..., 0] and uv[..., 1] of an interleaved (n, ch, cw, 2) NV12 array, which is uploaded as it is --, with
    resize=True and yuv_matrix a name of YUV_MATRICES or (y_off, ky, rv, gu, gv, bu): converted inside the device resize
    (iiv_resize_frames_yuv420); frames that already have the target size go through the same call.
    fit, sar, fill (with resize=True; fit_geometry): "stretch" -- the default, the reference's resize and today's
    bytes -- pulls every source over the whole screen; "letterbox" keeps the whole frame and pads the screen with the colour
    fill = (r, g, b); "crop" fills the screen with the frame's centred 4:3 part; sar = the source's pixel aspect ratio (num, den).
    temporal=(lo, hi): the temporal hold (iiv_temporal_hold, include/iivision.h f14) behind the resize and in front of
    every conversion -- a pixel within lo of its held value keeps the held bytes, one more than hi away takes the source's.
    ingest_frames and memory_maps stay functions of their arguments: what they return is the hold run over frames 0 .. first +
    count - 1, of which the last `count` are handed out.  The grabber keeps the held frame behind the last frame it converted and
    goes on from it when `first` is the next frame; otherwise it runs again from frame 0, `batch` frames at a time.
    temporal_counts() gives the pixels held, blended and passed of every frame converted so far.  None (the default) takes none
    of these paths.
    levels=Levels(...): picture levels (iiv_levels_histogram / iiv_levels_apply, include/iivision.h f15) behind the
    resize and in front of the temporal hold: black and white points, gamma, brightness, contrast, saturation.  With Levels(auto=)
    the points come from the clip's own histogram after the resize, computed once at first use, `batch` frames at a time, and
    then fixed, so ingest_frames and memory_maps stay functions of their arguments; levels_report() gives the points and tables
    in use.  None (the default) takes none of these paths and changes no byte.
    spatial=Spatial(...): the spatial filter (iiv_filter_frames, include/iivision.h f16) behind the levels and in
    front of the temporal hold: an edge-keeping denoise, an unsharp mask, or both.  Stateless per frame, so ingest_frames and
    memory_maps stay functions of their arguments.  None (the default) takes none of these paths and changes no byte."""

    def __init__(self, frames_rgb, mode: VideoMode, palette: Palette = Palette.NTSC, dither=32,
                 input_frame_rate: float = 30, batch: int = 256, resize: bool = False, amplitude: int = 0, yuv_matrix="bt601",
                 fit: str = "stretch", sar=(1, 1), fill=(0, 0, 0), temporal=None, levels=None, spatial=None):
        super().__init__(mode)
        if spatial is not None and not isinstance(spatial, Spatial):
            raise ValueError("spatial is None or a frame_grabber.Spatial, got %r" % (spatial,))
        self.spatial = spatial
        if levels is not None and not isinstance(levels, Levels):
            raise ValueError("levels is None or a frame_grabber.Levels, got %r" % (levels,))
        self.levels = levels
        self._levels_tables = None   # (report, lut (3, 256), matrix (3, 3)) once computed
        self.temporal = None if temporal is None else native.temporal_pair(temporal)
        self._held, self._held_next, self._held_counts = None, 0, []   # the held frame behind frame _held_next - 1, counts per call
        if fit not in FITS:
            raise ValueError("fit must be one of %s, got %r" % (", ".join(FITS), fit))
        if fit != "stretch" and not resize:
            raise ValueError("fit=%r is the device resize's: pass resize=True" % (fit,))
        self._yuv = None
        if isinstance(frames_rgb, tuple) and len(frames_rgb) == 3:
            if not resize:
                raise ValueError("(y, u, v) frames are converted inside the device resize: pass resize=True")
            y, u, v = (np.asarray(p) for p in frames_rgb)
            if y.dtype != np.uint8 or y.ndim != 3 or u.dtype != np.uint8 or v.dtype != np.uint8:
                raise ValueError("(y, u, v) frames must be uint8, y (n, h, w)")
            chroma = (y.shape[0], (y.shape[1] + 1) // 2, (y.shape[2] + 1) // 2)
            if u.shape != chroma or v.shape != chroma:
                raise ValueError("u and v have shapes %s and %s; y %s needs chroma planes %s" % (u.shape, v.shape, y.shape, chroma))
            self._yuv = (y, u, v)
            self._matrix = native.yuv_matrix(yuv_matrix)
            rgb = y   # (len() and the batching read the frame count from it)
        else:
            rgb = np.asarray(frames_rgb)
        mode_id = native.DHGR if mode == VideoMode.DHGR else native.HGR
        self.frame_size = native.MONO_SIZE[mode_id] if palette == Palette.MONO else native.RESIZE_SIZE   # (H, W)
        if self._yuv is not None:
            pass   # (checked above)
        elif resize:
            if rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[3] != 3:
                raise ValueError("frames must be uint8 (n, h, w, 3) RGB")
        elif rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[1:] != self.frame_size + (3,):
            raise ValueError("frames must be uint8 (n, %d, %d, 3)%s" % (self.frame_size + (
                " (one pixel per dot of a monochrome screen)" if palette == Palette.MONO else " (frame_grabber.py:75: 280x192 RGB)",)))
        self._rgb = rgb
        self.resize = bool(resize)
        self.fit = fit
        # (box, rect, fill) for the resize, or {} where the plain stretch does it
        self._fit = {}
        if fit != "stretch":
            box, rect = fit_geometry(rgb.shape[1], rgb.shape[2], self.frame_size[0], self.frame_size[1], fit, sar)
            native.fit_args(rgb.shape[1], rgb.shape[2], self.frame_size[0], self.frame_size[1], box, rect, fill)   # (refuses a bad fill now)
            self._fit = dict(box=box, rect=rect, fill=tuple(int(c) for c in fill))
        self.palette = palette
        # 0..255: amplitude of the 4x4 ordered dither; "diffusion" (= native.DITHER_DIFFUSION): Floyd-Steinberg error
        # diffusion, the kind of dither the reference asks bmp2dhr for (D9, frame_grabber.py:80-82,106-108)
        # a name of DIFFUSION_KERNELS, or (3 x 5 weights, divisor): error diffusion with that kernel (csrc/iiv_diffuse.hip)
        self.diffusion_kernel = None
        self.direct = dither == "direct"
        if not self.direct and amplitude != 0:
            raise ValueError("amplitude goes with dither=\"direct\" alone (an ordered dither's amplitude is `dither` itself)")
        if self.direct:
            if palette == Palette.MONO:
                raise ValueError("Palette.MONO shows dots, not windows: dither=\"direct\" is the colour conversion's")
            if not 0 <= int(amplitude) <= 255:
                raise ValueError("amplitude must be 0..255")
            dither = int(amplitude)
        if isinstance(dither, str) and dither != "diffusion":
            if dither not in DIFFUSION_KERNELS:
                raise ValueError("dither: unknown diffusion kernel %r (one of %s, or \"diffusion\")" % (dither, ", ".join(sorted(DIFFUSION_KERNELS))))
            self.diffusion_kernel = DIFFUSION_KERNELS[dither]
        elif isinstance(dither, (tuple, list)):
            if len(dither) != 2:
                raise ValueError("dither: a diffusion kernel is (3 x 5 weights, divisor)")
            self.diffusion_kernel = (dither[0], int(dither[1]))
        if self.diffusion_kernel is not None and palette == Palette.MONO:
            raise ValueError("Palette.MONO converts with dither=\"diffusion\" or an ordered amplitude: the diffusion kernels are the colour conversion's")
        self.dither = native.DITHER_DIFFUSION if dither == "diffusion" or self.diffusion_kernel is not None else int(dither)
        self.input_frame_rate = input_frame_rate
        self.batch = int(batch)

    def ingest_frames(self, first=0, count=None):
        """CUDA uint8 (count, H, W, 3): frames first .. first + count - 1 as the conversion takes them, after any resize, the
        levels, the spatial filter and the temporal hold -- the reference picture screen.render_error measures a screen against."""
        count = len(self._rgb) - first if count is None else count
        if self.temporal is None or count <= 0:
            return self._filtered_frames(first, count)
        if self._held is None or first != self._held_next:
            # not the next frame: the hold again from frame 0, a batch at a time, up to the frame in front of `first`
            self._held, self._held_next, self._held_counts = None, 0, []
            while self._held_next < first:
                self._hold(self._held_next, min(max(self.batch, 1), first - self._held_next))
        return self._hold(first, count)

    def _hold(self, first, count):
        """frames first .. first + count - 1 through the hold, from the state behind frame first - 1"""
        out, self._held, counts = native.temporal_hold(self._filtered_frames(first, count), *self.temporal, state=self._held, counts=True)
        self._held_next = first + count
        self._held_counts.append(counts)
        return out

    def temporal_counts(self):
        """numpy uint32 (frames converted so far, 3): the pixels held, blended and passed of frames 0 .. n - 1 of the run of the
        hold that the grabber's state belongs to (a call out of order starts that run again)."""
        if self.temporal is None:
            raise ValueError("temporal_counts() goes with temporal=(lo, hi)")
        if not self._held_counts:
            return np.zeros((0, 3), np.uint32)
        return np.concatenate([c.cpu().numpy() for c in self._held_counts]).view(np.uint32)

    def levels_report(self):
        """The levels in use: {"black", "white"} -- ints, or with per_channel three each --, the parameters of the Levels, and
        "lut" uint8 (3, 256) and "matrix" int16 (3, 3) as native.levels_apply takes them.  With Levels(auto=) the first call (or
        the first frame asked for) reads frames 0 .. auto_frames - 1 and fixes the points."""
        if self.levels is None:
            raise ValueError("levels_report() goes with levels=Levels(...)")
        if self._levels_tables is None:
            lv = self.levels
            points = [(lv.black, lv.white)] * 3
            if lv.auto is not None:
                n = len(self._rgb) if lv.auto_frames is None else min(lv.auto_frames, len(self._rgb))
                total = np.zeros((4, 256), np.int64)
                for first in range(0, n, max(self.batch, 1)):
                    hist = native.levels_histogram(self._source_frames(first, min(max(self.batch, 1), n - first)))
                    total += hist.long().sum(dim=0).cpu().numpy()   # (a count of 280x192 or 560x192 is far below 2^31)
                if lv.per_channel:
                    points = [native.levels_auto(total[c], *lv.auto) for c in range(3)]
                else:
                    points = [native.levels_auto(total[3], *lv.auto)] * 3
            lut = np.stack([levels_lut(b, w, lv.gamma, lv.brightness, lv.contrast) for b, w in points])
            per = lv.per_channel and lv.auto is not None
            report = {"black": [p[0] for p in points] if per else points[0][0], "white": [p[1] for p in points] if per else points[0][1],
                      "gamma": lv.gamma, "brightness": lv.brightness, "contrast": lv.contrast, "saturation": lv.saturation,
                      "auto": list(lv.auto) if lv.auto is not None else None, "per_channel": lv.per_channel, "auto_frames": lv.auto_frames}
            self._levels_tables = (report, lut, saturation_matrix(lv.s256))
        report, lut, matrix = self._levels_tables
        return dict(report, lut=lut.copy(), matrix=matrix.copy())

    def _filtered_frames(self, first, count):
        """frames first .. first + count - 1 after any resize, the levels and the spatial filter, in front of the hold"""
        frames = self._levelled_frames(first, count)
        if self.spatial is None or count <= 0:
            return frames
        return native.filter_frames(frames, self.spatial.taps_x, self.spatial.taps_y, self.spatial.gain)   # (out of place: a halo)

    def _levelled_frames(self, first, count):
        """frames first .. first + count - 1 after any resize and the levels, in front of the filter and the hold"""
        frames = self._source_frames(first, count)
        if self.levels is None or count <= 0:
            return frames
        if self._levels_tables is None:
            self.levels_report()
        _, lut, matrix = self._levels_tables
        return native.levels_apply(frames, lut, matrix.astype(np.int64), out=frames)   # (a tensor of this call's own: in place)

    def _source_frames(self, first, count):
        """frames first .. first + count - 1 after any resize, in front of the levels and the hold"""
        import torch
        if self._yuv is not None:
            y, u, v = (p[first:first + count] for p in self._yuv)
            d_u, d_v = _upload_chroma(torch, u, v)
            return native.resize_frames_yuv420(torch.from_numpy(np.ascontiguousarray(y)).cuda(), d_u, d_v, size=self.frame_size,
                                               matrix=self._matrix, **self._fit)
        rgb = torch.from_numpy(np.ascontiguousarray(self._rgb[first:first + count])).cuda()
        if self.resize and (self._fit or tuple(rgb.shape[1:3]) != self.frame_size):
            rgb = native.resize_frames(rgb, size=self.frame_size, **self._fit)   # on the same stream as the conversion behind it
        return rgb

    def memory_maps(self, first=0, count=None):
        """(main, aux) CUDA uint8 tensors (count, 32, 256) of frames first .. first + count - 1:
        the form stream_batch.StreamBatch consumes, without a trip through host memory maps."""
        rgb = self.ingest_frames(first, count)
        mode = native.DHGR if self.video_mode == VideoMode.DHGR else native.HGR
        if self.palette == Palette.MONO:
            return native.frames_to_memory_maps_mono(mode, rgb, self.dither)
        pal = palette_mod.PALETTES[self.palette].rgb_array()
        if self.direct:
            return native.frames_to_memory_maps_direct(mode, pal, rgb, self.dither)
        if self.diffusion_kernel is not None:
            return native.frames_to_memory_maps_diffused(mode, pal, rgb, *self.diffusion_kernel)
        return native.frames_to_memory_maps(mode, pal, rgb, self.dither)

    def frames(self):
        for first in range(0, len(self._rgb), self.batch):
            main, aux = self.memory_maps(first, min(self.batch, len(self._rgb) - first))
            main = main.cpu().numpy()
            aux = aux.cpu().numpy() if aux is not None else None
            for i in range(main.shape[0]):
                yield (screen.MemoryMap(screen_page=1, page_offset=main[i].copy()),
                       screen.MemoryMap(screen_page=1, page_offset=aux[i].copy()) if aux is not None else None)
