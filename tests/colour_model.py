"""The colour-difference front end at high precision: what iiv_cie2000_matrix and iiv_delta_e_cie2000 (csrc/iiv_tables.hip) and
the host oracle (oracle/iiv_oracle.c) are held to.

A restatement of colormath 3.0.0 as include/iivision.h and make_data_tables.py:55-70 describe it -- sRGBColor (upscaled bytes)
-> XYZ -> Lab with D65 / 2 degrees and no chromatic adaptation, then delta_e_cie2000 with Kl = Kc = Kh = 1, then int() --
evaluated in mpmath at 50 digits, or in numpy.longdouble (64-bit mantissa) where mpmath does not import.  Every input is the
double (or byte) the device receives, converted exactly; every constant is the double colormath holds (0.04045, 12.92, 2.4,
1.0 / 3.0, the matrix, the white point ...), converted exactly; pi is the backend's own.

    sRGB -> linear   v = byte / 255;  v <= 0.04045 ? v / 12.92 : ((v + 0.055) / 1.055) ** 2.4
    linear -> XYZ    colormath's low-precision sRGB matrix (its rows do not sum to the white point: a grey has a small chroma
                     of its own, hue about 266.6 degrees, black alone has none); a negative sum is clamped to 0
    XYZ -> Lab       t = X / Xn;  t > 216 / 24389 ? t ** (1 / 3) : 7.787 t + 16 / 116;  white (0.95047, 1, 1.08883)
    delta-E 2000     colormath's numpy form, quirks kept: h' = degrees(atan2(b, a')) + 360 (h' < 0), with atan2(0, 0) = 0;
                     the mean hue adds 360 whenever |h1' - h2'| > 180 -- also where the sum is already 360 or more -- so the
                     mean is not taken modulo 360 and the rotation term exp(-((mean - 275) / 25) ** 2) is not periodic;
                     delta-h' has 720 taken off where h2' > h1', which sin(delta-h' / 2) does not see
    int()            floor, the values being >= 0

Where the formula jumps.  The result is discontinuous in the inputs where |h1' - h2'| = 180 (the mean hue moves by 180) and,
because of the non-periodic mean, where a colour's h' crosses 0 / 360.  margins() returns the distances to these, in degrees.
With either chroma zero no hue term reaches the result at all.  The comparison |h1' - h2'| > 180 is decided here as exact
arithmetic decides it: a hue difference within `tie` degrees of 180 is 180, and 180 is not > 180 (at 50 digits `tie` is 1e-30:
180 pi / pi is 180 only to the last digit or so).  Two families of double inputs lie exactly on that edge, and for them this is
the required value:
    exact-axis pairs  every colour has a == 0 or b == 0: atan2 returns 0, pi / 2, pi or -pi / 2 in any libm, and
                      degrees() of those is 0, 90, 180, -90 exactly in IEEE double
    antipodal pairs   (a2, b2) == (-a1, -b1): the hues differ by exactly 180, 180 is not > 180.  In double this holds only if
                      the two atan2 calls round alike; rows 10 and 14 of Sharma's table are such pairs, and the published
                      values are those of exact arithmetic

Measured (tests/test_colour_model.py prints it): over the committed case set of tests/colour_cases.py -- 18 palettes, 1000
Lab pairs -- and the committed rounds of tests/stage_fuzz.py's colour stage, the largest |oracle - model| is 2.899e-12,
recorded as E_HOST = 2.9e-12.  It is IIGS's (NTSC: 2.0e-12, the cube's corners 6.6e-13), and it is double rounding, not libm: a
grey has a = 500 (fx - fy) of about 1e-3 with an absolute error of some 5e-14, so a hue good to 1e-10 radians or so, which
sqrt(C1' C2') of about 1 against a saturated colour carries into delta-H'.  Every other palette and every Lab pair, whose
inputs are doubles already, stays below 1.5e-13.  T = 8 E_HOST = 2.32e-11 is what the device is held to: glibc's pow, atan2,
cos, exp and sqrt are within 1 ulp, the device library is allowed a few, about ten such calls feed one value.

Measured on an MI355X (tests/test_gpu_colour.py prints it): the largest |device - model| is 6.84e-12, IIGS's again (NTSC
1.95e-12, the cube's corners 6.7e-13, every other palette below 1.5e-13, the Lab pairs 1.4e-13 at most): inside T by a factor
of three, and every integer equal.
"""
import numpy as np

try:
    import mpmath
    BACKEND = "mpmath"
except ImportError:                                   # pragma: no cover  (mpmath is there wherever the suite runs today)
    mpmath = None
    BACKEND = "longdouble"

DIGITS = 50
E_HOST = 2.9e-12              # the largest |oracle - model| over the committed cases, measured (see above)
T = min(8 * E_HOST, 1e-9)     # the device's bound, absolute, never above the bound the device-vs-oracle tests already hold

# colormath's constants, as the doubles it holds
_M = ((0.412424, 0.357579, 0.180464), (0.212656, 0.715158, 0.0721856), (0.0193324, 0.119193, 0.950444))
_WHITE = (0.95047, 1.00000, 1.08883)


class _Mp:
    """mpmath at DIGITS digits"""
    name = "mpmath"
    tie = 1e-30

    def __init__(self):
        self.ctx = mpmath.mp.clone()
        self.ctx.dps = DIGITS
        c = self.ctx
        self.sqrt, self.cos, self.sin, self.exp, self.atan2, self.pi = c.sqrt, c.cos, c.sin, c.exp, c.atan2, +c.pi

    def f(self, x):
        return self.ctx.mpf(float(x))                 # a double, exactly

    def power(self, x, y):
        return self.ctx.power(x, y)

    def floor(self, x):
        return int(self.ctx.floor(x))


class _Ld:
    """numpy.longdouble: the x87 80-bit format where there is one"""
    name = "longdouble"
    tie = 1e-13

    def __init__(self):
        L = np.longdouble
        self.sqrt, self.cos, self.sin, self.exp, self.atan2 = np.sqrt, np.cos, np.sin, np.exp, np.arctan2
        self.pi = 4 * np.arctan(L(1))

    def f(self, x):
        return np.longdouble(float(x))

    def power(self, x, y):
        return np.power(np.longdouble(x), np.longdouble(y))

    def floor(self, x):
        return int(np.floor(x))


_backends = {}


def backend(name=None):
    name = name or BACKEND
    if name not in _backends:
        _backends[name] = {"mpmath": _Mp, "longdouble": _Ld}[name]()
    return _backends[name]


def lab(rgb, be=None):
    """three bytes -> (L, a, b) in the backend's numbers"""
    B = be or backend()
    f = B.f
    lin = []
    for byte in rgb:
        v = f(int(byte)) / f(255.0)
        lin.append(v / f(12.92) if v <= f(0.04045) else B.power((v + f(0.055)) / f(1.055), f(2.4)))
    t = []
    for row, white in zip(_M, _WHITE):
        s = f(row[0]) * lin[0] + f(row[1]) * lin[1] + f(row[2]) * lin[2]
        if s < 0:
            s = f(0.0)
        v = s / f(white)
        t.append(B.power(v, f(1.0 / 3.0)) if v > f(216.0) / f(24389.0) else f(7.787) * v + f(16.0) / f(116.0))
    return (f(116.0) * t[1] - f(16.0), f(500.0) * (t[0] - t[1]), f(200.0) * (t[1] - t[2]))


def lab_double(rgb, be=None):
    """lab() rounded to the doubles a caller would hand to iiv_delta_e_cie2000"""
    return tuple(float(v) for v in lab(rgb, be))


def _hue(B, b, ap):
    """h' in degrees in [0, 360]: degrees(atan2(b, a')), 360 added below 0; atan2(0, 0) = 0"""
    if b == 0 and ap == 0:
        return B.f(0.0)
    h = B.atan2(b, ap) * 180 / B.pi
    return h + 360 if h < 0 else h


def _terms(lab1, lab2, B):
    f = B.f
    L1, a1, b1 = (f(v) if isinstance(v, (float, int)) else v for v in lab1)       # doubles come in exactly; lab()'s own numbers as they are
    L2, a2, b2 = (f(v) if isinstance(v, (float, int)) else v for v in lab2)
    C1, C2 = B.sqrt(a1 * a1 + b1 * b1), B.sqrt(a2 * a2 + b2 * b2)
    avg_C = (C1 + C2) / 2
    c7 = avg_C ** 7
    G = (1 - B.sqrt(c7 / (c7 + f(25.0) ** 7))) / 2
    a1p, a2p = (1 + G) * a1, (1 + G) * a2
    C1p, C2p = B.sqrt(a1p * a1p + b1 * b1), B.sqrt(a2p * a2p + b2 * b2)
    h1p, h2p = _hue(B, b1, a1p), _hue(B, b2, a2p)
    return L1, L2, C1p, C2p, h1p, h2p


def _apart(B, h1p, h2p):
    """|h1' - h2'| > 180, a difference within B.tie of 180 being 180"""
    return abs(h1p - h2p) - 180 >= B.tie


def delta_e(lab1, lab2, be=None):
    """colormath 3.0.0's delta_e_cie2000(lab1, lab2, Kl=1, Kc=1, Kh=1)"""
    B = be or backend()
    f = B.f
    L1, L2, C1p, C2p, h1p, h2p = _terms(lab1, lab2, B)
    rad = B.pi / 180
    avg_Lp = (L1 + L2) / 2
    avg_Cp = (C1p + C2p) / 2
    apart = _apart(B, h1p, h2p)
    avg_Hp = ((360 if apart else 0) + h1p + h2p) / 2                  # always-add-360: no "unless the sum is >= 360"
    T_ = (1 - f(0.17) * B.cos((avg_Hp - 30) * rad) + f(0.24) * B.cos(2 * avg_Hp * rad) + f(0.32) * B.cos((3 * avg_Hp + 6) * rad)
          - f(0.2) * B.cos((4 * avg_Hp - 63) * rad))
    delta_hp = h2p - h1p + (360 if apart else 0)
    if h2p > h1p:
        delta_hp = delta_hp - 720
    dLp, dCp = L2 - L1, C2p - C1p
    dHp = 2 * B.sqrt(C2p * C1p) * B.sin(delta_hp * rad / 2)
    l50 = (avg_Lp - 50) ** 2
    S_L = 1 + f(0.015) * l50 / B.sqrt(20 + l50)
    S_C = 1 + f(0.045) * avg_Cp
    S_H = 1 + f(0.015) * avg_Cp * T_
    d_ro = 30 * B.exp(-(((avg_Hp - 275) / 25) ** 2))
    c7 = avg_Cp ** 7
    R_C = B.sqrt(c7 / (c7 + f(25.0) ** 7))
    R_T = -2 * R_C * B.sin(2 * d_ro * rad)
    s = (dLp / S_L) ** 2 + (dCp / S_C) ** 2 + (dHp / S_H) ** 2 + R_T * (dCp / S_C) * (dHp / S_H)
    return B.sqrt(s)


def matrix(palette, be=None):
    """16 x 3 bytes -> (the 16 x 16 delta-E matrix as an object array of the backend's numbers, its floor as int32): the Lab
    values go on at full precision, as colormath keeps them in doubles without a detour"""
    B = be or backend()
    pal = np.asarray(palette).reshape(16, 3)
    labs = [lab(row, B) for row in pal]
    f = np.empty((16, 16), dtype=object)
    for i in range(16):
        for j in range(16):
            f[i, j] = delta_e(labs[i], labs[j], B)
    return f, np.array([[B.floor(v) for v in row] for row in f], dtype=np.int32)


def as_float(a):
    """an array (or one) of the backend's numbers rounded to doubles"""
    a = np.asarray(a, dtype=object)
    return np.array([float(v) for v in a.reshape(-1)], dtype=np.float64).reshape(a.shape)


def margin_terms(lab1, lab2, be=None):
    """(||h1' - h2'| - 180|, min(h1', 360 - h1') or None, min(h2', 360 - h2') or None) in degrees: None where the chroma is zero"""
    B = be or backend()
    _, _, C1p, C2p, h1p, h2p = _terms(lab1, lab2, B)
    return (float(abs(abs(h1p - h2p) - 180)),) + tuple(float(min(h, 360 - h)) if C != 0 else None for C, h in ((C1p, h1p), (C2p, h2p)))


def margins(lab1, lab2, be=None):
    """distances in degrees to the formula's discontinuities: ||h1' - h2'| - 180|, then min(h', 360 - h') of each colour whose
    chroma is not zero"""
    return [m for m in margin_terms(lab1, lab2, be) if m is not None]


def on_axis(lab_):
    """a == 0 or b == 0 (a signed zero is a zero): atan2 is exact, h' is 0, 90, 180 or 270 exactly"""
    return float(lab_[1]) == 0 or float(lab_[2]) == 0


def exact_axis(lab1, lab2):
    """every colour of the pair has a == 0 or b == 0 (a signed zero is a zero)"""
    return on_axis(lab1) and on_axis(lab2)


def antipodal(lab1, lab2):
    """(a2, b2) == (-a1, -b1), off the axes' origin: h2' = h1' +- 180 in exact arithmetic, whatever G is"""
    return float(lab2[1]) == -float(lab1[1]) and float(lab2[2]) == -float(lab1[2]) and (float(lab1[1]) != 0 or float(lab1[2]) != 0)
