"""CPU: what the clip stages share on the host (ii-vision_amd/csrc/iiv_clip.h): the refusals of iiv_temporal_hold,
iiv_levels_histogram and iiv_levels_apply, and the cut of a clip into lanes, runs and a capped grid.  That part of the header is
plain C++ (no HIP type), so a stand-alone program built by the host compiler, with a set_error of its own that prints code and
message, runs it over a fixed list of cases; what it prints is held to expectations written out here.  (The GPU tests of f14 and
f15 only ever see the binding's ValueErrors, which fire first: this is where the C side's refusals are met.)"""
import subprocess

import pytest

import levels_cases as LC
import temporal_cases as TC
from test_launch_choice_host import CSRC, _compiler

INVALID = -1                       # IIV_ERR_INVALID (include/iivision.h)
NAME = "iiv_some_clip_stage"
CEILINGS = (31, 40)                # the histogram's (a count fits its uint32) and the other two's
P = 1024                           # the pixels of a case that varies something else

NEGATIVE = "n_clips or n_frames < 0"
MULTIPLE = "pixels must be a positive multiple of 4, got %d"
ABOVE = "pixels above 2^%d"
ALIGNED = "every pointer and every stride must be 4-byte aligned"
STRIDE = "a frame stride is below the %d bytes of a frame"


def _cases():
    """[(n_clips, n_frames, pixels, ceiling, alignment word, frame strides), None or the refusal's text behind "<entry>: "]"""
    rows = []
    for log2 in CEILINGS:
        def case(want, n_clips=1, n_frames=1, pixels=P, aligned=0, strides=None):
            rows.append(((n_clips, n_frames, pixels, log2, aligned, strides or (3 * pixels, 3 * pixels)), want))
        for n in (-1, 0, 1):       # (empty work passes the refusals: the entry point answers IIV_OK behind its own)
            case(NEGATIVE if n < 0 else None, n_clips=n)
            case(NEGATIVE if n < 0 else None, n_frames=n)
        for pixels in (0, 3, 4, 6, 2 ** 31, 2 ** 31 + 4, 2 ** 40, 2 ** 40 + 4):
            case(MULTIPLE % pixels if pixels <= 0 or pixels % 4 else ABOVE % log2 if pixels > 2 ** log2 else None, pixels=pixels)
        for aligned in (0, 1, 2, 4):
            case(ALIGNED if aligned & 3 else None, aligned=aligned)
        for stride in (3 * P - 4, 3 * P, 3 * P + 4):
            want = STRIDE % (3 * P) if stride < 3 * P else None
            case(want, strides=(stride,))                    # the one stride of the histogram
            case(want, strides=(stride, 3 * P))              # either of the two of the others
            case(want, strides=(3 * P, stride))
        # the order, as the entry points have always had it: counts, multiple of 4, ceiling, alignment, frame stride
        case(NEGATIVE, n_clips=-1, pixels=6, aligned=1, strides=(0,))
        case(MULTIPLE % 6, pixels=6, aligned=1, strides=(0,))
        case(ABOVE % log2, pixels=2 ** 40 + 4, aligned=1, strides=(0,))
        case(ALIGNED, aligned=1, strides=(0,))
        case(ALIGNED, n_clips=0, aligned=2)                  # (and in front of the empty-work answer)
        case(STRIDE % (3 * P), n_frames=0, strides=(3 * P, 3 * P - 1))
    return rows


PIXELS = (4, 8, 252, 256, 260, 1024, 1028, 53760)
# (n_clips, n_frames, pixels): item counts of the three kernels on both sides of the grid cap
SHAPES = ((1, 1, 4), (2047, 1, 8), (2048, 1, 8), (2049, 1, 8), (3, 17, 53760), (38, 8, 53760), (39, 8, 53760), (39, 9, 53760),
          (1024, 1, 1028), (1025, 1, 1028), (256, 8, 252), (256, 9, 256), (4097, 3, 260), (2 ** 31 - 1, 2 ** 31 - 1, 1024))

PROGRAM = r"""
#include "iiv_clip.h"
#include <stdarg.h>
#include <stdio.h>
namespace iiv {
int set_error(int code, const char *fmt, ...)
{
    char text[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    printf("E %%d %%s\n", code, text);
    return code;
}
}
using namespace iiv;
struct Case { int n_clips, n_frames; long pixels; int log2; unsigned long aligned; int n_strides; unsigned long stride[2]; };
int main()
{
    const Case cases[] = {%(cases)s};
    for (const Case &c : cases) {
        const int rc = c.n_strides == 1
            ? clip_refuse("%(name)s", c.n_clips, c.n_frames, c.pixels, c.log2, (uintptr_t)c.aligned, {(size_t)c.stride[0]})
            : clip_refuse("%(name)s", c.n_clips, c.n_frames, c.pixels, c.log2, (uintptr_t)c.aligned, {(size_t)c.stride[0], (size_t)c.stride[1]});
        printf("R %%d\n", rc);
    }
    const long pixels[] = {%(pixels)s};
    for (long p : pixels) printf("L %%zu %%zu\n", clip_lanes(p), clip_runs(clip_lanes(p)));
    const unsigned long items[] = {%(items)s};
    for (unsigned long n : items) printf("G %%u\n", clip_grid((size_t)n));
    printf("K %%d %%d %%d\n", kClipThreads, kClipLanePixels, kClipGridCap);
    return 0;
}
"""


def _items():
    """the three kernels' item counts of every shape, from the tests' mirrors"""
    out = []
    for c, n, p in SHAPES:
        out += [c * TC.runs_per_clip(p), LC.hist_items(c, n), LC.apply_items(c, n, p)]
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("clip_host")
    src, exe = tmp / "clip.cpp", tmp / "clip"
    rows = ", ".join("{%d, %d, %dL, %d, %dUL, %d, {%s}}" % (a[0], a[1], a[2], a[3], a[4], len(a[5]), ", ".join("%dUL" % s for s in a[5]))
                     for a, _ in _cases())
    src.write_text(PROGRAM % dict(cases=rows, name=NAME, pixels=", ".join("%dL" % p for p in PIXELS),
                                  items=", ".join("%dUL" % n for n in _items())))
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    return {k: [line[2:] for line in lines if line[0] == k] for k in "ERLGK"}, lines


def test_refusals_case_by_case(printed):
    _, lines = printed
    cases = _cases()
    assert len(cases) == len(CEILINGS) * (6 + 8 + 4 + 9 + 6)
    at = 0
    for args, want in cases:
        if want is None:                                     # passed: no message, IIV_OK
            assert lines[at] == "R 0", (args, lines[at])
            at += 1
        else:                                                # refused: one message with the entry's name in front, its code returned
            assert lines[at] == "E %d %s: %s" % (INVALID, NAME, want), (args, lines[at])
            assert lines[at + 1] == "R %d" % INVALID, (args, lines[at + 1])
            at += 2
    assert lines[at][0] == "L"
    assert sum(want is None for _, want in cases) >= 20 and sum(want is not None for _, want in cases) >= 20


def test_every_listed_value_is_met():
    """the cases the shared refusals are held to, per argument, at both ceilings"""
    for log2 in CEILINGS:
        mine = [a for a, _ in _cases() if a[3] == log2]
        assert {-1, 0, 1} <= {a[0] for a in mine} and {-1, 0, 1} <= {a[1] for a in mine}
        assert {0, 3, 4, 6, 2 ** 31, 2 ** 31 + 4, 2 ** 40, 2 ** 40 + 4} <= {a[2] for a in mine}
        assert {0, 1, 2, 4} <= {a[4] for a in mine}
        assert {(3 * P - 4,), (3 * P,), (3 * P + 4,)} <= {a[5] for a in mine if a[2] == P}
    verdict = {(a[2], a[3]): want for a, want in _cases() if a[2] >= 2 ** 31 and a[4] == 0}
    assert verdict == {(2 ** 31, 31): None, (2 ** 31 + 4, 31): ABOVE % 31, (2 ** 40, 31): ABOVE % 31, (2 ** 40 + 4, 31): ABOVE % 31,
                       (2 ** 31, 40): None, (2 ** 31 + 4, 40): None, (2 ** 40, 40): None, (2 ** 40 + 4, 40): ABOVE % 40}


def test_item_arithmetic_is_the_mirrors(printed):
    out, _ = printed
    assert out["K"] == ["%d %d %d" % (TC.THREADS, TC.LANE_PIXELS, TC.GRID_CAP)]
    assert (LC.THREADS, LC.LANE_PIXELS, LC.GRID_CAP) == (TC.THREADS, TC.LANE_PIXELS, TC.GRID_CAP) == (256, 4, 2048)
    got = [tuple(map(int, line.split())) for line in out["L"]]
    assert got == [(p // 4, TC.runs_per_clip(p)) for p in PIXELS]
    assert [runs for _, runs in got] == [1, 1, 1, 1, 1, 1, 2, 53]          # (a run is 256 lanes = 1024 pixels)
    for (lanes, runs), p in zip(got, PIXELS):
        for c, n in ((1, 1), (3, 8), (3, 9), (7, 17)):
            assert c * runs * -(-n // LC.APPLY_FRAMES) == LC.apply_items(c, n, p) and c * n == LC.hist_items(c, n)
    items = _items()
    assert list(map(int, out["G"])) == [min(n, TC.GRID_CAP) for n in items]
    assert min(items) == 1 and {2047, 2048, 2049} <= set(items) and max(items) > 2 ** 32     # both sides of the cap, and past unsigned
