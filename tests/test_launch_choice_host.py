"""CPU: which greedy kernel a launch runs (ii-vision_amd/csrc/iiv_launch_choice.h), enumerated.  The header is plain host
arithmetic, so a stand-alone program built by the host compiler prints its answer for every combination of the options, batch
sizes on both sides of every threshold, what the tie statistics said and the round's bank; the rules are restated here, in
Python, from the behaviour the encoder has always had -- not from the header."""
import itertools
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ii-vision_amd", "csrc")

HGR, DHGR = 0, 1
WAVE, WORKGROUP, AUTO, TEAM, WAVE_SHARED, WAVE_PLAIN = range(6)
TARGET, JOINT, JOINT_SPLIT = range(3)
PLAIN_K, SHARED_K, TEAM_K, WORKGROUP_K = range(4)          # the indices of iiv_encoder_launch_forms

MODES = (HGR, DHGR)
GREEDY = (WAVE, WORKGROUP, AUTO, TEAM, WAVE_SHARED, WAVE_PLAIN)
CONTENT = (TARGET, JOINT, JOINT_SPLIT)
FOURTH = (0, 1)
TABLES = ((0, 0), (1, 0), (1, 1))                          # (split table built, its narrow form exact)
STREAMS = (1, 768, 769, 2047, 2048, 4095, 4096)
TIE_HEAVY = (-1, 0, 1)
BANK = (-1, 0, 1)
LDS_PAD = (0, 1024)
ORDER = (0, 1)

PROGRAM = r"""
#include "iiv_launch_choice.h"
#include <stdio.h>
using namespace iiv;
int main()
{
    const int modes[] = {%(modes)s}, greedy[] = {%(greedy)s}, content[] = {%(content)s}, tables[][2] = {{0, 0}, {1, 0}, {1, 1}};
    const int streams[] = {%(streams)s}, pads[] = {%(pads)s};
    for (int mode : modes) for (int g : greedy) for (int c : content) for (int f4 = 0; f4 < 2; f4++) for (auto &t : tables)
    for (int n : streams) for (int heavy = -1; heavy < 2; heavy++) for (int bank = -1; bank < 2; bank++) for (int pad : pads)
    for (int order = 0; order < 2; order++) {
        const LaunchInputs in{mode, n, g, c, f4, pad, order, t[0] != 0, t[1] != 0, heavy};
        const LaunchChoice r = choose_launch(in, bank);
        printf("%%d %%d %%d %%d %%d %%d %%d %%d\n", (int)r.kernel, r.joint, (int)r.count_stats, (int)r.ordered, r.uniform_bank, (int)r.zeroed_queue,
               (int)team_kernel_runs(in), (int)shared_form_now(in));
    }
    return 0;
}
"""


def expected(mode, greedy, content, fourth, split, exact, n, tie_heavy, bank, lds_pad, order):
    """(kernel, joint, count_stats, ordered, uniform_bank passed on, zeroed stream counters, team kernel runs, shared form now)"""
    wave = content == TARGET and bool(fourth or (split and exact and greedy != WORKGROUP))
    team = wave and (greedy == TEAM or (greedy == AUTO and n <= 768))
    big = n >= (4096 if mode == HGR else 2048)
    shared_wanted = greedy == WAVE_SHARED or (greedy != WAVE_PLAIN and big and (mode == HGR if tie_heavy < 0 else tie_heavy == 0))
    count_stats = bool(split and exact and greedy in (AUTO, WAVE) and content == TARGET and big)
    kernel, joint, ordered, bank_out = WORKGROUP_K, 0, False, bank
    if not wave:
        joint = 2 if content == JOINT else 1 if content == JOINT_SPLIT else 0
    elif team:
        kernel = TEAM_K
    else:
        bank_out = -1 if greedy == WAVE_PLAIN else bank
        kernel = SHARED_K if shared_wanted and bank_out >= 0 and lds_pad == 0 else PLAIN_K
        ordered = n >= 2048 and bool(order)
    return (kernel, joint, int(count_stats), int(ordered), bank_out, int(not team), int(team), int(shared_wanted))


def _compiler():
    """the host C++ compiler, or hipcc (which the library's build needs anyway): a .cpp file is host code to it"""
    for name in ("c++", "g++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no C++ compiler"
    return hipcc


def test_launch_choice_for_every_combination(tmp_path):
    src = tmp_path / "launch_choice.cpp"
    src.write_text(PROGRAM % dict(modes=", ".join(map(str, MODES)), greedy=", ".join(map(str, GREEDY)), content=", ".join(map(str, CONTENT)),
                                  streams=", ".join(map(str, STREAMS)), pads=", ".join(map(str, LDS_PAD))))
    exe = tmp_path / "launch_choice"
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    rows = list(itertools.product(MODES, GREEDY, CONTENT, FOURTH, TABLES, STREAMS, TIE_HEAVY, BANK, LDS_PAD, ORDER))
    assert len(lines) == len(rows) == 54432
    wrong = []
    for line, (mode, greedy, content, fourth, (split, exact), n, heavy, bank, pad, order) in zip(lines, rows):
        want = expected(mode, greedy, content, fourth, split, exact, n, heavy, bank, pad, order)
        if tuple(map(int, line.split())) != want:
            wrong.append(((mode, greedy, content, fourth, split, exact, n, heavy, bank, pad, order), line, want))
    assert not wrong, "%d rows differ, the first: %r" % (len(wrong), wrong[:3])
    assert {int(line.split()[0]) for line in lines} == {PLAIN_K, SHARED_K, TEAM_K, WORKGROUP_K}      # (every kernel occurs)


def test_the_thresholds_live_in_the_header_alone():
    """the batch-size and tie thresholds are named in iiv_launch_choice.h and nowhere else under csrc/"""
    import re
    names = re.compile(r"\bk(TeamMaxStreams|Shared(Hgr|Dhgr)MinStreams|TieHeavyPercent(DHGR|HGR)|SharedMinOpsPerLaunch)\b")
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".h")) and fn != "iiv_launch_choice.h":
            with open(os.path.join(CSRC, fn), errors="replace") as f:
                assert not names.search(f.read()), fn
