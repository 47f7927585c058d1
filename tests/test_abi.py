"""CPU: the C-ABI library loads and exports every symbol include/iivision.h
declares (no compute calls -- there is no GPU here), and the host layer refuses
to run without a GPU instead of falling back."""

import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    """include/iivision.h without its comments"""
    hdr = open(os.path.join(ROOT, "include", "iivision.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def _declared_symbols():
    return sorted(set(re.findall(r"\b(iiv_[a-z0-9_]+)\s*\(", _header())))


def test_header_symbols_exported(native):
    syms = _declared_symbols()
    assert len(syms) >= 20
    L = ctypes.CDLL(native.LIB_PATH)
    for s in syms:
        assert hasattr(L, s), "libiivision.so does not export %s" % s
    assert set(syms) == set(native.SYMBOLS)


_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "uint16_t": ctypes.c_uint16,
            "uint32_t": ctypes.c_uint32}


def _is_pointer(ctype):
    return ctype in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer))


def _name(ctype):
    return getattr(ctype, "__name__", repr(ctype))


def test_binding_declares_every_function_as_the_header_does(native):
    """The return type and every parameter of every prototype of include/iivision.h against the restype / argtypes the
    binding has set on the loaded library, by kind: a pointer or array <-> c_void_p / c_char_p / POINTER(...), int, long,
    size_t, uint16_t, uint32_t <-> the ctypes type of that name, void <-> None; the three struct pointers must be
    POINTER(Segment / VideoState / VideoBrief).  On x86-64 a wrong entry works until a value is large; here it fails."""
    structs = {"iiv_segment": native.Segment, "iiv_video_state": native.VideoState, "iiv_video_brief": native.VideoBrief}
    hdr = re.sub(r"^[ \t]*#.*$", "", _header(), flags=re.M)
    protos = re.findall(r"([^;{}()]+?)\b(iiv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)
    assert len(protos) >= len(native.SYMBOLS) and {p[1] for p in protos} == set(native.SYMBOLS)
    L = native.lib()
    wrong = []
    for ret, name, params in protos:
        f = getattr(L, name)
        ret = ret.strip()
        if "*" in ret:
            ok = _is_pointer(f.restype)
        elif ret == "void":
            ok = f.restype is None
        else:
            assert ret in _SCALARS, "%s: unknown C return type %r" % (name, ret)
            ok = f.restype is _SCALARS[ret]
        if not ok:
            wrong.append("%s returns %s, the binding declares %s" % (name, ret, _name(f.restype)))
        params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        got = list(f.argtypes or [])
        if len(got) != len(params):
            wrong.append("%s takes %d parameters, the binding declares %d" % (name, len(params), len(got)))
            continue
        for i, (p, a) in enumerate(zip(params, got)):
            words = [w for w in re.findall(r"\w+", p) if w != "const"]
            if "*" in p or "[" in p:
                ok = a is ctypes.POINTER(structs[words[0]]) if words[0] in structs else _is_pointer(a)
            else:
                ctype = " ".join(words[:-1])   # (the last word is the parameter's name)
                assert ctype in _SCALARS, "%s: unknown C type in parameter %d (%s)" % (name, i, p)
                ok = a is _SCALARS[ctype]
            if not ok:
                wrong.append("%s parameter %d (%s): the binding declares %s" % (name, i, p, _name(a)))
    assert not wrong, "\n".join(wrong)


def test_struct_sizes_follow_the_header(native):
    """sizeof(VideoState) / sizeof(VideoBrief) against the bytes the header's own field lists imply (element width from the
    type's name, count from the array bound; the fields are ordered so that no padding arises)."""
    sizes = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^}]*)\}\s*(iiv_\w+)\s*;", _header()):
        total = 0
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            ctype, fields = decl.split(None, 1)
            m = re.fullmatch(r"u?int(\d+)_t", ctype)
            assert m, "%s: field %r is of no fixed-width integer type; work its size and padding out here" % (name, decl)
            width = int(m.group(1)) // 8
            for field in fields.split(","):
                bound = re.search(r"\[([^\]]*)\]", field)
                count = 1
                for factor in (bound.group(1).split("*") if bound else []):
                    count *= int(factor)
                assert total % width == 0, "%s: %r would be padded; this sum assumes no padding" % (name, decl)
                total += width * count
        sizes[name] = total
    assert sizes["iiv_segment"] == ctypes.sizeof(native.Segment) == 16
    assert sizes["iiv_video_state"] == ctypes.sizeof(native.VideoState)
    assert sizes["iiv_video_brief"] == ctypes.sizeof(native.VideoBrief)


_STUB_C = 'const char *iiv_version(void) { return "iivision-stub"; }\nconst char *iiv_last_error(void) { return ""; }\n'

_STUB_CHILD = """
import importlib, os, sys
sys.path.insert(0, sys.argv[1])
os.environ.pop("IIV_LIB", None)
import _iiv_native as native
assert native.LIB_PATH == sys.argv[2], native.LIB_PATH
try:
    native.lib()
    print("default path: loaded")
except AttributeError as e:
    print("default path: AttributeError:", e)
os.environ["IIV_LIB"] = sys.argv[2]
native = importlib.reload(native)
print("IIV_LIB:", native.lib().iiv_version().decode())
"""


def test_a_missing_symbol_is_an_error_unless_iiv_lib_names_the_library(native, tmp_path):
    """A library that exports only iiv_version and iiv_last_error: found where the binding looks by default, lib() raises
    AttributeError naming a symbol it lacks; named by IIV_LIB (an A/B run against an older build, tools/ab_libs.sh), it
    loads.  In a child interpreter, on a copy of the binding, so that this session's library is left alone."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    pkg = tmp_path / "transcoder"
    pkg.mkdir()
    shutil.copy(native.__file__, pkg / "_iiv_native.py")
    (tmp_path / "stub.c").write_text(_STUB_C)
    stub = tmp_path / "libiivision.so"
    subprocess.run([cc, "-shared", "-fPIC", "-o", str(stub), str(tmp_path / "stub.c")], check=True)
    out = subprocess.run([sys.executable, "-c", _STUB_CHILD, str(pkg), str(stub)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    first, second = out.stdout.strip().splitlines()[-2:]
    assert first.startswith("default path: AttributeError:"), first
    named = set(re.findall(r"iiv_[a-z0-9_]+", first)) & set(native.SYMBOLS)
    assert named and not named & {"iiv_version", "iiv_last_error"}, first
    assert second == "IIV_LIB: iivision-stub"


def test_constants_without_gpu(native):
    L = native.lib()
    assert L.iiv_version().startswith(b"iivision")
    assert (L.iiv_masked_bits(0), L.iiv_masked_bits(1)) == (14, 13)
    assert (L.iiv_masked_dots(0), L.iiv_masked_dots(1)) == (18, 10)
    assert (L.iiv_num_offsets(0), L.iiv_num_offsets(1)) == (2, 4)
    assert L.iiv_table_entries(0) == 2 << 28 and L.iiv_table_entries(1) == 4 << 26
    assert L.iiv_store_table_entries(0) == 2 << 22 and L.iiv_store_table_entries(1) == 4 << 20


def test_no_cpu_fallback(native):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        native.cie2000_matrix([[0, 0, 0]] * 16)
    with pytest.raises(RuntimeError):
        native.build_table(1, [0] * 256)


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under ii-vision_amd/ may mention it."""
    pkg = os.path.join(ROOT, "ii-vision_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, fn), errors="replace").read()
                assert "import oracle" not in txt and "liboracle" not in txt and "iiv_oracle.h" not in txt, fn


def test_torch_custom_operators_are_registered_over_the_c_abi(native):
    """north_star: "hand-written HIP kernels via PyTorch-ROCm custom ops".  torch_ops.py registers the C ABI's hot entry
    points as torch.ops.iivision.*; registration needs no GPU, running them does (no CPU implementation)."""
    import torch
    import torch_ops
    assert set(torch_ops.NAMES) == {"cie2000_matrix", "build_table", "build_store_table", "encode", "encode_streams",
                                    "emit_chunk", "frames_to_memory_maps"}
    for name in torch_ops.NAMES:
        op = getattr(torch.ops.iivision, name)
        assert "iivision::" + name in str(op.default._schema)
    # the launch operators mutate their output buffer and return nothing: no hidden allocation, no hidden copy
    assert "ops_out" in str(torch.ops.iivision.encode.default._schema) and "-> ()" in str(torch.ops.iivision.encode.default._schema)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            torch.ops.iivision.cie2000_matrix(torch.zeros((16, 3), dtype=torch.uint8))


def test_library_and_committed_counters_are_of_the_current_sources():
    """The build id compiled into iiv_version() is a hash of csrc/, the headers and the flags (csrc/Makefile: BUILD_ID).  The
    in-tree library must be a build of the sources as they stand, and every entry of profiles/pmc_latest.json -- the counter run
    bench.py quotes -- must carry that id: a kernel (or header) change that is not followed by tools/round_evidence.sh would
    otherwise leave bench.py printing `counters: "stale"` at the driver's end-of-round run."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    want = subprocess.run(["make", "-s", "-C", os.path.join(root, "ii-vision_amd", "csrc"), "build-id"],
                          capture_output=True, text=True, check=True).stdout.strip()
    assert len(want) == 12
    import _iiv_native
    assert _iiv_native.build_id() == want, "ii-vision_amd/libiivision.so is not a build of the current sources: run make -C ii-vision_amd/csrc"
    with open(os.path.join(root, "profiles", "pmc_latest.json")) as f:
        latest = json.load(f)
    stale = {k: v.get("build_id") for k, v in latest.items() if v.get("build_id") != want}
    assert not stale, "profiles/pmc_latest.json holds counter runs of another build %s (this one: %s): run tools/round_evidence.sh" % (stale, want)
