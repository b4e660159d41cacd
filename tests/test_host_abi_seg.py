"""include/lvc_amd_seg.h (the lvcseg_ entries of csrc/sem_seg.hip) under the discipline tests/test_host_abi.py holds lvc_amd.h to: the
header is the one statement of these entries; the compiler holds the definitions to it (csrc/common.h includes it), ctypes holds the
Python calls to it (lvc_amd/_lib.py binds restype / argtypes from the parsed text).  Everything here runs on the host."""
import ast
import ctypes
import glob
import os
import shutil
import subprocess

import pytest

from helpers import ROOT

from lvc_amd import _lib

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRIES = {"lvcseg_upsample2_bilinear_nhwc", "lvcseg_sem_seg_postprocess", "lvcseg_panoptic_combine"}
V, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double


def test_the_second_header_parses_and_the_first_table_is_untouched():
    seg = _lib.signatures_seg()
    assert set(seg) == ENTRIES
    assert seg["lvcseg_upsample2_bilinear_nhwc"] == (I, [V, V, V, I, I, I, I, V])
    assert seg["lvcseg_sem_seg_postprocess"] == (I, [V, L, V, V, I, I, I, I, V, L, V, L, I, V])
    assert seg["lvcseg_panoptic_combine"] == (I, [V, L, V, V, I, I, V, V, V, L, I, I, V, V, I, D, D, D, V, L, V, L, V, V])
    first = _lib.signatures()
    assert not any(name.startswith("lvcseg_") for name in first) and all(name.startswith("lvc_") for name in first)
    assert not set(first) & set(seg)
    text = open(os.path.join(ROOT, "include", "lvc_amd.h")).read()
    assert "lvcseg_" not in text


def test_parse_header_takes_the_prefix_and_defaults_to_the_first():
    text = "int lvcseg_x(const float* a, long long n, double t, void* stream);"
    assert _lib.parse_header(text, prefix="lvcseg_") == {"lvcseg_x": (I, [V, L, D, V])}
    assert _lib.parse_header("int lvc_y(int n);") == {"lvc_y": (I, [I])}
    with pytest.raises(ValueError, match="lvcseg_"):
        _lib.parse_header("int lvc_y(int n);", prefix="lvcseg_")      # a declaration of another family in this header
    with pytest.raises(ValueError, match="size_t n.*lvcseg_x"):
        _lib.parse_header("int lvcseg_x(size_t n);", prefix="lvcseg_")


def _exported():
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.check_output([nm, "-D", "--defined-only", _lib._SO], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("lvcseg_")}


def test_declared_and_exported_symbols_are_the_same_set():
    assert _exported() == set(_lib.signatures_seg())


def test_every_bound_function_carries_the_header_signature():
    lib = _lib.lib()
    for name, (restype, argtypes) in _lib.signatures_seg().items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    with pytest.raises(TypeError):
        lib.lvcseg_upsample2_bilinear_nhwc(None, None, None, 1, 1, 1, 4)              # one argument short
    with pytest.raises(ctypes.ArgumentError):
        lib.lvcseg_upsample2_bilinear_nhwc(None, None, None, 1.0, 1, 1, 4, None)      # a float for an int
    # a host-side refusal comes back as a status and a text, no launch: N = 1 with null pointers
    assert lib.lvcseg_upsample2_bilinear_nhwc(None, None, None, 1, 1, 1, 4, None) == 1
    assert b"null pointer" in lib.lvc_last_error()
    assert lib.lvcseg_upsample2_bilinear_nhwc(None, None, None, 1, 1, 1, 6, None) == 1
    assert b"multiple of 4" in lib.lvc_last_error()


def test_every_call_site_passes_the_headers_number_of_arguments():
    sigs = _lib.signatures_seg()
    files = sorted(glob.glob(os.path.join(ROOT, "lvc_amd", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "scripts", "*.py")))
    called, seen = set(), 0
    for path in files:
        tree = ast.parse(open(path).read())
        calls = {id(n.func): n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Attribute) and node.attr.startswith("lvcseg_")):
                continue
            rel = os.path.relpath(path, ROOT)
            assert node.attr in sigs, "{}:{} names {}, which lvc_amd_seg.h does not declare".format(rel, node.lineno, node.attr)
            call = calls.get(id(node))
            assert call is not None, "{}:{}: {} taken as a value; the count of its arguments cannot be checked".format(rel, node.lineno, node.attr)
            assert not call.keywords and not any(isinstance(a, ast.Starred) for a in call.args), (rel, node.lineno)
            assert len(call.args) == len(sigs[node.attr][1]), (rel, node.lineno, node.attr, len(call.args), len(sigs[node.attr][1]))
            called.add(node.attr)
            seen += 1
    assert called == ENTRIES and seen >= 3


_UNIT = ('#include "{}"\nextern "C" int lvcseg_upsample2_bilinear_nhwc(const float* x, const float* acc, float* y, {} N, int H, int W, int C, '
         'void* stream) {{ return N + H; }}\n')


@pytest.mark.parametrize("n_type, compiles", [("int", True), ("long long", False)])
def test_a_definition_that_differs_from_the_header_does_not_compile(tmp_path, n_type, compiles):
    src = tmp_path / "unit.hip"
    src.write_text(_UNIT.format(os.path.join(ROOT, "lvc_amd", "csrc", "common.h"), n_type))
    r = subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert (r.returncode == 0) == compiles, r.stderr
    if not compiles:
        assert "lvcseg_upsample2_bilinear_nhwc" in r.stderr and "conflicting types" in r.stderr


def test_no_python_attribute_of_the_new_code_starts_with_the_first_prefix():
    """tests/test_host_abi.py reads every `.lvc_*` attribute in lvc_amd/ and scripts/ as an entry of lvc_amd.h."""
    for rel in ("lvc_amd/modeling/meta_arch/semantic_seg.py", "lvc_amd/modeling/meta_arch/panoptic_fpn.py", "scripts/make_golden_panoptic.py",
                "scripts/bench_panoptic.py"):
        tree = ast.parse(open(os.path.join(ROOT, rel)).read())
        bad = [n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr.startswith("lvc_") and n.attr != "lvc_amd"]
        assert bad == [], (rel, bad)
