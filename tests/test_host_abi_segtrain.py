"""include/lvc_amd_segtrain.h (the lvcst_ entries of csrc/sem_seg_train.hip) under the discipline tests/test_host_abi.py and
tests/test_host_abi_seg.py hold the other two headers to: the header is the one statement of these entries; the compiler holds the
definitions to it (csrc/common.h includes it), ctypes holds the Python calls to it (lvc_amd/_lib.py binds restype / argtypes from the
parsed text).  Everything here runs on the host."""
import ast
import ctypes
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import ROOT

from lvc_amd import _lib

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRIES = {"lvcst_upsample2_bilinear_bwd_nhwc", "lvcst_sem_seg_loss_workspace_bytes", "lvcst_sem_seg_loss_fwd", "lvcst_sem_seg_loss_bwd"}
V, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong


def test_the_third_header_parses_and_the_other_tables_are_untouched():
    st = _lib.signatures_segtrain()
    assert set(st) == ENTRIES
    assert st["lvcst_upsample2_bilinear_bwd_nhwc"] == (I, [V, V, I, I, I, I, V])
    assert st["lvcst_sem_seg_loss_workspace_bytes"] == (L, [I, I, I, I, I])
    assert st["lvcst_sem_seg_loss_fwd"] == (I, [V, I, I, I, I, I, I, V, L, I, L, V, V, V, V, V, V, L, V, V, V, V, V])
    assert st["lvcst_sem_seg_loss_bwd"] == (I, [V, I, I, I, I, I, I, V, L, I, L, V, V, V, V, V, V, V, V])
    first, seg = _lib.signatures(), _lib.signatures_seg()
    assert not any(n.startswith("lvcst_") for n in list(first) + list(seg))
    assert not any(n.startswith(("lvc_", "lvcseg_")) for n in st)
    assert len(seg) == 3 and not set(first) & set(st)
    for other in ("lvc_amd.h", "lvc_amd_seg.h"):
        assert "lvcst_" not in open(os.path.join(ROOT, "include", other)).read()
    assert _lib.parse_header("int lvcst_x(const float* a, long long n, void* stream);", prefix="lvcst_") == {"lvcst_x": (I, [V, L, V])}
    with pytest.raises(ValueError, match="lvcst_"):
        _lib.parse_header("int lvcseg_y(int n);", prefix="lvcst_")      # a declaration of another family in this header


def _exported():
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.check_output([nm, "-D", "--defined-only", _lib._SO], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("lvcst_")}


def test_declared_and_exported_symbols_are_the_same_set():
    assert _exported() == set(_lib.signatures_segtrain())


def test_every_bound_function_carries_the_header_signature():
    lib = _lib.lib()
    for name, (restype, argtypes) in _lib.signatures_segtrain().items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    with pytest.raises(TypeError):
        lib.lvcst_upsample2_bilinear_bwd_nhwc(None, None, 1, 1, 1, 4)              # one argument short
    with pytest.raises(ctypes.ArgumentError):
        lib.lvcst_upsample2_bilinear_bwd_nhwc(None, None, 1.0, 1, 1, 4, None)      # a float for an int


def test_every_call_site_passes_the_headers_number_of_arguments():
    sigs = _lib.signatures_segtrain()
    files = sorted(glob.glob(os.path.join(ROOT, "lvc_amd", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "scripts", "*.py")))
    called = set()
    for path in files:
        tree = ast.parse(open(path).read())
        calls = {id(n.func): n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Attribute) and node.attr.startswith("lvcst_")):
                continue
            rel = os.path.relpath(path, ROOT)
            assert node.attr in sigs, "{}:{} names {}, which lvc_amd_segtrain.h does not declare".format(rel, node.lineno, node.attr)
            call = calls.get(id(node))
            assert call is not None, "{}:{}: {} taken as a value; the count of its arguments cannot be checked".format(rel, node.lineno, node.attr)
            assert not call.keywords and not any(isinstance(a, ast.Starred) for a in call.args), (rel, node.lineno)
            assert len(call.args) == len(sigs[node.attr][1]), (rel, node.lineno, node.attr, len(call.args), len(sigs[node.attr][1]))
            called.add(node.attr)
    assert called == ENTRIES


_UNIT = ('#include "{}"\nextern "C" int lvcst_upsample2_bilinear_bwd_nhwc(const float* dy, float* dx, {} N, int H, int W, int C, '
         'void* stream) {{ return N + H; }}\n')


@pytest.mark.parametrize("n_type, compiles", [("int", True), ("long long", False)])
def test_a_definition_that_differs_from_the_header_does_not_compile(tmp_path, n_type, compiles):
    src = tmp_path / "unit.hip"
    src.write_text(_UNIT.format(os.path.join(ROOT, "lvc_amd", "csrc", "common.h"), n_type))
    r = subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert (r.returncode == 0) == compiles, r.stderr
    if not compiles:
        assert "lvcst_upsample2_bilinear_bwd_nhwc" in r.stderr and "conflicting types" in r.stderr


def _jobs(rows):
    t = np.ascontiguousarray(rows, dtype=np.int64)
    return t, ctypes.c_void_p(t.ctypes.data)


def test_argument_validation_returns_an_error_without_a_device():
    """Every refusal below is decided on the host, in front of any launch: a status and a text, with pointers that are never followed."""
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)      # (non-null, 16-byte aligned, never dereferenced: each call fails its check first)

    def err():
        return lib.lvc_last_error().decode()

    assert lib.lvcst_upsample2_bilinear_bwd_nhwc(fake, fake, 1, 1, 1, 6, None) == 1 and "multiple of 4" in err()
    assert lib.lvcst_upsample2_bilinear_bwd_nhwc(None, None, 1, 1, 1, 4, None) == 1 and "null pointer" in err()
    assert lib.lvcst_upsample2_bilinear_bwd_nhwc(ctypes.c_void_p(4100), fake, 1, 1, 1, 4, None) == 1 and "16-byte" in err()
    assert lib.lvcst_upsample2_bilinear_bwd_nhwc(None, None, 0, 1, 1, 4, None) == 0      # an empty batch launches nothing

    keep, jobs = _jobs([[0, 8, 12]])
    # (`lse` below: the max map, the first of the two maps the backward takes)
    fwd = lambda logits, K, ld, scale, numel, bytes_, j, lse: lib.lvcst_sem_seg_loss_fwd(      # noqa: E731
        logits, 1, 2, 3, K, ld, scale, fake, numel, bytes_, 255, j, fake, lse, fake, None, fake, 1 << 20, fake, fake, fake, fake, None)
    bwd = lambda logits, K, ld, scale, numel, bytes_, j, lse: lib.lvcst_sem_seg_loss_bwd(      # noqa: E731
        logits, 1, 2, 3, K, ld, scale, fake, numel, bytes_, 255, j, fake, lse, fake, fake, fake, fake, None)
    for call, name in ((fwd, "lvcst_sem_seg_loss_fwd"), (bwd, "lvcst_sem_seg_loss_bwd")):
        assert call(fake, 5, 4, 4, 96, 1, jobs, fake) == 1 and "ld >= K" in err() and name in err()
        assert call(fake, 5, 8, 0, 96, 1, jobs, fake) == 1 and "scale" in err()
        assert call(fake, 5, 8, 65, 96, 1, jobs, fake) == 1 and "scale" in err()
        assert call(fake, 4097, 4100, 4, 96, 1, jobs, fake) == 1 and "K <= 4096" in err()
        assert call(fake, 5, 8, 4, 96, 4, jobs, fake) == 1 and "label_bytes" in err()
        assert call(fake, 5, 8, 4, 95, 1, jobs, fake) == 1 and "a job's label map lies outside the buffer" in err()
        assert call(fake, 5, 8, 4, 96, 1, None, fake) == 1 and "null pointer" in err()
        assert call(None, 5, 8, 4, 96, 1, jobs, fake) == 1 and "null pointer" in err()
        assert call(fake, 5, 8, 4, 96, 1, jobs, None) == 1 and "null pointer" in err()
        keep2, big = _jobs([[0, 9, 12]])      # taller than scale x h = 8
        assert call(fake, 5, 8, 4, 200, 1, big, fake) == 1 and "exceeds scale x the logits" in err()
        keep3, neg = _jobs([[-1, 8, 12]])
        assert call(fake, 5, 8, 4, 200, 1, neg, fake) == 1 and "outside the buffer" in err()
    # the forward's workspace: the query's answer is what the call asks for
    need = lib.lvcst_sem_seg_loss_workspace_bytes(1, 2, 3, 5, 4)
    assert need == 16      # one workgroup: an fp64 sum and an int64 count
    assert lib.lvcst_sem_seg_loss_fwd(fake, 1, 2, 3, 5, 8, 4, fake, 96, 1, 255, jobs, fake, fake, fake, None, fake, need - 1, fake, fake, fake,
                                      fake, None) == 1 and "workspace too small" in err()
    assert lib.lvcst_sem_seg_loss_workspace_bytes(8, 200, 336, 54, 4) == 8 * 50 * 21 * 16      # 16 x 64 tiles of 800 x 1344
    assert lib.lvcst_sem_seg_loss_workspace_bytes(1, 2, 3, 5, 65) == -1 and lib.lvcst_sem_seg_loss_workspace_bytes(1, 0, 3, 5, 4) == -1
    assert lib.lvcst_sem_seg_loss_workspace_bytes(1, 2, 3, 4096, 4) == -1      # one pixel's 2 x 2 footprint of 4097 floats: past the LDS
    del keep, keep2, keep3


def test_no_python_attribute_of_the_new_code_starts_with_the_first_prefix():
    """tests/test_host_abi.py reads every `.lvc_*` attribute in lvc_amd/ and scripts/ as an entry of lvc_amd.h."""
    for rel in ("scripts/make_golden_panoptic_train.py", "scripts/bench_panoptic_train.py"):
        tree = ast.parse(open(os.path.join(ROOT, rel)).read())
        bad = [n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr.startswith("lvc_") and n.attr != "lvc_amd"]
        assert bad == [], (rel, bad)
