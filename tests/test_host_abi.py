"""The C ABI is stated once, in include/lvc_amd.h, and both of its other sides are held to it: the definitions by the compiler
(csrc/common.h includes the header), the Python calls by ctypes (lvc_amd/_lib.py binds restype / argtypes from the parsed header).
Everything here runs on the host; no kernel is launched."""
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
KINDS = {ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_float, ctypes.c_double, ctypes.c_void_p}
INTERNAL = {"lvc_cu_count"}      # exported for the other translation units, not part of the ABI (declared in csrc/conv_common.h)


# ------------------------------------------------------------------------------------------------ the parser
def test_every_declaration_parses_to_known_kinds():
    sigs = _lib.signatures()
    assert len(sigs) == 153 and "lvc_set_error" not in sigs      # 154 declarations, the variadic one is not bound
    for name, (restype, argtypes) in sigs.items():
        assert restype in (None, ctypes.c_char_p, ctypes.c_int, ctypes.c_longlong), name
        assert all(t in KINDS for t in argtypes), name
    assert sigs["lvc_last_error"] == (ctypes.c_char_p, [])
    assert sigs["lvc_set_range_slot"] == (None, [ctypes.c_int])
    assert sigs["lvc_batched_nms_workspace_bytes"] == (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int])
    assert sigs["lvc_subsample_batched"][1][:4] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_int]
    assert sigs["lvc_keypoint_loss"][1][7:9] == [ctypes.c_double, ctypes.c_double]
    assert sigs["lvc_rownorm"][1][7] is ctypes.c_float


def test_an_unknown_type_raises_and_names_the_declaration():
    ok = _lib.parse_header("/* c */ int lvc_x(const float* a, int n /* rows */, void* stream);   // tail\nlong long lvc_y(void);")
    assert ok == {"lvc_x": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]), "lvc_y": (ctypes.c_longlong, [])}
    with pytest.raises(ValueError, match="size_t n.*lvc_x"):
        _lib.parse_header("int lvc_x(const float* a, size_t n);")
    with pytest.raises(ValueError, match="float\\*.*lvc_x"):
        _lib.parse_header("float* lvc_x(int n);")


# ------------------------------------------------------------------------------------------------ exports
def _exported():
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.check_output([nm, "-D", "--defined-only", _lib._SO], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("lvc_")}


def test_declared_and_exported_symbols_are_the_same_set():
    declared = set(_lib.signatures()) | {"lvc_set_error"}
    exported = _exported()
    assert declared - exported == set(), "declared in lvc_amd.h, not exported by liblvc_amd.so"
    assert exported - declared == INTERNAL, "exported lvc_* symbols that are neither declared nor on the internal list"


def test_every_bound_function_carries_the_header_signature():
    L = _lib.lib()
    for name, (restype, argtypes) in _lib.signatures().items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert L.lvc_abi_version() == 1


# ------------------------------------------------------------------------------------------------ the compiler check bites
_UNIT = '#include "{}"\nextern "C" int lvc_colsum(const float* x, {} M, int N, int ldx, float* out, void* stream) {{ return M + N; }}\n'


@pytest.mark.parametrize("m_type, compiles", [("int", True), ("long long", False)])
def test_a_definition_that_differs_from_the_header_does_not_compile(tmp_path, m_type, compiles):
    src = tmp_path / "unit.hip"
    src.write_text(_UNIT.format(os.path.join(ROOT, "lvc_amd", "csrc", "common.h"), m_type))
    r = subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert (r.returncode == 0) == compiles, r.stderr
    if not compiles:
        assert "lvc_colsum" in r.stderr and "conflicting types" in r.stderr


# ------------------------------------------------------------------------------------------------ ctypes rejects bad calls
def test_ctypes_rejects_a_bad_call_of_a_host_only_query():
    L = _lib.lib()
    assert L.lvc_batched_nms_workspace_bytes(2, 1000) > 0
    with pytest.raises(TypeError):
        L.lvc_batched_nms_workspace_bytes(2)
    with pytest.raises(ctypes.ArgumentError):
        L.lvc_batched_nms_workspace_bytes(2, 1000.0)
    with pytest.raises(ctypes.ArgumentError):
        _lib.size_query("lvc_batched_nms_workspace_bytes", 2, 1000.0)
    assert L.lvc_batched_nms_workspace_bytes(ctypes.c_int(2), ctypes.c_int(1000)) == L.lvc_batched_nms_workspace_bytes(2, 1000)


def test_a_long_long_answer_beyond_32_bits_comes_back_whole():
    # csrc/vit.hip: 6 fp16 planes [B*H][N rounded up to 128][64]
    want = 6 * 64 * 64 * 1024 * 64 * 2
    assert want > 2 ** 31
    assert _lib.lib().lvc_mha_workspace_bytes(64, 1024, 64) == want
    assert _lib.size_query("lvc_mha_workspace_bytes", 64, 1024, 64) == want


# ------------------------------------------------------------------------------------------------ argument counts of the call sites
# Sites the walk cannot count: a starred argument, or an entry point chosen at run time (`getattr(lib, entry)(...)`, `fn = lib.a if
# .. else lib.b`).  (file, function) -> the entries it can reach; the entries of one site must share a signature, and a site without
# a star is counted against it.  The conv sites among them are the ones scripts/conv_dispatch_trace.py's recorder counts on every
# call (ctypes itself refuses too few arguments, not too many).
STARRED = {
    ("lvc_amd/_lib.py", "size_query"): None,          # its callers name the entry: counted below, one by one
    ("lvc_amd/kernels.py", "conv2d_nhwc"): None,      # any conv/GEMM entry the route names: `*ints` differs per entry
    ("lvc_amd/kernels.py", "conv3x3_levels"): None,   # _f16_levels / _f16_layers: `*weights` is three or L-fold
    ("lvc_amd/kernels.py", "retinanet_loss"): ("lvc_retinanet_loss",),
    ("lvc_amd/kernels.py", "retinanet_loss_grad"): ("lvc_retinanet_loss_grad",),
    ("lvc_amd/kernels.py", "group_norm_nhwc"): ("lvc_group_norm_fwd_nhwc",),
    ("lvc_amd/kernels.py", "group_norm_backward_nhwc"): ("lvc_group_norm_bwd_nhwc",),
}
DYNAMIC = {
    ("lvc_amd/kernels.py", "_train_input_call"): ("lvc_train_input_u8", "lvc_train_input_tiles_u8", "lvc_train_input_lsj_u8"),
    ("lvc_amd/kernels.py", "_conv_wgrad"): ("lvc_conv_wgrad_nhwc", "lvc_conv_wgrad_nhwc_bf16x3"),
    ("lvc_amd/kernels.py", "knn_verify_topk_vote"): ("lvc_knn_verify_topk_vote", "lvc_knn_verify_topk_vote_q15"),
}


def _sites():
    """(file, enclosing top-level function, entry name or None, call node or None) of every use of a native entry in lvc_amd/ and
    scripts/; a `size_query("lvc_...", ...)` comes as a call of that entry with the name taken off."""
    files = sorted(glob.glob(os.path.join(ROOT, "lvc_amd", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "scripts", "*.py")))
    for path in files:
        rel = os.path.relpath(path, ROOT)
        tree = ast.parse(open(path).read())
        called = set()

        def walk(node, func):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and func == "<module>":
                func = node.name
            if isinstance(node, ast.Call):
                f = node.func
                if isinstance(f, ast.Attribute) and f.attr.startswith("lvc_"):
                    called.add(id(f))
                    yield rel, func, f.attr, node
                elif isinstance(f, ast.Attribute) and f.attr == "size_query":
                    assert isinstance(node.args[0], ast.Constant), (rel, node.lineno)
                    yield rel, func, node.args[0].value, ast.Call(func=f, args=node.args[1:], keywords=node.keywords, lineno=node.lineno)
                elif isinstance(f, ast.Call) and isinstance(f.func, ast.Name) and f.func.id == "getattr" and "lib" in ast.unparse(f.args[0]):
                    yield rel, func, None, node
            elif isinstance(node, ast.Attribute) and node.attr.startswith("lvc_") and node.attr != "lvc_amd" and id(node) not in called:
                yield rel, func, node.attr, None      # an entry taken as a value
            for child in ast.iter_child_nodes(node):
                yield from walk(child, func)

        yield from walk(tree, "<module>")


def test_every_call_site_passes_the_headers_number_of_arguments():
    sigs = _lib.signatures()
    counted, starred, dynamic, wrong = 0, set(), set(), []
    for rel, func, name, call in _sites():
        if call is None:
            dynamic.add((rel, func))
            assert name in DYNAMIC.get((rel, func), ()), (rel, func, name)
            continue
        star = any(isinstance(a, ast.Starred) for a in call.args)
        assert not call.keywords, (rel, func)
        if star:
            starred.add((rel, func))
            assert name is None or name in (STARRED.get((rel, func)) or ()), (rel, func, name)
            continue
        if name is None:
            dynamic.add((rel, func))
            names = DYNAMIC.get((rel, func), ())
        else:
            names = (name,)
        for n in names:
            assert n in sigs, "{}:{} calls {}, which lvc_amd.h does not declare".format(rel, call.lineno, n)
            if len(call.args) != len(sigs[n][1]):
                wrong.append((rel, call.lineno, n, len(call.args), len(sigs[n][1])))
        counted += 1
    assert wrong == []
    assert counted >= 110
    assert starred == set(STARRED), "the list of starred call sites is not exact"
    assert dynamic == set(DYNAMIC), "the list of call sites with a run-time entry is not exact"
    for names in list(DYNAMIC.values()) + [v for v in STARRED.values() if v]:
        assert len({tuple(sigs[n][1]) for n in names}) == 1 and len({sigs[n][0] for n in names}) == 1, names


def test_the_recorder_counts_what_ctypes_lets_through():
    """scripts/conv_dispatch_trace.py stands in for the library on the starred conv sites: one argument too many raises there (ctypes
    would pass it on), and so does a float where the header has an int."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("conv_dispatch_trace", os.path.join(ROOT, "scripts", "conv_dispatch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec = mod.Recorder()
    assert rec.lvc_maxpool2d_nhwc(ctypes.c_void_p(1), None, 1, 8, 8, 32, 3, 2, 1, ctypes.c_void_p(0)) == 0
    assert rec.calls == [["lvc_maxpool2d_nhwc", [1, 8, 8, 32, 3, 2, 1], [0, 1, 1], 0]]
    with pytest.raises(TypeError, match="takes 10 arguments"):
        rec.lvc_maxpool2d_nhwc(ctypes.c_void_p(1), None, 1, 8, 8, 32, 3, 2, 1, ctypes.c_void_p(0), 0)
    with pytest.raises(TypeError):
        rec.lvc_maxpool2d_nhwc(ctypes.c_void_p(1), None, 1, 8.0, 8, 32, 3, 2, 1, ctypes.c_void_p(0))
    with pytest.raises(KeyError):
        rec.lvc_no_such_entry
