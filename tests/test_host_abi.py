"""The C ABI is stated once, in the headers that lvc_amd/_lib.py's HEADERS lists (include/lvc_amd.h, lvc_amd_seg.h, lvc_amd_segtrain.h),
and both of its other sides are held to it: the definitions by the compiler (csrc/common.h includes the headers), the Python calls by
ctypes (_lib.lib() binds restype / argtypes from the parsed headers).  This is the one test module of all of them: a new entry moves
the count below in the same commit, a new header is one row in HEADERS and one in ENTRIES.  Everything here runs on the host; no
kernel is launched."""
import ast
import ctypes
import functools
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
V, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
# the younger headers, entry by entry (lvc_amd.h is pinned by its count and spot checks)
ENTRIES = {
    "lvc_amd_seg.h": {
        "lvcseg_upsample2_bilinear_nhwc": (I, [V, V, V, I, I, I, I, V]),
        "lvcseg_sem_seg_postprocess": (I, [V, L, V, V, I, I, I, I, V, L, V, L, I, V]),
        "lvcseg_panoptic_combine": (I, [V, L, V, V, I, I, V, V, V, L, I, I, V, V, I, D, D, D, V, L, V, L, V, V]),
    },
    "lvc_amd_segtrain.h": {
        "lvcst_upsample2_bilinear_bwd_nhwc": (I, [V, V, I, I, I, I, V]),
        "lvcst_sem_seg_loss_workspace_bytes": (L, [I, I, I, I, I]),
        "lvcst_sem_seg_loss_fwd": (I, [V, I, I, I, I, I, I, V, L, I, L, V, V, V, V, V, V, L, V, V, V, V, V]),
        "lvcst_sem_seg_loss_bwd": (I, [V, I, I, I, I, I, I, V, L, I, L, V, V, V, V, V, V, V, V]),
    },
}


# ------------------------------------------------------------------------------------------------ the parser
def test_every_declaration_parses_to_known_kinds():
    sigs = _lib.signatures("lvc_amd.h")
    assert len(sigs) == 153 and "lvc_set_error" not in sigs      # 154 declarations, the variadic one is not bound
    for name, (restype, argtypes) in _lib.signatures().items():
        assert restype in (None, ctypes.c_char_p, ctypes.c_int, ctypes.c_longlong), name
        assert all(t in KINDS for t in argtypes), name
    assert sigs["lvc_last_error"] == (ctypes.c_char_p, [])
    assert sigs["lvc_set_range_slot"] == (None, [ctypes.c_int])
    assert sigs["lvc_batched_nms_workspace_bytes"] == (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int])
    assert sigs["lvc_subsample_batched"][1][:4] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_int]
    assert sigs["lvc_keypoint_loss"][1][7:9] == [ctypes.c_double, ctypes.c_double]
    assert sigs["lvc_rownorm"][1][7] is ctypes.c_float


@pytest.mark.parametrize("header", sorted(ENTRIES))
def test_the_younger_headers_parse_to_exactly_their_entries(header):
    assert _lib.signatures(header) == ENTRIES[header]


def test_the_tables_are_disjoint_and_each_keeps_to_its_prefix():
    assert [h for h, _ in _lib.HEADERS] == ["lvc_amd.h"] + sorted(ENTRIES)
    tables = {h: _lib.signatures(h) for h, _ in _lib.HEADERS}
    for i, (header, prefix) in enumerate(_lib.HEADERS):
        assert all(name.startswith(prefix) for name in tables[header]), header
        assert not any(name.startswith(theirs) for name in tables[header] for _, theirs in _lib.HEADERS if theirs != prefix), header
        text = open(os.path.join(ROOT, "include", header)).read()
        for other, theirs in _lib.HEADERS[i + 1:]:
            assert not set(tables[header]) & set(tables[other]), (header, other)
            # a younger header's comments refer to the older ones' entries; an older header's text, comments included, never names a
            # younger prefix (a declaration of another family anywhere does not parse: the prefix tests below)
            assert theirs not in text, "{} names the prefix of {}".format(header, other)
    assert len(_lib.signatures()) == 160 == sum(len(t) for t in tables.values())
    assert all(_lib.signatures()[name] == sig for t in tables.values() for name, sig in t.items())


def test_an_unknown_type_raises_and_names_the_declaration():
    ok = _lib.parse_header("/* c */ int lvc_x(const float* a, int n /* rows */, void* stream);   // tail\nlong long lvc_y(void);")
    assert ok == {"lvc_x": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]), "lvc_y": (ctypes.c_longlong, [])}
    with pytest.raises(ValueError, match="size_t n.*lvc_x"):
        _lib.parse_header("int lvc_x(const float* a, size_t n);")
    with pytest.raises(ValueError, match="float\\*.*lvc_x"):
        _lib.parse_header("float* lvc_x(int n);")


def test_parse_header_takes_the_prefix_and_defaults_to_the_first():
    text = "int lvcseg_x(const float* a, long long n, double t, void* stream);"
    assert _lib.parse_header(text, prefix="lvcseg_") == {"lvcseg_x": (I, [V, L, D, V])}
    assert _lib.parse_header("int lvc_y(int n);") == {"lvc_y": (I, [I])}
    with pytest.raises(ValueError, match="lvcseg_"):
        _lib.parse_header("int lvc_y(int n);", prefix="lvcseg_")      # a declaration of another family in this header
    with pytest.raises(ValueError, match="size_t n.*lvcseg_x"):
        _lib.parse_header("int lvcseg_x(size_t n);", prefix="lvcseg_")
    assert _lib.parse_header("int lvcst_x(const float* a, long long n, void* stream);", prefix="lvcst_") == {"lvcst_x": (I, [V, L, V])}
    with pytest.raises(ValueError, match="lvcst_"):
        _lib.parse_header("int lvcseg_y(int n);", prefix="lvcst_")      # a declaration of another family in this header


def test_parse_header_errors_name_the_header_being_read():
    for text in ("int lvc_y(int n);", "float* lvcst_x(int n);", "int lvcst_x(size_t n);"):
        with pytest.raises(ValueError, match="^lvc_amd_segtrain\\.h: "):
            _lib.parse_header(text, prefix="lvcst_", where="lvc_amd_segtrain.h")
    with pytest.raises(ValueError, match="^lvc_amd\\.h: "):
        _lib.parse_header("int lvc_x(size_t n);")


def test_the_loader_refuses_a_name_declared_twice_and_a_missing_header(monkeypatch):
    with pytest.raises(KeyError):
        _lib.signatures("lvc_amd_none.h")      # not a row of HEADERS
    monkeypatch.setattr(_lib, "_tables", {})
    monkeypatch.setattr(_lib, "HEADERS", _lib.HEADERS + (("lvc_amd_seg.h", "lvcseg_"),))
    with pytest.raises(ValueError, match="lvcseg_panoptic_combine.*declared in an earlier header"):
        _lib.signatures()
    monkeypatch.setattr(_lib, "HEADERS", _lib.HEADERS[:3] + (("lvc_amd_none.h", "lvcnone_"),))
    with pytest.raises(ImportError, match="lvc_amd_none\\.h not found"):
        _lib.signatures("lvc_amd.h")
    assert _lib._tables == {}      # a failed read leaves nothing half-loaded behind


# ------------------------------------------------------------------------------------------------ exports
@functools.lru_cache(maxsize=None)
def _exported():
    """Every exported symbol that starts with `lvc`: one nm call for the module."""
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.check_output([nm, "-D", "--defined-only", _lib._SO], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("lvc")}


def test_declared_and_exported_symbols_are_the_same_set():
    declared = set(_lib.signatures()) | {"lvc_set_error"}
    exported = _exported() - INTERNAL
    assert INTERNAL <= _exported() and not INTERNAL & declared
    assert declared - exported == set(), "declared in a header of the ABI, not exported by liblvc_amd.so"
    assert exported - declared == set(), "exported lvc* symbols that are neither declared nor on the internal list"


@pytest.mark.parametrize("header", sorted(ENTRIES))
def test_a_younger_header_declares_exactly_the_exports_under_its_prefix(header):
    """The comparison above, header by header: a failure there names the header here."""
    prefix = dict(_lib.HEADERS)[header]
    assert {name for name in _exported() if name.startswith(prefix)} == set(_lib.signatures(header))


def test_every_bound_function_carries_the_header_signature():
    lib = _lib.lib()
    for name, (restype, argtypes) in _lib.signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.lvc_abi_version() == 1


# ------------------------------------------------------------------------------------------------ the compiler check bites
_UNITS = {
    "lvc_colsum": 'int lvc_colsum(const float* x, {} M, int N, int ldx, float* out, void* stream) {{ return M + N; }}',
    "lvcseg_upsample2_bilinear_nhwc": ('int lvcseg_upsample2_bilinear_nhwc(const float* x, const float* acc, float* y, {} N, int H, int W, '
                                       'int C, void* stream) {{ return N + H; }}'),
    "lvcst_upsample2_bilinear_bwd_nhwc": ('int lvcst_upsample2_bilinear_bwd_nhwc(const float* dy, float* dx, {} N, int H, int W, int C, '
                                          'void* stream) {{ return N + H; }}'),
}


# (the ids of the lvc_colsum cases stay the ones they had when that was the only unit: `int-True`, `long long-False`)
@pytest.mark.parametrize("entry, first_int, compiles", [
    pytest.param(entry, first_int, compiles, id="{}{}-{}".format("" if entry == "lvc_colsum" else entry + "-", first_int, compiles))
    for entry in sorted(_UNITS) for first_int, compiles in (("int", True), ("long long", False))])
def test_a_definition_that_differs_from_the_header_does_not_compile(tmp_path, entry, first_int, compiles):
    src = tmp_path / "unit.hip"
    src.write_text('#include "{}"\nextern "C" {}\n'.format(os.path.join(ROOT, "lvc_amd", "csrc", "common.h"), _UNITS[entry].format(first_int)))
    r = subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert (r.returncode == 0) == compiles, r.stderr
    if not compiles:
        assert entry in r.stderr and "conflicting types" in r.stderr


# ------------------------------------------------------------------------------------------------ ctypes rejects bad calls
def test_ctypes_rejects_a_bad_call_of_a_host_only_query():
    lib = _lib.lib()
    assert lib.lvc_batched_nms_workspace_bytes(2, 1000) > 0
    with pytest.raises(TypeError):
        lib.lvc_batched_nms_workspace_bytes(2)
    with pytest.raises(ctypes.ArgumentError):
        lib.lvc_batched_nms_workspace_bytes(2, 1000.0)
    with pytest.raises(ctypes.ArgumentError):
        _lib.size_query("lvc_batched_nms_workspace_bytes", 2, 1000.0)
    assert lib.lvc_batched_nms_workspace_bytes(ctypes.c_int(2), ctypes.c_int(1000)) == lib.lvc_batched_nms_workspace_bytes(2, 1000)


@pytest.mark.parametrize("entry, ptrs", [("lvcseg_upsample2_bilinear_nhwc", 3), ("lvcst_upsample2_bilinear_bwd_nhwc", 2)])
def test_ctypes_rejects_a_bad_call_of_an_entry_of_the_younger_headers(entry, ptrs):
    fn = getattr(_lib.lib(), entry)
    nulls = (None,) * ptrs
    with pytest.raises(TypeError):
        fn(*nulls, 1, 1, 1, 4)              # one argument short
    with pytest.raises(ctypes.ArgumentError):
        fn(*nulls, 1.0, 1, 1, 4, None)      # a float for an int
    # a host-side refusal comes back as a status and a text, no launch: N = 1 with null pointers
    assert fn(*nulls, 1, 1, 1, 4, None) == 1
    assert b"null pointer" in _lib.lib().lvc_last_error()
    assert fn(*nulls, 1, 1, 1, 6, None) == 1
    assert b"multiple of 4" in _lib.lib().lvc_last_error()


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
    ("lvc_amd/kernels.py", "_mask_deconv"): ("lvc_mask_deconv_predict", "lvc_mask_deconv_logits"),
}


def _sites():
    """(file, enclosing top-level function, entry name or None, call node or None) of every use of a native entry in lvc_amd/ and
    scripts/: every attribute that starts with `lvc` (which every prefix of HEADERS does; the package's own name aside) has to be a
    declared entry; a `size_query("lvc...", ...)` comes as a call of that entry with the name taken off."""
    files = sorted(glob.glob(os.path.join(ROOT, "lvc_amd", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "scripts", "*.py")))
    for path in files:
        rel = os.path.relpath(path, ROOT)
        tree = ast.parse(open(path).read())
        called = set()

        def entry(node):
            return isinstance(node, ast.Attribute) and node.attr.startswith("lvc") and node.attr != "lvc_amd"

        def walk(node, func):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and func == "<module>":
                func = node.name
            if isinstance(node, ast.Call):
                f = node.func
                if entry(f):
                    called.add(id(f))
                    yield rel, func, f.attr, node
                elif isinstance(f, ast.Attribute) and f.attr == "size_query":
                    assert isinstance(node.args[0], ast.Constant), (rel, node.lineno)
                    yield rel, func, node.args[0].value, ast.Call(func=f, args=node.args[1:], keywords=node.keywords, lineno=node.lineno)
                elif isinstance(f, ast.Call) and isinstance(f.func, ast.Name) and f.func.id == "getattr" and "lib" in ast.unparse(f.args[0]):
                    yield rel, func, None, node
            elif entry(node) and id(node) not in called:
                yield rel, func, node.attr, None      # an entry taken as a value
            for child in ast.iter_child_nodes(node):
                yield from walk(child, func)

        yield from walk(tree, "<module>")


@functools.lru_cache(maxsize=None)
def _walked():
    """The one walk over the call sites: (sites counted, functions with a starred site, functions with a run-time entry, sites with
    another number of arguments than the header's, entries called at a counted site)."""
    sigs = _lib.signatures()
    counted, starred, dynamic, wrong, called = 0, set(), set(), [], set()
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
            assert n in sigs, "{}:{} calls {}, which no header of the ABI declares".format(rel, call.lineno, n)
            if len(call.args) != len(sigs[n][1]):
                wrong.append((rel, call.lineno, n, len(call.args), len(sigs[n][1])))
        called.update(names)
        counted += 1
    return counted, starred, dynamic, wrong, called


def test_every_call_site_passes_the_headers_number_of_arguments():
    sigs = _lib.signatures()
    counted, starred, dynamic, wrong, _ = _walked()
    assert wrong == []
    assert counted >= 110
    assert starred == set(STARRED), "the list of starred call sites is not exact"
    assert dynamic == set(DYNAMIC), "the list of call sites with a run-time entry is not exact"
    for names in list(DYNAMIC.values()) + [v for v in STARRED.values() if v]:
        assert len({tuple(sigs[n][1]) for n in names}) == 1 and len({sigs[n][0] for n in names}) == 1, names


@pytest.mark.parametrize("header", sorted(ENTRIES))
def test_every_entry_of_the_younger_headers_is_called_at_a_counted_site(header):
    """No entry of these headers is reached through a star or a run-time name (the lists above hold none), so each is counted."""
    prefix = dict(_lib.HEADERS)[header]
    assert {n for n in _walked()[4] if n.startswith(prefix)} == set(ENTRIES[header])


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
