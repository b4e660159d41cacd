"""ctypes loader of the C-ABI kernel library `liblvc_amd.so`.  The ABI is declared in the headers under include/ that `HEADERS`
lists, each with the prefix of its entries: lvc_amd.h (`lvc_`), lvc_amd_seg.h (the semantic / panoptic entries, `lvcseg_`) and
lvc_amd_segtrain.h (the entries that train the semantic branch, `lvcst_`).  `signatures()` is the one loader of all of them and
`lib()` binds every entry from it.  A new entry is declared in lvc_amd.h under `lvc_`, and the count in tests/test_host_abi.py moves
with it in the same commit; a new header is one row in `HEADERS`, with no loader and no test file of its own.

The product path has NO CPU fallback: if the library is missing or a call fails, this raises.
Errors follow the reference's behaviour for its native ops (C++ exception -> Python RuntimeError,
reference detectron2/layers/csrc/ROIAlign/ROIAlign_cuda.cu:318-324): every C function returns an
int status, non-zero is re-raised here as RuntimeError carrying `lvc_last_error()`.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# LVC_AMD_LIB: another build of the same library (A/B measurements of one kernel against its predecessor in alternating processes)
_SO = os.environ.get("LVC_AMD_LIB") or os.path.join(_HERE, "liblvc_amd.so")
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
# The headers of the ABI and the prefix every declaration of each carries: the one list of them.  A new header is one row here.
HEADERS = (("lvc_amd.h", "lvc_"), ("lvc_amd_seg.h", "lvcseg_"), ("lvc_amd_segtrain.h", "lvcst_"))
_lib = None
_tables = {}      # header file name -> its parsed table; None -> the union

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_float = ctypes.c_float
c_longlong = ctypes.c_longlong

_SCALARS = {"int": c_int, "long long": c_longlong, "unsigned long long": ctypes.c_ulonglong, "float": c_float, "double": ctypes.c_double}


class LvcNativeError(RuntimeError):
    pass


def parse_header(text, prefix="lvc_", where="lvc_amd.h"):
    """{entry point: (restype, [argtypes])} from the text of a header of the ABI (a row of `HEADERS`): every declaration names a
    function that starts with `prefix`, and an error names the header as `where`.  The header is plain
    C99 without typedefs, structs or function pointers, so a declaration is `ret name(type name, ...);`.  Every pointer parameter is
    a c_void_p, whatever it points to (it takes `ptr(t)`, None, a ctypes host array and `byref`); a type that is not listed here is
    an error that names the declaration, never a default.  The variadic lvc_set_error is not bound."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*|^[ \t]*#[^\n]*|extern\s+\"C\"\s*\{|^\s*\}\s*$", " ", text, flags=re.M)
    table = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(" + re.escape(prefix) + r"\w+) ?\((.*)\)", decl)
        if m is None:
            raise ValueError("{}: cannot read the declaration `{}` (a function named {}*)".format(where, decl, prefix))
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        if "..." in params:
            continue
        if ret == "const char*":
            restype = ctypes.c_char_p
        elif ret == "void":
            restype = None
        elif ret in _SCALARS:
            restype = _SCALARS[ret]
        else:
            raise ValueError("{}: unknown return type `{}` in `{}`".format(where, ret, decl))
        argtypes = []
        for param in ([] if params == "void" else params.split(",")):
            if "*" in param:
                argtypes.append(c_void_p)
                continue
            ctype = " ".join(t for t in param.split()[:-1] if t != "const")      # the last word is the parameter's name
            if ctype not in _SCALARS:
                raise ValueError("{}: unknown parameter type in `{}` of `{}`".format(where, param.strip(), decl))
            argtypes.append(_SCALARS[ctype])
        table[name] = (restype, argtypes)
    return table


def signatures(header=None):
    """The parsed table of one header of `HEADERS` (by file name), or with None the whole ABI: the union of the tables, where a name
    declared in two headers is an error.  Read once per process.  Needs no liblvc_amd.so (scripts/conv_dispatch_trace.py records
    without one)."""
    if not _tables:
        tables, union = {}, {}
        for name, prefix in HEADERS:
            path = os.path.join(_INCLUDE, name)
            if not os.path.exists(path):
                raise ImportError("lvc_amd: the C ABI header {} not found; the native calls are bound from it "
                                  "(there is no hand-written table to fall back on)".format(path))
            with open(path) as f:
                tables[name] = parse_header(f.read(), prefix, where=name)
            twice = sorted(set(union) & set(tables[name]))
            if twice:
                raise ValueError("{}: {} declared in an earlier header too".format(name, ", ".join(twice)))
            union.update(tables[name])
        tables[None] = union
        _tables.update(tables)
    return _tables[header]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise ImportError(
                "lvc_amd: native library {} not found; build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C lvc_amd/csrc` "
                "(there is no CPU fallback)".format(_SO)
            )
        L = ctypes.CDLL(_SO)
        # every call is checked by ctypes against the header from here on: the number of arguments (too few), an int for an int, a
        # pointer for a pointer, and a `long long` travels whole
        for name, (restype, argtypes) in signatures().items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        if os.environ.get("LVC_WINO_STREAMK", "0") != "0":
            L.lvc_set_wino_streamk(int(os.environ["LVC_WINO_STREAMK"]))
        if os.environ.get("LVC_NMS_REDUCE_GLOBAL", "0") != "0":      # read once, here: the library itself never looks at the environment
            L.lvc_set_nms_reduce_global(1)
        if os.environ.get("LVC_SELECT_ONELAUNCH", "3") != "3":
            L.lvc_set_select_onelaunch(int(os.environ["LVC_SELECT_ONELAUNCH"]))
        _lib = L
    return _lib


def check(status, what=""):
    if status != 0:
        msg = lib().lvc_last_error().decode("utf-8", "replace")
        # a failed launch must not leave the thread's range slot on the failing layer (it is reset on the success path only):
        # later un-slotted launches would raise that layer's word instead of the shared one
        lib().lvc_set_range_slot(0)
        raise LvcNativeError("{} failed (status {}): {}".format(what or "lvc_amd native call", status, msg))


def size_query(name, *args):
    """What a `*_workspace_bytes` entry answers for these C arguments, as a Python int (the header gives them a long long return);
    a negative answer means arguments outside the kernel's range."""
    nbytes = getattr(lib(), name)(*args)
    if nbytes < 0:
        raise LvcNativeError("{} answered {}: arguments outside the kernel's range".format(name, nbytes))
    return nbytes


def ptr(t):
    """Device (or host) pointer of a tensor, or NULL for None."""
    if t is None:
        return c_void_p(0)
    return c_void_p(t.data_ptr())


def current_stream(device=None):
    import torch

    return c_void_p(torch.cuda.current_stream(device).cuda_stream)
