"""Which native entry point does a conv/GEMM layer run on, with which integer arguments, under which switches?

Default mode (no GPU, no liblvc_amd.so): the native library is replaced by a recorder, the tensors are `device="meta"`, the layers
are attribute bags with PackedConv's fields -- the host dispatch of lvc_amd/kernels.py runs as it is and its launches are written
down.  The grid covers the distinct conv/GEMM layers of R50-FPN at the bench batch, the ViT's linear shapes, small maps, the f32
engine, every routing switch one at a time against the defaults, and the grouped / fused entry points.

    python scripts/conv_dispatch_trace.py --out tests/golden/conv_dispatch_trace.json

tests/test_host_conv_dispatch.py runs `trace()` on the working tree and compares with that file.

--model (needs the MI355X): the recorder forwards to the real library; the launch stream (entry points + integer arguments) of one
`inference_batched` of the bench model and of one training step is written to --out, to be compared between two checkouts.

A launch is recorded as [entry point, integer arguments, NULL flags of the pointer arguments, range slot in effect]; the calls of
lvc_set_range_slot themselves only show as that last field (and as the slot left behind, which must be 0).  The written file holds
what ran per case and a digest of the complete records per cell (`compact`); --full writes every record, to diff two checkouts.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from lvc_amd import _lib  # noqa: E402


# ------------------------------------------------------------------------------------------------ the recording library
def _arg(ctype, a):
    """('i', value) for a scalar parameter of the header's type `ctype`, ('p', is NULL) for a pointer one; a ctypes host array in a
    pointer's place is recorded by its entries."""
    if ctype is not ctypes.c_void_p:
        return "i", a.value if isinstance(a, ctype) else ctype(a).value      # ctype(a): what ctypes passes, or its TypeError
    if isinstance(a, ctypes.Array):
        if issubclass(a._type_, ctypes.c_void_p):
            return "p", [0 if v else 1 for v in a]
        return "i", [v for v in a]
    if isinstance(a, ctypes.c_void_p):
        return "p", 0 if a.value else 1
    if a is None or isinstance(a, ctypes._Pointer) or type(a).__name__ == "CArgObject":
        return "p", 1 if a is None else 0
    raise TypeError("unexpected native argument {!r} for a pointer parameter".format(a))


class _Fn:
    """One entry point of the recorder: checks the call against the header (ctypes itself lets extra arguments through), records,
    then returns the recorder's status or forwards to the real function."""

    def __init__(self, rec, name, real):
        self._rec, self._name, self._real = rec, name, real
        self._argtypes = _lib.signatures()[name][1]      # KeyError: not an entry point of any header of the ABI

    def __call__(self, *args):
        rec = self._rec
        if self._name == "lvc_last_error":
            return self._real(*args) if self._real is not None else b"recorded failure"
        if len(args) != len(self._argtypes):
            raise TypeError("{} takes {} arguments ({} given)".format(self._name, len(self._argtypes), len(args)))
        ints, nulls = [], []
        for ctype, a in zip(self._argtypes, args):
            kind, v = _arg(ctype, a)
            (ints if kind == "i" else nulls).append(v)
        rec.raw.append((self._name, ints))
        if self._name == "lvc_set_range_slot":
            rec.slot = ints[0]
        elif rec.keep(self._name):
            rec.calls.append([self._name, ints, nulls, rec.slot])
        if self._real is not None:
            return self._real(*args)
        return rec.status


class Recorder:
    """Stands in for `_lib.lib()`.  calls: the launches since `reset`; raw: every call, lvc_set_range_slot included."""

    def __init__(self, real=None, keep=lambda name: True):
        self.real, self.keep, self.status, self._fns = real, keep, 0, {}
        self.reset()

    def reset(self):
        self.calls, self.raw, self.slot = [], [], 0

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        fn = self._fns.get(name)
        if fn is None:
            fn = self._fns[name] = _Fn(self, name, getattr(self.real, name) if self.real is not None else None)
        return fn


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self, stream=None):
        pass

    def elapsed_time(self, other):
        return 0.0


def meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype)


class install_stubs:
    """Context manager: the recorder as the native library, and stubs for what needs a device (only names kernels.py has had
    all along are patched).  Restores everything on exit."""

    def __init__(self, rec):
        self.rec = rec

    def __enter__(self):
        from lvc_amd import kernels as K

        self.saved = [(_lib, "lib", _lib.lib), (torch.cuda, "Event", torch.cuda.Event)] + [
            (K, n, getattr(K, n)) for n in ("_req_cuda", "_stream", "conv_workspace", "pack_wino", "ptr")]
        rec = self.rec
        _lib.lib = lambda: rec
        torch.cuda.Event = _Event
        K._req_cuda = lambda *ts: None
        K._stream = lambda t: ctypes.c_void_p(0)
        K.conv_workspace = lambda device: meta(16, dtype=torch.uint8)
        K.pack_wino = lambda pc: (meta(3, pc.C // 16, 4, 2, (pc.K + 127) // 128 * 128, 16, dtype=torch.int16), meta(pc.K))
        K.ptr = lambda t: ctypes.c_void_p(0 if t is None else 1)      # meta tensors have no address: NULL-ness is what is recorded
        return K

    def __exit__(self, *exc):
        for obj, name, val in self.saved:
            setattr(obj, name, val)


# ------------------------------------------------------------------------------------------------ stand-in layers
class Layer:
    """PackedConv's fields without its device memory."""

    def __init__(self, R, S, C, K, stride=1, pad=0, mode=0, two_acc=False, tier=0, affine=True, slot=1):
        self.R, self.S, self.C, self.K, self.stride, self.pad, self.mode = R, S, C, K, stride, pad, mode
        self.Kg = R * 32 if mode == 1 else R * S * C
        self.rows = (K + 127) // 128 * 128
        self.w = meta(self.rows, self.Kg)
        self.scale = meta(K) if affine else None
        self.shift = meta(K)
        self.two_acc, self.slot, self.state = two_acc, slot, {"tier": tier}
        self.last_one = "unset"

    def split2s(self):
        return meta(2, self.rows, self.Kg, dtype=torch.float16), meta(self.K)

    def split2h(self):
        return meta(2, self.rows, self.Kg, dtype=torch.float16)

    def split3(self):
        return meta(3, self.rows, self.Kg, dtype=torch.bfloat16)


# name: (R, S, C, K, stride, pad, mode, (N, H, W) of the input).  R50-FPN at the bench batch (8 images of 800 x 1333, padded to
# 800 x 1344: p2 200 x 336 ... p6 13 x 21); the first 1x1 layer of a stage carries its stride.
P = {2: (200, 336), 3: (100, 168), 4: (50, 84), 5: (25, 42), 6: (13, 21)}
LAYERS = {}


def _add(name, R, S, C, K, stride, pad, nhw, mode=0):
    LAYERS[name] = (R, S, C, K, stride, pad, mode, nhw)


def _layers():
    N = 8
    cin = 64
    for stage, mid in ((2, 64), (3, 128), (4, 256), (5, 512)):
        out, s = 4 * mid, 1 if stage == 2 else 2
        Hi, Wi = P[stage - 1] if stage > 2 else P[2]
        Ho, Wo = P[stage]
        _add("res%d.0.conv1" % stage, 1, 1, cin, mid, s, 0, (N, Hi, Wi))
        _add("res%d.0.shortcut" % stage, 1, 1, cin, out, s, 0, (N, Hi, Wi))
        _add("res%d.conv2" % stage, 3, 3, mid, mid, 1, 1, (N, Ho, Wo))
        _add("res%d.conv3" % stage, 1, 1, mid, out, 1, 0, (N, Ho, Wo))
        _add("res%d.1.conv1" % stage, 1, 1, out, mid, 1, 0, (N, Ho, Wo))
        _add("fpn.lateral%d" % stage, 1, 1, out, 256, 1, 0, (N, Ho, Wo))
        _add("fpn.output%d" % stage, 3, 3, 256, 256, 1, 1, (N, Ho, Wo))
        cin = out
    _add("res3.0.conv2_s2", 3, 3, 128, 128, 2, 1, (N,) + P[2])          # the stride on the 3x3 layer instead (STRIDE_IN_1X1 off)
    _add("res2.0.fused_projection", 1, 1, 128, 256, 1, 0, (N,) + P[2])
    for lvl in range(2, 7):
        _add("rpn.conv.p%d" % lvl, 3, 3, 256, 256, 1, 1, (N,) + P[lvl])
        _add("rpn.pred.p%d" % lvl, 1, 1, 256, 15, 1, 0, (N,) + P[lvl])
    _add("box.fc1", 1, 1, 12544, 1024, 1, 0, (8000, 1, 1))
    _add("box.fc2", 1, 1, 1024, 1024, 1, 0, (8000, 1, 1))
    _add("box.cls_score", 1, 1, 1024, 81, 1, 0, (8000, 1, 1))
    _add("box.bbox_pred", 1, 1, 1024, 320, 1, 0, (8000, 1, 1))
    _add("box.fc1.train", 1, 1, 12544, 1024, 1, 0, (4096, 1, 1))
    # ViT-S/8: 8 crops of 785 tokens, width 384
    _add("vit.qkv", 1, 1, 384, 1152, 1, 0, (6280, 1, 1))
    _add("vit.proj", 1, 1, 384, 384, 1, 0, (6280, 1, 1))
    _add("vit.fc1", 1, 1, 384, 1536, 1, 0, (6280, 1, 1))
    _add("vit.fc2", 1, 1, 1536, 384, 1, 0, (6280, 1, 1))
    _add("vit.head.cls", 1, 1, 384, 384, 1, 0, (8, 1, 1))               # fewer than 2048 rows
    # small maps: the tile-count threshold
    _add("fpn.output5.n2", 3, 3, 256, 256, 1, 1, (2,) + P[5])
    _add("fpn.output6", 3, 3, 256, 256, 1, 1, (8,) + P[6])
    # the f32 engine: fewer than 64 output channels, and the stem's row mode
    _add("narrow3x3", 3, 3, 64, 32, 1, 1, (8,) + P[4])
    _add("narrow1x1.fewrows", 1, 1, 256, 32, 1, 0, (1,) + P[5])
    _add("narrow1x1.k48", 1, 1, 256, 48, 1, 0, (8,) + P[3])             # with a residual: rows the LDS-DMA kernel does not move
    _add("stem", 7, 7, 4, 64, 2, 3, (8, 800, 1344), mode=1)


_layers()

# every switch setting is one change against the defaults
SETTINGS = [("default", {}), ("CONV_ENGINE=f32", {"CONV_ENGINE": "f32"}), ("CONV_SPLIT=bf16x3", {"CONV_SPLIT": "bf16x3"}),
            ("CONV_HALO=False", {"CONV_HALO": False})]
SETTINGS += [("HALO_S1=%d" % v, {"HALO_S1": v}) for v in (0, 1, 2)] + [("PW_S1=%d" % v, {"PW_S1": v}) for v in (0, 1, 2)]
SETTINGS += [("PW_W2=False", {"PW_W2": False}), ("CONV_WINO=False", {"CONV_WINO": False}), ("WINO_RPN=True", {"WINO_RPN": True}),
             ("PRESPLIT=True", {"PRESPLIT": True}), ("_HALO_H2_MIN_TILES=0", {"_HALO_H2_MIN_TILES": 0})]
DEFAULTS = {"CONV_ENGINE": "bf16x3", "CONV_SPLIT": "f16x2", "CONV_HALO": True, "HALO_S1": 2, "PW_S1": 2, "PW_W2": True,
            "CONV_WINO": True, "WINO_RPN": False, "PRESPLIT": False, "_HALO_H2_MIN_TILES": 64, "_WINO_MIN_TILES": 512}

TIERS = (0, 1, 2)
FORMS = (False, True)
SPLITS = (None, "f16x2", "bf16x3")
RESIDUALS = (0, 1, 2)
ACTS = ((False, None), (True, None), (False, "gelu"), (True, "gelu"))


class Tracer:
    def __init__(self, K, rec):
        self.K, self.rec = K, rec
        self.blobs, self.blob_ids = [], {}      # distinct outcomes of a call
        self.lists, self.list_ids = [], {}      # distinct outcome lists of a (setting, layer) cell

    def settings(self, change):
        for k, v in DEFAULTS.items():
            setattr(self.K, k, change.get(k, v))

    def run(self, fn, layers):
        """Outcome of one dispatch call: its launches, the timer's records and the layers' last_one."""
        K, rec = self.K, self.rec
        rec.reset()
        K._NEXT_SLOT[0] = 500
        K._GROUP_SLOTS.clear()
        K._SLOT_OWNERS.clear()
        K.CONV_TIMER = timer = K.LaunchTimer()
        try:
            ret = fn()
            ret = "none" if ret is None else "ok"
        except (AssertionError, ValueError, RuntimeError) as e:
            ret = type(e).__name__
        finally:
            K.CONV_TIMER = None
        out = {"ret": ret, "calls": rec.calls, "end_slot": rec.slot, "timer": [[r[3], r[0], r[4]] for r in timer.records],
               "last_one": [q.last_one for q in layers]}
        key = json.dumps(out, sort_keys=True)
        i = self.blob_ids.get(key)
        if i is None:
            i = self.blob_ids[key] = len(self.blobs)
            self.blobs.append(out)
        return i

    def cell(self, ids):
        key = tuple(ids)
        i = self.list_ids.get(key)
        if i is None:
            i = self.list_ids[key] = len(self.lists)
            self.lists.append(list(ids))
        return i

    def conv2d_case(self, name, tier, two_acc, split, res, relu, act, out=None, n=None):
        R, S, C, Kc, stride, pad, mode, (N, H, W) = LAYERS[name]
        N = n or N
        pc = Layer(R, S, C, Kc, stride, pad, mode, two_acc=two_acc, tier=tier)
        Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
        x = meta(N, H, W, C)
        residual = None if res == 0 else meta(N, Ho, Wo, Kc) if res == 1 else meta(N, (Ho + 1) // 2, (Wo + 1) // 2, Kc)
        o = None if out is None else out(N, Ho, Wo, Kc)
        return self.run(lambda: self.K.conv2d_nhwc(x, pc, relu=relu, residual=residual, res_mode=res, out=o, split=split, act=act), [pc])

    def conv2d_grid(self, name):
        return [self.conv2d_case(name, tier, two_acc, split, res, relu, act)
                for tier in TIERS for two_acc in FORMS for split in SPLITS for res in RESIDUALS for relu, act in ACTS]

    # ---- the entry points beyond conv2d_nhwc
    def extras(self):
        K = self.K
        ids = []

        def note(label, i):
            ids.append([label, i])

        # a non-contiguous `out` (a channel slice of a wider buffer) and an `out` with a wider last dimension
        for name in ("res2.conv2", "fpn.output2", "res4.conv3", "res2.0.conv1", "fpn.lateral3", "box.bbox_pred"):
            for two_acc in FORMS:
                note("out_slice/%s/%d" % (name, two_acc), self.conv2d_case(
                    name, 0, two_acc, None, 0, True, None, out=lambda N, Ho, Wo, Kc: meta(N, Ho, Wo, Kc + 64)[..., :Kc]))
                note("out_wide/%s/%d" % (name, two_acc), self.conv2d_case(
                    name, 0, two_acc, None, 0, True, None, out=lambda N, Ho, Wo, Kc: meta(N, Ho, Wo, Kc + 64)))
        # 2^29 elements in one tensor: the image-group split
        for name, n in (("fpn.output2", 32), ("res2.conv3", 32), ("fpn.lateral2", 40), ("res2.0.conv1", 160)):
            for res in (0, 1):
                note("batch_split/%s/n%d/res%d" % (name, n, res), self.conv2d_case(name, 0, False, None, res, True, None, n=n))
        # conv3x3_levels: the shared layer (RPN head) and a layer per map (FPN outputs); mixed forms; a big level
        for levels in ((2, 3, 4, 5, 6), (4, 5, 6), (3, 4), (2,)):
            xs = [meta(8, P[l][0], P[l][1], 256) for l in levels]
            for tier in TIERS:
                for two_acc in FORMS:
                    pc = Layer(3, 3, 256, 256, 1, 1, two_acc=two_acc, tier=tier, slot=7)
                    note("levels_shared/%s/t%d/f%d" % (levels, tier, two_acc), self.run(lambda: K.conv3x3_levels(xs, pc, relu=True), [pc]))
                    pcs = [Layer(3, 3, 256, 256, 1, 1, two_acc=two_acc, tier=tier, slot=10 + i) for i in range(len(xs))]
                    note("levels_list/%s/t%d/f%d" % (levels, tier, two_acc), self.run(lambda: K.conv3x3_levels(xs, pcs, relu=False), pcs))
            pcs = [Layer(3, 3, 256, 256, 1, 1, two_acc=(i == 1), slot=10 + i) for i in range(len(xs))]
            note("levels_list_mixed/%s" % (levels,), self.run(lambda: K.conv3x3_levels(xs, pcs), pcs))
            pcs = [Layer(3, 3, 256, 256, 1, 1, slot=10 + i, affine=(i != 0)) for i in range(len(xs))]
            outs = [meta(8, P[l][0], P[l][1], 256) for l in levels]
            note("levels_list_outs/%s" % (levels,), self.run(lambda: K.conv3x3_levels(xs, pcs, relu=True, outs=outs), pcs))
        xs = [meta(8, P[l][0], P[l][1], 64) for l in (4, 5)]
        pcs = [Layer(3, 3, 64, 64, 1, 1, slot=10 + i) for i in range(2)]
        note("levels_list_k64", self.run(lambda: K.conv3x3_levels(xs, pcs, relu=True), pcs))
        # conv3x3_levels_pred: the RPN head with its predictors in the epilogue
        for levels in ((2, 3, 4, 5, 6), (4, 5, 6), (6,), (2, 3)):
            xs = [meta(8, P[l][0], P[l][1], 256) for l in levels]
            for tier in TIERS:
                for two_acc in FORMS:
                    for ptier in (0, 2):
                        pc = Layer(3, 3, 256, 256, 1, 1, two_acc=two_acc, tier=tier, slot=7)
                        pred = Layer(1, 1, 256, 15, two_acc=True, tier=ptier, slot=8)
                        note("levels_pred/%s/t%d/f%d/p%d" % (levels, tier, two_acc, ptier),
                             self.run(lambda: K.conv3x3_levels_pred(xs, pc, pred, relu=True), [pc, pred]))
        pc, pred = Layer(3, 3, 256, 512, 1, 1, two_acc=True, slot=7), Layer(1, 1, 512, 15, two_acc=True, slot=8)
        xs = [meta(8, P[l][0], P[l][1], 256) for l in (4, 5)]
        note("levels_pred_k512", self.run(lambda: K.conv3x3_levels_pred(xs, pc, pred), [pc, pred]))
        # the chained pair, the fused bottleneck, the pre-split pair
        for k1, n1, n2, res in ((64, 256, 64, False), (128, 256, 64, False), (128, 512, 128, True)):
            ch = K.PackedChain()
            ch.slot, ch.state, ch.K1, ch.N1, ch.N2 = 21, {"off": False}, k1, n1, n2
            ch.wa, ch.sa, ch.ta = meta(2, (n1 + 127) // 128 * 128, k1, dtype=torch.float16), meta(n1), meta(n1)
            ch.wb, ch.sb, ch.tb = meta(2, (n2 + 127) // 128 * 128, n1, dtype=torch.float16), meta(n2), meta(n2)
            x = meta(8, 100, 168, k1)
            residual = meta(8, 100, 168, n1) if res else None
            note("chain/%d-%d-%d" % (k1, n1, n2), self.run(lambda: K.conv1x1_chain(x, ch, residual=residual, relu2=not res), []))
        for cin, proj in ((256, False), (64, True)):
            bk = K.PackedBneck()
            bk.slot, bk.state, bk.cin, bk.proj = 22, {"off": False}, cin, proj
            bk.w = meta(1024, dtype=torch.float16)
            bk.s1 = bk.t1 = bk.s2 = bk.t2 = meta(64)
            bk.s3 = bk.t3 = meta(256)
            x = meta(8, 200, 336, cin)
            note("bneck/%d/%d" % (cin, proj), self.run(lambda: K.bottleneck_fused(x, bk), []))
        for stage, mid in ((3, 128), (4, 256), (5, 512)):
            for res in (False, True):
                for relu in (False, True):
                    pc2, pc3 = Layer(3, 3, mid, mid, 1, 1, slot=31), Layer(1, 1, mid, 4 * mid, slot=32)
                    x = meta(8, P[stage][0], P[stage][1], mid)
                    residual = meta(8, P[stage][0], P[stage][1], 4 * mid) if res else None
                    note("presplit/res%d/res%d/relu%d" % (stage, res, relu),
                         self.run(lambda: K.conv3x3_conv1x1_presplit(x, pc2, pc3, residual=residual, relu=relu), [pc2, pc3]))
        return ids

    def presplit_pairs(self):
        """presplit_pair_ok of every (3x3, 1x1) pair of the layer table on the 3x3 layer's input, per range tier and form, with the
        PRESPLIT switch on under every setting (off, every pair is refused: the last bit is the first case under the setting's own)."""
        K = self.K
        own, K.PRESPLIT = K.PRESPLIT, True
        names2 = [n for n, l in LAYERS.items() if l[0] == 3]
        names3 = [n for n, l in LAYERS.items() if l[0] == 1]
        out = []
        for n2 in names2:
            R, S, C, K2, stride, pad, mode, (N, H, W) = LAYERS[n2]
            x = meta(N, H, W, C)
            for n3 in names3:
                l3 = LAYERS[n3]
                bits = ""
                for t2, f2, t3, f3, res in ((0, False, 0, False, 0), (0, False, 0, False, 1), (1, False, 0, False, 0), (0, True, 0, False, 0),
                                            (0, False, 1, False, 0), (0, False, 0, True, 0), (0, False, 2, False, 1)):
                    pc2 = Layer(R, S, C, K2, stride, pad, mode, two_acc=f2, tier=t2)
                    pc3 = Layer(1, 1, l3[2], l3[3], l3[4], l3[5], l3[6], two_acc=f3, tier=t3)
                    residual = meta(N, H, W, l3[3]) if res else None
                    bits += "1" if K.presplit_pair_ok(x, pc2, pc3, residual) else "0"
                K.PRESPLIT = own
                bits += "1" if K.presplit_pair_ok(x, Layer(R, S, C, K2, stride, pad, mode), Layer(1, 1, *l3[2:7]), None) else "0"
                K.PRESPLIT = True
                out.append(bits)
        K.PRESPLIT = own
        return {"conv2": names2, "conv3": names3, "cases": "(tier2, two_acc2, tier3, two_acc3, residual) x 7, PRESPLIT on; then the first under the setting's PRESPLIT",
                "ok": self.cell(out)}


def trace():
    """The whole grid on the lvc_amd package that `import lvc_amd` finds -> the JSON-able trace."""
    rec = Recorder()
    with install_stubs(rec) as K:
        saved = {k: getattr(K, k) for k in DEFAULTS}
        saved["CONV_TIMER"] = K.CONV_TIMER
        slots = (K._NEXT_SLOT[0], dict(K._GROUP_SLOTS), dict(K._SLOT_OWNERS))
        try:
            t = Tracer(K, rec)
            grid, extras, pairs = {}, {}, {}
            for label, change in SETTINGS:
                t.settings(change)
                grid[label] = {name: t.cell(t.conv2d_grid(name)) for name in LAYERS}
                extras[label] = t.cell([i for _, i in t.extras()])
                pairs[label] = t.presplit_pairs()["ok"]
            t.settings({})
            extra_labels = [lab for lab, _ in t.extras()]
            pair_axes = t.presplit_pairs()
            del pair_axes["ok"]
        finally:
            for k, v in saved.items():
                setattr(K, k, v)
            K._NEXT_SLOT[0] = slots[0]
            K._GROUP_SLOTS.clear(); K._GROUP_SLOTS.update(slots[1])
            K._SLOT_OWNERS.clear(); K._SLOT_OWNERS.update(slots[2])
    return {"axes": {"tier": TIERS, "two_acc": FORMS, "split": SPLITS, "residual": RESIDUALS, "relu_act": ACTS,
                     "order": "conv2d[setting][layer] -> list id; the list holds one outcome id per (tier, two_acc, split, residual, relu_act), last axis fastest",
                     "extras": extra_labels, "presplit_pairs": pair_axes},
            "layers": {n: list(v[:7]) + [list(v[7])] for n, v in LAYERS.items()},
            "settings": [s for s, _ in SETTINGS], "conv2d": grid, "extras": extras, "presplit_pair_ok": pairs,
            "lists": t.lists, "outcomes": t.blobs}


ALPHABET = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def compact(tr):
    """The committed form of `trace()`'s result.  A case's outcome becomes its signature -- what ran: return, [entry point, range slot]
    per launch, the slot left behind, the timer's tags, the layers' last_one -- and every cell (the cases of one layer under one
    setting, or a setting's extras) carries a SHA-256 over its complete outcomes: integer arguments, NULL flags, flops and bytes."""
    sigs, sig_ids, cells, cell_ids = [], {}, [], {}

    def sig(o):
        s = {"ret": o["ret"], "launches": [[c[0], c[3]] for c in o["calls"]], "end_slot": o["end_slot"],
             "timer": [t[0] for t in o["timer"]], "last_one": o["last_one"]}
        key = json.dumps(s, sort_keys=True)
        if key not in sig_ids:
            sig_ids[key] = len(sigs)
            sigs.append(s)
        return sig_ids[key]

    def cell(list_id):
        if list_id not in cell_ids:
            outs = [tr["outcomes"][i] for i in tr["lists"][list_id]]
            ids = [sig(o) for o in outs]
            sha = hashlib.sha256("\n".join(json.dumps(o, sort_keys=True) for o in outs).encode()).hexdigest()[:24]
            # one signature per case: a character of ALPHABET each where they all fit, the plain ids otherwise
            cells.append({"routes": "".join(ALPHABET[i] for i in ids) if max(ids) < len(ALPHABET) else ids, "sha256": sha})
            cell_ids[list_id] = len(cells) - 1
        return cell_ids[list_id]

    pairs = ["%s + %s" % (a, b) for a in tr["axes"]["presplit_pairs"]["conv2"] for b in tr["axes"]["presplit_pairs"]["conv3"]]
    conv2d = {s: {n: cell(i) for n, i in tr["conv2d"][s].items()} for s in tr["settings"]}      # (their signatures first: they fit)
    extras = {s: cell(tr["extras"][s]) for s in tr["settings"]}
    return {"axes": tr["axes"], "layers": tr["layers"], "settings": tr["settings"], "signatures": sigs, "cells": cells, "conv2d": conv2d,
            "extras": extras, "presplit_pair_ok": {s: {k: v for k, v in zip(pairs, tr["lists"][i]) if "1" in v}       # (the others: False)
                                                   for s, i in tr["presplit_pair_ok"].items()}}


def dumps(c, rows=("signatures", "cells")):
    """JSON with one line per top-level key, and one per element of the long tables."""
    def one(v):
        return json.dumps(v, separators=(",", ":"), sort_keys=True)
    return "{\n" + ",\n".join('"%s":[\n%s\n]' % (k, ",\n".join(one(e) for e in c[k])) if k in rows else '"%s":%s' % (k, one(c[k]))
                              for k in sorted(c)) + "\n}\n"


# ------------------------------------------------------------------------------------------------ --model: the real launch stream
def model_stream(out_path):
    """Launch stream of one `inference_batched` of the bench model on the bench input, and of one training step (bench.py's cfg 3:
    R50-FPN novel fine-tune), through the real library.  Every native call is kept, not only the conv/GEMM ones."""
    from lvc_amd import kernels as K  # noqa: F401
    from lvc_amd.config import set_global_cfg
    from lvc_amd.config.presets import base_rcnn_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.structures import Boxes, Instances
    from lvc_amd.utils import synthetic as syn
    from lvc_amd.utils.events import EventStorage

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    rec = Recorder(real=_lib.lib())
    _lib.lib = lambda: rec
    streams = {}

    model = build_model(base_rcnn_fpn(device="cuda:0")).eval()
    syn.conditioned_r50_fpn_(model)
    batch = [{"image": syn.synthetic_image(1 + i).to(dev), "height": 800, "width": 1333} for i in range(8)]
    with torch.no_grad():
        model.inference_batched(batch)          # packs the weights, settles the range tiers
        torch.cuda.synchronize()
        rec.reset()
        model.inference_batched(batch)
        torch.cuda.synchronize()
    streams["inference_batched"] = [[c[0], c[1], c[3]] for c in rec.calls]
    del model
    torch.cuda.empty_cache()

    cfg = base_rcnn_fpn(num_classes=20, device="cuda:0")
    cfg.MODEL.BACKBONE.FREEZE = True
    cfg.MODEL.PROPOSAL_GENERATOR.FREEZE = True
    cfg.MODEL.ROI_HEADS.FREEZE_FEAT = True
    set_global_cfg(cfg)
    model = build_model(cfg)
    syn.conditioned_r50_fpn_(model, depth=50)
    model.train()
    torch.manual_seed(20)
    g = torch.Generator().manual_seed(1)
    tb = []
    for i in range(8):
        h, w, n = 800, 1333, 8
        x1, y1 = torch.rand(n, generator=g) * (w - 300), torch.rand(n, generator=g) * (h - 300)
        bw, bh = 40 + torch.rand(n, generator=g) * 250, 40 + torch.rand(n, generator=g) * 250
        inst = Instances((h, w))
        inst.gt_boxes = Boxes(torch.stack([x1, y1, x1 + bw, y1 + bh], 1))
        inst.gt_classes = torch.randint(0, 20, (n,), generator=g)
        tb.append({"image": syn.synthetic_image(1 + i).to(dev), "instances": inst, "height": h, "width": w})
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=1e-4)
    with EventStorage(0):
        for it in range(2):
            torch.manual_seed(20)               # the same proposal sampling in both steps
            if it == 1:
                torch.cuda.synchronize()
                rec.reset()
            losses = model(tb)
            opt.zero_grad()
            sum(losses.values()).backward()
            opt.step()
        torch.cuda.synchronize()
    streams["train_step"] = [[c[0], c[1], c[3]] for c in rec.calls]
    text = dumps(streams)
    with open(out_path, "w") as f:
        f.write(text)
    print(json.dumps({k: len(v) for k, v in streams.items()}), "sha256", hashlib.sha256(text.encode()).hexdigest(), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--model", action="store_true", help="record the real launch stream of the bench model (needs the GPU)")
    ap.add_argument("--full", action="store_true", help="every outcome in full instead of signatures + digests (to diff two checkouts)")
    a = ap.parse_args()
    if a.model:
        return model_stream(a.out)
    tr = trace()
    text = dumps(tr, rows=("outcomes", "lists")) if a.full else dumps(compact(tr))
    with open(a.out, "w") as f:
        f.write(text)
    used = sorted({c[0] for o in tr["outcomes"] for c in o["calls"]})
    print("%d bytes, %d outcomes, entry points reached: %s" % (len(text), len(tr["outcomes"]), ", ".join(used)))


if __name__ == "__main__":
    main()
