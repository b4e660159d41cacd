"""Python host bindings of the gfx950 kernels (one function per C-ABI entry point of
include/lvc_amd.h).  torch is used for device memory and streams only; all arithmetic of the
hot path happens inside liblvc_amd.so.  Every function requires CUDA(HIP) tensors and raises if
the native library is missing -- there is deliberately no CPU path here.
"""
import collections
import ctypes

import torch

from . import _lib
from ._lib import LvcNativeError, c_float, c_int, c_longlong, c_void_p, check, ptr      # the c_* types build host arrays only

BK = 32  # gemm-K chunk of the implicit-GEMM kernel
BN = 128


def _stream(t):
    return c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("lvc_amd kernels need device tensors (got a CPU tensor); there is no CPU path")


def _float3(v):
    return (c_float * 3)(*[float(x) for x in v])


# --------------------------------------------------------------------------- convolution / GEMM
class PackedConv:
    """Weights of one conv/linear layer in the kernel's layout + folded per-channel affine.

    w_packed: [Kpad, Kg] fp32, rows = out channel (zero rows up to a multiple of 128),
              k = (c//32, r, s, c%32) (mode 0) or (r, 8 pixels x 4 ch) (mode 1, the stem: BasicStem's 7x7, DeepStem's 3x3).
    scale/shift: y = conv * scale + shift  (FrozenBN fold and/or bias), or None.
    """

    __slots__ = ("w", "scale", "shift", "K", "C", "R", "S", "stride", "pad", "Kg", "mode", "_w3", "_w2h", "_w2s", "two_acc",
                 "slot", "state", "_last_one", "groups", "__weakref__")

    def __init__(self, w, scale, shift, K, C, R, S, stride, pad, Kg, mode):
        self.w, self.scale, self.shift = w, scale, shift
        self.K, self.C, self.R, self.S, self.stride, self.pad, self.Kg, self.mode = K, C, R, S, stride, pad, Kg, mode
        self._w3 = None
        self._w2h = None
        self._w2s = None
        self.groups = 1        # > 1: a grouped 3x3 layer, `w` is the operand of csrc/conv_grouped.hip (`_pack_grouped`)
        self.two_acc = False   # True: never the single-accumulator form of the 3x3 fp16-split kernel (see HALO_S1)
        # range routing of THIS layer (`check_conv_error_word`): its own range word in the workspace, and the tier it runs on --
        # 0: as configured (one accumulator where the policy allows it, |a| <= 4094), 1: two accumulators (|a| <= 65504),
        # 2: the range-free bf16x3 kernels.  `state` may be a dict the owning module keeps across re-packs.
        self.slot = _new_range_slot(self)
        self.state = {"tier": 0}
        self._last_one = False

    @property
    def last_one(self):
        """True when the layer's most recent launch ran on the single-accumulator form (|a| <= 4094)."""
        return self._last_one

    @last_one.setter
    def last_one(self, one):
        # ... and, per (device, stream) workspace, the (tier, form) that launch ran on: a range word is read with the workspace of the
        # stream it was raised on, possibly after another stream's pass already moved the layer (PipelinedInference) -- the reaction
        # is chosen from the form the word was raised by, not from the layer's present one
        self._last_one = bool(one)
        dev = self.w.device
        if dev.type == "cuda":
            # one layer may launch several forms in a pass (the RPN head: single-accumulator Winograd on p2 / p3, two accumulators on
            # p4 - p6, all on this slot): the narrowest form seen at this tier decides the reaction, not the last launch
            at = self.state.setdefault("at", {})
            key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
            prev = at.get(key)
            at[key] = (self.state["tier"], bool(one) or (prev is not None and prev[0] == self.state["tier"] and prev[1]))

    def _split(self, planes):
        n = self.w.numel()
        dt = torch.bfloat16 if planes == 3 else torch.float16
        out = torch.empty((planes,) + tuple(self.w.shape), device=self.w.device, dtype=dt)
        err = _conv_error_view(self.w.device) if planes == 2 else None
        check(_lib.lib().lvc_split_weights(ptr(self.w), n, planes, ptr(out), ptr(err), _stream(self.w)),
              "lvc_split_weights")
        return out

    def split3(self):
        """[3, Kpad, Kg] bf16 planes (hi, mid, lo) of the packed weights: w == hi + mid + lo exactly."""
        if self._w3 is None:
            self._w3 = self._split(3)
        return self._w3

    def split2h(self):
        """[2, Kpad, Kg] fp16 planes of the packed weights for the two-way fp16 split (csrc/conv3x3_halo_h2.hip):
        w1 = fp16(w), w2 = fp16((w - w1) * 2048)  ->  w ~= w1 + w2 / 2048 to 2^-23 relative (|w| >= 2.4e-4).  A weight
        beyond the fp16 range raises bit 1 of the conv error word (`check_conv_error_word`: use LVC_CONV_SPLIT=bf16x3)."""
        if self._w2h is None:
            self._w2h = self._split(2)
        return self._w2h


    def split2s(self):
        """([2, Kpad, Kg] fp16 planes of the ROW-SCALED weights, scale' [K] fp32) for the single-accumulator form of the two-way
        fp16 split (csrc/conv3x3_halo_s1.hip): row k is multiplied by 2^e_k (largest entry into [2^13, 2^14)) and split
        without a plane scale, w 2^e = w1 + w2; scale' = (the layer's per-channel scale or 1) * 2^-(e_k + 4) undoes that and
        the kernel's 2^4 activation scale in the epilogue.  Powers of two: the scaling itself is exact."""
        if self._w2s is None:
            rows, Kg = self.w.shape
            planes = torch.empty((2, rows, Kg), device=self.w.device, dtype=torch.float16)
            fac = torch.empty(rows, device=self.w.device, dtype=torch.float32)
            check(_lib.lib().lvc_split_weights_rowscaled(ptr(self.w), rows, Kg, ptr(planes), ptr(fac), _stream(self.w)),
                  "lvc_split_weights_rowscaled")
            fac = fac[: self.K]
            self._w2s = (planes, (fac * self.scale if self.scale is not None else fac).contiguous())
        return self._w2s


_RANGE_SLOTS = 1024
_NEXT_SLOT = [0]
_SLOT_OWNERS = {}
RANGE_EPOCH = 0      # counts the re-routings: passes launched under an older epoch ran on the narrower kernels


def _new_range_slot(owner):
    """Slots 1 .. 1023, handed out round-robin; a slot shared by two layers (more than 1023 packed layers alive) only makes
    the re-routing coarser (both move to the wider tier)."""
    import weakref

    _NEXT_SLOT[0] = _NEXT_SLOT[0] % (_RANGE_SLOTS - 1) + 1
    slot = _NEXT_SLOT[0]
    owners = [r for r in _SLOT_OWNERS.get(slot, []) if r() is not None]
    owners.append(weakref.ref(owner))
    _SLOT_OWNERS[slot] = owners
    return slot


def conv_affine(bias=None, bn=None, eps=1e-5):
    """(scale, shift) of y = conv * scale + shift: FrozenBatchNorm2d fold (reference detectron2/layers/batch_norm.py:
    45-65: scale = w * rsqrt(var + eps), shift = b - mean * scale) and/or the conv bias; None where absent."""
    scale = shift = None
    if bn is not None:
        bw, bb, rm, rv = [t.detach().float() for t in bn]
        scale = bw * (rv + eps).rsqrt()
        shift = bb - rm * scale
        if bias is not None:
            shift = shift + bias.detach().float() * scale
    elif bias is not None:
        shift = bias.detach().float().clone()
    if scale is not None:
        scale = scale.contiguous()
    if shift is not None:
        shift = shift.contiguous()
    return scale, shift


def _pack_weights(weight, scale, rows_pad, cin_pad, mode, planes=0):
    """Packed fp32 operand and, with planes = 2 / 3, its fp16 / bf16 split planes from the same launch (else None)."""
    K, C, R, S = weight.shape
    w = weight.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    wp = torch.empty(rows_pad, R * S * cin_pad, device=w.device, dtype=torch.float32)
    if planes:
        out = torch.empty((planes,) + tuple(wp.shape), device=w.device, dtype=torch.float16 if planes == 2 else torch.bfloat16)
        err = _conv_error_view(w.device) if planes == 2 else None
        check(_lib.lib().lvc_pack_split_conv_weights(ptr(w), ptr(scale), ptr(wp), ptr(out), planes, ptr(err), K,
                                                     C, R, S, rows_pad, cin_pad,
                                                     mode, _stream(w)), "lvc_pack_split_conv_weights")
        return wp, out
    check(_lib.lib().lvc_pack_conv_weights(ptr(w), ptr(scale), ptr(wp), K, C, R, S,
                                           rows_pad, cin_pad, mode, _stream(w)),
          "lvc_pack_conv_weights")
    return wp, None


def _planes_hint(R, S, contraction, split):
    """The split the conv routing will most likely ask of a layer (conv2d_nhwc: two-way fp16 for the 3x3 layers and the
    1x1 layers with a long contraction, three-way bf16 otherwise); a wrong guess only costs the lazy split later."""
    if CONV_ENGINE != "bf16x3":
        return 0
    if (split or CONV_SPLIT) == "f16x2" and ((R == 3 and S == 3) or (R == 1 and S == 1 and contraction >= _H2_PW_MIN_C)):
        return 2
    return 3


def _with_planes(pc, planes, out):
    if planes == 2:
        pc._w2h = out
    elif planes == 3:
        pc._w3 = out
    return pc


GROUPED_CG = (4, 8, 16, 32, 64)      # channels per group of csrc/conv_grouped.hip


def grouped_conv_check(in_channels, out_channels, groups, kernel_size=3, stride=1, padding=1):
    """Raise NotImplementedError for a grouped convolution outside csrc/conv_grouped.hip: 3x3, pad 1, stride 1 or 2, as many output
    as input channels, 4 / 8 / 16 / 32 / 64 channels per group (ResNeXt 32x4d, 32x8d, 64x4d at res2..res5), channels a multiple of 64.
    Pure: it answers on a machine without a GPU."""
    if kernel_size != 3 or padding != 1 or stride not in (1, 2):
        raise NotImplementedError("grouped convolution is built for kernel_size=3, padding=1, stride 1 or 2 (a ResNeXt bottleneck's conv2); "
                                  "got kernel_size={}, padding={}, stride={}, groups={}".format(kernel_size, padding, stride, groups))
    cg = in_channels // groups if groups > 0 and in_channels % groups == 0 else 0
    if in_channels != out_channels or cg not in GROUPED_CG or in_channels % 64:
        raise NotImplementedError(
            "grouped 3x3 convolution {} -> {} with groups={}: the kernel takes {} channels per group (in == out, a multiple of 64); "
            "choose MODEL.RESNETS.NUM_GROUPS / WIDTH_PER_GROUP accordingly (32x4d, 32x8d, 64x4d)".format(
                in_channels, out_channels, groups, " / ".join(str(c) for c in GROUPED_CG)))


def _pack_grouped(weight, scale, groups, mode):
    """The operand of lvc_conv3x3_grouped_nhwc from the reference's [K, C/G, 3, 3] weight.  mode 0: forward; mode 1: the data gradient
    (taps flipped, per-group transpose, times `scale`)."""
    _req_cuda(weight, scale)
    K, cg, R, S = weight.shape
    grouped_conv_check(cg * groups, K, groups, R if R == S else 0)
    w = weight.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    lib = _lib.lib()
    wp = torch.empty(lib.lvc_conv3x3_grouped_packed_floats(K, groups), device=w.device, dtype=torch.float32)
    check(lib.lvc_pack_conv3x3_grouped(ptr(w), ptr(scale), ptr(wp), K, groups, mode, _stream(w)),
          "lvc_pack_conv3x3_grouped")
    return wp


def pack_conv(weight, bias=None, bn=None, stride=1, pad=0, eps=1e-5, stem=False, affine=None, split=None, groups=1):
    """weight: [K, C, R, S] (OIHW, the reference's state_dict layout) on the target device.
    bn: None or (weight, bias, running_mean, running_var) of a FrozenBatchNorm2d; affine: a precomputed
    `conv_affine(bias, bn, eps)` (the fold only changes when those tensors do, the weights change every step).
    stem=True packs a 3-channel stem layer (BasicStem's 7x7, DeepStem's 3x3 conv1) for the NHWC4 "row mode" of the kernel.
    groups > 1: weight is [K, C/groups, 3, 3], packed for the grouped kernel (`grouped_conv_check`).
    """
    _req_cuda(weight)
    if groups != 1:
        grouped_conv_check(weight.shape[1] * groups, weight.shape[0], groups, weight.shape[2], stride, pad)
        scale, shift = affine if affine is not None else conv_affine(bias, bn, eps)
        pc = PackedConv(_pack_grouped(weight, None, groups, 0), scale, shift, weight.shape[0], weight.shape[0], 3, 3, stride, pad,
                        9 * weight.shape[1], 0)
        pc.groups = groups
        return pc
    K, C, R, S = weight.shape
    dev = weight.device
    Kpad = (K + BN - 1) // BN * BN
    if stem:
        assert C <= 4 and S <= 8
        w = weight.detach().float()
        wk = torch.zeros(K, R, 8, 4, device=dev, dtype=torch.float32)
        wk[:, :, :S, :C] = w.permute(0, 2, 3, 1)
        Kg = R * BK
        wp = torch.zeros(Kpad, Kg, device=dev, dtype=torch.float32)
        wp[:K] = wk.reshape(K, Kg)
        Cphys, mode = 4, 1
    else:
        assert C % BK == 0, "implicit-GEMM kernel needs in_channels % 32 == 0 (got {})".format(C)
        Kg = R * S * C
        # k = (c // 32, r, s, c % 32): the taps of one 32-channel chunk are consecutive gemm-k chunks
        planes = _planes_hint(R, S, C, split)
        wp, pl = _pack_weights(weight, None, Kpad, C, 0, planes)
        scale, shift = affine if affine is not None else conv_affine(bias, bn, eps)
        return _with_planes(PackedConv(wp, scale, shift, K, C, R, S, stride, pad, Kg, 0), planes, pl)
    scale, shift = affine if affine is not None else conv_affine(bias, bn, eps)
    return PackedConv(wp, scale, shift, K, Cphys, R, S, stride, pad, Kg, mode)


PREPACK = __import__("os").environ.get("LVC_PREPACK", "1") != "0"


class PrepackPlan:
    """The packed operands of many layers in a few launches (csrc/weights.hip pack_group_kernel) instead of two or three launches
    per layer: what `pack_conv` (+ `PackedConv.split2s`) and `pack_conv_dgrad` produce, for the layers whose parameters an
    optimizer step just changed.  jobs: list of dicts {"weight", "kind": "fwd" | "dgrad", "stride", "pad", "affine": (scale, shift),
    "two_acc", "tier", "scale"}; `.packed`: the PackedConv objects (same fields as the per-layer functions fill).
    The plan owns its buffers: `relaunch()` packs the (changed) parameters into the SAME operands again -- the host side of a
    training step's re-packing is then one kernel-argument table per 24 layers, not ~10 tensor views per layer."""

    def __init__(self, jobs):
        import ctypes

        dev = jobs[0]["weight"].device
        metas, total = [], 0

        def take(nbytes):
            nonlocal total
            o = total
            total += (nbytes + 255) // 256 * 256
            return o

        for jb in jobs:
            w = jb["weight"]
            Kc, C, R, S = w.shape
            if jb["kind"] == "fwd":
                assert C % BK == 0
                rows_pad, cin_pad, mode = (Kc + BN - 1) // BN * BN, C, 0
                hint = _planes_hint(R, S, C, None)
                one = (hint == 2 and not jb.get("two_acc") and jb.get("tier", 0) == 0
                       and ((R == 3 and HALO_S1 == 2) or (R == 1 and PW_S1 == 2 and C >= _PW_S1_ONE_MIN_C)))
                fmt = 4 if one else hint
            else:
                cin_pad = (Kc + 31) // 32 * 32
                rows_pad, mode = (C + BN - 1) // BN * BN, 1
                fmt = _planes_hint(R, S, cin_pad, DGRAD_SPLIT)
            Kg = R * S * cin_pad
            nplanes = 3 if fmt == 3 else 2 if fmt in (2, 4) else 0
            metas.append((rows_pad, cin_pad, mode, fmt, Kg, take(rows_pad * Kg * 4), take(nplanes * rows_pad * Kg * 2) if nplanes else -1,
                          take(rows_pad * 4) if fmt == 4 else -1))
        self.buf = buf = torch.empty(total, dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        self.n = n = len(jobs)
        self.ptrs = ptrs = (ctypes.c_void_p * (6 * n))()
        self.shapes = shapes = (c_int * (8 * n))()
        self.packed, self.planes, self.keep = [], [], []
        self.reusable = True
        for j, (jb, (rows_pad, cin_pad, mode, fmt, Kg, o_wp, o_pl, o_fac)) in enumerate(zip(jobs, metas)):
            w = jb["weight"].detach()
            if w.dtype != torch.float32 or not w.is_contiguous():
                w = w.float().contiguous()
                self.reusable = False          # a converted copy: its address is not the parameter's
            self.keep.append(w)
            Kc, C, R, S = w.shape
            aff = jb.get("affine") or (None, None)
            wp = buf[o_wp: o_wp + rows_pad * Kg * 4].view(torch.float32).view(rows_pad, Kg)
            pl = fac = None
            if fmt in (2, 4):
                pl = buf[o_pl: o_pl + 2 * rows_pad * Kg * 2].view(torch.float16).view(2, rows_pad, Kg)
            elif fmt == 3:
                pl = buf[o_pl: o_pl + 3 * rows_pad * Kg * 2].view(torch.bfloat16).view(3, rows_pad, Kg)
            if fmt == 4:
                fac = buf[o_fac: o_fac + rows_pad * 4].view(torch.float32)
            dg_scale = jb.get("scale") if mode == 1 else None
            self.keep.append((dg_scale, aff))
            ptrs[6 * j: 6 * j + 6] = [w.data_ptr(), dg_scale.data_ptr() if dg_scale is not None else None,
                                      aff[0].data_ptr() if (fmt == 4 and aff[0] is not None) else None, base + o_wp,
                                      (base + o_pl) if pl is not None else None, (base + o_fac) if fac is not None else None]
            shapes[8 * j: 8 * j + 8] = [Kc, C, R, S, rows_pad, cin_pad, mode, fmt]
            if mode == 0:
                pc = PackedConv(wp, aff[0], aff[1], Kc, C, R, S, jb["stride"], jb["pad"], Kg, 0)
            else:
                pc = PackedConv(wp, None, None, C, cin_pad, R, S, 1, R - 1 - jb["pad"], Kg, 0)
            self.packed.append(pc)
            self.planes.append((fmt, pl, fac[:Kc] if fac is not None else None))
        self._err = _conv_error_view(dev)
        self.relaunch()

    def relaunch(self):
        for pc, (fmt, pl, fac) in zip(self.packed, self.planes):
            pc._w2h = pl if fmt == 2 else None          # lazily made planes of the previous parameters go too
            pc._w3 = pl if fmt == 3 else None
            pc._w2s = (pl, fac) if fmt == 4 else None
            pc.state.pop("_wino", None)
        check(_lib.lib().lvc_pack_group(self.n, self.ptrs, self.shapes, ptr(self._err), _stream(self.buf)), "lvc_pack_group")


def prepack_group(jobs):
    return PrepackPlan(jobs).packed if jobs else []


def pack_linear(weight, bias=None, split=None, two_acc=True):
    """weight [K_out, K_in] -> a 1x1 'conv' over M x 1 x 1 x K_in rows.  split: the operand split the GEMM will be
    asked for (None = LVC_CONV_SPLIT), so that the matching planes are produced by the packing launch.
    two_acc (default True): fully-connected layers feed scores, box deltas and kNN rankings -- they keep the main + cross
    accumulator form of the fp16 split (kernels.PW_S1); the descriptor network's linears pass False."""
    pc = pack_conv(weight[:, :, None, None], bias=bias, split=split)
    pc.two_acc = bool(two_acc)
    return pc


_CONV_WS = {}
_ERR_OFF = None      # byte offset of the range / error words (word 0 = shared, words 1.. = per layer): the library's, set by conv_workspace


def conv_workspace(device):
    """Per-(device, stream) scratch of the stream-K conv kernel (zeroed once; see include/lvc_amd.h)."""
    global _ERR_OFF
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _CONV_WS.get(key)
    if ws is None:
        if _ERR_OFF is None:
            _ERR_OFF = _lib.lib().lvc_conv_range_words_offset()
        ws = torch.zeros(_lib.size_query("lvc_conv_workspace_bytes"), dtype=torch.uint8, device=device)
        _CONV_WS[key] = ws
    return ws


def _conv_error_view(device):
    ws = conv_workspace(device)
    return ws[_ERR_OFF: _ERR_OFF + 4]


def _range_words(device):
    ws = conv_workspace(device)
    return ws[_ERR_OFF: _ERR_OFF + 4 * _RANGE_SLOTS].view(torch.int32)


def range_summary(device):
    """[1] int32 device tensor, non-zero iff any error / range word of this stream's workspace is set: lets a caller fold the
    check into a device->host read it does anyway (`roi_heads.instances_from_batched`) and call `check_conv_error_word` only
    when something is up."""
    return _range_words(device).amax().view(1)


def conv_error_word(device):
    """OR of the kernels' error words (0 = fine; bit 0: spin timeout, bit 1: a finite operand beyond the range of the form, bit 2: a
    non-finite operand in a range-checked kernel); reading it synchronises."""
    e = 0
    for w in _range_words(device).tolist():
        e |= w
    return e


def clear_conv_error_word(device):
    _range_words(device).zero_()


class Fp16RangeError(LvcNativeError):
    """An operand beyond the range of a two-way fp16 split kernel reached it (|a| > 4094 on the single-accumulator form,
    > 65504 on the two-accumulator form, or NaN): the results of that pass are invalid.  `rerouted`: the layers that raised
    their own range word were moved to the next wider form (`check_conv_error_word`); the model entry points run the pass
    again.  Otherwise (shared word: stem, weights, descriptor network) they switch the process to the bf16x3 kernels."""

    rerouted = False


_RANGE_FALLBACK_LOGGED = False
_LOGGED_ONCE = set()


def _log_once(key, msg, *args):
    if key not in _LOGGED_ONCE:
        _LOGGED_ONCE.add(key)
        import logging

        logging.getLogger("lvc_amd").warning(msg, *args)


def use_range_free_split(reason=""):
    """Switch every conv/GEMM of this process from the two-way fp16 split to the exact three-way bf16 split (no range
    limit, ~1.5x slower); logged once.  Packed layers keep both plane sets lazily, so this takes effect at the next call.
    Only for conditions that cannot be pinned on one layer (the shared error word); a layer that overflows its own range
    word is re-routed alone (`check_conv_error_word`)."""
    global CONV_SPLIT, _RANGE_FALLBACK_LOGGED
    CONV_SPLIT = "bf16x3"
    if not _RANGE_FALLBACK_LOGGED:
        _RANGE_FALLBACK_LOGGED = True
        import logging

        logging.getLogger("lvc_amd").warning(
            "an operand beyond fp16's range (|a| > 65504 or NaN) reached an fp16x2 kernel that has no per-layer range word%s; "
            "re-running on the range-free bf16x3 kernels and keeping them for the rest of the process", (" (" + reason + ")") if reason else "")


def check_conv_error_word(device):
    """Raise for a set bit of the conv workspace's error words.  Bit 0 (any word): a stream-K worker timed out waiting for a
    partial tile.  Bit 1 of a LAYER's word: an activation left the range of the form that layer ran on -> the layer moves to
    the next wider one -- single accumulator (|a| <= 4094) -> two accumulators (|a| <= 65504) -> bf16x3 (no limit) -- and
    stays there; every other layer keeps its kernels.  Bit 1 of the shared word: `Fp16RangeError` without `rerouted`
    (process-wide bf16x3, `use_range_free_split`).  The words are cleared: every pass is judged on its own.
    Synchronises: call it where the results are read anyway."""
    global RANGE_EPOCH
    words = _range_words(device).tolist()
    if not any(words):
        return
    if any(w & 1 for w in words):
        raise LvcNativeError("conv/GEMM kernel: a stream-K worker timed out waiting for a partial tile")
    clear_conv_error_word(device)
    moved, stale = [], 0
    ws_key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    # bit 1: a finite operand beyond the form's range -- that layer moves.  bit 2 alone: the layer saw inf (NaN is not tracked); when
    # another layer reports bit 1 in the same pass that is what the overflowing layer handed down, and the layer stays where it is
    # (the repeated pass will tell); with no bit 1 anywhere the non-finite values are the data's own and the layers move as before
    finite_somewhere = any(w & 2 for w in words[1:])
    for slot in range(1, _RANGE_SLOTS):
        if words[slot] & 2 or (words[slot] & 4 and not finite_somewhere):
            for ref in _SLOT_OWNERS.get(slot, []):
                o = ref()
                if o is None:
                    continue
                if isinstance(o, PackedChain):
                    if not o.state.get("off"):
                        o.state["off"] = True
                        moved.append("chained pair %dx%d->%d->%d: two launches" % (o.K1, o.N1, o.N1, o.N2))
                    continue
                if isinstance(o, PackedBneck):
                    if not o.state.get("off"):
                        o.state["off"] = True
                        moved.append("fused bottleneck %d->64->256: separate launches" % o.cin)
                    continue
                tier = o.state["tier"]
                t_launch, one = o.state.get("at", {}).get(ws_key, (tier, o.last_one))
                new = 1 if (one and t_launch < 1) else 2
                if new > tier:
                    o.state["tier"] = new
                    moved.append("%dx%d %d->%d: |a| > %s -> %s" % (o.R, o.S, o.C, o.K, "4094" if one else "65504",
                                                                   "two accumulators" if new == 1 else "bf16x3"))
                elif tier > t_launch:
                    stale += 1      # raised by a pass launched before the layer was moved: that pass is run again, nothing moves
    if moved:
        RANGE_EPOCH += 1
        import logging

        logging.getLogger("lvc_amd").warning("activation range: %d layer(s) re-routed and kept there (%s); re-running the pass",
                                             len(moved), "; ".join(moved[:8]))
    e = Fp16RangeError("conv/GEMM kernel: an operand beyond the range of the fp16 split form it ran on (|a| > 4094 single-accumulator, "
                       "> 65504 two-accumulator, or NaN)" + ("; the layers concerned were moved to the next wider form" if moved else
                                                             "; set LVC_CONV_SPLIT=bf16x3 for range-free kernels"))
    e.rerouted = (bool(moved) or stale > 0) and not (words[0] & 6)
    raise e


class LaunchTimer:
    """Optional per-launch HIP-event bracket for the conv/GEMM kernel (bench.py's roofline leg).
    Events are recorded on the stream the kernel is launched on (torch's current stream)."""

    def __init__(self, only=None, every=1):
        self.records = []  # (algorithmic flops, start event, end event, engine, algorithmic bytes)
        self.only = only   # None = bracket every launch; else the set of engine tags to bracket
        self.every = max(1, int(every))   # bracket the launches of every `every`-th step only (`next_step` counts them): an
        self.step = 0                     # event pair costs ~6 us of stream bubbles around a launch
        self.active = True

    def next_step(self):
        """Call at the start of a step: launches are bracketed in steps 0, every, 2*every, ..."""
        self.active = self.step % self.every == 0
        self.step += 1

    def steps_timed(self):
        return (self.step + self.every - 1) // self.every

    def algorithmic_bytes(self, engine=None):
        return sum(r[4] for r in self.records if (engine is None or r[3] == engine) and len(r) > 4)

    def flops_and_ms(self, engine=None):
        torch.cuda.synchronize()
        recs = [r for r in self.records if engine is None or r[3] == engine]
        fl = sum(r[0] for r in recs)
        ms = sum(r[1].elapsed_time(r[2]) for r in recs)
        return fl, ms, len(recs)


CONV_TIMER = None  # set to a LaunchTimer to instrument the conv/GEMM launches (`_launch`)
# Inner-product engine of the conv/GEMM layers with >= 128 output channels:
#   "bf16x3" = fp32-accurate 3-way bf16 operand split on the bf16 matrix cores (csrc/conv_bf16x3.hip)
#   "f32"    = v_mfma_f32_32x32x2_f32 (csrc/conv_igemm.hip); always used for the stem and the 64-channel layers
import os as _os

CONV_ENGINE = _os.environ.get("LVC_CONV_ENGINE", "bf16x3")
_BF16X3_MIN_K = 128
# 3x3 / stride 1 / pad 1 layers of the bf16x3 engine go to the halo kernel (csrc/conv3x3_halo.hip)
CONV_HALO = True       # False: the generic kernels (tests compare the two)
# BasicStem (conv 7x7/2 + FrozenBN + ReLU + max-pool 3x3/2) as one fused split-precision kernel (csrc/stem_pool.hip)
STEM_FUSED = True
_PW_NARROW = True
_PW_NARROW_MIN_C = 64
# operand split of the split-precision kernels that have both forms: "f16x2" = two fp16 planes, 3 MFMAs per block
# (Ootomo & Yokota; csrc/conv3x3_halo_h2.hip), "bf16x3" = three bf16 planes, 6 MFMAs per block (no range limit)
CONV_SPLIT = _os.environ.get("LVC_CONV_SPLIT", "f16x2")
# Operand split of the DATA-gradient convolutions.  "bf16x3" keeps fp32's exponent range (raw gradients of a mean-reduced
# loss sit around 1e-6 .. 1e-3, below fp16's normal range); "f16x2" is the faster two-way fp16 split and needs the
# gradients scaled into fp16's range first -- lvc_amd.solver.LossScaler does that with a power of two (exact) and switches
# this on for the backward pass it wraps.
DGRAD_SPLIT = _os.environ.get("LVC_DGRAD_SPLIT", "bf16x3")
# weight gradients without a loss scale: "bf16x3" = three-way bf16 split on the bf16 matrix cores, "f32" = fp32 MFMA
WGRAD_ENGINE = _os.environ.get("LVC_WGRAD_ENGINE", "bf16x3")
# inference: conv3 + stride-1 projection shortcut of res2.0 as one GEMM over [conv2 output | block input] (resnet.py)
FUSE_PROJECTION = _os.environ.get("LVC_FUSE_PROJECTION", "1") != "0"
_H2_PW_MIN_C = 64   # 64-channel streams too since the LDS-DMA kernel (0.32 -> 0.27 ms on res2 conv3)
# 3x3 fp16x2 layers of the FORWARD pass on the software-pipelined kernel (csrc/conv3x3_halo_s1.hip):
#   2 (default) = its single-accumulator form (row-scaled weight planes, activations x 2^4: |a| <= 4094; ~7 % faster on the 3x3
#       set -- the accumulate of the small cross products into the large sum costs the matrix pipe less power than a second full
#       accumulator -- at 1.7x the rounding noise of the two-accumulator form, 7.2e-8 of the output scale against 8e-8 .. 1.2e-7
#       for the reference's own fp32 CPU convolution, scripts/probe_halo_set.py), EXCEPT layers packed with `two_acc` (the RPN
#       head: its outputs feed top-k / NMS decisions and the post-trunk chain is held to the literal 1e-3, tests/test_gpu_chain.py);
#   1 = the numerics of conv3x3_halo_h2.hip everywhere (main + cross accumulators, same weight planes, |a| <= 65504);
#   0 = the round-1 kernel (conv3x3_halo_h2.hip), which data gradients (explicit `split`) always use.
HALO_S1 = 2
# pointwise fp16x2 layers with at least LVC_PW_S1_MIN_C input channels on the pipelined kernel (csrc/conv_pw_s1.hip): 2 = its
# single-accumulator form except `two_acc` layers, 1 = two accumulators everywhere, 0 = off (the LDS-DMA kernel for all of them)
PW_S1 = 2
_PW_S1_MIN_C = 64
_PW_S1_ONE_MIN_C = 256
_PW_S1_RES = 1     # 1: layers with a residual / upsample-add operand qualify too
# single-accumulator pointwise layers with >= 256 input channels and a multiple of 256 output channels on the 256 x 256 tile
# (csrc/conv_pw_w2.hip); 0 = the 256 x 128 tile of conv_pw_s1.hip for all of them
PW_W2 = _os.environ.get("LVC_PW_W2", "1") != "0"
# ... from 4096 input channels on (box-head fc1: 0.609 -> 0.599 / 0.593 -> 0.566 ms on two boxes).  Measured per layer in
# profiles/r05_pw_w2.txt: the stage loop is ~10 % faster per MFMA, but with 16 - 64 stages per tile (res4 / res5, the laterals) a tile's
# fill, hand-off and epilogue outweigh it -- and half as many, twice as large tiles split worse over 256 CUs -- so those stay on the 256 x 128 tile
_PW_W2_MIN_C = 4096
_PW_W2_MIN_ROWS = 4096
# inference: conv3 (+ shortcut add + ReLU) of a bottleneck and conv1 (+ ReLU) of the next one as ONE launch (csrc/conv_pw_chain.hip;
# modeling/backbone/resnet.py `BottleneckBlock.chain_to`); 0 = the two launches
CHAIN = _os.environ.get("LVC_CHAIN", "1") != "0"
_HALO_H2_MIN_TILES = 64    # smaller 3x3 layers (p6; p5 of fewer than seven images) use the bf16 kernels (tests set 0): scripts/probe_small_maps.py -- p5 of the batch of eight (80 tiles) 0.052 / 0.056 ms on the fp16-split kernel against 0.077 / 0.069, p6 (32 tiles) 0.041 / 0.050 against 0.040


# inference: a bottleneck's conv2 (3x3, direct single-accumulator kernel) hands its output to conv3 (pointwise, single accumulator) as the
# two fp16 planes conv3 multiplies -- conv3 skips the split (csrc/conv3x3_halo_s1.hip / conv_pw_s1.hip `_presplit`); bit-identical results.
# OFF by default: measured (scripts/probe_presplit.py, profiles/r06_presplit.txt) the pair of launches gets 2.2 % (res4) / 2.8 % (res5)
# shorter -- conv3 there moves 2.6 TB/s of fp32 rows, the split it skips was not what bounds it -- which is +0.15 % on the step
# (same-box A/B, four alternations, inside the noise): not worth a second hand-over format in the default path.  LVC_PRESPLIT=1 enables it.
PRESPLIT = _os.environ.get("LVC_PRESPLIT", "0") == "1"


def _launch(tag, flops, nbytes, slot, what, call):
    """The bracket around every conv/GEMM launch.  tag: the engine the LaunchTimer files it under (None: never timed) with its
    algorithmic flops and bytes; slot: the range slot the launch raises its range word on (None: the shared word); what: the entry
    point `call()` calls and returns the status of.  The thread's slot is back to 0 whatever `call` does."""
    timer = CONV_TIMER
    if timer is not None and (tag is None or not timer.active or (timer.only is not None and tag not in timer.only)):
        timer = None
    if timer is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if slot is None:
        st = call()
    else:
        _lib.lib().lvc_set_range_slot(slot)
        try:
            st = call()
        finally:
            _lib.lib().lvc_set_range_slot(0)
    check(st, what)
    if timer is not None:
        e1.record()
        timer.records.append((flops, e0, e1, tag, nbytes))


def halo_tiles(N, HW, K):
    """256-pixel x 128-channel tiles of a direct 3x3 launch over N maps of (at most) HW pixels (see _HALO_H2_MIN_TILES)."""
    return N * ((HW + 255) // 256) * ((K + 127) // 128)


def wino_sized(N, H, W, K):
    """The map fills the chip with the Winograd kernel's one-workgroup tiles (see _WINO_MIN_TILES)."""
    return CONV_WINO and K >= 128 and wino_tiles(N, H, W, K) >= _WINO_MIN_TILES


def _out_hw(pc, H, W):
    return (H + 2 * pc.pad - pc.R) // pc.stride + 1, (W + 2 * pc.pad - pc.S) // pc.stride + 1


# engine: the LaunchTimer's tag; entry: the C-ABI function; one: the single-accumulator form (|a| <= 4094: what `last_one` becomes);
# slotted: the launch raises the LAYER's range word (and sets `last_one`), not the shared one
ConvRoute = collections.namedtuple("ConvRoute", "engine entry one slotted")


def conv_route(pc, N, H, W, ldo=None, out_contiguous=True, out_numel=None, ldr=None, res_numel=0, split=None):
    """Which kernel `conv2d_nhwc` runs layer `pc` on for an [N,H,W,pc.C] input, under the module's switches as they are now.
    pc: anything with R, S, C, K, stride, pad, mode, two_acc and state["tier"] (a PackedConv); ldo / out_contiguous / out_numel: last
    dimension, contiguity and element count of the output buffer (default: a fresh [N,Ho,Wo,K]); ldr / res_numel: last dimension and
    element count of the residual operand (ldr None: no residual); split: the caller's explicit operand split.
    Pure: no tensor, no library call -- it answers on a machine without a GPU."""
    if getattr(pc, "groups", 1) != 1:
        # a grouped 3x3 layer (ResNeXt conv2; forward and data gradient): exact fp32 MFMA, range-free -- no tier, no range word
        return ConvRoute("f32_grouped", "lvc_conv3x3_grouped_nhwc", False, False)
    Ho, Wo = _out_hw(pc, H, W)
    rows = N * Ho * Wo
    if ldo is None:
        ldo = pc.K
    if out_numel is None:
        out_numel = rows * ldo
    has_res = ldr is not None
    # this layer's range tier (check_conv_error_word): 1 = two accumulators, 2 = the range-free bf16x3 kernels
    tier = pc.state["tier"] if split is None else 0
    two_acc = pc.two_acc or tier >= 1
    configured = split is None and tier < 2      # the configured fp16 split: launches raise the LAYER's range word
    f16 = tier < 2 and (split or CONV_SPLIT) == "f16x2"
    pw = pc.R == 1 and pc.S == 1 and pc.pad == 0
    halo = CONV_HALO and pc.R == 3 and pc.S == 3 and pc.stride == 1 and pc.pad == 1 and pc.C % 32 == 0
    # narrow 1x1 layers (256 -> 64 reductions, the 15-channel RPN predictors) go to the 64- / 32-channel tiles of the
    # 256-row pointwise shape
    pw_narrow = _PW_NARROW and pw and pc.C >= _PW_NARROW_MIN_C and pc.C % 32 == 0 and rows >= 2048
    if not (CONV_ENGINE == "bf16x3" and pc.mode == 0 and pc.K >= (64 if halo else 4 if pw_narrow else _BF16X3_MIN_K)
            and pc.K % 4 == 0 and ldo % 4 == 0 and (ldr or 0) % 4 == 0):
        return ConvRoute("f32", "lvc_conv2d_nhwc_f32", False, False)
    if halo:
        if not (f16 and halo_tiles(N, H * W, pc.K) >= _HALO_H2_MIN_TILES):
            return ConvRoute("bf16x3_halo", "lvc_conv3x3_nhwc_bf16x3", False, False)
        if configured and HALO_S1 == 2:
            # Winograd F(2,3) along x on the maps that fill the chip with its one-workgroup tiles (csrc/conv3x3_wino.hip)
            if (tier == 0 and (not pc.two_acc or WINO_RPN) and not has_res and out_contiguous and ldo == pc.K
                    and wino_sized(N, H, W, pc.K)):
                return ConvRoute("f16x2_wino", "lvc_conv3x3_nhwc_wino", True, True)
            if not two_acc:
                return ConvRoute("f16x2_halo", "lvc_conv3x3_nhwc_f16s1", True, True)
        if configured and HALO_S1 >= 1:
            return ConvRoute("f16x2_halo", "lvc_conv3x3_nhwc_f16x2_pipe", False, True)
        return ConvRoute("f16x2_halo", "lvc_conv3x3_nhwc_f16x2", False, configured)
    # the 256-row pointwise shape; 64-channel streams stay bf16x3 (f16x2 there: 0.312 vs 0.335 ms alone, no gain end to end)
    if f16 and pw and pc.C >= _H2_PW_MIN_C and rows >= 2048:
        if configured and PW_S1 and pc.C >= _PW_S1_MIN_C and pc.K >= 64 and (not has_res or _PW_S1_RES) and out_numel < (1 << 29):
            # pointwise layers with >= 64 input channels on the pipelined kernel (csrc/conv_pw_s1.hip: fc1 0.75 -> 0.59 ms, res4 / res5
            # conv1 -10..15 %, the memory-bound res2 / res3 conv3 -2..9 % since its epilogue stopped serialising rows:
            # scripts/probe_pw_set.py); precision policy as for the 3x3 layers, and the layers with < 256 input channels keep the
            # two-accumulator form -- bit-identical to the LDS-DMA kernel they ran on before (they are memory-bound: the form costs nothing)
            one = PW_S1 == 2 and not two_acc and pc.C >= _PW_S1_ONE_MIN_C
            if one and PW_W2 and pc.C >= _PW_W2_MIN_C and pc.K >= 256 and pc.K % 256 == 0 and rows >= _PW_W2_MIN_ROWS:
                # >= 256 input and output channels: the 256 x 256 tile (csrc/conv_pw_w2.hip; same operands, 0.67 x the bytes per MFMA)
                return ConvRoute("f16x2_pws1", "lvc_conv1x1_nhwc_f16s1_w2", True, True)
            return ConvRoute("f16x2_pws1", "lvc_conv1x1_nhwc_f16s1" if one else "lvc_conv1x1_nhwc_f16x2_pipe", one, True)
        # the LDS-DMA kernel addresses outputs / residuals through 32-bit buffer descriptors (< 2^29 elements) and moves
        # residual rows in 32-channel chunks; anything else stays on the register-staged kernel
        dma_ok = out_numel < (1 << 29) and (not has_res or (res_numel < (1 << 29) and pc.K % 32 == 0))
        return ConvRoute("f16x2_pw", "lvc_conv2d_nhwc_f16x2_dma" if dma_ok else "lvc_conv2d_nhwc_f16x2", False, configured)
    return ConvRoute("bf16x3", "lvc_conv2d_nhwc_bf16x3", False, False)


# Every entry point of `conv_route` but the Winograd one is called as
#   (x, weights, scale, shift, residual, out, N, H, W, C, K, <tail>, activation code, res_mode, ldo, ldr, <last>, workspace, stream).
# entry point: (weight operand -- "w" packed fp32, "3" bf16 planes, "h" fp16 planes, "s" row-scaled fp16 planes with their own scale --,
#               tail(pc, weights), last(pc)).  A new kernel of that shape is one ConvRoute in `conv_route` and one row here.
_TAIL_GENERIC = lambda pc, wts: (pc.R, pc.S, pc.stride, pc.pad, pc.Kg)
_TAIL_3X3 = lambda pc, wts: (pc.Kg,)
_TAIL_1X1 = lambda pc, wts: (pc.stride,)
_NO_LAST = lambda pc: ()
_CONV_ARGS = {
    "lvc_conv2d_nhwc_f32": ("w", _TAIL_GENERIC, lambda pc: (pc.mode,)),
    "lvc_conv2d_nhwc_bf16x3": ("3", _TAIL_GENERIC, _NO_LAST),
    "lvc_conv2d_nhwc_f16x2": ("h", _TAIL_GENERIC, _NO_LAST),
    "lvc_conv2d_nhwc_f16x2_dma": ("h", _TAIL_GENERIC, _NO_LAST),
    "lvc_conv3x3_nhwc_bf16x3": ("3", _TAIL_3X3, _NO_LAST),
    "lvc_conv3x3_nhwc_f16x2": ("h", _TAIL_3X3, _NO_LAST),
    "lvc_conv3x3_nhwc_f16x2_pipe": ("h", _TAIL_3X3, _NO_LAST),
    "lvc_conv3x3_nhwc_f16s1": ("s", _TAIL_3X3, _NO_LAST),
    "lvc_conv1x1_nhwc_f16x2_pipe": ("h", _TAIL_1X1, _NO_LAST),
    "lvc_conv1x1_nhwc_f16s1": ("s", _TAIL_1X1, _NO_LAST),
    "lvc_conv1x1_nhwc_f16s1_w2": ("s", lambda pc, wts: (wts.shape[1], pc.stride), _NO_LAST),
    "lvc_conv3x3_grouped_nhwc": ("w", lambda pc, wts: (pc.groups, pc.stride), _NO_LAST),
}
# the kernels with torch.nn.GELU() in their epilogue (activation code 2)
_GELU_EPILOGUE = ("lvc_conv1x1_nhwc_f16x2_pipe", "lvc_conv1x1_nhwc_f16s1", "lvc_conv1x1_nhwc_f16s1_w2", "lvc_conv2d_nhwc_f16x2_dma")


def presplit_pair_ok(x, pc2, pc3, residual=None):
    """True where `conv2d_nhwc` would run pc2 on lvc_conv3x3_nhwc_f16s1 and pc3 on lvc_conv1x1_nhwc_f16s1: the pair
    `conv3x3_conv1x1_presplit` replaces launch for launch."""
    if not (PRESPLIT and pc3.C == pc2.K and pc2.K % 32 == 0):
        return False
    N, H, W, C = x.shape
    rows = N * H * W
    # the pair's own limits: no image-group split, no small-row shape, more than 64 outputs, a conv3 that keeps the map
    if not (C == pc2.C and 2048 <= rows and max(x.numel(), rows * pc2.K, rows * pc3.K) < (1 << 29) and pc3.K > 64
            and _out_hw(pc3, H, W) == (H, W)):
        return False
    r2 = conv_route(pc2, N, H, W)
    r3 = conv_route(pc3, N, H, W, ldr=None if residual is None else residual.shape[-1],
                    res_numel=0 if residual is None else residual.numel())
    return r2.entry == "lvc_conv3x3_nhwc_f16s1" and r3.entry == "lvc_conv1x1_nhwc_f16s1"


def conv3x3_conv1x1_presplit(x, pc2, pc3, residual=None, relu=True):
    """relu(conv3x3(x) * s2 + t2) -> act(conv1x1(.) * s3 + t3 (+ residual)) where `presplit_pair_ok`: two launches, the tensor between
    them written as the second one's operand planes (include/lvc_amd.h, `_presplit`).  Reference resnet.py:200-212."""
    _req_cuda(x, residual)
    assert x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32
    N, H, W, C = x.shape
    mid = torch.empty(N, H, W, pc2.K, device=x.device, dtype=torch.float32)      # (planes: same bytes, not fp32 values)
    out = torch.empty(N, H, W, pc3.K, device=x.device, dtype=torch.float32)
    if residual is not None:
        assert residual.is_contiguous() and residual.dtype == torch.float32 and residual.shape[:3] == out.shape[:3]
    ldr = residual.shape[-1] if residual is not None else 0
    ws = ptr(conv_workspace(x.device))
    planes2, scale2 = pc2.split2s()
    planes3, scale3 = pc3.split2s()
    rows = N * H * W
    pc2.last_one = True
    pc3.last_one = True
    _launch("f16x2_halo", 2.0 * rows * pc2.K * C * 9, 4.0 * (rows * C + rows * pc2.K + pc2.K * C * 9), pc2.slot,
            "lvc_conv3x3_nhwc_f16s1_presplit", lambda: _lib.lib().lvc_conv3x3_nhwc_f16s1_presplit(
                ptr(x), ptr(planes2), ptr(scale2), ptr(pc2.shift), ptr(mid), N, H, W, C, pc2.K,
                pc2.Kg, pc3.slot, ws, _stream(x)))
    _launch("f16x2_pws1", 2.0 * rows * pc3.K * pc3.C,
            4.0 * (rows * pc3.C + rows * pc3.K + (residual.numel() if residual is not None else 0) + pc3.K * pc3.C), pc3.slot,
            "lvc_conv1x1_nhwc_f16s1_presplit", lambda: _lib.lib().lvc_conv1x1_nhwc_f16s1_presplit(
                ptr(mid), ptr(planes3), ptr(scale3), ptr(pc3.shift), ptr(residual), ptr(out), N, H, W, pc3.C,
                pc3.K, 1 if relu else 0, 1 if residual is not None else 0, pc3.K, ldr, ws, _stream(x)))
    return out


def conv2d_nhwc(x, pc, relu=False, residual=None, res_mode=0, out=None, split=None, act=None):
    """x: [N,H,W,C] fp32 contiguous (NHWC).  Returns [N,Ho,Wo,K].
    act="gelu": torch.nn.GELU() (erf form) on the result -- in the epilogue of the pointwise kernels that have it, where the layer
    runs on one (bit-identical to a separate lvc_gelu pass), as a second launch otherwise.
    split: None = the configured split (LVC_CONV_SPLIT); "bf16x3" keeps the fp32 exponent range (gradients).
    res_mode 1: residual has the output's shape; 2: residual is [N,Ho/2,Wo/2,K] and is
    nearest-x2-upsampled on the fly (FPN top-down path, reference fpn.py:131-133).
    Which kernel runs is `conv_route`'s answer; its arguments are `_CONV_ARGS`' row."""
    _req_cuda(x, residual)
    assert x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32
    N, H, W, C = x.shape
    assert C == pc.C, "channel mismatch: tensor {} vs packed {}".format(C, pc.C)
    Ho, Wo = _out_hw(pc, H, W)
    if out is None:
        out = torch.empty(N, Ho, Wo, pc.K, device=x.device, dtype=torch.float32)
    grouped = getattr(pc, "groups", 1) != 1
    if grouped and out.numel() == 0:
        return out      # an empty batch: nothing to launch (the grouped kernel's grid is its tile count)
    if residual is not None:
        assert residual.is_contiguous() and residual.dtype == torch.float32
        if res_mode == 0:
            res_mode = 1
    # The split-precision kernels address their operands through 32-bit buffer descriptors (< 2 GiB per tensor).  A batch whose
    # input / output / residual reaches 2^29 elements (32 images on the p2 map) is run in image groups that stay below it --
    # same kernels, same values (a tile never spans two images) -- instead of failing (logged once)
    res_numel = residual.numel() if residual is not None else 0
    big = max(x.numel(), out.numel(), res_numel)
    if big >= (1 << 29) and N > 1 and out.is_contiguous() and out.shape[-1] == pc.K:
        per_image = (big + N - 1) // N
        nb = max(1, ((1 << 29) - 1) // per_image)
        _log_once("conv_batch_split", "conv/GEMM layer with %d elements in one tensor (batch %d): run in groups of %d images to stay "
                  "inside the kernels' 2 GiB buffer descriptors", big, N, nb)
        for n0 in range(0, N, nb):
            n1 = min(N, n0 + nb)
            conv2d_nhwc(x[n0:n1], pc, relu=relu, residual=residual[n0:n1] if residual is not None else None, res_mode=res_mode,
                        out=out[n0:n1], split=split, act=act)
        return out
    ldo = out.shape[-1]
    ldr = residual.shape[-1] if residual is not None else 0
    route = conv_route(pc, N, H, W, ldo, out.is_contiguous(), out.numel(), None if residual is None else ldr, res_numel, split)
    entry = route.entry
    if route.slotted:
        pc.last_one = route.one
    if entry == "lvc_conv3x3_nhwc_wino":
        def call():
            return _wino_launch(x, pc, relu, out)
    else:
        if entry == "lvc_conv2d_nhwc_f16x2" and route.engine == "f16x2_pw":
            _log_once("pw_dma_fallback", "pointwise layer %dx%d->%d (%d output elements, residual %s) is outside the LDS-DMA "
                      "kernel's range; it runs on the register-staged fp16x2 kernel", N * H * W, C, pc.K, out.numel(),
                      "yes" if residual is not None else "no")
        code = 1 if relu else 0
        if act == "gelu" and not relu and entry in _GELU_EPILOGUE:
            code, act = 2, None
        operand, tail, last = _CONV_ARGS[entry]

        def call():
            wts, scale = (pc.split2s() if operand == "s" else
                          ((pc.split2h() if operand == "h" else pc.split3() if operand == "3" else pc.w), pc.scale))
            ints = (N, H, W, C, pc.K) + tail(pc, wts) + (code, res_mode, ldo, ldr) + last(pc)
            return getattr(_lib.lib(), entry)(ptr(x), ptr(wts), ptr(scale), ptr(pc.shift), ptr(residual), ptr(out),
                                              *ints, ptr(conv_workspace(x.device)), _stream(x))
    c_real = 3 if pc.mode == 1 else C
    # algorithmic bytes of the launch: the input pixels it needs, its output, the residual operand, the weights -- each once
    nbytes = 4.0 * (N * (Ho * Wo if (pc.R == 1 and pc.S == 1) else H * W) * c_real + N * Ho * Wo * pc.K + res_numel
                    + pc.K * c_real * pc.R * pc.S)
    if grouped:
        c_real = C // pc.groups
        nbytes = 4.0 * (N * H * W * C + N * Ho * Wo * pc.K + res_numel + pc.K * c_real * 9)
    _launch(route.engine, 2.0 * N * Ho * Wo * pc.K * c_real * pc.R * pc.S, nbytes, pc.slot if route.slotted else None, entry, call)
    if act == "gelu":
        check(_lib.lib().lvc_gelu(ptr(out), ptr(out), out.numel(), _stream(out)), "lvc_gelu")
    elif act is not None:
        raise ValueError("unknown activation {!r}".format(act))
    return out


class PackedChain:
    """Weights of two chained pointwise layers for lvc_conv1x1_chain_nhwc_f16s1 (csrc/conv_pw_chain.hip)."""

    __slots__ = ("wa", "sa", "ta", "wb", "sb", "tb", "K1", "N1", "N2", "slot", "state", "__weakref__")


_PERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)
CHAIN_SHAPES = {(64, 256, 64), (128, 256, 64), (128, 512, 128)}


def _chain_planes(pc):
    """Row-scaled fp16 planes of a pointwise layer's packed weights with the contraction index permuted within every 16
    (position p holds channel 16 * (p // 16) + _PERM16[p % 16]): the order in which an accumulator lane of the transposed MFMA
    holds a block's channels (csrc/conv_pw_chain.hip)."""
    assert pc.R == 1 and pc.S == 1 and pc.mode == 0 and pc.stride == 1 and pc.pad == 0
    rows, Kg = pc.w.shape
    idx = torch.arange(Kg, device=pc.w.device).view(-1, 16)[:, list(_PERM16)].reshape(-1)
    wperm = pc.w[:, idx].contiguous()
    planes = torch.empty((2, rows, Kg), device=pc.w.device, dtype=torch.float16)
    fac = torch.empty(rows, device=pc.w.device, dtype=torch.float32)
    check(_lib.lib().lvc_split_weights_rowscaled(ptr(wperm), rows, Kg, ptr(planes), ptr(fac), _stream(pc.w)),
          "lvc_split_weights_rowscaled")
    fac = fac[: pc.K]
    return planes, (fac * pc.scale if pc.scale is not None else fac).contiguous()


# 3x3 / stride 1 single-accumulator layers as Winograd F(2,3) along x (csrc/conv3x3_wino.hip: two thirds of the MFMAs at the direct
# evaluation's fp32 error, scripts/winograd_error.py) where the launch has at least _WINO_MIN_TILES 256-pixel x 128-channel tiles --
# the kernel is one workgroup per tile, no stream-K: small maps keep the direct kernel
CONV_WINO = _os.environ.get("LVC_CONV_WINO", "1") != "0"
# the Winograd kernel's work distribution: 0 = one workgroup per tile (default: fastest on every routed layer, csrc/conv3x3_wino.hip),
# 1 = stream-K, 2 = persistent workgroups on whole tiles
WINO_STREAMK = int(_os.environ.get("LVC_WINO_STREAMK", "0"))


def set_wino_streamk(mode):
    global WINO_STREAMK
    WINO_STREAMK = int(mode)
    _lib.lib().lvc_set_wino_streamk(int(mode))
# The RPN head's large levels on the Winograd kernel too (kernels.conv3x3_levels_pred).  Off: its single-accumulator form puts p2 proposal
# boxes of the bench batch up to 3.5e-3 px from the exact (fp64) box, past the post-trunk chain test's bar (2 x the oracle's own fp32
# error, ~1.3e-3 px); the two-accumulator direct kernel stays within it for all levels, at +0.3 ms per 8-image step.
WINO_RPN = False
_WINO_MIN_TILES = 512


def pack_wino(pc):
    """Transformed, row-scaled fp16 weight planes of a packed 3x3 layer for lvc_conv3x3_nhwc_wino, cached on the PackedConv:
    U0 = g0, U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2 per filter row (formed in fp64, one fp32 rounding), split by
    lvc_split_weights_rowscaled (rows scaled by a power of two so that neither plane leaves fp16's normal range), stored
    [3 rows][C/16][4 positions][2 planes][Kpad][16].  -> (planes uint16, scale [K] = row factor x the layer's scale)."""
    cached = pc.state.get("_wino")
    if cached is not None and cached[0] is pc.w:
        return cached[1], cached[2]
    assert pc.R == 3 and pc.S == 3 and pc.mode == 0 and pc.C % 32 == 0
    K, C = pc.K, pc.C
    w = pc.w[:K].view(K, C // 32, 3, 3, 32).permute(0, 1, 4, 2, 3).reshape(K, C, 3, 3).double()       # OIHW from the (c/32, r, s, c%32) packing
    g0, g1, g2 = w[..., 0], w[..., 1], w[..., 2]
    U = torch.stack([g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2], dim=-1).float()                 # [K, C, 3 rows, 4 positions]
    Kpad = (K + 127) // 128 * 128
    flat = torch.zeros(Kpad, C * 12, device=pc.w.device)
    flat[:K] = U.reshape(K, C * 12)
    planes = torch.empty(2, Kpad, C * 12, dtype=torch.int16, device=pc.w.device)
    fac = torch.empty(Kpad, device=pc.w.device)
    check(_lib.lib().lvc_split_weights_rowscaled(ptr(flat), Kpad, C * 12, ptr(planes), ptr(fac), _stream(flat)), "lvc_split_weights_rowscaled")
    u = planes.view(2, Kpad, C // 16, 16, 3, 4).permute(4, 2, 5, 0, 1, 3).contiguous()                 # [r][kc][p][plane][Kpad][16]
    scale = (fac[:K] * pc.scale if pc.scale is not None else fac[:K]).contiguous()
    pc.state["_wino"] = (pc.w, u, scale)
    return u, scale


def _wino_launch(x, pc, relu, out):
    _req_cuda(x)
    N, H, W, C = x.shape
    u, scale = pack_wino(pc)
    return _lib.lib().lvc_conv3x3_nhwc_wino(ptr(x), ptr(u), ptr(scale), ptr(pc.shift), ptr(out), N, H, W, C, pc.K,
                                            u.shape[4], 1 if relu else 0, out.stride(2), ptr(conv_workspace(x.device)), _stream(x))


def conv3x3_wino(x, pc, relu=False, out=None):
    """y = act(conv3x3(x) * scale + shift) on the Winograd F(2,3) kernel.  x [N,H,W,C] fp32 NHWC contiguous."""
    if out is None:
        out = torch.empty(x.shape[0], x.shape[1], x.shape[2], pc.K, device=x.device, dtype=torch.float32)
    check(_wino_launch(x, pc, relu, out), "lvc_conv3x3_nhwc_wino")
    return out


def wino_tiles(N, H, W, K):
    return N * ((H + 7) // 8) * ((W + 31) // 32) * ((K + 127) // 128)


def _direct_f16_3x3(pc, C):
    """pc is a 3x3 / stride 1 / pad 1 layer over C channels that the switches and its range tier put on the direct fp16-split kernels."""
    return (CONV_ENGINE == "bf16x3" and CONV_SPLIT == "f16x2" and CONV_HALO and HALO_S1 >= 1 and pc.state["tier"] < 2 and pc.mode == 0
            and pc.R == 3 and pc.S == 3 and pc.stride == 1 and pc.pad == 1 and pc.C == C and C % 32 == 0)


def _level_maps_ok(xs, N, C, K):
    """The maps of a grouped 3x3 launch: [N,H_l,W_l,C] fp32 below 2 GiB each, the largest with enough tiles for the fp16-split kernel."""
    return (all(x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32 and x.shape[0] == N and x.shape[3] == C
                and x.numel() < (1 << 29) for x in xs)
            and halo_tiles(N, max(x.shape[1] * x.shape[2] for x in xs), K) >= _HALO_H2_MIN_TILES)


def _wino_levels(xs, K):
    """(big, rest): indices of the maps large enough for the Winograd kernel, each launched alone, and of those that stay grouped."""
    big = [i for i, x in enumerate(xs) if wino_sized(x.shape[0], x.shape[1], x.shape[2], K)]
    return big, [i for i in range(len(xs)) if i not in big]


_GROUP_SLOTS = {}


def _group_slot(pcs):
    """One range slot owned by all layers of a grouped launch: a raised word moves every one of them to the next wider form."""
    key = tuple(id(pc.state) for pc in pcs)
    ent = _GROUP_SLOTS.get(key)
    if ent is None or any(r() is None for r in ent[1]):
        import weakref

        slot = _new_range_slot(pcs[0])
        for pc in pcs[1:]:
            _SLOT_OWNERS[slot].append(weakref.ref(pc))
        if len(_GROUP_SLOTS) > 64:
            _GROUP_SLOTS.clear()
        ent = _GROUP_SLOTS[key] = (slot, [weakref.ref(pc) for pc in pcs])
    else:
        # the packed layers may have been rebuilt (new objects, same range state): keep the slot's owners current
        import weakref

        # (merged with the live owners: a slot handed out twice after the round-robin wrapped keeps its other layer)
        live = [r for r in _SLOT_OWNERS.get(ent[0], []) if r() is not None and all(r() is not pc for pc in pcs)]
        _SLOT_OWNERS[ent[0]] = live + [weakref.ref(pc) for pc in pcs]
    return ent[0]


def conv3x3_levels(xs, pc, relu=False, outs=None):
    """A 3x3 / stride 1 / pad 1 layer over several maps xs[l] [N,H_l,W_l,C] in ONE launch of the pipelined fp16-split kernel (one
    stream-K split over the row tiles of all maps: the small maps no longer pay a launch each that cannot fill the chip).  `pc`: one
    PackedConv -- the SAME layer on every map (the RPN head over the pyramid levels, lvc_conv3x3_nhwc_f16_levels) -- or a list with a
    layer per map, all of one shape and precision form (the FPN output convs, lvc_conv3x3_nhwc_f16_layers).  outs[l] (optional):
    [N,H_l,W_l,K] contiguous buffers to write.  Falls back to one conv2d_nhwc call per map where that kernel is not the layers'
    route (another engine or split, a range tier on the bf16x3 kernels, mixed forms, maps of 2 GiB)."""
    _req_cuda(*xs)
    pcs = list(pc) if isinstance(pc, (list, tuple)) else [pc] * len(xs)
    shared = not isinstance(pc, (list, tuple))
    p0 = pcs[0]
    N, C = xs[0].shape[0], xs[0].shape[3]
    if outs is None:
        outs = [torch.empty(x.shape[0], x.shape[1], x.shape[2], q.K, device=x.device, dtype=torch.float32) for x, q in zip(xs, pcs)]
    forms = {(q.two_acc or q.state["tier"] >= 1) for q in pcs}
    ok = (len(xs) > 1 and len(xs) <= 6 and len(pcs) == len(xs) and len(forms) == 1
          and all(_direct_f16_3x3(q, C) and q.K == p0.K and q.Kg == p0.Kg for q in pcs) and p0.K >= 64 and p0.K % 4 == 0
          and _level_maps_ok(xs, N, C, p0.K)
          and all(o.is_contiguous() and o.shape == (x.shape[0], x.shape[1], x.shape[2], p0.K) for o, x in zip(outs, xs)))
    if not ok:
        for x, q, o in zip(xs, pcs, outs):
            conv2d_nhwc(x, q, relu=relu, out=o)
        return outs
    one = HALO_S1 == 2 and not (True in forms)
    # (`two_acc` layers -- the RPN head outside its fused-predictor launch, e.g. in a training forward -- qualify under WINO_RPN: the
    # Winograd form's error is below the one-accumulator direct form's and passes the head's chain test, see conv3x3_levels_pred)
    if CONV_WINO and HALO_S1 == 2 and all(q.state["tier"] == 0 and (not q.two_acc or WINO_RPN) for q in pcs):
        # maps large enough to fill the chip with one-workgroup tiles run on the Winograd F(2,3) kernel (two thirds of the MFMAs), each
        # alone; the small ones stay one grouped launch of the direct kernel
        big, rest = _wino_levels(xs, p0.K)
        if big:
            for i in big:
                conv2d_nhwc(xs[i], pcs[i], relu=relu, out=outs[i])
            if rest:
                conv3x3_levels([xs[i] for i in rest], pc if shared else [pcs[i] for i in rest], relu=relu, outs=[outs[i] for i in rest])
            return outs
    L = len(xs)
    XP, IP = c_void_p * L, c_int * L
    xp, yp = XP(*[x.data_ptr() for x in xs]), XP(*[o.data_ptr() for o in outs])
    hs, ws = IP(*[x.shape[1] for x in xs]), IP(*[x.shape[2] for x in xs])
    for q in pcs:
        q.last_one = one
    ops = [q.split2s() if one else (q.split2h(), q.scale) for q in (pcs[:1] if shared else pcs)]
    if shared:
        weights = (ptr(ops[0][0]), ptr(ops[0][1]), ptr(p0.shift))
    else:
        weights = [XP(*[0 if t is None else t.data_ptr() for t in ts]) for ts in ([o[0] for o in ops], [o[1] for o in ops], [q.shift for q in pcs])]
    entry = "lvc_conv3x3_nhwc_f16_levels" if shared else "lvc_conv3x3_nhwc_f16_layers"
    px = sum(x.shape[0] * x.shape[1] * x.shape[2] for x in xs)
    _launch("f16x2_halo", 2.0 * px * p0.K * C * 9, 4.0 * (px * C + px * p0.K + (1 if shared else L) * p0.K * C * 9),
            p0.slot if shared else _group_slot(pcs), entry, lambda: getattr(_lib.lib(), entry)(
                1 if one else 0, xp, yp, hs, ws, L, *weights, N, C, p0.K, p0.Kg,
                1 if relu else 0, ptr(conv_workspace(xs[0].device)), _stream(xs[0])))
    return outs


def conv3x3_levels_pred(xs, pc, pred, relu=True, _outs=None):
    """act(conv3x3(xs[l])) through the pointwise layer `pred` (<= 32 outputs) in the ONE launch of `conv3x3_levels`: the hidden maps are
    never written -- every workgroup of the 3x3 kernel contracts its 128 hidden channels with the pointwise weights in its epilogue and
    adds the slice to the (zeroed) output atomically (two slices per element: order-free, csrc/conv3x3_halo_s1.hip).  The RPN head:
    conv + ReLU, then objectness | anchor deltas.  Returns the list of [N,H_l,W_l,pred.K] outputs (views of one [sum of pixels, pred.K]
    buffer), or None where the launch does not apply (the caller runs the two layers one after the other)."""
    _req_cuda(*xs)
    N, C = xs[0].shape[0], xs[0].shape[3]
    ok = (1 <= len(xs) <= 6 and _direct_f16_3x3(pc, C)
          and (pc.two_acc or pc.state["tier"] == 1 or HALO_S1 == 1)      # the two-accumulator instance
          and pc.K in (128, 256) and pc.Kg == 9 * C
          and pred.mode == 0 and pred.R == 1 and pred.S == 1 and pred.stride == 1 and pred.pad == 0 and pred.C == pc.K and pred.Kg == pc.K
          and 1 <= pred.K <= 32 and pred.w.shape[0] >= 32 and pred.state["tier"] < 2
          and _level_maps_ok(xs, N, C, pc.K))
    if not ok:
        return None
    ms = [x.shape[0] * x.shape[1] * x.shape[2] for x in xs]
    if _outs is None:
        y = torch.zeros(sum(ms), pred.K, device=xs[0].device, dtype=torch.float32)
        outs, off = [], 0
        for x, m in zip(xs, ms):
            outs.append(y[off:off + m].view(x.shape[0], x.shape[1], x.shape[2], pred.K))
            off += m
    else:
        outs = _outs
    if CONV_WINO and WINO_RPN and HALO_S1 == 2 and pc.state["tier"] == 0:
        # The levels that fill the chip with one-workgroup tiles on the Winograd kernel, each alone, with the same epilogue; the small
        # ones stay one grouped launch of the two-accumulator direct kernel.  (The head is packed `two_acc`: its logits decide top-k and
        # NMS.  The Winograd form's measured error lies between the two direct forms' -- rms 4.8e-8 of the output scale against 6.7e-8
        # one accumulator / ~4e-8 two -- but its largest box errors miss the post-trunk chain test's bar: off by default, see WINO_RPN.)
        big, rest = _wino_levels(xs, pc.K)
        if big:
            u, scale = pack_wino(pc)
            pplanes = pred.split2h()
            pc.last_one = True
            pred.last_one = False
            for i in big:
                x, o = xs[i], outs[i]
                px = x.shape[0] * x.shape[1] * x.shape[2]
                _launch("f16x2_wino", 2.0 * px * pc.K * (C * 9 + pred.K), 4.0 * (px * C + px * pred.K + pc.K * (C * 9 + pred.K)), pc.slot,
                        "lvc_conv3x3_nhwc_wino_pred", lambda: _lib.lib().lvc_conv3x3_nhwc_wino_pred(
                            ptr(x), ptr(u), ptr(scale), ptr(pc.shift), ptr(o), N, x.shape[1], x.shape[2],
                            C, pc.K, u.shape[4], 1 if relu else 0, pred.K, ptr(pplanes),
                            ptr(pred.scale), ptr(pred.shift), pred.K, pred.w.shape[0], pred.slot,
                            ptr(conv_workspace(x.device)), _stream(x)))
            if rest:
                sub = conv3x3_levels_pred([xs[i] for i in rest], pc, pred, relu=relu, _outs=[outs[i] for i in rest])
                assert sub is not None
            return outs
    L = len(xs)
    XP, IP = c_void_p * L, c_int * L
    xp, yp = XP(*[x.data_ptr() for x in xs]), XP(*[o.data_ptr() for o in outs])
    hs, ws = IP(*[x.shape[1] for x in xs]), IP(*[x.shape[2] for x in xs])
    pc.last_one = False
    pred.last_one = False
    planes, pplanes = pc.split2h(), pred.split2h()
    px = sum(ms)
    _launch("f16x2_halo", 2.0 * px * pc.K * (C * 9 + pred.K), 4.0 * (px * C + px * pred.K + pc.K * (C * 9 + pred.K)), pc.slot,
            "lvc_conv3x3_nhwc_f16_levels_pred", lambda: _lib.lib().lvc_conv3x3_nhwc_f16_levels_pred(
                0, xp, yp, hs, ws, L, ptr(planes), ptr(pc.scale), ptr(pc.shift), N,
                C, pc.K, pc.Kg, 1 if relu else 0, ptr(pplanes),
                ptr(pred.scale), ptr(pred.shift), pred.K, pred.w.shape[0],
                pred.K, pred.slot, ptr(conv_workspace(xs[0].device)), _stream(xs[0])))
    return outs


def pack_chain(pc_a, pc_b, state=None):
    """pc_a: the first pointwise layer (K1 -> N1), pc_b: the second (N1 -> N2), both `pack_conv` results of 1x1 layers.
    state: a dict the owner keeps across re-packs; state["off"] is set when the pair overflowed the kernel's range
    (|a| > 4094 for its input or the intermediate: `check_conv_error_word`) and must run as two launches from then on."""
    assert pc_b.C == pc_a.K
    ch = PackedChain()
    ch.slot = _new_range_slot(ch)
    ch.state = state if state is not None else {"off": False}
    ch.wa, ch.sa = _chain_planes(pc_a)
    ch.wb, ch.sb = _chain_planes(pc_b)
    ch.ta, ch.tb = pc_a.shift, pc_b.shift
    ch.K1, ch.N1, ch.N2 = pc_a.C, pc_a.K, pc_b.K
    return ch


def conv1x1_chain(x, ch, residual=None, relu1=True, relu2=True, out1=None, out2=None):
    """y1 = act1(x Wa^T * sa + ta (+ residual)), y2 = act2(y1 Wb^T * sb + tb) in one launch; x [..., ldx] NHWC whose first K1
    channels are the first layer's input (a row stride wider than K1 is allowed).  Returns (y1, y2)."""
    _req_cuda(x, residual)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] >= ch.K1
    M = x.numel() // x.shape[-1]
    lead = tuple(x.shape[:-1])
    if out1 is None:
        out1 = torch.empty(lead + (ch.N1,), device=x.device, dtype=torch.float32)
    if out2 is None:
        out2 = torch.empty(lead + (ch.N2,), device=x.device, dtype=torch.float32)
    if residual is not None:
        assert residual.is_contiguous() and residual.dtype == torch.float32 and residual.numel() // residual.shape[-1] == M
    nbytes = 4.0 * (M * (ch.K1 + ch.N1 + ch.N2 + (ch.N1 if residual is not None else 0)) + ch.K1 * ch.N1 + ch.N1 * ch.N2)
    _launch("f16s1_chain", 2.0 * M * (ch.K1 * ch.N1 + ch.N1 * ch.N2), nbytes, ch.slot, "lvc_conv1x1_chain_nhwc_f16s1",
            lambda: _lib.lib().lvc_conv1x1_chain_nhwc_f16s1(
                ptr(x), x.shape[-1], ptr(ch.wa), ch.wa.shape[1], ptr(ch.sa), ptr(ch.ta), ptr(residual),
                residual.shape[-1] if residual is not None else 0, ptr(out1), out1.shape[-1], 1 if relu1 else 0,
                ptr(ch.wb), ch.wb.shape[1], ptr(ch.sb), ptr(ch.tb), ptr(out2), out2.shape[-1], 1 if relu2 else 0,
                M, ch.K1, ch.N1, ch.N2, ptr(conv_workspace(x.device)), _stream(x)))
    return out1, out2


class PackedBneck:
    """One bottleneck block's weights as the stage images of lvc_bottleneck_nhwc_f16s1 (csrc/conv_bneck.hip)."""

    __slots__ = ("w", "s1", "t1", "s2", "t2", "s3", "t3", "cin", "proj", "slot", "state", "__weakref__")


BNECK = _os.environ.get("LVC_BNECK", "1") != "0"      # whole res2 blocks (64 mid, 256 out channels, stride 1) as one launch
BNECK_SHAPES = {(256, 64, 256, False), (64, 64, 256, True)}      # (in, mid, out channels, projection shortcut)
_BNECK_IDX = {}


def _bneck_index(cin, proj, device):
    """Gather indices (plane, row, column) into the three layers' [2][rows][Kg] split planes for every fp16 of the stage images:
    a stage is a run of 1 KB fragments in lane order -- lane l holds row l % 32 of the fragment's 32-row block and the 8
    contraction entries of k half l // 32 in the permuted order of csrc/conv_pw_chain.hip (`_PERM16`)."""
    key = (cin, proj, str(device))
    if key in _BNECK_IDX:
        return _BNECK_IDX[key]
    import numpy as np

    lane = np.arange(64)
    rowl = (lane % 32)[:, None].repeat(8, 1)                                    # [64, 8]
    kpos = np.asarray(_PERM16)[(lane // 32)[:, None] * 8 + np.arange(8)[None]]   # natural k16 offset held at (lane, slot)

    def frags(specs):
        pl = np.stack([np.full((64, 8), s[0]) for s in specs])
        rows = np.stack([s[1] + rowl for s in specs])
        cols = np.stack([np.asarray(s[2])[kpos] for s in specs])
        return pl, rows, cols

    a16 = np.arange(16)
    p1 = [(pl, 32 * cb, 32 * c + 16 * sp + a16) for c in range(cin // 32) for sp in range(2) for cb in range(2) for pl in range(2)]

    def col2(ch, r, s_):      # pack_conv's contraction order: (c // 32, r, s, c % 32)
        return (ch // 32) * 288 + (r * 3 + s_) * 32 + ch % 32

    # conv2: the 36 (k16 step, tap) pairs in the order the kernel walks them, two a stage
    p2 = [(pl, 32 * cb, col2(16 * (u // 9) + a16, (u % 9) // 3, (u % 9) % 3)) for u in range(36) for cb in range(2) for pl in range(2)]
    p3 = [(pl, 32 * j, 64 * half + 16 * s + a16) for j in range(8) for half in range(2 if proj else 1) for s in range(4)
          for pl in range(2)]
    out = tuple(tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in frags(sp)) for sp in (p1, p2, p3))
    _BNECK_IDX[key] = out
    return out


def pack_bottleneck(pc1, pc2, pc3, proj, state=None):
    """pc1 / pc2 / pc3: `pack_conv` results of a bottleneck's conv1 (1x1), conv2 (3x3, pad 1) and conv3 (1x1; with proj the fused
    [conv3 | projection shortcut] pack of BottleneckBlock._fused_projection, 128 contraction channels), FrozenBN folded."""
    assert pc1.R == 1 and pc2.R == 3 and pc2.S == 3 and pc2.pad == 1 and pc2.stride == 1 and pc3.R == 1 and pc1.stride == 1
    cin = pc1.C
    assert (cin, pc1.K, pc3.K, bool(proj)) in BNECK_SHAPES and pc2.C == 64 and pc2.K == 64 and pc3.C == (128 if proj else 64)
    dev = pc1.w.device
    bk = PackedBneck()
    bk.slot = _new_range_slot(bk)
    bk.state = state if state is not None else {"off": False}
    bk.cin, bk.proj = cin, bool(proj)
    parts = []
    affine = []
    for pc, (pl, rows, cols) in zip((pc1, pc2, pc3), _bneck_index(cin, bool(proj), dev)):
        nrows, Kg = pc.w.shape
        planes = torch.empty((2, nrows, Kg), device=dev, dtype=torch.float16)
        fac = torch.empty(nrows, device=dev, dtype=torch.float32)
        check(_lib.lib().lvc_split_weights_rowscaled(ptr(pc.w), nrows, Kg, ptr(planes), ptr(fac), _stream(pc.w)),
              "lvc_split_weights_rowscaled")
        parts.append(planes[pl, rows, cols].reshape(-1))
        fac = fac[: pc.K]
        affine.append(((fac * pc.scale) if pc.scale is not None else fac).contiguous())
        affine.append(pc.shift.contiguous() if pc.shift is not None else torch.zeros(pc.K, device=dev, dtype=torch.float32))
    bk.w = torch.cat(parts).contiguous()
    bk.s1, bk.t1, bk.s2, bk.t2, bk.s3, bk.t3 = affine
    return bk


def bottleneck_fused(x, bk, out=None):
    """relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + shortcut(x)) in ONE launch (reference resnet.py:195-211);
    x [N,H,W,ldx] NHWC fp32 whose first bk.cin channels are the block's input."""
    _req_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[-1] >= bk.cin
    N, H, W, ldx = x.shape
    if out is None:
        out = torch.empty(N, H, W, 256, device=x.device, dtype=torch.float32)
    M = N * H * W
    kk = bk.cin * 64 + 64 * 64 * 9 + 64 * 256 + (bk.cin * 256 if bk.proj else 0)
    _launch("f16s1_bneck", 2.0 * M * kk, 4.0 * (M * (bk.cin + 256) + kk), bk.slot, "lvc_bottleneck_nhwc_f16s1",
            lambda: _lib.lib().lvc_bottleneck_nhwc_f16s1(
                ptr(x), ldx, ptr(out), out.shape[-1], N, H, W,
                bk.cin, 1 if bk.proj else 0, ptr(bk.w), ptr(bk.s1), ptr(bk.t1), ptr(bk.s2),
                ptr(bk.t2), ptr(bk.s3), ptr(bk.t3), ptr(conv_workspace(x.device)), _stream(x)))
    return out


def split_planes_f16x2(w):
    """[2, *w.shape] fp16 planes (w1 = fp16(w), w2 = fp16((w - w1) * 2048)) of an fp32 tensor (lvc_split_weights)."""
    _req_cuda(w)
    w = w.detach().float().contiguous()
    out = torch.empty((2,) + tuple(w.shape), device=w.device, dtype=torch.float16)
    check(_lib.lib().lvc_split_weights(ptr(w), w.numel(), 2, ptr(out), ptr(_conv_error_view(w.device)), _stream(w)),
          "lvc_split_weights")
    return out


def stem_conv_pool(x4, pc, relu=True, second=None):
    """x4 [N,H,W,4] NHWC4, pc = pack_conv(stem weight 64x3x7x7, bn=..., stride=2, pad=3, stem=True) ->
    [N,Hp,Wp,64]: conv 7x7/2 + affine + ReLU + max-pool 3x3/2 in one launch."""
    _req_cuda(x4)
    assert x4.dim() == 4 and x4.shape[3] == 4 and x4.is_contiguous() and x4.dtype == torch.float32
    assert pc.mode == 1 and pc.K == 64 and pc.R == 7 and pc.stride == 2 and pc.pad == 3
    N, H, W, _ = x4.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    out = torch.empty(N, Hp, Wp, 64, device=x4.device, dtype=torch.float32)
    y2 = second(out.shape) if second is not None else None     # [N,Hp,Wp,64] view with a wider row stride
    if y2 is not None:
        assert y2.shape == out.shape and y2.stride(3) == 1 and y2.stride(1) == Wp * y2.stride(2) and y2.stride(0) == Hp * y2.stride(1)
    if CONV_SPLIT == "f16x2":
        err = _conv_error_view(x4.device)   # the conv error word
        st = _lib.lib().lvc_stem_conv_pool_nhwc4_f16x2(ptr(x4), ptr(pc.split2h()), ptr(pc.scale), ptr(pc.shift), ptr(out),
                                                       N, H, W, pc.w.shape[0],
                                                       1 if relu else 0, ptr(err), ptr(y2),
                                                       y2.stride(2) if y2 is not None else 0, _stream(x4))
        check(st, "lvc_stem_conv_pool_nhwc4_f16x2")
        return out
    raise RuntimeError("the fused stem exists for the fp16 split only; BasicStem runs conv + max-pool as two launches otherwise")


def linear(x, pc, relu=False, split=None):
    """x: [M, K_in] -> [M, K_out] through the same MFMA kernel.  split: as conv2d_nhwc (gradient GEMMs pass
    DGRAD_SPLIT: unscaled gradients sit below fp16's normal range, and the fp16 split's range word only sees overflow)."""
    M, Kin = x.shape
    y = conv2d_nhwc(x.view(M, 1, 1, Kin), pc, relu=relu, split=split)
    return y.view(M, pc.K)


# --------------------------------------------------------------------------- ROIAlign
def new_status(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


# the bits of the status word, as the kernels set them (roi_heads.check_status raises for each)
ROI_NEGATIVE_SIZE = 1     # ROIAlign: a RoI of negative width or height
DET_OVERFLOW = 2          # lvc_fast_rcnn_inference: more (roi, class) candidates in one image than the candidate list holds
RETINA_OVERFLOW = 4       # lvc_retinanet_select: more entries on one (image, level) than the survivor list holds
MASK_BAD_CLASS = 8        # lvc_mask_deconv_predict / _logits / _grad: a class index outside [0, K)
KEYPOINT_BAD_TARGET = 16  # lvc_keypoint_loss: a heatmap target outside [0, 16 S^2) on a valid entry (the entry is skipped)


def roi_align_forward(input, rois, spatial_scale, pooled_h, pooled_w, sampling_ratio, aligned, status=None):
    """Reference-shaped op (csrc/vision.cpp:96): NCHW input, rois [K,5], returns [K,C,ph,pw]."""
    _req_cuda(input, rois)
    input = input.contiguous().float()
    rois = rois.contiguous().float()
    B, C, H, W = input.shape
    K = rois.shape[0]
    out = torch.empty(K, C, pooled_h, pooled_w, device=input.device, dtype=torch.float32)
    st = _lib.lib().lvc_roi_align_forward_nchw(
        ptr(input), ptr(rois), ptr(out), B, C, H, W, K,
        pooled_h, pooled_w, spatial_scale, sampling_ratio,
        1 if aligned else 0, ptr(status), _stream(input))
    check(st, "lvc_roi_align_forward_nchw")
    return out


ROI_FWD_ROUTES = ("scalar", "nhwc4", "wave")      # lvc_roi_align_route, forward: its answers by name
ROI_BWD_ROUTES = ("scatter", "rows")              # ... and backward


def roi_align_route(backward, nhwc, C, pooled_h, pooled_w, has_num_valid=False, largest_level_elems=0):
    """The kernel a ROIAlign call of these shapes runs, by name, from the library's own dispatch (host only, nothing is launched);
    largest_level_elems: max over the levels of H * W * C."""
    r = _lib.lib().lvc_roi_align_route(1 if backward else 0, 1 if nhwc else 0, C, pooled_h, pooled_w, 1 if has_num_valid else 0,
                                       largest_level_elems)
    return (ROI_BWD_ROUTES if backward else ROI_FWD_ROUTES)[r]


ROI_ORDER_MIN = 1024     # RoIs per launch from which a work order is computed (lvc_roi_work_order: one small launch)


def roi_align_fpn_nhwc(feats, scales, rois, levels, pooled_h, pooled_w, sampling_ratio, aligned,
                       num_valid=None, status=None, order=None, out=None):
    """feats: list of NHWC level tensors [B,H_l,W_l,C]; rois [K,5]; levels [K] int32 (or None when one
    level).  Returns [K, ph, pw, C] (written into `out` when one is given)."""
    _req_cuda(rois, *feats)
    L = len(feats)
    B, _, _, C = feats[0].shape
    K = rois.shape[0]
    rois = rois.contiguous().float()
    if out is None:
        out = torch.empty(K, pooled_h, pooled_w, C, device=rois.device, dtype=torch.float32)
    assert out.shape == (K, pooled_h, pooled_w, C) and out.is_contiguous() and out.dtype == torch.float32
    FP = c_void_p * L
    IP = c_int * L
    FL = c_float * L
    fp = FP(*[f.data_ptr() for f in feats])
    hs = IP(*[f.shape[1] for f in feats])
    ws = IP(*[f.shape[2] for f in feats])
    sc = FL(*[float(s) for s in scales])
    for f in feats:
        assert f.is_contiguous() and f.dtype == torch.float32 and f.shape[0] == B and f.shape[3] == C
    if levels is not None:
        assert levels.dtype == torch.int32 and levels.is_contiguous()
    if order is not None:       # a caller's own work order ([K] int32 permutation; experiments)
        assert order.dtype == torch.int32 and order.is_contiguous() and order.numel() == K
    elif K >= ROI_ORDER_MIN:
        # the workgroups take the RoIs largest window first (the launch's time follows the window area; in proposal order a few
        # large RoIs start last and finish alone)
        order = torch.empty(K, device=rois.device, dtype=torch.int32)
        if B <= 16:
            # image b's RoIs on XCD b % 8, inside an image by (level, band of rows): what an XCD reads close in time shares its L2
            check(_lib.lib().lvc_roi_work_order_xcd(ptr(rois), ptr(levels), K, B, ptr(order), _stream(rois)), "lvc_roi_work_order_xcd")
        else:
            check(_lib.lib().lvc_roi_work_order(ptr(rois), ptr(levels), sc, L, K, pooled_h, ptr(order), _stream(rois)),
                  "lvc_roi_work_order")
    st = _lib.lib().lvc_roi_align_fpn_nhwc_ordered(
        fp, hs, ws, sc, L, B, C, ptr(rois), ptr(levels), ptr(num_valid), K,
        pooled_h, pooled_w, sampling_ratio, 1 if aligned else 0, ptr(out),
        ptr(status), ptr(order), _stream(rois))
    check(st, "lvc_roi_align_fpn_nhwc")
    return out


def roi_align_backward(grad, rois, spatial_scale, pooled_h, pooled_w, batch_size, channels, height, width,
                       sampling_ratio, aligned, status=None):
    """Reference-shaped op (csrc/vision.cpp:97): grad [K,C,ph,pw], rois [K,5] -> grad_input [B,C,H,W]."""
    _req_cuda(grad, rois)
    grad = grad.contiguous().float()
    rois = rois.contiguous().float()
    K = rois.shape[0]
    assert grad.shape == (K, channels, pooled_h, pooled_w)
    gin = torch.empty(batch_size, channels, height, width, device=grad.device, dtype=torch.float32)
    st = _lib.lib().lvc_roi_align_backward_nchw(
        ptr(grad), ptr(rois), ptr(gin), batch_size, channels, height, width, K,
        pooled_h, pooled_w, spatial_scale, sampling_ratio,
        1 if aligned else 0, ptr(status), _stream(grad))
    check(st, "lvc_roi_align_backward_nchw")
    return gin


def roi_align_fpn_backward_nhwc(grad, shapes, scales, rois, levels, sampling_ratio, aligned, num_valid=None,
                                status=None, outs=None):
    """Gradient of roi_align_fpn_nhwc.  grad [K,ph,pw,C]; shapes: list of (B,H_l,W_l,C).  Returns the list of
    NHWC level gradients (zeroed and written into `outs` when they are given)."""
    _req_cuda(grad, rois)
    grad = grad.contiguous().float()
    rois = rois.contiguous().float()
    K, ph, pw, C = grad.shape
    L = len(shapes)
    B = shapes[0][0]
    if outs is None:
        outs = [torch.empty(*sh, device=grad.device, dtype=torch.float32) for sh in shapes]
    assert len(outs) == L
    for o, sh in zip(outs, shapes):
        assert o.shape == tuple(sh) and o.is_contiguous() and o.dtype == torch.float32 and sh[0] == B and sh[3] == C
    FP = c_void_p * L
    IP = c_int * L
    FL = c_float * L
    if levels is not None:
        assert levels.dtype == torch.int32 and levels.is_contiguous()
    st = _lib.lib().lvc_roi_align_fpn_backward_nhwc(
        ptr(grad), FP(*[o.data_ptr() for o in outs]), IP(*[sh[1] for sh in shapes]), IP(*[sh[2] for sh in shapes]),
        FL(*[float(s) for s in scales]), L, B, C, ptr(rois), ptr(levels), ptr(num_valid),
        K, ph, pw, sampling_ratio, 1 if aligned else 0, ptr(status),
        _stream(grad))
    check(st, "lvc_roi_align_fpn_backward_nhwc")
    return outs


# --------------------------------------------------------------------------- NMS
# Proposal / detection selection (csrc/boxes.hip, csrc/nms.hip): bit 0 = the RPN's per-level top-k as a wide key pass + one workgroup per
# (image, level) (with bit 2: that workgroup alone, one launch, slower), bit 1 = the detection NMS sorts only its head rows.  3 (default) =
# both; 0 = the multi-launch top-k and the full sort they replace, kept as the parity witness of tests/test_gpu_select_onelaunch.py /
# test_gpu_nms_headsort.py and as the A/B arm.  Same outputs for every value.
SELECT_ONELAUNCH = int(_os.environ.get("LVC_SELECT_ONELAUNCH", "3"))


def set_select_onelaunch(mode):
    global SELECT_ONELAUNCH
    SELECT_ONELAUNCH = int(mode)
    _lib.lib().lvc_set_select_onelaunch(int(mode))


def batched_nms_batch(boxes, scores, idxs, counts, iou_threshold, max_keep=0):
    """boxes [B,Nmax,4], scores [B,Nmax], idxs [B,Nmax] int32 or None, counts [B] int32 device or None.
    Returns (keep [B,Nmax] int32, num_keep [B] int32), all on device, no sync."""
    _req_cuda(boxes, scores, idxs, counts)
    B, Nmax = scores.shape
    boxes = boxes.contiguous().float()
    scores = scores.contiguous().float()
    if idxs is not None:
        idxs = idxs.contiguous()
        assert idxs.dtype == torch.int32
    keep = torch.empty(B, Nmax, dtype=torch.int32, device=boxes.device)
    num_keep = torch.empty(B, dtype=torch.int32, device=boxes.device)
    wsb = _lib.size_query("lvc_batched_nms_workspace_bytes", B, Nmax)
    ws = torch.empty(wsb, dtype=torch.uint8, device=boxes.device)
    st = _lib.lib().lvc_batched_nms(
        ptr(boxes), ptr(scores), ptr(idxs), ptr(counts), B, Nmax, iou_threshold,
        max_keep, ptr(keep), ptr(num_keep), ptr(ws), wsb, _stream(boxes))
    check(st, "lvc_batched_nms")
    return keep, num_keep


def batched_nms(boxes, scores, idxs, iou_threshold):
    """Drop-in for reference detectron2/layers/nms.py:10-29 (single image): int64 keep indices,
    score-descending."""
    n = boxes.shape[0]
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    idx32 = idxs.to(torch.int32)[None] if idxs is not None else None
    keep, nk = batched_nms_batch(boxes[None], scores[None], idx32, None, iou_threshold)
    return keep[0, : int(nk.item())].to(torch.int64)


def nms(boxes, scores, iou_threshold):
    """Drop-in for torchvision.ops.nms as imported by reference detectron2/layers/nms.py:7."""
    return batched_nms(boxes, scores, None, iou_threshold)


# --------------------------------------------------------------------------- box pipeline
SCALE_CLAMP = 4.135166556742356  # log(1000/16), reference detectron2/modeling/box_regression.py:11-12


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def rpn_proposals(logits, deltas, cell_anchors, strides, image_sizes, pre_nms_topk, post_nms_topk,
                  nms_thresh, min_box_size=0.0):
    """find_top_rpn_proposals on device (reference proposal_utils.py:13-118 + rpn.py:489-508).

    logits[l]: [B,H,W,ld] view whose channel a holds the objectness of anchor a (any channel stride);
    deltas[l]: [B,H,W,ld'] view whose channel a*4+c holds delta c of anchor a.  Both may be channel
    slices of one fused NHWC tensor (pass tensor[..., :A] and tensor[..., A:]).
    cell_anchors[l]: [A,4] device tensors; image_sizes: [B,2] int32 device (h, w).
    Returns (boxes [B,post,4], objectness_logits [B,post], count [B] int32); rows past count are zero.
    """
    L = len(logits)
    B, A = logits[0].shape[0], cell_anchors[0].shape[0]
    dev = logits[0].device
    _req_cuda(*logits, *deltas, *cell_anchors, image_sizes)
    for t in list(logits) + list(deltas):
        assert t.dtype == torch.float32 and t.stride(-1) == 1 and t.dim() == 4
        assert t.stride(2) == t.stride(3) * 0 + t.stride(2)  # pixel-major view
    Hs = [t.shape[1] for t in logits]
    Ws = [t.shape[2] for t in logits]
    for t, h, w in zip(list(logits) + list(deltas), Hs * 2, Ws * 2):
        # rows must be dense pixels: stride(1) == W*stride(2), stride(0) == H*W*stride(2)
        assert t.stride(1) == w * t.stride(2) and t.stride(0) == h * w * t.stride(2), "need an NHWC channel slice"
    VP, IP = c_void_p * L, c_int * L
    lp = VP(*[t.data_ptr() for t in logits])
    dp = VP(*[t.data_ptr() for t in deltas])
    ap = VP(*[t.contiguous().data_ptr() for t in cell_anchors])
    ldl = IP(*[t.stride(2) for t in logits])
    ldd = IP(*[t.stride(2) for t in deltas])
    hs, ws_, st = IP(*Hs), IP(*Ws), IP(*strides)
    lib = _lib.lib()
    nbytes = _lib.size_query("lvc_rpn_proposals_workspace_bytes", B, L, A, hs, ws_, pre_nms_topk)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    boxes = torch.empty(B, post_nms_topk, 4, device=dev, dtype=torch.float32)
    olog = torch.empty(B, post_nms_topk, device=dev, dtype=torch.float32)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    assert image_sizes.dtype == torch.int32 and image_sizes.is_contiguous()
    rc = lib.lvc_rpn_proposals(lp, ldl, dp, ldd, ap, hs, ws_, st, L, A, B, ptr(image_sizes),
                               pre_nms_topk, post_nms_topk, nms_thresh,
                               min_box_size, SCALE_CLAMP, ptr(boxes), ptr(olog), ptr(count),
                               ptr(ws), nbytes, _stream(boxes))
    check(rc, "lvc_rpn_proposals")
    return boxes, olog, count


def assign_levels_rois(boxes, min_level, max_level, canonical_box_size=224, canonical_level=4):
    """boxes [B,R,4] -> (levels [B*R] int32, rois [B*R,5]) (reference poolers.py:23-59, 69-96)."""
    _req_cuda(boxes)
    B, R, _ = boxes.shape
    boxes = boxes.contiguous()
    levels = torch.empty(B * R, dtype=torch.int32, device=boxes.device)
    rois = torch.empty(B * R, 5, dtype=torch.float32, device=boxes.device)
    rc = _lib.lib().lvc_assign_levels_rois(ptr(boxes), B, R, min_level, max_level,
                                           canonical_box_size, canonical_level, ptr(levels), ptr(rois),
                                           _stream(boxes))
    check(rc, "lvc_assign_levels_rois")
    return levels, rois


def fast_rcnn_inference(cls_logits, deltas, proposals, prop_count, image_sizes, num_classes, box_weights,
                        score_thresh, nms_thresh, topk, post=None, status=None, max_candidates=16384):
    """predict_boxes/predict_probs + fast_rcnn_inference (+ detector_postprocess when `post` is given).

    cls_logits [B*R, >=K+1], deltas [B*R, 4K or 4] (row-contiguous, any row stride), proposals [B,R,4],
    prop_count [B] int32 or None, image_sizes [B,2] int32, post [B,4] fp32 = (scale_x, scale_y, out_h, out_w).
    Returns (boxes [B,topk,4], scores [B,topk], classes [B,topk] int32, rows [B,topk] int32, count [B] int32).
    max_candidates: capacity of the per-image (roi, class) candidate list; None = R*K (cannot overflow).  The default
    keeps the NMS in its one-block form; an overflow sets status bit 1 (value 2) -> `CandidateOverflow` where the status
    is read, and the model entry points re-run with the full capacity.
    """
    _req_cuda(cls_logits, deltas, proposals, prop_count, image_sizes, post)
    B, R, _ = proposals.shape
    K = num_classes
    dev = proposals.device
    assert cls_logits.stride(1) == 1 and deltas.stride(1) == 1
    cls_agnostic = 1 if deltas.shape[1] == 4 else 0
    if status is None:
        status = new_status(dev)
    lib = _lib.lib()
    max_candidates = max(1, R * K) if max_candidates is None else min(max_candidates, max(1, R * K))
    nbytes = _lib.size_query("lvc_fast_rcnn_inference_workspace_bytes", B, max_candidates)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ob = torch.empty(B, topk, 4, device=dev, dtype=torch.float32)
    osc = torch.empty(B, topk, device=dev, dtype=torch.float32)
    ocl = torch.empty(B, topk, device=dev, dtype=torch.int32)
    orow = torch.empty(B, topk, device=dev, dtype=torch.int32)
    cnt = torch.empty(B, device=dev, dtype=torch.int32)
    wx, wy, ww, wh = box_weights
    rc = lib.lvc_fast_rcnn_inference(
        ptr(cls_logits), cls_logits.stride(0), ptr(deltas), deltas.stride(0), K,
        cls_agnostic, ptr(proposals.contiguous()), ptr(prop_count), B, R, ptr(image_sizes),
        wx, wy, ww, wh, SCALE_CLAMP, score_thresh,
        nms_thresh, topk, max_candidates, ptr(post), ptr(ob), ptr(osc), ptr(ocl), ptr(orow),
        ptr(cnt), ptr(status), ptr(ws), nbytes, _stream(proposals))
    check(rc, "lvc_fast_rcnn_inference")
    return ob, osc, ocl, orow, cnt


RETINANET_MAX_SURVIVORS = 1 << 16     # default capacity of the per-(image, level) list of entries above the score threshold
RETINANET_OVERFLOW = RETINA_OVERFLOW  # the status bit lvc_retinanet_select raises when such a list overflows


def retinanet_select(logits, deltas, cell_anchors, strides, anchor_offset, num_classes, topk, score_thresh,
                     box_weights=(1.0, 1.0, 1.0, 1.0), max_survivors=RETINANET_MAX_SURVIVORS, status=None):
    """The per-level candidate selection of RetinaNet's inference (reference retinanet.py:327-353) for all images and levels in one
    call (csrc/retinanet.hip): one pass over the logits, no host read.

    logits[l]: [B,H,W,>=A*K] view whose channel a*K + k holds the logit of class k of anchor a; deltas[l]: [B,H,W,>=4A] view whose
    channel a*4 + c holds delta c of anchor a.  Both may be channel slices of wider NHWC tensors (padded rows).
    cell_anchors[l]: [A,4] device tensors.  max_survivors: capacity of the per-(image, level) list of entries above the threshold;
    None = H*W*A*K (cannot overflow).  An overflow sets `RETINANET_OVERFLOW` in the status word and leaves this call's outputs
    unspecified: the caller that reads the status repeats the call with None (`retinanet_select_checked`, or the model's
    `run_with_fallbacks`).
    Returns (boxes [B,L*topk,4], scores [B,L*topk], classes [B,L*topk] int32, index [B,L*topk] int32 -- the flat index
    (p*A + a)*K + k inside the level --, count [B] int32, status [1] int32); rows past count are zero."""
    L = len(logits)
    if not (L == len(deltas) == len(cell_anchors) == len(strides) and 1 <= L <= 8):
        raise ValueError("retinanet_select: 1..8 levels with logits, deltas, cell anchors and a stride each")
    _req_cuda(*logits, *deltas, *cell_anchors, status)
    B, A, K = logits[0].shape[0], cell_anchors[0].shape[0], int(num_classes)
    dev = logits[0].device
    if not (0 < topk <= 2048):
        raise ValueError("retinanet_select: topk must be in 1..2048 (got {})".format(topk))
    if any(c.shape != (A, 4) for c in cell_anchors):
        raise NotImplementedError("retinanet_select: a different number of anchors per level is not built")
    Hs = [t.shape[1] for t in logits]
    Ws = [t.shape[2] for t in logits]
    for t, d, h, w in zip(logits, deltas, Hs, Ws):
        for u, need in ((t, A * K), (d, 4 * A)):
            if not (u.dtype == torch.float32 and u.dim() == 4 and u.shape[:3] == (B, h, w) and u.shape[3] >= need and u.stride(3) == 1
                    and u.stride(1) == w * u.stride(2) and u.stride(0) == h * w * u.stride(2)):
                raise ValueError("retinanet_select: need fp32 NHWC channel slices [B,H,W,>=A*K] / [B,H,W,>=4A] of dense pixel rows")
        if h * w * A * K >= (1 << 31) or h * w * t.stride(2) >= (1 << 31):
            raise ValueError("retinanet_select: a level with 2^31 entries per image")
    full = max(h * w * A * K for h, w in zip(Hs, Ws))
    max_survivors = full if max_survivors is None else max(1, min(int(max_survivors), full))
    if status is None:
        status = new_status(dev)
    VP, IP = c_void_p * L, c_int * L
    lp = VP(*[t.data_ptr() for t in logits])
    dp = VP(*[t.data_ptr() for t in deltas])
    anchors = [t.contiguous().float() for t in cell_anchors]
    ap = VP(*[t.data_ptr() for t in anchors])
    ldl = IP(*[t.stride(2) for t in logits])
    ldd = IP(*[t.stride(2) for t in deltas])
    hs, ws_, st = IP(*Hs), IP(*Ws), IP(*[int(s) for s in strides])
    lib = _lib.lib()
    try:
        nbytes = _lib.size_query("lvc_retinanet_select_workspace_bytes", B, L, A, K, hs, ws_, topk, max_survivors)
    except _lib.LvcNativeError:
        raise ValueError("retinanet_select: shapes outside the kernel's range") from None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rows = L * topk
    boxes = torch.empty(B, rows, 4, device=dev, dtype=torch.float32)
    scores = torch.empty(B, rows, device=dev, dtype=torch.float32)
    classes = torch.empty(B, rows, device=dev, dtype=torch.int32)
    index = torch.empty(B, rows, device=dev, dtype=torch.int32)
    count = torch.empty(B, device=dev, dtype=torch.int32)
    wx, wy, ww, wh = [float(v) for v in box_weights]
    rc = lib.lvc_retinanet_select(lp, ldl, dp, ldd, ap, hs, ws_, st, anchor_offset, L, A, K, B,
                                  topk, score_thresh, wx, wy, ww, wh,
                                  SCALE_CLAMP, max_survivors, ptr(boxes), ptr(scores), ptr(classes), ptr(index),
                                  ptr(count), ptr(status), ptr(ws), nbytes, _stream(boxes))
    check(rc, "lvc_retinanet_select")
    return boxes, scores, classes, index, count, status


def retinanet_select_checked(*args, max_survivors=RETINANET_MAX_SURVIVORS, **kw):
    """`retinanet_select` for callers outside a model pass: reads the status word (ONE device->host read) and, where a list
    overflowed, repeats the call with the full capacity.  Same return values; the status word comes back clear of the bit."""
    out = retinanet_select(*args, max_survivors=max_survivors, **kw)
    if max_survivors is not None and int(out[5].item()) & RETINANET_OVERFLOW:
        _log_once("retinanet_overflow", "more than %d entries above the score threshold on one (image, level): the selection is "
                  "repeated with the list sized for H*W*A*K", max_survivors)
        kw.pop("status", None)
        out = retinanet_select(*args, max_survivors=None, **kw)
    return out


class RetinaNetLossArgs:
    """The arguments `retinanet_loss` and `retinanet_loss_grad` share, checked once: the head's per-level NHWC outputs
    logits[l] [B,H,W,>=A*K] / deltas[l] [B,H,W,>=4A] (channel slices of wider rows allowed; the padding is never read), anchors [R,4]
    in `Boxes.cat(anchors)` order, matches int32 [B,R] / labels int8 [B,R] from `match_boxes_batched`, gt [G,4], gt_classes int64 [G],
    gt_off int32 [B+1] from `cat_ground_truth`."""

    def __init__(self, logits, deltas, num_anchors, num_classes, anchors, matches, labels, gt, gt_classes, gt_off,
                 alpha=0.25, gamma=2.0, beta=0.1, box_weights=(1.0, 1.0, 1.0, 1.0)):
        L = len(logits)
        if not (L == len(deltas) and 1 <= L <= 8):
            raise ValueError("retinanet_loss: 1..8 levels with logits and deltas each")
        if 0.0 < float(gamma) < 1.0 or float(gamma) < 0.0:
            raise NotImplementedError("MODEL.RETINANET.FOCAL_LOSS_GAMMA = {}: an exponent in (0, 1) has an unbounded derivative at "
                                      "saturation (and a negative one is no focal loss); 0 or >= 1 are built".format(gamma))
        _req_cuda(*logits, *deltas, anchors, matches, labels, gt_off, gt_classes)
        A, Kc = int(num_anchors), int(num_classes)
        B = logits[0].shape[0]
        self.Hs = [t.shape[1] for t in logits]
        self.Ws = [t.shape[2] for t in logits]
        for t, d, h, w in zip(logits, deltas, self.Hs, self.Ws):
            for u, need in ((t, A * Kc), (d, 4 * A)):
                if not (u.dtype == torch.float32 and u.dim() == 4 and u.shape[:3] == (B, h, w) and u.shape[3] >= need and u.stride(3) == 1
                        and u.stride(1) == w * u.stride(2) and u.stride(0) == h * w * u.stride(2)):
                    raise ValueError("retinanet_loss: need fp32 NHWC channel slices [B,H,W,>=A*K] / [B,H,W,>=4A] of dense pixel rows")
        R = sum(h * w for h, w in zip(self.Hs, self.Ws)) * A
        G = gt.shape[0]
        if not (anchors.shape == (R, 4) and anchors.dtype == torch.float32 and anchors.is_contiguous()):
            raise ValueError("retinanet_loss: anchors must be a contiguous fp32 [R,4], R = sum_l H_l W_l A = {}".format(R))
        if not (matches.shape == (B, R) and matches.dtype == torch.int32 and matches.is_contiguous()
                and labels.shape == (B, R) and labels.dtype == torch.int8 and labels.is_contiguous()):
            raise ValueError("retinanet_loss: matches int32 [B,R] and labels int8 [B,R] (match_boxes_batched)")
        if not (gt_off.dtype == torch.int32 and gt_off.numel() == B + 1 and gt.dtype == torch.float32 and gt.shape == (G, 4)
                and gt.is_contiguous() and gt_classes.dtype == torch.int64 and gt_classes.numel() == G and gt_classes.is_contiguous()):
            raise ValueError("retinanet_loss: gt fp32 [G,4], gt_classes int64 [G], gt_off int32 [B+1]")
        self.logits, self.deltas = list(logits), list(deltas)
        self.L, self.A, self.K, self.B, self.R = L, A, Kc, B, R
        self.tensors = (anchors, matches, labels, gt, gt_classes, gt_off)
        self.scalars = (float(alpha), float(gamma), float(beta)) + tuple(float(v) for v in box_weights)
        self.dev = logits[0].device

    def _levels(self, ts):
        VP, IP = c_void_p * self.L, c_int * self.L
        return VP(*[t.data_ptr() for t in ts]), IP(*[t.stride(2) for t in ts])

    def common(self):
        lp, ldl = self._levels(self.logits)
        dp, ldd = self._levels(self.deltas)
        IP = c_int * self.L
        return ([lp, ldl, dp, ldd, IP(*self.Hs), IP(*self.Ws), self.L, self.A, self.K, self.B]
                + [ptr(t) for t in self.tensors] + list(self.scalars))


def retinanet_loss(args, normalizer_in, normalizer_out, momentum=0.9, one_minus_momentum=1 - 0.9, return_sums=False):
    """RetinaNet.losses (reference retinanet.py:184-236) in two launches (csrc/retinanet_loss.hip): one streaming pass over the logits
    and deltas, one finish.  args: `RetinaNetLossArgs`; normalizer_in / normalizer_out: DIFFERENT device float64 [1] tensors -- the
    EMA `momentum * in + one_minus_momentum * max(num_pos, 1)` is written to `normalizer_out` in the reference's Python float
    arithmetic (`one_minus_momentum` is formed by the caller as `1 - momentum`: 0.09999999999999998 for 0.9, not 0.1) and divides both
    sums.  -> (losses fp32 [2] = (loss_cls, loss_box_reg), num_pos int32 [1]); no host read.  return_sums: a third value, the two sums
    before the division as float64 [2]."""
    _req_cuda(normalizer_in, normalizer_out)
    if not (normalizer_in.dtype == normalizer_out.dtype == torch.float64 and normalizer_in.numel() == normalizer_out.numel() == 1
            and normalizer_in.data_ptr() != normalizer_out.data_ptr()):
        raise ValueError("retinanet_loss: normalizer_in / normalizer_out must be two different float64 [1] device tensors")
    lib = _lib.lib()
    IP = c_int * args.L
    try:
        nbytes = _lib.size_query("lvc_retinanet_loss_workspace_bytes", args.B, args.L, args.A, args.K, IP(*args.Hs), IP(*args.Ws))
    except _lib.LvcNativeError:
        raise ValueError("retinanet_loss: shapes outside the kernel's range") from None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=args.dev)
    out = torch.empty(2, dtype=torch.float32, device=args.dev)
    num_pos = torch.empty(1, dtype=torch.int32, device=args.dev)
    sums = torch.empty(2, dtype=torch.float64, device=args.dev) if return_sums else None
    rc = lib.lvc_retinanet_loss(*args.common(), momentum, one_minus_momentum, ptr(normalizer_in), ptr(normalizer_out),
                                ptr(out), ptr(sums), ptr(num_pos), ptr(ws), nbytes, _stream(out))
    check(rc, "lvc_retinanet_loss")
    return (out, num_pos, sums) if return_sums else (out, num_pos)


def retinanet_loss_grad(args, normalizer, g_cls, g_box, dlogits=None, ddeltas=None):
    """The gradient of `retinanet_loss` in one launch: dlogits[l] / ddeltas[l] (dense [B,H,W,A*K] / [B,H,W,4A] unless given: any
    [B,H,W,>=A*K] / [B,H,W,>=4A] tensors with contiguous rows, whose padding channels are written as zero) = the derivative of the two
    losses times the upstream scalars g_cls / g_box (fp32 [1] device) over `normalizer` (float64 [1] device, `retinanet_loss`'s
    normalizer_out).  Zero on ignored anchors; ddeltas zero on every anchor that is not positive.  No host read."""
    _req_cuda(normalizer, g_cls, g_box)
    assert normalizer.dtype == torch.float64 and g_cls.dtype == g_box.dtype == torch.float32
    if dlogits is None:
        dlogits = [torch.empty(t.shape[:3] + (args.A * args.K,), dtype=torch.float32, device=args.dev) for t in args.logits]
    if ddeltas is None:
        ddeltas = [torch.empty(t.shape[:3] + (4 * args.A,), dtype=torch.float32, device=args.dev) for t in args.deltas]
    for outs, ins, need in ((dlogits, args.logits, args.A * args.K), (ddeltas, args.deltas, 4 * args.A)):
        if len(outs) != args.L or any(not (o.is_contiguous() and o.dtype == torch.float32 and o.shape[:3] == t.shape[:3] and o.shape[3] >= need)
                                      for o, t in zip(outs, ins)):
            raise ValueError("retinanet_loss_grad: gradient tensors must be contiguous fp32 [B,H,W,>=A*K] / [B,H,W,>=4A]")
    glp, gldl = args._levels(dlogits)
    gdp, gldd = args._levels(ddeltas)
    rc = _lib.lib().lvc_retinanet_loss_grad(*args.common(), ptr(normalizer), ptr(g_cls), ptr(g_box), glp, gldl, gdp, gldd, _stream(g_cls))
    check(rc, "lvc_retinanet_loss_grad")
    return dlogits, ddeltas


def gather_detections(boxes, scores, classes, rows, keep, num_keep, topk, post=None):
    """The rows an NMS kept (`batched_nms_batch`), in its order, at most topk per image, through detector_postprocess when
    post [B,4] fp32 = (scale_x, scale_y, out_h, out_w) is given.  boxes [B,Nmax,4], scores / classes / rows [B,Nmax].
    Returns (boxes [B,topk,4], scores, classes int32, rows int32 [B,topk], count [B] int32); rows past count are zero; no sync."""
    _req_cuda(boxes, scores, classes, rows, keep, num_keep, post)
    B, Nmax = scores.shape
    dev = boxes.device
    for t in (classes, rows, keep):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.shape == (B, Nmax)
    assert boxes.is_contiguous() and scores.is_contiguous() and boxes.dtype == scores.dtype == torch.float32 and boxes.shape == (B, Nmax, 4)
    assert num_keep.dtype == torch.int32 and num_keep.numel() == B
    if post is not None:
        assert post.dtype == torch.float32 and post.is_contiguous() and post.shape == (B, 4)
    ob = torch.empty(B, topk, 4, device=dev, dtype=torch.float32)
    osc = torch.empty(B, topk, device=dev, dtype=torch.float32)
    ocl = torch.empty(B, topk, device=dev, dtype=torch.int32)
    orow = torch.empty(B, topk, device=dev, dtype=torch.int32)
    cnt = torch.empty(B, device=dev, dtype=torch.int32)
    check(_lib.lib().lvc_gather_detections(ptr(boxes), ptr(scores), ptr(classes), ptr(rows), ptr(keep), ptr(num_keep), B, Nmax,
                                           topk, ptr(post), ptr(ob), ptr(osc), ptr(ocl), ptr(orow), ptr(cnt), _stream(boxes)),
          "lvc_gather_detections")
    return ob, osc, ocl, orow, cnt


# --------------------------------------------------------------------------- trunk elementwise
def preprocess_into(image, out_slot, mean, std):
    """image: CHW (3,h,w) float32 or uint8 device tensor; out_slot: [Hp,Wp,4] view of the batch tensor.
    out = (image - mean) / std, zero padded, 4th channel zero (reference rcnn.py:324-333, image_list.py:95-119)."""
    _req_cuda(image, out_slot)
    assert image.dim() == 3 and image.shape[0] == 3
    if image.dtype == torch.uint8:
        dt = 1
    else:
        image = image.float()
        dt = 0
    image = image.contiguous()
    Hp, Wp, four = out_slot.shape
    assert four == 4 and out_slot.is_contiguous()
    m = _float3(mean)
    s = _float3(std)
    rc = _lib.lib().lvc_preprocess_nhwc4(ptr(image), dt, image.shape[1], image.shape[2], m, s,
                                         ptr(out_slot), Hp, Wp, _stream(image))
    check(rc, "lvc_preprocess_nhwc4")


def preprocess_batch_into(images, out, mean, std):
    """images: list of CHW (3,h,w) device tensors (all float32 or all uint8); out: [B,Hp,Wp,4] batch tensor.  One launch per
    16 images (lvc_preprocess_batch_nhwc4); the same values as `preprocess_into` image by image."""
    _req_cuda(out, *images)
    B = len(images)
    assert out.dim() == 4 and out.shape[0] == B and out.shape[3] == 4 and out.is_contiguous() and out.dtype == torch.float32
    u8 = images[0].dtype == torch.uint8
    imgs = []
    for im in images:
        assert im.dim() == 3 and im.shape[0] == 3
        if u8:
            assert im.dtype == torch.uint8
        else:
            im = im.float()
        imgs.append(im.contiguous())
    P = (c_void_p * B)(*[im.data_ptr() for im in imgs])
    hs = (c_int * B)(*[int(im.shape[1]) for im in imgs])
    ws = (c_int * B)(*[int(im.shape[2]) for im in imgs])
    m = _float3(mean)
    s_ = _float3(std)
    rc = _lib.lib().lvc_preprocess_batch_nhwc4(P, 1 if u8 else 0, hs, ws, B, m, s_, ptr(out), out.shape[1],
                                               out.shape[2], _stream(out))
    check(rc, "lvc_preprocess_batch_nhwc4")
    return imgs   # keeps converted copies alive until the caller drops them (the launch is asynchronous)


def resize_bilinear_u8(img, new_h, new_w, coeffs_fn, out_slot=None, mean=None, std=None):
    """Pillow-exact bilinear resize of a uint8 [H,W,3] image on the device (csrc/resize.hip).  coeffs_fn(in, out,
    device) -> (bounds, coefficients, ksize) (lvc_amd.data.transforms.resample_coeffs).  Returns the uint8
    [new_h,new_w,3] result; with out_slot [Hp,Wp,4] fp32 also writes the normalised, zero-padded NHWC4 pixels."""
    if not img.is_cuda:
        raise RuntimeError("resize_bilinear_u8 needs a device tensor (move the uint8 image first: 1 byte per sample)")
    img = img.contiguous()
    H, W, _ = img.shape
    dev = img.device
    xb = xk = yb = yk = tmp = None
    kxs = kys = 0
    if new_w != W:
        xb, xk, kxs = coeffs_fn(W, new_w, dev)
        tmp = torch.empty(H * new_w * 3, dtype=torch.uint8, device=dev)
    if new_h != H:
        yb, yk, kys = coeffs_fn(H, new_h, dev)
    out = torch.empty(new_h, new_w, 3, dtype=torch.uint8, device=dev)
    Hp = Wp = 0
    m = s = None
    if out_slot is not None:
        Hp, Wp, four = out_slot.shape
        assert four == 4 and out_slot.is_contiguous() and out_slot.dtype == torch.float32
        m = _float3(mean)
        s = _float3(std)
    rc = _lib.lib().lvc_resize_bilinear_u8(ptr(img), H, W, new_h, new_w, ptr(xb), ptr(xk),
                                           kxs, ptr(yb), ptr(yk), kys, ptr(tmp), ptr(out), ptr(out_slot),
                                           Hp, Wp, m, s, _stream(img))
    check(rc, "lvc_resize_bilinear_u8")
    return out


def tta_resize_u8(img, H, W, strides, hjobs, vjobs, mean, std):
    """All ResizeShortestEdge sizes (and their mirrors) of one uint8 device image in two launches (csrc/tta.hip
    lvc_tta_resize_u8).  img: uint8 device tensor of an H x W image whose element (y, x, c) sits at element strides
    strides = (sy, sx, sc) from its data pointer (CHW and HWC alike);
    hjobs: list of (bounds, coefficients, ksize, new_w, tmp) device tensors, one per distinct output width != W; vjobs: list of
    (hjob index or -1, bounds or None, coefficients or None, ksize, new_h, new_w, u8 or None, mirrored u8 or None, slot or None,
    mirrored slot or None), slots being [Hp,Wp,4] fp32 contiguous views of batch buffers.  Nothing is returned: the outputs
    are written in place."""
    _req_cuda(img)
    assert img.dtype == torch.uint8
    hrows = []
    for xb, xk, ks, nw, tmp in hjobs:
        _req_cuda(xb, xk, tmp)
        assert tmp.numel() >= H * nw * 3
        hrows += [xb.data_ptr(), xk.data_ptr(), ks, nw, tmp.data_ptr()]
    vrows = []
    for hj, yb, yk, ks, nh, nw, u8, u8m, f, fm in vjobs:
        for o in (u8, u8m):
            assert o is None or (o.is_cuda and o.is_contiguous() and tuple(o.shape) == (nh, nw, 3) and o.dtype == torch.uint8)
        for o in (f, fm):
            assert o is None or (o.is_cuda and o.is_contiguous() and o.dim() == 3 and o.shape[2] == 4 and o.dtype == torch.float32)
        vrows += [hj, yb.data_ptr() if yb is not None else 0, yk.data_ptr() if yk is not None else 0, ks, nh, nw,
                  u8.data_ptr() if u8 is not None else 0, u8m.data_ptr() if u8m is not None else 0,
                  f.data_ptr() if f is not None else 0, f.shape[0] if f is not None else 0, f.shape[1] if f is not None else 0,
                  fm.data_ptr() if fm is not None else 0, fm.shape[0] if fm is not None else 0, fm.shape[1] if fm is not None else 0]
    hj = (c_longlong * max(1, len(hrows)))(*hrows)
    vj = (c_longlong * len(vrows))(*vrows)
    m = _float3(mean)
    s = _float3(std)
    sy, sx, sc = strides
    rc = _lib.lib().lvc_tta_resize_u8(ptr(img), H, W, sy, sx, sc, hj,
                                      len(hjobs), vj, len(vjobs), m, s, _stream(img))
    check(rc, "lvc_tta_resize_u8")


# --------------------------------------------------------------------------- training input: job blobs
# Every entry below takes ONE pinned blob -- an int64 job table with the int32 resample tables behind it (layouts: include/lvc_amd.h)
# -- that is uploaded once per call.
TRAIN_INPUT_LAUNCHES = []  # kernel launches of the last (up to 64) lvc_train_input_u8 calls, as the library counted them
TRAIN_INPUT_FIELDS = 24   # int64 words per job of lvc_train_input_u8 (include/lvc_amd.h)
TRAIN_INPUT_TILES_LAUNCHES = []   # ... of the last (up to 64) lvc_train_input_tiles_u8 calls
TRAIN_INPUT_TILES_HEAD, TRAIN_INPUT_TILES_TILE, TRAIN_INPUT_TILES_MAX = 20, 12, 9   # job layout of lvc_train_input_tiles_u8
TRAIN_INPUT_TILES_FIELDS = TRAIN_INPUT_TILES_HEAD + TRAIN_INPUT_TILES_MAX * TRAIN_INPUT_TILES_TILE      # (include/lvc_amd.h)
TRAIN_INPUT_LSJ_LAUNCHES = []   # ... of the last (up to 64) lvc_train_input_lsj_u8 calls
TRAIN_INPUT_LSJ_HEAD = 32       # int64 words in front of the tiles of a job of lvc_train_input_lsj_u8 (include/lvc_amd.h)
TRAIN_INPUT_LSJ_FIELDS = TRAIN_INPUT_LSJ_HEAD + TRAIN_INPUT_TILES_MAX * TRAIN_INPUT_TILES_TILE
COLOR_JITTER_LAUNCHES = []   # ... of the last (up to 64) lvc_color_jitter_tiles_u8 calls
COLOR_JITTER_FIELDS = TRAIN_INPUT_TILES_FIELDS      # int64 words per job of lvc_color_jitter_tiles_u8 (include/lvc_amd.h)
COLOR_JITTER_OPS = ("brightness", "contrast", "saturation", "hue")      # step ids 0..3, torchvision's


class TrainInputWorkspace:
    """Buffers of one job-blob call, reused from batch to batch (grown, never shrunk): the pinned host blob (job table +
    coefficient tables), its device copy and a device scratch buffer (`tmp`: the horizontal pass's uint8 intermediate).  `uploaded`
    is recorded after the blob's copy is queued: the host blob must not be rewritten before it has passed (`wait_host`)."""
    MIN_BLOB = 1 << 16

    def __init__(self, device):
        self.device = torch.device(device)
        self.host = self.dev = self.scratch = self.uploaded = None

    tmp = property(lambda self: self.scratch)

    def wait_host(self):
        if self.uploaded is not None:
            self.uploaded.synchronize()      # this event only: the copy out of the pinned blob, queued two batches ago

    def reserve(self, blob_bytes, scratch_bytes):
        if self.host is None or self.host.numel() < blob_bytes:
            n = max(blob_bytes * 3 // 2, self.MIN_BLOB)
            self.host = torch.empty(n, dtype=torch.uint8).pin_memory()
            self.dev = torch.empty(n, dtype=torch.uint8, device=self.device)
        if self.scratch is None or self.scratch.numel() < scratch_bytes:
            self.scratch = torch.empty(max(scratch_bytes * 3 // 2, 1 << 16), dtype=torch.uint8, device=self.device)

    def upload(self, tab, tables, scratch_bytes, device):
        """The job table and the int32 tables behind it into the pinned blob and, on `device`'s current stream, into its device
        copy; -> the bytes of the blob."""
        import numpy as np

        nbytes = tab.nbytes + sum(t.nbytes for t in tables)
        self.wait_host()
        self.reserve(nbytes, scratch_bytes)
        hb, at = self.host.numpy(), tab.nbytes
        hb[:at] = tab.reshape(-1).view(np.uint8)
        for t in tables:
            hb[at:at + t.nbytes] = np.ascontiguousarray(t, np.int32).reshape(-1).view(np.uint8)
            at += t.nbytes
        self.dev[:nbytes].copy_(self.host[:nbytes], non_blocking=True)
        self.uploaded = torch.cuda.Event()
        self.uploaded.record(torch.cuda.current_stream(device))
        return nbytes


class ColorJitterWorkspace(TrainInputWorkspace):
    """The workspace of one lvc_color_jitter_tiles_u8 call: its blob is the job table alone, and `scratch` receives the jittered
    crops (the results are views of it: they live until the next call on this workspace)."""
    MIN_BLOB = 1 << 14


def _log_launches(log, n):
    log.append(n)
    del log[:-64]


def _image_words(img):
    """Words 0-5 of a tile or of a plain job: (pointer, H, W, sy, sx, sc) of a uint8 [H,W,3] tensor of any strides, or that tuple."""
    return img if isinstance(img, tuple) else (img.data_ptr(), img.shape[0], img.shape[1], img.stride(0), img.stride(1), img.stride(2))


def _req_image(img, device):
    _req_cuda(img)
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3 and img.device == device


def _write_tiles(row, head, tiles, device=None):
    """The 12 words of every tile (image, canvas rectangle, tile pixel at its first corner) from word `head` of a job on.  device:
    where the images must lie (None: not checked -- train_input_lsj_blob, whose images may be the tuples of _image_words)."""
    assert 1 <= len(tiles) <= TRAIN_INPUT_TILES_MAX, "an item has 1 to 9 tiles"
    for t, (img, rect, origin) in enumerate(tiles):
        if device is not None:
            _req_image(img, device)
        at = head + t * TRAIN_INPUT_TILES_TILE
        row[at:at + TRAIN_INPUT_TILES_TILE] = (*_image_words(img), *rect, *origin)


def _axis_tables(row, at, x_sizes, y_sizes, coeffs_fn, tables, off):
    """The two resample axes of a job, (size in, size out) each: words at.. = (bounds offset, coefficient offset, ksize) of the
    columns, then of the rows, the offset -1 where the size stays.  Appends the tables; -> the blob offset behind them."""
    for (size_in, size_out), w in ((x_sizes, at), (y_sizes, at + 3)):
        row[w] = -1
        if size_in != size_out:
            b, k, ks = coeffs_fn(size_in, size_out)
            row[w], row[w + 1], row[w + 2] = off, off + b.nbytes, ks
            tables += [b, k]
            off += b.nbytes + k.nbytes
    return off


def _train_input_call(entry, log, ws, tab, tables, tmp_bytes, out, mean, std):
    """Upload the blob and call one of the three lvc_train_input*_u8 entries (one signature) on out's current stream."""
    nbytes = ws.upload(tab, tables, tmp_bytes, out.device)
    n = c_int(0)
    rc = getattr(_lib.lib(), entry)(ptr(ws.host), ptr(ws.dev), nbytes, len(tab), ptr(ws.scratch), ws.scratch.numel(),
                                    ptr(out), out.shape[0], out.shape[1], out.shape[2], _float3(mean), _float3(std),
                                    ctypes.byref(n), _stream(out))
    check(rc, entry)
    _log_launches(log, n.value)


def _req_batch(out, B):
    _req_cuda(out)
    assert B > 0 and out.dim() == 4 and out.shape[3] == 4 and out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] >= B


def train_input_u8(images, jobs, out, mean, std, coeffs_fn, want_u8=False, workspace=None):
    """RandomCrop -> ResizeShortestEdge -> RandomFlip -> normalise + pad of a whole batch in two launches (csrc/train_input.hip
    lvc_train_input_u8), on the current stream.  images: uint8 device tensors [H,W,3] (any strides: an HWC view of a CHW tensor
    is read in place); jobs: per image (x0, y0, crop_w, crop_h, new_h, new_w, flip); out [n_slots,Hp,Wp,4] fp32 contiguous: image i
    fills slot i completely.  coeffs_fn(in, out) -> (bounds, coefficients, ksize) numpy tables (data.transforms.resample_coeffs).
    Returns the uint8 [new_h,new_w,3] results when want_u8 (else None).  One host->device copy carries every table."""
    import numpy as np

    B = len(images)
    assert B == len(jobs)
    _req_batch(out, B)
    ws = workspace if workspace is not None else TrainInputWorkspace(out.device)
    tab = np.zeros((B, TRAIN_INPUT_FIELDS), np.int64)
    tables, off, tmp_off = [], tab.nbytes, 0
    u8 = []
    for i, (img, (x0, y0, cw, ch, nh, nw, flip)) in enumerate(zip(images, jobs)):
        _req_image(img, out.device)
        row = tab[i]
        row[0:6] = _image_words(img)
        row[6:12] = (x0, y0, cw, ch, nh, nw)
        off = _axis_tables(row, 12, (cw, nw), (ch, nh), coeffs_fn, tables, off)
        row[18], row[19] = int(bool(flip)), i
        if want_u8:
            u8.append(torch.empty(nh, nw, 3, dtype=torch.uint8, device=out.device))
            row[20] = u8[-1].data_ptr()
        if nw != cw:
            row[21] = tmp_off
            tmp_off += (ch * nw * 3 + 255) & ~255
    _train_input_call("lvc_train_input_u8", TRAIN_INPUT_LAUNCHES, ws, tab, tables, tmp_off, out, mean, std)
    return u8 if want_u8 else None


def train_input_tiles_u8(items, out, mean, std, coeffs_fn, want_u8=False, workspace=None, table_hook=None):
    """train_input_u8 for images that are mosaics of 1 to 9 tiles, read in place (csrc/train_input.hip lvc_train_input_tiles_u8: two
    launches, no canvas in memory), on the current stream.  items: per output slot (tiles, (X0, Y0, crop_w, crop_h), new_h, new_w,
    flip) with the crop window in canvas coordinates and tiles a list of (uint8 device tensor [H,W,3] of any strides, its canvas
    rectangle (x1a, y1a, x2a, y2a), the tile pixel (x1b, y1b) at the rectangle's first corner); later tiles are painted over earlier
    ones, what no tile covers is 114.  A plain image is one tile.  out, coeffs_fn, want_u8, workspace: as train_input_u8.
    table_hook(tab): called with the int64 job table [B,128] before it is uploaded (tests of the library's refusals)."""
    import numpy as np

    B = len(items)
    _req_batch(out, B)
    ws = workspace if workspace is not None else TrainInputWorkspace(out.device)
    tab = np.zeros((B, TRAIN_INPUT_TILES_FIELDS), np.int64)
    tables, off, tmp_off = [], tab.nbytes, 0
    u8 = []
    for i, (tiles, (X0, Y0, cw, ch), nh, nw, flip) in enumerate(items):
        row = tab[i]
        row[0:6] = (X0, Y0, cw, ch, nh, nw)
        off = _axis_tables(row, 6, (cw, nw), (ch, nh), coeffs_fn, tables, off)
        row[12], row[13] = int(bool(flip)), i
        if want_u8:
            u8.append(torch.empty(nh, nw, 3, dtype=torch.uint8, device=out.device))
            row[14] = u8[-1].data_ptr()
        row[15] = tmp_off
        tmp_off += (ch * nw * 3 + 255) & ~255
        row[16] = len(tiles)
        _write_tiles(row, TRAIN_INPUT_TILES_HEAD, tiles, out.device)
    if table_hook is not None:
        table_hook(tab)
    _train_input_call("lvc_train_input_tiles_u8", TRAIN_INPUT_TILES_LAUNCHES, ws, tab, tables, tmp_off, out, mean, std)
    return u8 if want_u8 else None


def lsj_band(size_in, size_out, o0, on, coeffs_fn):
    """The source rows [b0, b0 + bn) that the taps of output rows [o0, o0 + on) of the full size_in -> size_out resize touch (the
    rows themselves when the size stays: Pillow skips the pass)."""
    if size_in == size_out:
        return int(o0), int(on)
    b = coeffs_fn(size_in, size_out)[0][o0:o0 + on]
    lo = int(b[:, 0].min())
    return lo, int((b[:, 0] + b[:, 1]).max()) - lo


def train_input_lsj_blob(items, coeffs_fn, u8_ptrs=None):
    """The host half of train_input_lsj_u8, numpy only: (job table int64 [B,140], the int32 tables behind it, blob bytes, bytes of
    the intermediate).  items: per output slot (tiles, (X0, Y0, crop_w, crop_h), (sh, sw), (ox, oy, ow, oh), (th, tw), fill, flip);
    a tile is (image, rectangle, origin) as train_input_tiles_u8, or (pointer, H, W, sy, sx, sc) in place of the image."""
    import numpy as np

    tab = np.zeros((len(items), TRAIN_INPUT_LSJ_FIELDS), np.int64)
    tables, off, tmp_off = [], tab.nbytes, 0
    for i, (tiles, (X0, Y0, cw, ch), (sh, sw), (ox, oy, ow, oh), (th, tw), fill, flip) in enumerate(items):
        row = tab[i]
        row[0:6] = (X0, Y0, cw, ch, sh, sw)
        off = _axis_tables(row, 6, (cw, sw), (ch, sh), coeffs_fn, tables, off)      # Pillow's tables of the FULL resize; the window selects rows of them
        row[12], row[13] = int(bool(flip)), i
        if u8_ptrs is not None:
            row[14] = u8_ptrs[i]
        row[16] = len(tiles)
        row[17:24] = (ox, oy, ow, oh, th, tw, fill)
        row[24:26] = lsj_band(ch, sh, oy, oh, coeffs_fn) if 0 <= oy and 0 < oh and oy + oh <= sh else (oy, oh)
        row[15] = tmp_off
        tmp_off += (int(row[25]) * int(ow) * 3 + 255) & ~255
        _write_tiles(row, TRAIN_INPUT_LSJ_HEAD, tiles)
    return tab, tables, off, tmp_off


def train_input_lsj_u8(items, out, mean, std, coeffs_fn, want_u8=False, workspace=None, table_hook=None):
    """INPUT.LSJ of a whole batch in two launches (csrc/train_input.hip lvc_train_input_lsj_u8), on the current stream: the crop
    window of each item is resized whole to (sh, sw) -- Pillow's bilinear, bit for bit -- of which only the window (ox, oy, ow, oh)
    is computed; it lands at the top left of a (th, tw) canvas filled with `fill`, mirrored when `flip`.  items: see
    train_input_lsj_blob (tiles: uint8 device tensors of any strides; a plain image is one tile).  out [n_slots,Hp,Wp,4] fp32: item
    i fills slot i completely ((canvas - mean) / std, zero outside the canvas).  Returns the uint8 [th,tw,3] canvases when want_u8.
    coeffs_fn, workspace, table_hook(tab): as train_input_tiles_u8.  One host->device copy carries every table."""
    _req_batch(out, len(items))
    for it in items:
        for img, _, _ in it[0]:
            _req_image(img, out.device)
    ws = workspace if workspace is not None else TrainInputWorkspace(out.device)
    u8 = [torch.empty(it[4][0], it[4][1], 3, dtype=torch.uint8, device=out.device) for it in items] if want_u8 else []
    tab, tables, _, tmp_off = train_input_lsj_blob(items, coeffs_fn, [t.data_ptr() for t in u8] if want_u8 else None)
    if table_hook is not None:
        table_hook(tab)
    _train_input_call("lvc_train_input_lsj_u8", TRAIN_INPUT_LSJ_LAUNCHES, ws, tab, tables, tmp_off, out, mean, std)
    return u8 if want_u8 else None


def color_jitter_tiles_u8(items, workspace=None, table_hook=None, device=None):
    """INPUT.COLOR_JITTER of a whole batch in two launches (csrc/color_jitter.hip lvc_color_jitter_tiles_u8), on the current stream.
    items: per image (tiles, (X0, Y0, crop_w, crop_h), ops, factors) -- tiles and window as train_input_tiles_u8 (a plain image is one
    tile), ops the step ids in the order they are applied (0 brightness, 1 contrast, 2 saturation, 3 hue; at most 4, at most one
    contrast), factors their fp32 factors.  Returns the jittered windows, uint8 [crop_h, crop_w, 3] views of the workspace's scratch:
    bytes equal to torchvision's ColorJitter steps on a PIL image of the window.  table_hook(tab): called with the int64 job table
    [B,128] before it is uploaded (tests of the library's refusals)."""
    import numpy as np

    B = len(items)
    assert B > 0
    if device is None:
        device = workspace.device if workspace is not None else items[0][0][0][0].device
    ws = workspace if workspace is not None else ColorJitterWorkspace(device)
    tab = np.zeros((B, COLOR_JITTER_FIELDS), np.int64)
    out_off, shapes = 0, []
    for i, (tiles, (X0, Y0, cw, ch), ops, factors) in enumerate(items):
        assert len(ops) == len(factors) <= 4, "an item has at most 4 steps"
        row = tab[i]
        row[0:4] = (X0, Y0, cw, ch)
        row[4], row[5] = out_off, len(ops)
        row[6:6 + len(ops)] = [int(o) for o in ops]
        row[10:10 + len(ops)] = np.asarray(factors, np.float32).view(np.uint32)
        row[14] = len(tiles)
        shapes.append((out_off, int(ch), int(cw)))
        out_off += (int(ch) * int(cw) * 3 + 255) & ~255
        _write_tiles(row, TRAIN_INPUT_TILES_HEAD, tiles, ws.device)
    if table_hook is not None:
        table_hook(tab)
    nbytes = ws.upload(tab, [], out_off, ws.device)
    n = c_int(0)
    rc = _lib.lib().lvc_color_jitter_tiles_u8(ptr(ws.host), ptr(ws.dev), nbytes, B, ptr(ws.scratch),
                                              ws.scratch.numel(), ctypes.byref(n), _stream(ws.scratch))
    check(rc, "lvc_color_jitter_tiles_u8")
    _log_launches(COLOR_JITTER_LAUNCHES, n.value)
    return [ws.scratch[off:off + h * w * 3].view(h, w, 3) for off, h, w in shapes]


TTA_PARAM_STRIDE = 16    # floats per augmentation in lvc_tta_merge's inverse-transform table
TTA_MAX_STEPS = 4


def tta_merge(boxes, scores, classes, counts, params, tab, num_images, nmax, score_thresh, nms_thresh, topk):
    """Union + inverse transforms + finite filter + clip + score filter + per-class NMS + first `topk` for `num_images` images
    (csrc/tta.hip lvc_tta_merge).  boxes [A,T,4], scores [A,T], classes [A,T] int32, counts [A] int32: every augmentation's
    detections; params [A,16] fp32 and tab [B,4] int32 device tables.  Returns (boxes [B,topk,4], scores [B,topk], classes
    [B,topk] int32, count [B] int32) on the device, no sync."""
    _req_cuda(boxes, scores, classes, counts, params, tab)
    A, T = scores.shape
    assert boxes.shape == (A, T, 4) and classes.shape == (A, T) and counts.shape == (A,) and params.shape == (A, TTA_PARAM_STRIDE)
    assert tab.shape == (num_images, 4) and tab.dtype == torch.int32 and params.dtype == torch.float32
    assert classes.dtype == torch.int32 and counts.dtype == torch.int32
    dev = boxes.device
    B = num_images
    ob = torch.empty(B, max(topk, 1), 4, device=dev, dtype=torch.float32)
    osc = torch.empty(B, max(topk, 1), device=dev, dtype=torch.float32)
    ocl = torch.empty(B, max(topk, 1), device=dev, dtype=torch.int32)
    cnt = torch.zeros(B, device=dev, dtype=torch.int32)
    if topk == 0 or B == 0:
        return ob[:, :0], osc[:, :0], ocl[:, :0], cnt
    wsb = _lib.size_query("lvc_tta_merge_workspace_bytes", B, nmax)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    ws = ws[off:off + wsb]
    rc = _lib.lib().lvc_tta_merge(ptr(boxes.contiguous()), ptr(scores.contiguous()), ptr(classes.contiguous()), ptr(counts), T,
                                  ptr(params), ptr(tab), B, nmax, score_thresh, nms_thresh,
                                  topk, ptr(ob), ptr(osc), ptr(ocl), ptr(cnt), ptr(ws), wsb, _stream(boxes))
    check(rc, "lvc_tta_merge")
    return ob, osc, ocl, cnt


def maxpool2d_nhwc(x, k, stride, pad):
    _req_cuda(x)
    assert x.is_contiguous() and x.dtype == torch.float32
    N, H, W, C = x.shape
    Ho = (H + 2 * pad - k) // stride + 1
    Wo = (W + 2 * pad - k) // stride + 1
    y = torch.empty(N, Ho, Wo, C, device=x.device, dtype=torch.float32)
    rc = _lib.lib().lvc_maxpool2d_nhwc(ptr(x), ptr(y), N, H, W, C, k, stride,
                                       pad, _stream(x))
    check(rc, "lvc_maxpool2d_nhwc")
    return y


def rownorm(x, mu=None, eps=1e-5, mode=0, out=None):
    """y = (x - mu) / (|x - mu| + eps)  (mode 0)   or   / max(|x - mu|, eps)  (mode 1), row-wise."""
    _req_cuda(x, mu)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32
    M, D = x.shape
    if out is None:
        out = torch.empty(M, D, device=x.device, dtype=torch.float32)
    rc = _lib.lib().lvc_rownorm(ptr(x), ptr(mu), ptr(out), M, D, x.stride(0), out.stride(0),
                                eps, mode, _stream(x))
    check(rc, "lvc_rownorm")
    return out


def rownorm_backward(x, dy, eps=1e-5, accumulate_into=None):
    """Gradient of `rownorm(x, eps=eps, mode=0)` w.r.t. x; accumulate_into: a [M,D] tensor the result is added to."""
    _req_cuda(x, dy)
    x, dy = x.contiguous(), dy.contiguous()
    M, D = x.shape
    dx = accumulate_into if accumulate_into is not None else torch.empty_like(x)
    assert dx.is_contiguous() and dx.shape == x.shape
    check(_lib.lib().lvc_rownorm_backward(ptr(x), ptr(dy), ptr(dx), M, D, eps,
                                          1 if accumulate_into is not None else 0, _stream(x)), "lvc_rownorm_backward")
    return dx


# --------------------------------------------------------------------------- label-verification kNN
def colmean(x):
    _req_cuda(x)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32
    mu = torch.empty(x.shape[1], device=x.device, dtype=torch.float32)
    rc = _lib.lib().lvc_colmean(ptr(x), ptr(mu), x.shape[0], x.shape[1], x.stride(0), _stream(x))
    check(rc, "lvc_colmean")
    return mu


def knn_topk_vote(sims, num_shots, shot_classes, det_classes, k):
    """sims [Q, >=S] fp32; shot_classes [S] int64; det_classes [Q] int64 or None.
    Returns (top10 class ids [Q,10] int64, keep [Q] int64 or None)."""
    _req_cuda(sims, shot_classes, det_classes)
    Q = sims.shape[0]
    assert sims.stride(1) == 1 and shot_classes.dtype == torch.int64 and shot_classes.is_contiguous()
    top = torch.empty(Q, 10, dtype=torch.int64, device=sims.device)
    keep = torch.empty(Q, dtype=torch.int64, device=sims.device) if det_classes is not None else None
    if det_classes is not None:
        det_classes = det_classes.contiguous()
        assert det_classes.dtype == torch.int64
    rc = _lib.lib().lvc_knn_topk_vote(ptr(sims), sims.stride(0), Q, num_shots, ptr(shot_classes),
                                      ptr(det_classes), k, ptr(top), ptr(keep), _stream(sims))
    check(rc, "lvc_knn_topk_vote")
    return top, keep


def knn_topk_vote_blocks(sims, num_shots, shot_classes, det_classes, k, block=4096):
    """`knn_topk_vote` for any number of shots (LVIS-sized sets): the columns are cut into equal blocks of <= 4096 shots, each
    block's ten best (similarity, shot index) pairs per row are found (lvc_knn_topk_candidates), and one merge launch ranks
    the lists, gathers the classes and votes (lvc_knn_merge_vote).  The exact top ten of a row are among the per-block top
    tens, and both steps use the reference's tie rule (lower shot index first): the same answer as one launch over the row."""
    _req_cuda(sims, shot_classes, det_classes)
    Q = sims.shape[0]
    assert sims.stride(1) == 1 and shot_classes.dtype == torch.int64 and shot_classes.is_contiguous()
    nblk = (num_shots + block - 1) // block
    assert 1 <= nblk <= 64, "at most 64 x 4096 shots"
    per = (num_shots + nblk - 1) // nblk
    cv = torch.empty(nblk, Q, 10, dtype=torch.float32, device=sims.device)
    ci = torch.empty(nblk, Q, 10, dtype=torch.int32, device=sims.device)
    lib = _lib.lib()
    for b in range(nblk):
        s0, s1 = b * per, min(num_shots, (b + 1) * per)
        check(lib.lvc_knn_topk_candidates(ptr(sims[:, s0:]), sims.stride(0), Q, s1 - s0, s0, ptr(cv[b]),
                                          ptr(ci[b]), _stream(sims)), "lvc_knn_topk_candidates")
    top = torch.empty(Q, 10, dtype=torch.int64, device=sims.device)
    keep = torch.empty(Q, dtype=torch.int64, device=sims.device) if det_classes is not None else None
    if det_classes is not None:
        det_classes = det_classes.contiguous()
        assert det_classes.dtype == torch.int64
    check(lib.lvc_knn_merge_vote(ptr(cv), ptr(ci), nblk, Q, ptr(shot_classes), ptr(det_classes), k, ptr(top),
                                 ptr(keep), _stream(sims)), "lvc_knn_merge_vote")
    return top, keep


def max_f32(x):
    """[1] fp32 device tensor: the maximum of x (lvc_max_f32)."""
    _req_cuda(x)
    x = x.contiguous()
    assert x.dtype == torch.float32
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    check(_lib.lib().lvc_max_f32(ptr(x), x.numel(), ptr(out), _stream(x)), "lvc_max_f32")
    return out


def knn_margins(qres, sres_max, acc, extra=0.0):
    """The two-stage sweep's per-row margins (label_verification.pre_filter_margins + extra) in one launch (lvc_knn_margins).
    qres [Q] fp32, sres_max [1] fp32 device tensor."""
    _req_cuda(qres, sres_max)
    qres = qres.contiguous()
    assert qres.dtype == torch.float32 and sres_max.dtype == torch.float32 and sres_max.numel() == 1
    out = torch.empty_like(qres)
    check(_lib.lib().lvc_knn_margins(ptr(qres), ptr(sres_max), acc, extra, qres.numel(), ptr(out), _stream(qres)),
          "lvc_knn_margins")
    return out


def rownorm_h(x, mu=None, eps=1e-5, mode=0, want_rows=True, want_resid=False):
    """`rownorm` for the two-stage kNN sweep: (y fp32 [M,D] or None, yh fp16 [M,D], den [M]); y equals (x - mu) / den[:, None]
    exactly and is bit-identical to `rownorm`'s output, except that 16-byte aligned rows wider than 2048 are summed in another order there
    (fp64 sums, one rounding of den: equal to fp32 rounding, bit-equal unless den falls on a rounding boundary).  want_resid: also resid [M] = |row - fp16(row)|_2."""
    _req_cuda(x, mu)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32
    M, D = x.shape
    y = torch.empty(M, D, device=x.device, dtype=torch.float32) if want_rows else None
    yh = torch.empty(M, D, device=x.device, dtype=torch.float16)
    den = torch.empty(M, device=x.device, dtype=torch.float32)
    resid = torch.empty(M, device=x.device, dtype=torch.float32) if want_resid else None
    rc = _lib.lib().lvc_rownorm_h(ptr(x), ptr(mu), ptr(y), ptr(yh), ptr(den), ptr(resid), M, D, x.stride(0),
                                  eps, mode, _stream(x))
    check(rc, "lvc_rownorm_h")
    return (y, yh, den, resid) if want_resid else (y, yh, den)


def gemm_f16(a, b, n=None, ldb=None, q15=False):
    """a [M,C] . b^T on fp16 operands with fp32 accumulation -> [M,N] fp32 (lvc_gemm_f16): the pre-filter of the two-stage
    kNN sweep.  n / ldb: use n rows of b that lie ldb elements apart (a strided subset of a contiguous [*, C] tensor).
    q15: the result as 16-bit fixed point, rint(32766 * value), NaN -> 32767 (lvc_gemm_f16_q15; rows padded to a multiple of 8 columns,
    returned as the [M, N] view)."""
    _req_cuda(a, b)
    M, C = a.shape
    assert a.is_contiguous() and b.is_contiguous() and a.dtype == torch.float16 and b.dtype == torch.float16 and b.shape[1] == C
    N = b.shape[0] if n is None else n
    ldb = C if ldb is None else ldb
    assert (N - 1) * ldb + C <= b.numel()
    if q15:
        ld = (N + 7) // 8 * 8
        y = torch.empty(M, ld, device=a.device, dtype=torch.int16)
        rc = _lib.lib().lvc_gemm_f16_q15(ptr(a), ptr(b), ldb, ptr(y), M, N, C, ld, _stream(a))
        check(rc, "lvc_gemm_f16_q15")
        return y[:, :N]
    y = torch.empty(M, N, device=a.device, dtype=torch.float32)
    rc = _lib.lib().lvc_gemm_f16(ptr(a), ptr(b), ldb, ptr(y), M, N, C, N, _stream(a))
    check(rc, "lvc_gemm_f16")
    return y


KNN_LIST_CAP = 256


def knn_verify_topk_vote(approx, q, sn, margin, shot_classes, det_classes, k, mu=None, den=None, margins=None):
    """approx [Q,S] from gemm_f16 over the fp16 roundings of the normalised rows; q [Q,D] the raw query descriptors with the
    mu / den `rownorm_h` used (or the normalised rows themselves with mu = den = None); sn [S,D] normalised shots.
    Exact top-10 classes + vote (csrc/knn.hip)."""
    _req_cuda(approx, q, sn, shot_classes, det_classes, mu, den, margins)
    Q, S = approx.shape[0], sn.shape[0]
    assert margins is None or (margins.dtype == torch.float32 and margins.is_contiguous() and margins.numel() == Q)
    assert approx.stride(1) == 1 and q.stride(1) == 1 and sn.is_contiguous() and shot_classes.dtype == torch.int64
    assert q.dtype == torch.float32 and sn.dtype == torch.float32 and q.shape[1] == sn.shape[1]
    top = torch.empty(Q, 10, dtype=torch.int64, device=approx.device)
    keep = torch.empty(Q, dtype=torch.int64, device=approx.device) if det_classes is not None else None
    if det_classes is not None:
        det_classes = det_classes.contiguous()
        assert det_classes.dtype == torch.int64
    fn = _lib.lib().lvc_knn_verify_topk_vote_q15 if approx.dtype == torch.int16 else _lib.lib().lvc_knn_verify_topk_vote
    assert approx.dtype in (torch.int16, torch.float32)
    rc = fn(ptr(approx), approx.stride(0), Q, S, ptr(q), q.stride(0),
            ptr(mu), ptr(den), ptr(sn), sn.shape[1], margin, ptr(margins),
            ptr(shot_classes), ptr(det_classes), k, ptr(top), ptr(keep), _stream(approx))
    check(rc, "lvc_knn_verify_topk_vote")
    return top, keep


# --------------------------------------------------------------------------- training-time kernels
def match_boxes(gt_boxes, boxes, thresholds, labels, allow_low_quality_matches):
    """pairwise_iou + Matcher on device.  gt_boxes [G,4] (G >= 1), boxes [N,4].
    thresholds: 1 or 2 floats, labels: len(thresholds)+1 ints.  Returns (matches int64 [N], labels int8 [N], vals [N])."""
    _req_cuda(gt_boxes, boxes)
    G, N = gt_boxes.shape[0], boxes.shape[0]
    gt_boxes = gt_boxes.contiguous().float()
    boxes = boxes.contiguous().float()
    dev = boxes.device
    matches = torch.empty(N, dtype=torch.int64, device=dev)
    mlabels = torch.empty(N, dtype=torch.int8, device=dev)
    vals = torch.empty(N, dtype=torch.float32, device=dev)
    scratch = torch.empty(max(G, 1), dtype=torch.int32, device=dev)
    nthr = len(thresholds)
    assert nthr in (1, 2) and len(labels) == nthr + 1
    t = list(thresholds) + [0.0]
    lab = list(labels) + [0]
    rc = _lib.lib().lvc_match_boxes(ptr(gt_boxes), G, ptr(boxes), N, t[0], t[1],
                                    nthr, lab[0], lab[1], lab[2],
                                    1 if allow_low_quality_matches else 0, ptr(matches), ptr(mlabels), ptr(vals),
                                    ptr(scratch), _stream(boxes))
    check(rc, "lvc_match_boxes")
    return matches, mlabels, vals


def cat_ground_truth(gt_instances):
    """The images' gt boxes one after the other + the prefix of their counts as a device int32 [B+1] (pinned staging, asynchronous copy:
    a plain torch.tensor(..., device=) would wait for everything queued on the stream -- the trunk).  -> (gt [G,4], gt_off, counts list)."""
    dev = gt_instances[0].gt_boxes.tensor.device
    lens = [len(t) for t in gt_instances]
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    gt = torch.cat([t.gt_boxes.tensor for t in gt_instances], 0).float().contiguous() if off[-1] else torch.zeros(0, 4, device=dev)
    gt_off = torch.tensor(off, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    return gt, gt_off, lens


def match_boxes_batched(gt, gt_off, B, boxes, nbox, thresholds, labels, allow_low_quality_matches, return_vals=False):
    """pairwise_iou + Matcher for B images in two launches (csrc/train_targets.hip).  gt [G,4] / gt_off int32 [B+1] from
    `cat_ground_truth`; boxes [N,4] shared by the images (anchors) or [B,N,4] with nbox int32 [B] rows in use per image (None: all).
    -> (matches int32 [B,N], labels int8 [B,N])."""
    _req_cuda(gt_off, boxes)
    shared = boxes.dim() == 2
    N = boxes.shape[-2]
    boxes = boxes.contiguous()
    assert boxes.dtype == torch.float32 and gt.dtype == torch.float32 and gt_off.dtype == torch.int32
    dev = boxes.device
    matches = torch.empty(B, N, dtype=torch.int32, device=dev)
    mlabels = torch.empty(B, N, dtype=torch.int8, device=dev)
    vals = torch.empty(B, N, dtype=torch.float32, device=dev)
    G = gt.shape[0]
    scratch = torch.empty(max(G, 1), dtype=torch.int32, device=dev)
    nthr = len(thresholds)
    assert nthr in (1, 2) and len(labels) == nthr + 1
    t = list(thresholds) + [0.0]
    lab = list(labels) + [0]
    rc = _lib.lib().lvc_match_boxes_batched(ptr(gt.contiguous()), ptr(gt_off), G, B, ptr(boxes), 0 if shared else N * 4,
                                            ptr(nbox), N, t[0], t[1], nthr, lab[0], lab[1],
                                            lab[2], 1 if allow_low_quality_matches else 0, ptr(matches), ptr(mlabels), ptr(vals),
                                            ptr(scratch), _stream(boxes))
    check(rc, "lvc_match_boxes_batched")
    if return_vals:
        return matches, mlabels, vals       # vals: the best IoU of each box (Matcher's matched_vals)
    return matches, mlabels


_SUBSAMPLE_WS = {}


def randperm_is_patched():
    """True when torch.randperm has been replaced (the parity tests substitute arange to obtain the reference's deterministic choice):
    the samplers then take their keys from it instead of generating them in the kernel."""
    return getattr(torch.randperm, "__name__", "") != "randperm"


def sampling_keys(B, N, device):
    """(keys, seed) for `subsample_batched`: normally (None, a 62-bit seed from torch's CPU generator -- torch.manual_seed governs it, no
    device work); with a patched torch.randperm its B * N values as int64 [B,N]."""
    if randperm_is_patched():
        return torch.randperm(B * N, device=device).view(B, N), 0
    return None, int(torch.randint(0, 1 << 62, (1,)).item())


def subsample_batched(labels, keys, cap_pos, bs, seed=0):
    """subsample_labels (reference sampling.py:10-54) for every row of labels int8 [B,N] (1 positive, 0 negative, else ignored) in one
    launch: the min(#pos, cap_pos) positives and min(#neg, bs - num_pos) negatives with the smallest keys (int64 [B,N], distinct, e.g.
    torch.randperm(B * N); None: generated in the kernel from `seed`, see `sampling_keys`).  -> (sel int32 [B,bs]: positives first, each group by increasing key, -1 padded; counts int32 [B,2])."""
    _req_cuda(labels)
    B, N = labels.shape
    assert labels.dtype == torch.int8 and (keys is None or (keys.is_cuda and keys.dtype == torch.int64 and keys.shape == labels.shape))
    sel = torch.empty(B, bs, dtype=torch.int32, device=labels.device)
    counts = torch.empty(B, 2, dtype=torch.int32, device=labels.device)
    nbits = max(1, int(B * N - 1).bit_length())
    lib = _lib.lib()
    key = (labels.device.index, torch.cuda.current_stream(labels.device).cuda_stream, B)
    ws = _SUBSAMPLE_WS.get(key)
    if ws is None:      # zeroed once; the kernels leave it zeroed (per stream: two launches in flight must not share the histograms)
        if len(_SUBSAMPLE_WS) > 16:
            _SUBSAMPLE_WS.clear()
        ws = _SUBSAMPLE_WS[key] = torch.zeros(_lib.size_query("lvc_subsample_workspace_bytes", B), dtype=torch.uint8, device=labels.device)

    rc = lib.lvc_subsample_batched(ptr(labels.contiguous()), ptr(keys.contiguous() if keys is not None else None), int(seed),
                                   B, N, nbits, cap_pos, bs, ptr(sel), ptr(counts), ptr(ws), _stream(labels))
    check(rc, "lvc_subsample_batched")
    return sel, counts


def rpn_gather_sampled(fused, A, cell_anchors, strides, sel, counts, matches, gt, gt_off):
    """Rows of the sampled anchors straight from the head's per-level outputs fused[l] [B,H,W,ld] (channel a = objectness, A + 4 a + c =
    delta c).  -> (logits [S], deltas [S,4], anchors [S,4], matched gt boxes [S,4], labels int8 [S]) with S = B * bs; padding rows carry
    label -1 (logit 0, deltas 0, anchor and gt (0,0,1,1)), which `rpn_losses` ignores.  Contract: sel[b, j] for j < counts[b].sum()
    is -1 or an anchor index below sum_l H_l W_l A, and matches[b, sel] lies inside image b's ground truth; neither is checked."""
    L = len(fused)
    B, bs = sel.shape
    dev = sel.device
    for t in fused:
        assert t.dim() == 4 and t.dtype == torch.float32 and t.stride(3) == 1 and t.stride(1) == t.shape[2] * t.stride(2) and t.stride(0) == t.shape[1] * t.shape[2] * t.stride(2)
    VP, IP = c_void_p * L, c_int * L
    S = B * bs
    logits = torch.empty(S, device=dev)
    deltas = torch.empty(S, 4, device=dev)
    anchors = torch.empty(S, 4, device=dev)
    gtb = torch.empty(S, 4, device=dev)
    labels = torch.empty(S, dtype=torch.int8, device=dev)
    cells = [c.contiguous() for c in cell_anchors]
    rc = _lib.lib().lvc_rpn_gather_sampled(VP(*[t.data_ptr() for t in fused]), IP(*[t.stride(2) for t in fused]), VP(*[c.data_ptr() for c in cells]),
                                           IP(*[t.shape[1] for t in fused]), IP(*[t.shape[2] for t in fused]), IP(*[int(s) for s in strides]),
                                           L, A, B, bs, ptr(sel), ptr(counts), ptr(matches), ptr(gt), ptr(gt_off),
                                           ptr(logits), ptr(deltas), ptr(anchors), ptr(gtb), ptr(labels), _stream(sel))
    check(rc, "lvc_rpn_gather_sampled")
    return logits, deltas, anchors, gtb, labels


def roi_build_table(pboxes, plogits, pcount, gt, gt_off, gt_logit, Wt):
    """proposals [B,P,4] / [B,P] / count int32 [B] + gt -> (boxes [B,Wt,4], logits [B,Wt], rows in use int32 [B]): every image's proposals
    followed by its gt boxes (add_ground_truth_to_proposals)."""
    _req_cuda(pboxes, plogits, pcount, gt_off)
    B, P = plogits.shape
    dev = pboxes.device
    boxes = torch.empty(B, Wt, 4, device=dev)
    logits = torch.empty(B, Wt, device=dev)
    nrow = torch.empty(B, dtype=torch.int32, device=dev)
    rc = _lib.lib().lvc_roi_build_table(ptr(pboxes.contiguous()), ptr(plogits.contiguous()), ptr(pcount), B, P, ptr(gt), ptr(gt_off),
                                        gt_logit, Wt, ptr(boxes), ptr(logits), ptr(nrow), _stream(pboxes))
    check(rc, "lvc_roi_build_table")
    return boxes, logits, nrow


def roi_gather_sampled(boxes, logits, matches, sel, counts, gt_classes, gt_off, num_classes):
    """Sampled rows of the table -> (boxes [B,bs,4], logits [B,bs], classes int64 [B,bs] (K = background AND padding: the rows behind
    an image's counts are zero boxes of class K with match 0; callers cut them off or check the counts), matched gt index int64
    [B,bs]).  Contract: sel[b, j] for j < counts[b].sum() lies in [0, Wt) and matches[b, sel] in [0, number of gt of image b); the
    kernel does not check either."""
    B, Wt = logits.shape
    bs = sel.shape[1]
    dev = boxes.device
    sb = torch.empty(B, bs, 4, device=dev)
    sl = torch.empty(B, bs, device=dev)
    sc = torch.empty(B, bs, dtype=torch.int64, device=dev)
    sm = torch.empty(B, bs, dtype=torch.int64, device=dev)
    assert gt_classes.dtype == torch.int64
    rc = _lib.lib().lvc_roi_gather_sampled(ptr(boxes), ptr(logits), ptr(matches), ptr(sel), ptr(counts), ptr(gt_classes.contiguous()), ptr(gt_off),
                                           B, Wt, bs, num_classes, ptr(sb), ptr(sl), ptr(sc), ptr(sm), _stream(boxes))
    check(rc, "lvc_roi_gather_sampled")
    return sb, sl, sc, sm


def fast_rcnn_losses(logits, deltas, proposals, gt_boxes, gt_classes, num_classes, box_weights, smooth_l1_beta):
    """Returns (losses [2] = (loss_cls, loss_box_reg), dlogits [R,K+1], ddeltas [R,4K|4]).
    logits [R, >=K+1] and deltas [R, 4K | 4] may be column slices of a wider tensor (unit column stride).
    Contract: every gt_classes[r] lies in [0, K] (K = background).  The kernel indexes the row's logits with it unchecked: a
    negative or larger class reads outside the row."""
    _req_cuda(logits, deltas, proposals, gt_boxes, gt_classes)
    R = logits.shape[0]
    K = num_classes
    nreg = deltas.shape[1] if deltas.shape[1] == 4 else 4 * K
    dev = logits.device
    out = torch.empty(2, device=dev, dtype=torch.float32)
    dl = torch.empty(R, K + 1, device=dev, dtype=torch.float32)
    dd = torch.empty(R, nreg, device=dev, dtype=torch.float32)
    row_terms = torch.empty(2 * R, device=dev, dtype=torch.float64)
    wx, wy, ww, wh = box_weights
    assert logits.stride(1) == 1 and deltas.stride(1) == 1 and gt_classes.dtype == torch.int64
    rc = _lib.lib().lvc_fast_rcnn_losses(ptr(logits), logits.stride(0), ptr(deltas), deltas.stride(0), K,
                                         1 if nreg == 4 else 0, ptr(proposals.contiguous()), ptr(gt_boxes.contiguous()),
                                         ptr(gt_classes.contiguous()), R, wx, wy, ww,
                                         wh, smooth_l1_beta, ptr(out), ptr(dl), ptr(dd), ptr(row_terms),
                                         _stream(logits))
    check(rc, "lvc_fast_rcnn_losses")
    return out, dl, dd


def giou_box_loss(deltas, proposals, gt_boxes, gt_classes, num_classes, box_weights, scale_clamp, iterate=False,
                  lambda_=0.0):
    """Box-corrector regression loss.  Returns (loss [1], ddeltas [R,4])."""
    _req_cuda(deltas, proposals, gt_boxes, gt_classes)
    R = deltas.shape[0]
    out = torch.empty(1, device=deltas.device, dtype=torch.float32)
    dd = torch.empty(R, 4, device=deltas.device, dtype=torch.float32)
    wx, wy, ww, wh = box_weights
    assert deltas.stride(1) == 1 and gt_classes.dtype == torch.int64
    rc = _lib.lib().lvc_giou_box_loss(ptr(deltas), deltas.stride(0), ptr(proposals.contiguous()),
                                      ptr(gt_boxes.contiguous()), ptr(gt_classes.contiguous()), R,
                                      num_classes, wx, wy, ww, wh,
                                      scale_clamp, 1 if iterate else 0, lambda_, ptr(out),
                                      ptr(dd), _stream(deltas))
    check(rc, "lvc_giou_box_loss")
    return out, dd


def relu_backward(dy, y):
    _req_cuda(dy, y)
    dy, y = dy.contiguous(), y.contiguous()
    out = torch.empty_like(dy)
    check(_lib.lib().lvc_relu_backward(ptr(dy), ptr(y), dy.numel(), ptr(out), _stream(dy)), "lvc_relu_backward")
    return out


def relu(x):
    """max(x, 0) as a pass of its own (where no producer's epilogue can take it: LastLevelP6P7 outputs p6 un-rectified and feeds
    relu(p6) to p7).  One launch of lvc_relu_backward with dy = y = x, which writes x where x > 0 and 0 elsewhere."""
    return relu_backward(x, x)


def colsum(x):
    """x [M,N] row-major -> [N] column sums (rows added in order)."""
    _req_cuda(x)
    x = x.contiguous()
    M, N = x.shape
    out = torch.empty(N, device=x.device, dtype=torch.float32)
    check(_lib.lib().lvc_colsum(ptr(x), M, N, N, ptr(out), _stream(x)), "lvc_colsum")
    return out


def colsum_rows(x2d):
    """x2d [M,N] row-major with M up to 10^5-10^6 (conv bias gradients): slab sums + fp32 atomics."""
    _req_cuda(x2d)
    x2d = x2d.contiguous()
    M, N = x2d.shape
    out = torch.empty(N, device=x2d.device, dtype=torch.float32)
    check(_lib.lib().lvc_colsum_atomic(ptr(x2d), M, N, N, ptr(out), _stream(x2d)), "lvc_colsum_atomic")
    return out


BWD_TIMER = None     # a list: every weight- / data-gradient launch appends (kind, engine, flops, algorithmic bytes, start, end events)


def _bwd_timed(kind, engine, flops, nbytes, fn, tag=""):
    if BWD_TIMER is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    BWD_TIMER.append((kind, engine, flops, nbytes, e0, e1, tag))
    return out


def conv_wgrad(x, dy, scale, R, S, stride, pad, split=None):
    """dW of y = conv(x, W) (* scale per output channel): x [N,H,W,C], dy [N,Ho,Wo,K] -> [K,R,S,C] fp32."""
    if BWD_TIMER is not None:
        eng = "f16x2" if (split or DGRAD_SPLIT) == "f16x2" else WGRAD_ENGINE
        if eng == "f16x2" and dy.shape[0] * dy.shape[1] * dy.shape[2] < 16:
            eng = "f32"      # fewer pixels than one k-step of the fp16 MFMA: lvc_conv_wgrad_nhwc_f16x2 runs the exact fp32 form
        fl = 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * dy.shape[3] * x.shape[3] * R * S
        nb = 4.0 * (x.numel() + dy.numel() + dy.shape[3] * R * S * x.shape[3])
        tag = "%dx%dx%d %d>%d %dx%d s%d" % (dy.shape[0], dy.shape[1], dy.shape[2], x.shape[3], dy.shape[3], R, S, stride)
        return _bwd_timed("wgrad", eng, fl, nb, lambda: _conv_wgrad(x, dy, scale, R, S, stride, pad, split), tag)
    return _conv_wgrad(x, dy, scale, R, S, stride, pad, split)


def _conv_wgrad(x, dy, scale, R, S, stride, pad, split=None):
    _req_cuda(x, dy, scale)
    assert x.dim() == 4 and dy.dim() == 4 and x.is_contiguous() and dy.is_contiguous()
    assert x.dtype == torch.float32 and dy.dtype == torch.float32
    N, H, W, C = x.shape
    K = dy.shape[3]
    assert dy.shape[0] == N and dy.shape[1] == (H + 2 * pad - R) // stride + 1 and dy.shape[2] == (W + 2 * pad - S) // stride + 1
    dw = torch.empty(K, R, S, C, device=x.device, dtype=torch.float32)
    if (split or DGRAD_SPLIT) == "f16x2":   # gradients scaled into fp16's range (solver.LossScaler): fp16 MFMA path
        check(_lib.lib().lvc_conv_wgrad_nhwc_f16x2(ptr(x), ptr(dy), ptr(scale), ptr(dw), N, H, W,
                                                   C, K, R, S, stride, pad,
                                                   K, ptr(_conv_error_view(x.device)), _stream(x)),
              "lvc_conv_wgrad_nhwc_f16x2")
        return dw
    fn = "lvc_conv_wgrad_nhwc_bf16x3" if WGRAD_ENGINE == "bf16x3" else "lvc_conv_wgrad_nhwc"
    check(getattr(_lib.lib(), fn)(ptr(x), ptr(dy), ptr(scale), ptr(dw), N, H, W, C, K,
                                  R, S, stride, pad, K, _stream(x)), fn)
    return dw


def conv_wgrad_grouped(x, dy, scale, groups, stride):
    """dW [K, C/groups, 3, 3] (the parameter's layout) of a grouped 3x3 / pad 1 layer y = conv(x, W) (* scale per output channel):
    x [N,H,W,C], dy [N,Ho,Wo,K].  One launch of its own per layer (it does not join the deferred launch of the dense layers); partial
    sums are added in a fixed order -- two runs are bit-identical."""
    _req_cuda(x, dy, scale)
    assert x.dim() == 4 and dy.dim() == 4 and x.is_contiguous() and dy.is_contiguous()
    assert x.dtype == torch.float32 and dy.dtype == torch.float32
    N, H, W, C = x.shape
    assert tuple(dy.shape) == (N, (H - 1) // stride + 1, (W - 1) // stride + 1, C), (dy.shape, x.shape, stride)
    grouped_conv_check(C, C, groups, 3, stride, 1)
    cg = C // groups
    dw = torch.empty(C, cg, 3, 3, device=x.device, dtype=torch.float32)
    if x.numel() == 0:
        return dw.zero_()
    lib = _lib.lib()
    nbytes = _lib.size_query("lvc_conv3x3_grouped_wgrad_workspace_bytes", N, H, W, C, groups, stride)
    scratch = torch.empty(nbytes, device=x.device, dtype=torch.uint8)

    def run():
        check(lib.lvc_conv3x3_grouped_wgrad_nhwc(ptr(x), ptr(dy), ptr(scale), ptr(dw), N, H, W, C, groups,
                                                 stride, C, ptr(scratch), _stream(x)), "lvc_conv3x3_grouped_wgrad_nhwc")
        return dw

    return _bwd_timed("wgrad", "f32_grouped", 2.0 * dy.numel() * cg * 9, 4.0 * (x.numel() + dy.numel() + dw.numel()), run,
                      "grouped %dx%dx%d %d g%d s%d" % (N, H, W, C, groups, stride))


# ---- deferred, grouped weight gradients (csrc/conv_wgrad.hip: conv_wgrad_group_bf16x3_kernel) --------------------------------------
DEFER_WGRAD = _os.environ.get("LVC_DEFER_WGRAD", "1") != "0"
_WGRAD_GROUP = 24            # jobs per launch (kernel-argument table)
_WGRAD_Q = []                # (param, x, g, scale, R, stride, pad)
_WGRAD_ARMED = [False]
_WGRAD_SINKS = {}            # id(param) -> (destination(param) -> tensor the gradient is written into, ready(param))
# "1": the grouped launches on a second stream.  Measured on the box-corrector step (2 images per GPU): 28.41 / 28.46 / 28.49 ms against
# 28.28 / 28.68 / 29.24 on the pass's own stream -- the step is bound by the host's launch rate there, not by the chip; off by default
WGRAD_SIDE_STREAM = _os.environ.get("LVC_WGRAD_SIDE_STREAM", "0") != "0"
_WGRAD_SIDE = {}             # device index -> the stream the grouped launches run on
_WGRAD_PENDING = []          # (event, deliveries, operands kept alive) of groups in flight on the side stream


_WGRAD_USES = {}             # id(param) -> differentiable forward uses whose backward node has not run yet (layers.wrappers._ConvFn)


def register_wgrad_sink(param, destination, ready, owner=None):
    """A gradient exchange that owns flat buckets hands out the bucket slice as the place the deferred weight gradient is written
    to (no copy into the bucket afterwards) and is told when it is there (`lvc_amd.distributed.GradientBuckets`).  The sink dies with
    the exchange: bound methods are held through weak references (and `owner`, if given, through another) -- a dropped exchange must
    not keep receiving gradients into its dead buckets, nor be kept alive by this table.  One live sink per parameter."""
    import weakref

    def weak(fn):
        try:
            return weakref.WeakMethod(fn)
        except TypeError:          # a plain function: nothing to die with
            return lambda: fn

    if _wgrad_sink(param) is not None:
        raise RuntimeError("lvc_amd: parameter already has a deferred-gradient sink (a second GradientBuckets over the same parameters? "
                           "call remove() on the first)")
    _WGRAD_SINKS[id(param)] = (weak(destination), weak(ready), weakref.ref(param), weakref.ref(owner) if owner is not None else None)


def unregister_wgrad_sink(param):
    _WGRAD_SINKS.pop(id(param), None)


def _wgrad_sink(param):
    """(destination, ready) of the live sink of `param`, or None (and the entry is dropped) when its parameter, its owner or its
    callables are gone -- ids are reused."""
    sink = _WGRAD_SINKS.get(id(param))
    if sink is None:
        return None
    dst, rdy = sink[0](), sink[1]()
    if sink[2]() is not param or (sink[3] is not None and sink[3]() is None) or dst is None or rdy is None:
        del _WGRAD_SINKS[id(param)]
        return None
    return dst, rdy


def reset_wgrad_queue():
    del _WGRAD_Q[:]
    del _WGRAD_PENDING[:]
    _WGRAD_USES.clear()
    _WGRAD_ARMED[0] = False


def in_backward():
    """True while the autograd engine is executing a graph task on this thread."""
    return torch._C._current_graph_task_id() != -1


def note_wgrad_use(param):
    """A differentiable forward use of `param` (layers.wrappers._ConvFn.forward): its backward node will deliver one weight gradient."""
    _WGRAD_USES[id(param)] = _WGRAD_USES.get(id(param), 0) + 1


def wgrad_use_done(param):
    """That use's backward node ran (it queued a deferred job or handed its gradient to AccumulateGrad)."""
    n = _WGRAD_USES.get(id(param), 0)
    if n > 0:
        _WGRAD_USES[id(param)] = n - 1


def wgrad_job_queued(param):
    """True while a deferred weight gradient of `param` waits in the queue: its gradient is not final
    (lvc_amd.distributed.GradientBuckets._hook).  That is all a post-accumulate hook needs to know: the engine
    runs a parameter's AccumulateGrad node only after every use of this pass has run its backward node, so by then whatever is still to
    come is in the queue -- the use counts say nothing there, and a forward whose backward never ran leaves them positive."""
    return any(j[0] is param for j in _WGRAD_Q)


def forget_wgrad_uses(params):
    """Drop the use counts of `params`: the step is over (`GradientBuckets.finish`).  Counts left by forwards whose backward never ran
    -- a pass repeated after Fp16RangeError, an exception, a loss that was skipped -- would otherwise hold the parameters back in every
    later non-final flush, and for ever where no deferred job is queued (LVC_DEFER_WGRAD=0, another weight-gradient engine)."""
    for p in params:
        _WGRAD_USES.pop(id(p), None)


def can_defer_wgrad(x, g):
    """Deferred grouped launch: the default unscaled bf16x3 path inside a `backward()` (not torch.autograd.grad: the gradient is
    written to `param.grad` by a callback at the end of the pass, as AccumulateGrad would)."""
    return (DEFER_WGRAD and WGRAD_ENGINE == "bf16x3" and DGRAD_SPLIT != "f16x2" and x.numel() * 4 < (1 << 31) and g.numel() * 4 < (1 << 31)
            and x.is_contiguous() and g.is_contiguous())


def defer_wgrad(param, x, g, scale, R, stride, pad):
    """Queue dW of y = conv(x, param) (* scale) for the grouped launch; `param.grad` holds it when `backward()` returns."""
    _WGRAD_Q.append((param, x, g, scale, R, stride, pad))
    if not _WGRAD_ARMED[0]:
        _WGRAD_ARMED[0] = True
        torch.autograd.Variable._execution_engine.queue_callback(_flush_wgrad_end)
    if sum(1 for j in _WGRAD_Q if _WGRAD_USES.get(id(j[0]), 0) == 0) >= _WGRAD_GROUP:
        flush_wgrad()


def _flush_wgrad_end():
    _WGRAD_ARMED[0] = False
    flush_wgrad(final=True)


def flush_wgrad(final=False):
    """Launch the queued weight gradients: one zeroing, one grouped wgrad launch, one grouped layout / accumulate launch."""
    if final:
        q = list(_WGRAD_Q)
        del _WGRAD_Q[:]
        # uses counted by a forward whose backward never ran (two forwards, one backward): the pass is over, the counts go, and a sink
        # whose parameter got its whole gradient through AccumulateGrad is told once more (a report it has seen already changes nothing)
        stale = [i for i, n in _WGRAD_USES.items() if n > 0]
        _WGRAD_USES.clear()
        queued = {id(j[0]) for j in q}
        for i in stale:
            entry = _WGRAD_SINKS.get(i)
            if entry is not None and i not in queued:
                prm = entry[2]()
                sink = _wgrad_sink(prm) if prm is not None else None
                if sink is not None and prm.grad is not None:
                    sink[1](prm)
    else:
        # a flush DELIVERS its parameters (p.grad is set, a bucketed exchange may start reducing them): only parameters whose every use
        # of this pass has run its backward node go out -- the RPN head's convolutions are used once per pyramid level, and a weight
        # whose uses straddled two flushes was accumulated into a bucket slice that was already being reduced
        q = [j for j in _WGRAD_Q if _WGRAD_USES.get(id(j[0]), 0) == 0]
        _WGRAD_Q[:] = [j for j in _WGRAD_Q if _WGRAD_USES.get(id(j[0]), 0) != 0]
    if not q:
        if final:
            _retire_wgrad()
        return
    import ctypes

    dev = q[0][1].device
    n = len(q)
    first = {}               # a parameter used several times in the pass (the RPN head over the pyramid levels): ONE accumulation buffer
    offs, total = [], 0
    for j, (p, *_r) in enumerate(q):
        if id(p) in first:
            offs.append(offs[first[id(p)]])
        else:
            first[id(p)] = j
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
    flat = torch.zeros(total, device=dev, dtype=torch.float32)
    PA = ctypes.c_void_p * n
    xs, dys, scs, dws = PA(), PA(), PA(), PA()
    nf = len(first)
    PF = ctypes.c_void_p * nf
    srcs, dsts = PF(), PF()
    shapes = (c_int * (10 * n))()
    fshapes = (c_int * (4 * nf))()
    outs = []
    flops = nbytes = 0.0
    f = 0
    for j, (p, x, g, scale, R, stride, pad) in enumerate(q):
        N, H, W, C = x.shape
        Kc = g.shape[3]
        xs[j], dys[j], scs[j] = x.data_ptr(), g.data_ptr(), (scale.data_ptr() if scale is not None else None)
        dws[j] = flat.data_ptr() + 4 * offs[j]
        shapes[10 * j: 10 * j + 10] = [N, H, W, C, Kc, R, R, stride, pad, Kc]
        flops += 2.0 * g.shape[0] * g.shape[1] * g.shape[2] * Kc * C * R * R
        nbytes += 4.0 * (x.numel() + g.numel() + p.numel())
        if first[id(p)] != j:
            continue
        sink = _wgrad_sink(p)
        if p.grad is not None:
            dst, beta = p.grad, 1
            assert dst.is_contiguous() and dst.dtype == torch.float32
        else:
            dst = sink[0](p) if sink is not None else torch.empty_like(p, memory_format=torch.contiguous_format)
            beta = 0
        outs.append((p, dst, beta, sink))
        srcs[f], dsts[f] = dws[j], dst.data_ptr()
        fshapes[4 * f: 4 * f + 4] = [Kc, C, R * R, beta]
        f += 1
    main = torch.cuda.current_stream(dev)
    side = main
    if WGRAD_SIDE_STREAM and BWD_TIMER is None:
        # off the critical path in time as well: the group runs on a second stream next to the data-gradient chain, whose launches
        # (8 400-pixel maps at 2 images per GPU) leave most of the chip idle
        side = _WGRAD_SIDE.get(dev.index)
        if side is None:
            side = _WGRAD_SIDE[dev.index] = torch.cuda.Stream(dev)
        side.wait_stream(main)              # x, dy, the zeroed buffer and the destinations are complete on the main stream
    st = c_void_p(side.cuda_stream)

    def launch():
        check(_lib.lib().lvc_conv_wgrad_group_bf16x3(n, xs, dys, scs, dws, shapes, st), "lvc_conv_wgrad_group_bf16x3")

    _bwd_timed("wgrad", "bf16x3", flops, nbytes, launch, "group of %d" % n)
    check(_lib.lib().lvc_wgrad_finalize_group(nf, srcs, dsts, fshapes, st), "lvc_wgrad_finalize_group")
    if side is main:
        _deliver_wgrad(outs)
        return
    ev = torch.cuda.Event()
    ev.record(side)
    _WGRAD_PENDING.append((ev, outs, (q, flat)))     # operands stay alive until the main stream has passed the group's event
    _retire_wgrad(keep=0 if final else 1)


def _deliver_wgrad(outs):
    for p, dst, beta, sink in outs:
        if not beta:
            p.grad = dst
        if sink is not None:
            sink[1](p)


def _retire_wgrad(keep=0):
    """Hand the finished groups' gradients over (main stream ordered behind them); the newest `keep` groups stay in flight."""
    while len(_WGRAD_PENDING) > keep:
        ev, outs, _alive = _WGRAD_PENDING.pop(0)
        torch.cuda.current_stream().wait_event(ev)
        _deliver_wgrad(outs)


def scatter_stride2(x, H, W):
    """x [N,(H-1)//2+1,(W-1)//2+1,C] -> [N,H,W,C] with x at the even pixels and zeros elsewhere."""
    _req_cuda(x)
    x = x.contiguous()
    N, Hs, Ws, C = x.shape
    assert Hs == (H - 1) // 2 + 1 and Ws == (W - 1) // 2 + 1
    y = torch.empty(N, H, W, C, device=x.device, dtype=torch.float32)
    check(_lib.lib().lvc_scatter_stride2_nhwc(ptr(x), ptr(y), N, H, W, C, _stream(x)),
          "lvc_scatter_stride2_nhwc")
    return y


def subsample2_into(x, out):
    """out[n, i, j, :C] = x[n, 2i, 2j, :] where out is a [N,Hs,Ws,C] view with unit channel stride (rows may be wider: the tail
    channels of a concat buffer)."""
    _req_cuda(x, out)
    N, H, W, C = x.shape
    Hs, Ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert x.is_contiguous() and x.dtype == torch.float32 and out.dtype == torch.float32 and out.shape == (N, Hs, Ws, C)
    ld = out.stride(2)
    assert out.stride(3) == 1 and out.stride(1) == Ws * ld and out.stride(0) == Hs * Ws * ld
    check(_lib.lib().lvc_subsample2_nhwc(ptr(x), ptr(out), N, H, W, C, ld, _stream(x)),
          "lvc_subsample2_nhwc")
    return out


def downsum2x2(x):
    """x [N,2Hs,2Ws,C] -> [N,Hs,Ws,C] sums of the 2x2 blocks."""
    _req_cuda(x)
    x = x.contiguous()
    N, H, W, C = x.shape
    assert H % 2 == 0 and W % 2 == 0
    y = torch.empty(N, H // 2, W // 2, C, device=x.device, dtype=torch.float32)
    check(_lib.lib().lvc_downsum2x2_nhwc(ptr(x), ptr(y), N, H // 2, W // 2, C, _stream(x)),
          "lvc_downsum2x2_nhwc")
    return y


def _avgpool2_pitch(t):
    """Floats between consecutive pixels of the [N,H,W,C] tensor t (a dimension of size 1 has no say)."""
    N, H, W, C = t.shape
    return t.stride(2) if W > 1 else t.stride(1) if H > 1 else t.stride(0) if N > 1 else C


def _avgpool2_is_slice(t):
    """t [N,H,W,C] is laid out as an NHWC tensor or a channel slice of one: unit channel stride, one pitch for all three outer dimensions."""
    N, H, W, C = t.shape
    ld = _avgpool2_pitch(t)
    return not t.numel() or (t.stride(3) == 1 and ld >= C and (H == 1 or t.stride(1) == W * ld) and (N == 1 or t.stride(0) == H * W * ld))


def _avgpool2_dims(t, what):
    """[N,H,W,C] and the row pitch of `t`, a unit-channel-stride NHWC tensor or channel slice of one; ValueError for what
    csrc/avgpool.hip does not take (raised before any device is touched: it answers on a machine without a GPU)."""
    if t.dim() != 4 or t.dtype != torch.float32:
        raise ValueError("avgpool2: {} must be a float32 [N,H,W,C] tensor (got {} {})".format(what, t.dtype, tuple(t.shape)))
    N, H, W, C = t.shape
    ld = _avgpool2_pitch(t)
    if C < 1 or C % 4 or ld % 4 or t.storage_offset() % 4:
        raise ValueError("avgpool2: channels, row pitch and channel offset of {} must be multiples of 4 (16-byte loads and stores); got "
                         "C={}, pitch {}, offset {}".format(what, C, ld, t.storage_offset()))
    if not _avgpool2_is_slice(t):
        raise ValueError("avgpool2: {} must be an NHWC tensor or a channel slice of one (strides {})".format(what, t.stride()))
    return N, H, W, C, ld


def avgpool2_into(x, out=None):
    """nn.AvgPool2d(2) on NHWC: x [N,H,W,C] contiguous -> [N,H//2,W//2,C] (an odd last row / column is dropped), each value
    (((x00 + x01) + x10) + x11) * 0.25f.  out: a [N,H//2,W//2,C] view with unit channel stride that receives it -- rows may be wider
    (a channel slice of a concat buffer: the other channels are not touched).  ValueError for H < 2, W < 2, or a channel count /
    row pitch that is no multiple of 4."""
    N, H, W, C, ldx = _avgpool2_dims(x, "the input")
    if H < 2 or W < 2:
        raise ValueError("avgpool2: the map must be at least 2 x 2 (got {} x {})".format(H, W))
    if ldx != C:
        raise ValueError("avgpool2: the input must be contiguous")
    if out is not None:
        No, Ho, Wo, Co, ldo = _avgpool2_dims(out, "the output")
        if (No, Ho, Wo, Co) != (N, H // 2, W // 2, C):
            raise ValueError("avgpool2: output {} for input {}".format(tuple(out.shape), tuple(x.shape)))
    _req_cuda(x, out)
    if out is None:
        out, ldo = torch.empty(N, H // 2, W // 2, C, device=x.device, dtype=torch.float32), C
    if N:
        check(_lib.lib().lvc_avgpool2_nhwc(ptr(x), ptr(out), N, H, W, C, ldo, _stream(x)),
              "lvc_avgpool2_nhwc")
    return out


def avgpool2_backward(dy, H, W):
    """dx [N,H,W,C] = 0.25 * dy[n, h // 2, w // 2, :], zeros in a dropped odd row / column.  dy: [N,H//2,W//2,C], contiguous or a
    channel slice of a wider buffer."""
    N, Ho, Wo, C, ldi = _avgpool2_dims(dy, "the gradient")
    if H < 2 or W < 2 or (Ho, Wo) != (H // 2, W // 2):
        raise ValueError("avgpool2: gradient {} for a {} x {} map".format(tuple(dy.shape), H, W))
    _req_cuda(dy)
    dx = torch.empty(N, H, W, C, device=dy.device, dtype=torch.float32)
    if N:
        check(_lib.lib().lvc_avgpool2_bwd_nhwc(ptr(dy), ptr(dx), N, H, W, C, ldi, _stream(dy)),
              "lvc_avgpool2_bwd_nhwc")
    return dx


class _AvgPool2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.hw = (x.shape[1], x.shape[2])
        return avgpool2_into(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        if not _avgpool2_is_slice(dy) or _avgpool2_pitch(dy) % 4 or dy.storage_offset() % 4:
            dy = dy.contiguous()      # any other view autograd hands over (permuted, expanded, odd outer strides, unaligned)
        return avgpool2_backward(dy, *ctx.hw)


def avgpool2_nhwc(x):
    """`avgpool2_into` as a differentiable function of x (both pools of a BottleneckBlockCLIP under autograd)."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _AvgPool2Fn.apply(x)
    return avgpool2_into(x)


def pack_conv_dgrad(weight, scale, pad, groups=1):
    """groups > 1 (weight [K, C/groups, 3, 3], pad 1): the grouped kernel's operand in its data-gradient mode; a stride-2 layer's
    gradient is zero-stuffed onto the input grid before it (`conv_dgrad`).  Otherwise:
    Packed weights of the DATA gradient of y = conv(x, weight, stride 1 after sub-sampling, pad) * scale:
    dx = conv(dy, Wt, pad = R-1-pad) with Wt[c][k][r][s] = scale[k] * weight[k][c][R-1-r][S-1-s].  A strided 1x1 is
    the same product on the sub-sampled grid followed by `scatter_stride2`; a stride-2 3x3 / pad 1 layer's gradient is
    zero-stuffed onto the input grid first (`conv_dgrad`), so the operand does not depend on the stride.  Output channels of the forward conv
    (the contraction here) are zero-padded to the kernels' 32-channel chunk."""
    Kout, C, R, S = weight.shape
    if groups != 1:
        grouped_conv_check(C * groups, Kout, groups, R, 1, pad)
        pc = PackedConv(_pack_grouped(weight, scale, groups, 1), None, None, Kout, Kout, 3, 3, 1, 1, 9 * C, 0)
        pc.groups = groups
        return pc
    kin_pad = (Kout + 31) // 32 * 32
    rows_pad = (C + BN - 1) // BN * BN
    planes = _planes_hint(R, S, kin_pad, DGRAD_SPLIT)
    wp, pl = _pack_weights(weight, scale, rows_pad, kin_pad, 1, planes)
    return _with_planes(PackedConv(wp, None, None, C, kin_pad, R, S, 1, R - 1 - pad, R * S * kin_pad, 0), planes, pl)


def conv_dgrad(dy, pcd, x_shape, stride):
    """dx [x_shape] of a conv whose `pack_conv_dgrad` is pcd.  dy [N,Ho,Wo,K] contiguous."""
    N, H, W, C = x_shape
    if pcd.groups != 1:
        # grouped 3x3: a stride-2 layer's gradient is zero-stuffed onto the input grid, then the stride-1 kernel on the flipped operand
        g = dy.contiguous() if stride == 1 else scatter_stride2(dy, H, W)
        fl = 2.0 * g.shape[0] * g.shape[1] * g.shape[2] * pcd.K * (pcd.C // pcd.groups) * 9
        nb = 4.0 * (dy.numel() + N * H * W * C + pcd.K * (pcd.C // pcd.groups) * 9)
        dxs = _bwd_timed("dgrad", "f32_grouped", fl, nb, lambda: conv2d_nhwc(g, pcd), "grouped %dx%dx%d %d g%d s%d" % (N, H, W, C, pcd.groups, stride))
        assert tuple(dxs.shape) == (N, H, W, C), (dxs.shape, x_shape)
        return dxs
    if stride != 1:
        one, three = (pcd.R, pcd.S, pcd.pad) == (1, 1, 0), (pcd.R, pcd.S, pcd.pad) == (3, 3, 1)
        if stride != 2 or not (one or three):
            raise NotImplementedError("data gradient of a {}x{} convolution with stride {} and padding {}: strided layers are built for "
                                      "1x1 / padding 0 and 3x3 / padding 1 at stride 2".format(pcd.R, pcd.S, stride, pcd.R - 1 - pcd.pad))
        if three:
            # dense 3x3 / pad 1 / stride 2 (conv2 of res3.0 / res4.0 / res5.0 with STRIDE_IN_1X1: False): as the grouped branch above,
            # the gradient is zero-stuffed onto the input grid, then the stride-1 product on the flipped operand
            dy, stride = scatter_stride2(dy, H, W), 1
    if dy.shape[3] != pcd.C:   # contraction padded to 32 channels
        dy = torch.nn.functional.pad(dy, (0, pcd.C - dy.shape[3]))
    if BWD_TIMER is not None:
        fl = 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * dy.shape[3] * pcd.K * pcd.R * pcd.S
        nb = 4.0 * (dy.numel() + dy.shape[0] * dy.shape[1] * dy.shape[2] * pcd.K + pcd.K * pcd.R * pcd.S * dy.shape[3])
        tag = "%dx%dx%d %d>%d %dx%d" % (dy.shape[0], dy.shape[1], dy.shape[2], dy.shape[3], pcd.K, pcd.R, pcd.S)
        dxs = _bwd_timed("dgrad", DGRAD_SPLIT, fl, nb, lambda: conv2d_nhwc(dy.contiguous(), pcd, split=DGRAD_SPLIT), tag)
    else:
        dxs = conv2d_nhwc(dy.contiguous(), pcd, split=DGRAD_SPLIT)
    if stride == 1:
        assert tuple(dxs.shape) == (N, H, W, C), (dxs.shape, x_shape)
        return dxs
    return scatter_stride2(dxs, H, W)      # a strided 1x1: the product ran on the sub-sampled grid


def linear_backward(x, weight, dz, need_dx=True, need_dw=True):
    """Gradients of y = x @ weight.T on the conv/GEMM kernel.  x [M,Kin], weight [Kout,Kin], dz [M,Kout] (already
    masked by the activation).  Returns (dx [M,Kin] or None, dw [Kout,Kin] or None).  Both products contract over a
    dimension that is zero-padded to the kernel's 32-wide k chunk (Kout for dx, M for dw)."""
    M, Kin = x.shape
    Kout = weight.shape[0]
    dev = x.device
    dx = dw = None
    if need_dx:   # dx = dz @ W: contraction over Kout, "weights" = W^T [Kin rows, Kout]
        pk = (-Kout) % 32
        wt = torch.zeros(Kin, Kout + pk, device=dev)
        wt[:, :Kout] = weight.detach().t()
        dzp = dz
        if pk:
            dzp = torch.zeros(M, Kout + pk, device=dev)
            dzp[:, :Kout] = dz
        dx = linear(dzp.contiguous(), pack_linear(wt, split=DGRAD_SPLIT), split=DGRAD_SPLIT)
    if need_dw and Kout % 4 == 0 and Kin % 4 == 0:   # dw = dz^T @ x on the pixel-contraction kernel (no transposes)
        dw = conv_wgrad(x.detach().contiguous().view(M, 1, 1, Kin), dz.contiguous().view(M, 1, 1, Kout), None, 1, 1, 1, 0)
        dw = dw.view(Kout, Kin)
    elif need_dw:   # dw = dz^T @ x: contraction over M, "weights" = x^T [Kin rows, M]
        pm = (-M) % 32
        xt = torch.zeros(Kin, M + pm, device=dev)
        xt[:, :M] = x.detach().t()
        dzt = torch.zeros(Kout, M + pm, device=dev)
        dzt[:, :M] = dz.t()
        dw = linear(dzt, pack_linear(xt, split=DGRAD_SPLIT), split=DGRAD_SPLIT)
    return dx, dw


def rpn_losses(logits, deltas, anchors, gt_boxes, labels, smooth_l1_beta, normalizer, with_grad=False):
    """Sampled-anchor RPN losses.  All inputs are rows gathered at the sampled anchors; labels int8: 1 positive, 0 negative,
    negative = ignored (the padding rows of `rpn_gather_sampled`): such a row adds nothing to either loss and has a zero gradient.
    with_grad: also returns d(loss_cls)/d(logits) [S] and d(loss_loc)/d(deltas) [S,4]."""
    _req_cuda(logits, deltas, anchors, gt_boxes, labels)
    S = logits.shape[0]
    out = torch.zeros(2, device=logits.device, dtype=torch.float32)
    assert labels.dtype == torch.int8
    if with_grad:
        dl = torch.empty(S, device=logits.device, dtype=torch.float32)
        dd = torch.empty(S, 4, device=logits.device, dtype=torch.float32)
        rc = _lib.lib().lvc_rpn_losses_grad(ptr(logits.contiguous()), ptr(deltas.contiguous()), ptr(anchors.contiguous()),
                                            ptr(gt_boxes.contiguous()), ptr(labels.contiguous()), S,
                                            smooth_l1_beta, normalizer, ptr(out), ptr(dl), ptr(dd),
                                            _stream(logits))
        check(rc, "lvc_rpn_losses_grad")
        return out, dl, dd
    rc = _lib.lib().lvc_rpn_losses(ptr(logits.contiguous()), ptr(deltas.contiguous()), ptr(anchors.contiguous()),
                                   ptr(gt_boxes.contiguous()), ptr(labels.contiguous()), S, smooth_l1_beta,
                                   normalizer, ptr(out), _stream(logits))
    check(rc, "lvc_rpn_losses")
    return out


def decode_boxes(deltas, boxes, weights, image_sizes=None):
    """Class-agnostic apply_deltas (+ clip to the row's image): deltas [B*R, >=4], boxes [B,R,4] -> [B,R,4]."""
    _req_cuda(deltas, boxes, image_sizes)
    B, R, _ = boxes.shape
    boxes = boxes.contiguous()
    out = torch.empty_like(boxes)
    assert deltas.stride(1) == 1 and deltas.shape[0] == B * R
    wx, wy, ww, wh = weights
    rc = _lib.lib().lvc_decode_boxes(ptr(deltas), deltas.stride(0), ptr(boxes), B * R, R, ptr(image_sizes),
                                     wx, wy, ww, wh, SCALE_CLAMP, ptr(out),
                                     _stream(boxes))
    check(rc, "lvc_decode_boxes")
    return out


def crop_resize_nearest(image, windows, out_size=224):
    """image [C,H,W] fp32 device; windows [K,8] int32 device (x1,y1,x2,y2,l_pad,t_pad,side_w,side_h) -> [K,C,out,out]."""
    _req_cuda(image, windows)
    C, H, W = image.shape
    Kn = windows.shape[0]
    image = image.contiguous().float()
    assert windows.dtype == torch.int32 and windows.is_contiguous()
    out = torch.empty(Kn, C, out_size, out_size, device=image.device, dtype=torch.float32)
    rc = _lib.lib().lvc_crop_resize_nearest(ptr(image), C, H, W, ptr(windows), Kn, out_size,
                                            ptr(out), _stream(image))
    check(rc, "lvc_crop_resize_nearest")
    return out


# --------------------------------------------------------------------------- descriptor network (ViT) pieces
def vit_patchify(img, patch_size, kpad=None, mean=None, std=None):
    """img [B,C,H,W] fp32 -> [B*P, kpad] rows (column c*ps*ps + r*ps + s; zero columns up to kpad, a multiple of 32).
    mean / std (sequences of C floats): the rows of (img - mean[c]) / std[c] -- get_descriptors' crop normalisation fused in."""
    _req_cuda(img)
    B, C, H, W = img.shape
    kc = C * patch_size * patch_size
    kpad = kpad or kc
    P = (H // patch_size) * (W // patch_size)
    if kpad == kc:
        out = torch.empty(B * P, kc, device=img.device, dtype=torch.float32)
        if mean is not None:
            m = (c_float * C)(*[float(v) for v in mean])
            s_ = (c_float * C)(*[float(v) for v in std])
            check(_lib.lib().lvc_vit_patchify_norm(ptr(img), m, s_, ptr(out), B, C, H, W, patch_size,
                                                   _stream(img)), "lvc_vit_patchify_norm")
            return out
        check(_lib.lib().lvc_vit_patchify(ptr(img), ptr(out), B, C, H, W, patch_size, _stream(img)),
              "lvc_vit_patchify")
        return out
    tmp = vit_patchify(img, patch_size, mean=mean, std=std)
    out = torch.zeros(B * P, kpad, device=img.device, dtype=torch.float32)
    out[:, :kc] = tmp
    return out


def vit_tokens(emb, cls, pos, B):
    _req_cuda(emb, cls, pos)
    D = emb.shape[1]
    P = emb.shape[0] // B
    out = torch.empty(B * (P + 1), D, device=emb.device, dtype=torch.float32)
    check(_lib.lib().lvc_vit_tokens(ptr(emb.contiguous()), ptr(cls.detach().contiguous()), ptr(pos.detach().contiguous()), ptr(out),
                                    B, P, D, _stream(emb)), "lvc_vit_tokens")
    return out


def layernorm(x, weight, bias, eps):
    _req_cuda(x, weight, bias)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32
    M, D = x.shape
    y = torch.empty(M, D, device=x.device, dtype=torch.float32)
    check(_lib.lib().lvc_layernorm(ptr(x), x.stride(0), ptr(weight.detach()), ptr(bias.detach()), ptr(y), D, M,
                                   D, eps, _stream(x)), "lvc_layernorm")
    return y


def gelu(x):
    _req_cuda(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_lib.lib().lvc_gelu(ptr(x), ptr(y), x.numel(), _stream(x)), "lvc_gelu")
    return y


MHA_MFMA = True   # 0: the one-thread-per-query fp32 VALU kernel of round 2 (lvc_mha)


QKV_PLANES = _os.environ.get("LVC_QKV_PLANES", "1") != "0"
_MHA_PLANES_WS = {}


def can_qkv_planes(x, pc, num_heads, head_dim):
    """The qkv GEMM may write the attention's fp16 operand planes from its epilogue (csrc/conv_pw_s1.hip PLANES instance): the layer
    runs on the single-accumulator pointwise kernel and the attention on the matrix-core kernel."""
    return (QKV_PLANES and MHA_MFMA and CONV_ENGINE == "bf16x3" and CONV_SPLIT == "f16x2" and PW_S1 == 2 and head_dim == 64
            and not pc.two_acc and pc.state.get("tier", 0) == 0 and pc.R == 1 and pc.stride == 1 and pc.C >= _PW_S1_ONE_MIN_C and pc.C % 32 == 0
            and pc.K == 3 * num_heads * 64 and x.numel() * 4 < (1 << 31)
            and x.shape[0] >= 2048 and x.shape[0] * pc.K < (1 << 29))      # the rows for which `conv2d_nhwc` takes that kernel too


def qkv_attention(x, pc, B, N, num_heads, scale):
    """softmax(q k^T scale) v of a ViT block from the block's normalised input x [B*N, C] and its packed qkv layer: the qkv GEMM writes
    q * scale * log2(e), k, v as fp16 (hi, lo) planes from its epilogue (lvc_conv1x1_qkv_planes_f16s1: the fp32 qkv tensor and the
    split pass of lvc_mha_mfma do not exist), lvc_mha_mfma_planes consumes them.  Bit-identical to `mha(linear(x, pc), ...)`.
    -> [B*N, H*64]."""
    _req_cuda(x)
    x = x.contiguous()
    dev = x.device
    lib = _lib.lib()
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, B, N, num_heads)
    ws = _MHA_PLANES_WS.get(key)
    if ws is None:      # zeroed ONCE: the epilogue never writes the padding rows N..Npad-1, which must stay zero
        if len(_MHA_PLANES_WS) > 8:
            _MHA_PLANES_WS.clear()
        ws = _MHA_PLANES_WS[key] = torch.zeros(max(16, _lib.size_query("lvc_mha_workspace_bytes", B, N, num_heads)), dtype=torch.uint8, device=dev)
    planes, scale2 = pc.split2s()
    pc.last_one = True
    _launch(None, 0.0, 0.0, pc.slot, "lvc_conv1x1_qkv_planes_f16s1", lambda: lib.lvc_conv1x1_qkv_planes_f16s1(
        ptr(x), ptr(planes), ptr(scale2), ptr(pc.shift), ptr(ws), B, N, pc.C, num_heads, scale,
        ptr(_conv_error_view(dev)), ptr(conv_workspace(dev)), _stream(x)))
    out = torch.empty(B * N, num_heads * 64, device=dev, dtype=torch.float32)
    check(lib.lvc_mha_mfma_planes(ptr(ws), ptr(out), B, N, num_heads, _stream(x)), "lvc_mha_mfma_planes")
    return out


def mha_cls(qkv, B, N, num_heads, head_dim, scale):
    """qkv [B*N, 3*H*64] -> [B, H*64]: softmax(q_0 k^T scale) v for the class token of every image (the descriptor network's last block)."""
    _req_cuda(qkv)
    assert head_dim == 64      # more than 1024 keys: refused by the entry point
    qkv = qkv.contiguous()
    out = torch.empty(B, num_heads * head_dim, device=qkv.device, dtype=torch.float32)
    check(_lib.lib().lvc_mha_cls(ptr(qkv), ptr(out), B, N, num_heads, scale, _stream(qkv)), "lvc_mha_cls")
    return out


def mha(qkv, B, N, num_heads, head_dim, scale, mfma=None):
    """qkv [B*N, 3*H*head_dim] -> [B*N, H*head_dim] (softmax(q k^T scale) v per image and head).  Default: the matrix-core
    kernel (lvc_mha_mfma: fp32-accurate two-way fp16 split, probabilities kept in registers between the two products);
    mfma=False, or the range-free split (CONV_SPLIT "bf16x3"): the scalar fp32 kernel.  q * scale, k or v beyond fp16's range
    (or NaN) raises bit 1 of the shared conv error word, like the conv kernels' operands (`check_conv_error_word`)."""
    _req_cuda(qkv)
    qkv = qkv.contiguous()
    out = torch.empty(B * N, num_heads * head_dim, device=qkv.device, dtype=torch.float32)
    if ((MHA_MFMA and CONV_SPLIT == "f16x2") if mfma is None else mfma) and head_dim == 64:
        lib = _lib.lib()
        ws = torch.empty(max(16, _lib.size_query("lvc_mha_workspace_bytes", B, N, num_heads)), dtype=torch.uint8, device=qkv.device)
        check(lib.lvc_mha_mfma(ptr(qkv), ptr(out), ptr(ws), B, N, num_heads, scale,
                                   ptr(_conv_error_view(qkv.device)), _stream(qkv)), "lvc_mha_mfma")
        return out
    check(_lib.lib().lvc_mha(ptr(qkv), ptr(out), B, N, num_heads, head_dim, scale, _stream(qkv)),
          "lvc_mha")
    return out


# --------------------------------------------------------------------------- GroupNorm (csrc/group_norm.hip)
GN_SPLIT_MIN_HW = 512     # pixels per sample from which the statistics are split over row tiles (below: one workgroup owns whole samples)
GN_TILE_ROWS = None       # image rows per tile of the split regime; None: `_gn_tile_rows`
_GN_TARGET_WGS = 1024     # workgroups a split launch aims for (four per compute unit)
_GN_MIN_TILE_PIXELS = 128


def _gn_tile_rows(N, H, W):
    """0 = the whole-sample regime; else the tile height of the split regime."""
    if H * W < GN_SPLIT_MIN_HW:
        return 0
    if GN_TILE_ROWS is not None:
        return max(1, min(int(GN_TILE_ROWS), H))
    tiles = min(H, max(1, -(-_GN_TARGET_WGS // N)))
    return min(H, max(-(-H // tiles), -(-_GN_MIN_TILE_PIXELS // W)))


def _gn_workspace(x, N, H, W, C, G, rows, backward):
    nbytes = _lib.size_query("lvc_group_norm_workspace_bytes", N, H, W, C, G, rows, backward)
    return torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None, nbytes


def _gn_strides(x):
    return tuple(s for s in x.stride())


def group_norm_nhwc(x, gamma, beta, num_groups, eps=1e-5, relu=False, residual=None, res_mode=0):
    """x [N,H,W,C] fp32 -> (y, mean [N,G], rstd [N,G]);  y = act(GN(x)) (+ residual: res_mode 1 same shape, 2 the coarser map
    [N,(H+1)//2,(W+1)//2,C] nearest-x2-upsampled, as `conv2d_nhwc`'s res_mode).  Bad arguments (C % G, a non-contiguous x, ReLU
    with a residual) come back from the library as LvcNativeError."""
    _req_cuda(x, gamma, beta, residual)
    assert x.dim() == 4 and x.dtype == torch.float32 and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    N, H, W, C = x.shape
    G = int(num_groups)
    assert gamma.numel() == C and beta.numel() == C and gamma.is_contiguous() and beta.is_contiguous()
    if residual is not None:
        if res_mode == 0:
            res_mode = 1
        want = (N, H, W, C) if res_mode == 1 else (N, (H + 1) // 2, (W + 1) // 2, C)
        assert residual.dtype == torch.float32 and residual.is_contiguous() and tuple(residual.shape) == want, \
            "residual {} for res_mode {} must be {}".format(tuple(residual.shape), res_mode, want)
    else:
        res_mode = 0
    y = torch.empty((N, H, W, C), device=x.device, dtype=torch.float32)
    mean = torch.empty((N, G), device=x.device, dtype=torch.float32)
    rstd = torch.empty((N, G), device=x.device, dtype=torch.float32)
    if N == 0:
        return y, mean, rstd
    rows = _gn_tile_rows(N, H, W)
    ws, nbytes = _gn_workspace(x, N, H, W, C, G, rows, 0)
    rc = _lib.lib().lvc_group_norm_fwd_nhwc(ptr(x), ptr(gamma), ptr(beta), ptr(residual), ptr(y), ptr(mean), ptr(rstd), N, H,
                                            W, C, G, *_gn_strides(x), eps, 1 if relu else 0,
                                            res_mode, rows, ptr(ws), nbytes, _stream(x))
    check(rc, "lvc_group_norm_fwd_nhwc")
    return y, mean, rstd


def group_norm_backward_nhwc(dy, x, mean, rstd, gamma, beta, num_groups, relu=False):
    """(dx [N,H,W,C], dgamma [C], dbeta [C]) of `group_norm_nhwc`; relu: rebuild the forward's mask from x, gamma, beta."""
    _req_cuda(dy, x, mean, rstd, gamma, beta)
    assert x.dim() == 4 and x.dtype == torch.float32 and dy.dtype == torch.float32 and dy.shape == x.shape
    dy = dy.contiguous()
    N, H, W, C = x.shape
    G = int(num_groups)
    dx = torch.empty((N, H, W, C), device=x.device, dtype=torch.float32)
    dgamma = torch.empty(C, device=x.device, dtype=torch.float32)
    dbeta = torch.empty(C, device=x.device, dtype=torch.float32)
    if N == 0:
        return dx, dgamma.zero_(), dbeta.zero_()
    rows = _gn_tile_rows(N, H, W)
    ws, nbytes = _gn_workspace(x, N, H, W, C, G, rows, 1)
    rc = _lib.lib().lvc_group_norm_bwd_nhwc(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(dx), ptr(dgamma), ptr(dbeta),
                                            N, H, W, C, G, *_gn_strides(x), 1 if relu else 0,
                                            rows, ptr(ws), nbytes, _stream(x))
    check(rc, "lvc_group_norm_bwd_nhwc")
    return dx, dgamma, dbeta


def upsample2_residual_grad(g, res_shape):
    """Gradient of the coarser map of a res_mode-2 add: the 2x2 down-sum of g [N,H,W,C] (`downsum2x2`; with an odd H / W, where the
    last row / column of the coarser map received one fine row / column only, lvc_upsample2_add_grad_nhwc)."""
    _req_cuda(g)
    g = g.contiguous()
    N, H, W, C = g.shape
    if H % 2 == 0 and W % 2 == 0 and C % 4 == 0:
        out = downsum2x2(g)
    else:
        out = torch.empty(N, (H + 1) // 2, (W + 1) // 2, C, device=g.device, dtype=torch.float32)
        check(_lib.lib().lvc_upsample2_add_grad_nhwc(ptr(g), ptr(out), N, H, W, C, _stream(g)),
              "lvc_upsample2_add_grad_nhwc")
    assert tuple(out.shape) == tuple(res_shape)
    return out


# --------------------------------------------------------------------------- Mask R-CNN inference
MASK_DECONV_CHANNELS = (64, 128, 192, 256)
PASTE_FIELDS = 8          # int64 words per job of lvc_paste_masks (include/lvc_amd.h)


def mask_deconv_check(cin, cmid):
    if cin not in MASK_DECONV_CHANNELS or cmid not in MASK_DECONV_CHANNELS:
        raise NotImplementedError("the mask head's deconvolution kernel takes channel counts of 64, 128, 192 or 256, got {} -> {} "
                                  "(MODEL.ROI_MASK_HEAD.CONV_DIM)".format(cin, cmid))


def pack_mask_deconv(weight):
    """ConvTranspose2d weight [Cin, Cmid, 2, 2] -> [4 * Cmid, Cin], row (dy*2+dx)*Cmid + co."""
    cin, cmid = weight.shape[0], weight.shape[1]
    mask_deconv_check(cin, cmid)
    return weight.detach().permute(2, 3, 1, 0).reshape(4 * cmid, cin).contiguous().float()


def _upload_table(table, device):
    """A host int64 table as a device tensor: pinned and asynchronous, the upload is ordered on the stream and the host does not
    wait for the device."""
    return torch.from_numpy(table).pin_memory().to(device, non_blocking=True)


def _check_num_valid(num_valid):
    """The `num_valid` operand of the mask and keypoint kernels: None or ONE device int32."""
    if num_valid is not None:
        assert num_valid.dtype == torch.int32 and num_valid.numel() == 1


def _mask_tail_args(x, w_deconv, b_deconv, w_pred, b_pred, classes, num_valid):
    M, S, S_, cin = x.shape
    assert S == S_ and x.is_contiguous() and x.dtype == torch.float32
    cmid = w_deconv.shape[0] // 4
    mask_deconv_check(cin, cmid)
    Kc = w_pred.shape[0]
    assert w_deconv.shape == (4 * cmid, cin) and w_deconv.is_contiguous() and w_deconv.dtype == torch.float32
    w_pred = w_pred.reshape(Kc, -1)
    assert w_pred.shape == (Kc, cmid) and w_pred.is_contiguous() and w_pred.dtype == torch.float32
    for b, n in ((b_deconv, cmid), (b_pred, Kc)):
        assert b is None or (b.numel() == n and b.is_contiguous() and b.dtype == torch.float32)
    if classes is not None:
        assert classes.dtype == torch.int32 and classes.is_contiguous() and classes.numel() == M
    _check_num_valid(num_valid)
    return M, S, cin, cmid, Kc, w_pred


def _mask_deconv(entry, x, w_deconv, b_deconv, w_pred, b_pred, classes, num_valid, status, out):
    """The body of `mask_deconv_predict` and `mask_deconv_logits`: `entry` names the one of the two kernels, which share a signature."""
    _req_cuda(x, w_deconv, b_deconv, w_pred, b_pred, classes, num_valid, status)
    M, S, cin, cmid, Kc, w_pred = _mask_tail_args(x, w_deconv, b_deconv, w_pred, b_pred, classes, num_valid)
    if out is None:
        out = torch.empty(M, 2 * S, 2 * S, device=x.device, dtype=torch.float32)
    assert out.shape == (M, 2 * S, 2 * S) and out.is_contiguous() and out.dtype == torch.float32
    check(getattr(_lib.lib(), entry)(ptr(x), ptr(w_deconv), ptr(b_deconv), ptr(w_pred), ptr(b_pred), ptr(classes), ptr(num_valid),
                                     ptr(out), M, S, cin, cmid, Kc, ptr(status), _stream(x)), entry)
    return out


def mask_deconv_predict(x, w_deconv, b_deconv, w_pred, b_pred, classes=None, num_valid=None, status=None, out=None):
    """Deconv 2x2 s2 + bias + ReLU + 1x1 predictor of one class per row + bias + sigmoid (csrc/mask_deconv.hip).
    x [M,S,S,Cin] NHWC; w_deconv [4*Cmid,Cin] (`pack_mask_deconv`); w_pred [K,Cmid]; classes [M] int32 or None (class 0);
    num_valid: device int32, rows past it are neither read nor written.  Returns prob [M,2S,2S] (`out` when given)."""
    return _mask_deconv("lvc_mask_deconv_predict", x, w_deconv, b_deconv, w_pred, b_pred, classes, num_valid, status, out)


def paste_jobs(rows, boxes, sizes, offsets):
    """The host job table of `paste_masks`: rows [n] (row of prob), boxes [n,4] fp32 in output coordinates, sizes [n,2] = (out_h, out_w),
    offsets [n] = byte offset of each [out_h, out_w] plane.  -> int64 numpy [n, PASTE_FIELDS]."""
    import numpy as np

    n = len(rows)
    jobs = np.zeros((n, PASTE_FIELDS), dtype=np.int64)
    if n:
        jobs[:, 0] = np.asarray(rows, dtype=np.int64)
        jobs[:, 1:5] = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(n, 4)).view(np.uint32).astype(np.int64)
        jobs[:, 5:7] = np.asarray(sizes, dtype=np.int64).reshape(n, 2)
        jobs[:, 7] = np.asarray(offsets, dtype=np.int64)
    return jobs


def paste_masks(prob, jobs, out_bytes, threshold=0.5, out=None):
    """paste_masks_in_image for every job in one launch (csrc/mask_paste.hip).  prob [R, Sm, Sm] fp32; jobs: `paste_jobs`' table;
    out_bytes: the size of the uint8 output buffer the offsets refer to.  Returns the buffer (uint8 [out_bytes rounded up to 16]);
    bytes outside the jobs' planes are not written (the padding at the end of a fresh buffer stays as allocated)."""
    import numpy as np

    if not threshold >= 0:
        raise NotImplementedError("paste_masks: the threshold < 0 visualisation branch of the reference's paste_masks_in_image "
                                  "is not built")
    _req_cuda(prob)
    assert prob.dim() == 3 and prob.shape[1] == prob.shape[2] and prob.is_contiguous() and prob.dtype == torch.float32
    jobs = np.ascontiguousarray(jobs, dtype=np.int64).reshape(-1, PASTE_FIELDS)
    padded = (int(out_bytes) + 15) // 16 * 16
    if out is None:
        out = torch.empty(padded, dtype=torch.uint8, device=prob.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == padded
    n = jobs.shape[0]
    if n == 0:
        return out
    d_jobs = _upload_table(jobs, prob.device)
    check(_lib.lib().lvc_paste_masks(ptr(prob), prob.shape[0], prob.shape[1], c_void_p(jobs.ctypes.data), ptr(d_jobs),
                                     n, ptr(out), padded, threshold, _stream(prob)),
          "lvc_paste_masks")
    return out


# --------------------------------------------------------------------------- Keypoint R-CNN inference
KEYPOINT_DECONV_CIN = 16      # granularity of Cin in lvc_keypoint_deconv
KEYPOINT_DECONV_MAX_K = 64
KEYPOINT_MAX_SIDE = 64        # up * P of lvc_heatmaps_to_keypoints


def keypoint_deconv_check(cin, k):
    if cin < KEYPOINT_DECONV_CIN or cin % KEYPOINT_DECONV_CIN or cin > 4096:
        raise NotImplementedError("the keypoint head's transposed convolution takes input channels in multiples of {} (up to 4096), got {} "
                                  "(MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS)".format(KEYPOINT_DECONV_CIN, cin))
    if not 1 <= k <= KEYPOINT_DECONV_MAX_K:
        raise NotImplementedError("the keypoint head's transposed convolution takes 1 to {} keypoints, got {} "
                                  "(MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS)".format(KEYPOINT_DECONV_MAX_K, k))


def pack_keypoint_deconv(weight):
    """ConvTranspose2d weight [Cin, K, 4, 4] (kernel 4, stride 2, padding 1) -> the operand of `keypoint_deconv`:
    [4 parities][4 taps][K rounded up to 32][Cin] as rows of Cin floats (csrc/keypoint.hip)."""
    _req_cuda(weight)
    cin, k = weight.shape[0], weight.shape[1]
    keypoint_deconv_check(cin, k)
    assert tuple(weight.shape[2:]) == (4, 4), weight.shape
    w = weight.detach().contiguous().float()
    rows = _lib.lib().lvc_keypoint_deconv_packed_rows(k)
    packed = torch.empty(rows, cin, device=w.device, dtype=torch.float32)
    check(_lib.lib().lvc_keypoint_deconv_pack(ptr(w), ptr(packed), cin, k, _stream(w)), "lvc_keypoint_deconv_pack")
    return packed


def keypoint_deconv(x, packed, bias, num_keypoints, num_valid=None, out=None):
    """ConvTranspose2d(Cin, K, 4, stride 2, padding 1) + bias (csrc/keypoint.hip).  x [M,S,S,Cin] NHWC; packed: `pack_keypoint_deconv`;
    bias [K] or None; num_valid: device int32 [1], rows past it are neither read nor written.  Returns the planes [M,K,2S,2S]
    (`out` when given)."""
    _req_cuda(x, packed, bias, num_valid)
    M, S, S_, cin = x.shape
    k = int(num_keypoints)
    keypoint_deconv_check(cin, k)
    assert S == S_ and x.is_contiguous() and x.dtype == torch.float32
    rows = _lib.lib().lvc_keypoint_deconv_packed_rows(k)
    assert packed.shape == (rows, cin) and packed.is_contiguous() and packed.dtype == torch.float32
    assert bias is None or (bias.numel() == k and bias.is_contiguous() and bias.dtype == torch.float32)
    _check_num_valid(num_valid)
    if out is None:
        out = torch.empty(M, k, 2 * S, 2 * S, device=x.device, dtype=torch.float32)
    assert out.shape == (M, k, 2 * S, 2 * S) and out.is_contiguous() and out.dtype == torch.float32
    check(_lib.lib().lvc_keypoint_deconv(ptr(x), ptr(packed), ptr(bias), ptr(num_valid), ptr(out), M, S, cin,
                                         k, _stream(x)), "lvc_keypoint_deconv")
    return out


def heatmaps_to_keypoints(maps, rois, up=1, num_valid=None, maps_out=None, out=None):
    """heatmaps_to_keypoints of every (RoI, keypoint) in one launch (csrc/keypoint_decode.hip).  maps: planes [M,K,P,P]; rois [M,4];
    up 1 or 2 (2: the bilinear x2 map is formed on chip first); maps_out: None, or [M,K,up*P,up*P] to receive the decoded map;
    num_valid: device int32 [1], rows past it keep their bytes.  Among equal maxima the lowest flat index y*w + x wins.
    Returns [M,K,4] = (x, y, logit, score) (`out` when given)."""
    _req_cuda(maps, rois, num_valid, maps_out, out)
    assert maps.dim() == 4 and maps.shape[2] == maps.shape[3] and maps.is_contiguous() and maps.dtype == torch.float32, maps.shape
    M, k, P, _ = maps.shape
    if up not in (1, 2):
        raise NotImplementedError("heatmaps_to_keypoints: up = {} (1 or 2 are built)".format(up))
    if up * P > KEYPOINT_MAX_SIDE:
        raise NotImplementedError("heatmaps_to_keypoints: a heatmap of side {} (up to {} is built)".format(up * P, KEYPOINT_MAX_SIDE))
    assert rois.shape == (M, 4) and rois.is_contiguous() and rois.dtype == torch.float32, rois.shape
    _check_num_valid(num_valid)
    if maps_out is not None:
        assert maps_out.shape == (M, k, up * P, up * P) and maps_out.is_contiguous() and maps_out.dtype == torch.float32
    if out is None:
        out = torch.empty(M, k, 4, device=maps.device, dtype=torch.float32)
    assert out.shape == (M, k, 4) and out.is_contiguous() and out.dtype == torch.float32
    if M == 0 or k == 0:
        return out
    check(_lib.lib().lvc_heatmaps_to_keypoints(ptr(maps), ptr(rois), ptr(num_valid), ptr(maps_out), ptr(out), M, k, P,
                                               up, _stream(maps)), "lvc_heatmaps_to_keypoints")
    return out


# --------------------------------------------------------------------------- Mask R-CNN training
MASK_TABLE_FIELDS = 4    # int64 words per image of lvc_mask_targets' plane table (include/lvc_amd.h)


def mask_targets(boxes, matched, count, planes, mask_size, out=None):
    """BitMasks.crop_and_resize + >= 0.5 for the first count[b] rows of every image in one launch (csrc/mask_targets.hip).
    boxes [B,R,4] fp32; matched int64 [B,R]: the row's plane among its image's; count int32 [B] (or a strided [B] view, e.g. the
    sampler's cnt[:, 0]); planes: B tensors bool / uint8 [n_b, H_b, W_b], each contiguous on the device (sizes may differ).
    Returns uint8 [B*R, T, T] (`out` when given); rows past an image's count are not written.  No host read."""
    import numpy as np

    _req_cuda(boxes, matched, count, *planes)
    B, R, _ = boxes.shape
    T = int(mask_size)
    assert boxes.is_contiguous() and boxes.dtype == torch.float32 and boxes.shape == (B, R, 4)
    assert matched.dtype == torch.int64 and matched.is_contiguous() and matched.shape == (B, R)
    assert count.dtype == torch.int32 and count.dim() == 1 and count.shape[0] == B and len(planes) == B
    table = np.zeros((max(B, 1), MASK_TABLE_FIELDS), dtype=np.int64)
    for b, pl in enumerate(planes):
        assert pl.dim() == 3 and pl.is_contiguous() and pl.dtype in (torch.bool, torch.uint8), "planes: contiguous bool / uint8 [n,H,W]"
        table[b] = (pl.data_ptr() if pl.numel() else 0, pl.shape[0], pl.shape[1], pl.shape[2])
    if out is None:
        out = torch.empty(B * R, T, T, dtype=torch.uint8, device=boxes.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == (B * R, T, T)
    if B == 0 or R == 0:
        return out
    d_table = _upload_table(table, boxes.device)
    check(_lib.lib().lvc_mask_targets(ptr(boxes), ptr(matched), ptr(count), count.stride(0), c_void_p(table.ctypes.data), ptr(d_table),
                                      B, R, T, ptr(out), _stream(boxes)), "lvc_mask_targets")
    return out


def mask_deconv_logits(x, w_deconv, b_deconv, w_pred, b_pred, classes=None, num_valid=None, status=None, out=None):
    """`mask_deconv_predict` without the sigmoid: the logits [M,2S,2S] of each row's class (training: the ground-truth class)."""
    return _mask_deconv("lvc_mask_deconv_logits", x, w_deconv, b_deconv, w_pred, b_pred, classes, num_valid, status, out)


def mask_loss(logits, targets, num_valid=None):
    """Mean binary cross-entropy with logits over the rows below num_valid (csrc/mask_train.hip): logits fp32 [M,P,P], targets uint8 /
    bool [M,P,P].  -> (loss fp32 [1], sum float64 [1], counts int64 [3] = (incorrect, positive, false positive pixels)); no host read;
    0 when there is no row."""
    _req_cuda(logits, targets, num_valid)
    M, P, P_ = logits.shape
    assert P == P_ and P % 2 == 0 and logits.is_contiguous() and logits.dtype == torch.float32
    assert targets.shape == logits.shape and targets.is_contiguous() and targets.dtype in (torch.uint8, torch.bool)
    _check_num_valid(num_valid)
    lib = _lib.lib()
    nbytes = _lib.size_query("lvc_mask_loss_workspace_bytes", M, P // 2)
    dev = logits.device
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    check(lib.lvc_mask_loss(ptr(logits), ptr(targets), ptr(num_valid), M, P // 2, ptr(loss), ptr(total), ptr(counts), ptr(ws),
                            nbytes, _stream(logits)), "lvc_mask_loss")
    return loss, total, counts


def mask_deconv_grad(x, w_deconv, b_deconv, w_pred, classes, logits, targets, num_valid, upstream, status=None,
                     need_dx=True, need_dw=True):
    """The backward of the tail + loss (csrc/mask_train.hip): lvc_mask_deconv_grad, then dx = dh @ Wd on the forward GEMM kernel and
    dWd = dh^T @ x on lvc_mask_deconv_wgrad (neither reads a row of x past num_valid).  x [M,S,S,Cin]; w_deconv the packed operand [4*Cmid,Cin]; logits / targets [M,2S,2S];
    upstream: fp32 [1] ON THE DEVICE (the loss's incoming gradient, not read back).  -> (dx [M,S,S,Cin], dWd [Cin,Cmid,2,2], dbd [Cmid],
    dWp [K,Cmid], dbp [K]); dx / dWd None when not needed.  The one large intermediate is dh [M*S*S, 4*Cmid].  Bit-identical between runs."""
    _req_cuda(x, w_deconv, b_deconv, w_pred, classes, logits, targets, num_valid, upstream, status)
    M, S, cin, cmid, Kc, w_pred = _mask_tail_args(x, w_deconv, b_deconv, w_pred, None, classes, num_valid)
    assert logits.shape == (M, 2 * S, 2 * S) and logits.is_contiguous() and logits.dtype == torch.float32
    assert targets.shape == logits.shape and targets.is_contiguous() and targets.dtype in (torch.uint8, torch.bool)
    assert upstream.dtype == torch.float32 and upstream.numel() == 1
    dev = x.device
    lib = _lib.lib()
    nbytes = _lib.size_query("lvc_mask_deconv_grad_workspace_bytes", M, S, cmid)
    ws = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.float32, device=dev)
    dh = torch.empty(M * S * S, 4 * cmid, dtype=torch.float32, device=dev)
    dwp = torch.empty(Kc, cmid, dtype=torch.float32, device=dev)
    dbp = torch.empty(Kc, dtype=torch.float32, device=dev)
    dbd = torch.empty(cmid, dtype=torch.float32, device=dev)
    check(lib.lvc_mask_deconv_grad(ptr(x), ptr(w_deconv), ptr(b_deconv), ptr(w_pred), ptr(classes), ptr(logits), ptr(targets),
                                   ptr(num_valid), ptr(upstream), ptr(dh), ptr(dwp), ptr(dbp), ptr(dbd), M, S,
                                   cin, cmid, Kc, ptr(status), ptr(ws), ws.numel() * 4, _stream(x)),
          "lvc_mask_deconv_grad")
    dx = dwd = None
    if M > 0 and need_dx:       # dx = dh @ Wd_packed on the forward GEMM kernel (range-free split: unscaled gradients are tiny)
        dx = linear_backward(x.view(M * S * S, cin), w_deconv, dh, need_dx=True, need_dw=False)[0].view(M, S, S, cin)      # (x: its shape only)
    if M > 0 and need_dw:       # dWd = dh^T @ x: conv_wgrad joins its pixel slices with atomics, this product must be bit-stable
        wbytes = _lib.size_query("lvc_mask_deconv_wgrad_workspace_bytes", M, S, cin, cmid)
        wws = torch.empty(wbytes // 4, dtype=torch.float32, device=dev)
        dw = torch.empty(4 * cmid, cin, dtype=torch.float32, device=dev)
        check(lib.lvc_mask_deconv_wgrad(ptr(dh), ptr(x), ptr(num_valid), ptr(dw), M, S, cin, cmid, ptr(wws),
                                        wbytes, _stream(x)), "lvc_mask_deconv_wgrad")
        # packed row (dy*2+dx)*Cmid + co -> the parameter's [Cin, Cmid, 2, 2]
        dwd = dw.view(2, 2, cmid, cin).permute(3, 2, 0, 1).contiguous()
    if M == 0:
        dx = torch.zeros(0, S, S, cin, device=dev) if need_dx else None
        dwd = torch.zeros(cin, cmid, 2, 2, device=dev) if need_dw else None
    return dx, dwd, dbd, dwp, dbp


# --------------------------------------------------------------------------- Keypoint R-CNN training
KEYPOINT_TABLE_FIELDS = 2    # int64 words per image of lvc_keypoint_targets' keypoint table (include/lvc_amd.h)
KEYPOINT_TRAIN_MAX_S = 16    # lvc_keypoint_loss forms the [4S,4S] map in LDS: side at most 64, as the decode


def keypoint_targets(boxes, matched, count, keypoints, size, apply_selection=True):
    """Keypoints.to_heatmap and select_proposals_with_visible_keypoints for the first count[b] rows of every image in one launch
    (csrc/keypoint_targets.hip).  boxes [B,R,4] fp32; matched int64 [B,R]: the row's instance among its image's; count int32 [B] (or
    a strided [B] view); keypoints: B tensors fp32 [n_b,K,3] = (x, y, v), each contiguous on the device, gathered by the kernel.
    -> (target int32 [B*R,K], valid uint8 [B*R,K], selected uint8 [B*R], sel_count int32 [B]); with apply_selection valid is
    valid & selected[row].  Rows past an image's count are zero (allocated so; the kernel does not write them).  No host read."""
    import numpy as np

    _req_cuda(boxes, matched, count, *keypoints)
    B, R, _ = boxes.shape
    assert boxes.is_contiguous() and boxes.dtype == torch.float32 and boxes.shape == (B, R, 4)
    assert matched.dtype == torch.int64 and matched.is_contiguous() and matched.shape == (B, R)
    assert count.dtype == torch.int32 and count.dim() == 1 and count.shape[0] == B and len(keypoints) == B
    k = None
    table = np.zeros((max(B, 1), KEYPOINT_TABLE_FIELDS), dtype=np.int64)
    for b, kp in enumerate(keypoints):
        assert kp.dim() == 3 and kp.shape[2] == 3 and kp.is_contiguous() and kp.dtype == torch.float32, "keypoints: contiguous fp32 [n,K,3]"
        assert k is None or kp.shape[1] == k, "keypoints: every image with the same K"
        k = kp.shape[1]
        table[b] = (kp.data_ptr() if kp.numel() else 0, kp.shape[0])
    dev = boxes.device
    k = int(k or 1)
    target = torch.zeros(B * R, k, dtype=torch.int32, device=dev)
    valid = torch.zeros(B * R, k, dtype=torch.uint8, device=dev)
    selected = torch.zeros(B * R, dtype=torch.uint8, device=dev)
    sel_count = torch.zeros(B, dtype=torch.int32, device=dev)
    if B == 0:
        return target, valid, selected, sel_count
    d_table = _upload_table(table, dev)
    check(_lib.lib().lvc_keypoint_targets(ptr(boxes), ptr(matched), ptr(count), count.stride(0), c_void_p(table.ctypes.data),
                                          ptr(d_table), B, R, k, int(size), 1 if apply_selection else 0,
                                          ptr(target), ptr(valid), ptr(selected), ptr(sel_count), _stream(boxes)), "lvc_keypoint_targets")
    return target, valid, selected, sel_count


def keypoint_dlow_channels(k):
    """Channels of `keypoint_loss_grad`'s channels-last dlow: K rounded up to 4."""
    return (int(k) + 3) // 4 * 4


def _keypoint_entry_args(low, target, valid, num_valid):
    assert low.dim() == 4 and low.shape[2] == low.shape[3] and low.shape[2] % 2 == 0 and low.is_contiguous() and low.dtype == torch.float32
    M, k, P, _ = low.shape
    if P // 2 > KEYPOINT_TRAIN_MAX_S:
        raise NotImplementedError("keypoint loss: a pooled side of {} (up to {} is built: MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION)"
                                  .format(P // 2, KEYPOINT_TRAIN_MAX_S))
    keypoint_deconv_check(KEYPOINT_DECONV_CIN, k)
    assert target.dtype == torch.int32 and target.is_contiguous() and target.numel() == M * k
    assert valid.dtype == torch.uint8 and valid.is_contiguous() and valid.numel() == M * k
    _check_num_valid(num_valid)
    return M, k, P // 2


def keypoint_loss(low, target, valid, num_valid=None, normalizer=None, loss_weight=1.0, status=None, out=None):
    """Softmax cross-entropy over the bilinear x2 map of every valid (row, keypoint) (csrc/keypoint_train.hip).  low: planes
    [M,K,2S,2S] (`keypoint_deconv`); target int32 / valid uint8 [M,K]; normalizer: None = the counted valid entries, else the number.
    -> (loss fp32 [1], sum fp64 [1], count int64 [1], term fp64 [M,K], plane_max fp32 [M,K], plane_lse fp64 [M,K]); the last three are
    written for valid entries below num_valid only (`out`: those three tensors, else zeros).  Sets KEYPOINT_BAD_TARGET in `status`.
    No host read; count 0 gives a loss of exactly 0."""
    _req_cuda(low, target, valid, num_valid, status)
    M, k, S = _keypoint_entry_args(low, target, valid, num_valid)
    dev = low.device
    if out is None:
        out = (torch.zeros(M, k, dtype=torch.float64, device=dev), torch.zeros(M, k, dtype=torch.float32, device=dev),
               torch.zeros(M, k, dtype=torch.float64, device=dev))
    term, pmax, plse = out
    assert term.dtype == torch.float64 and pmax.dtype == torch.float32 and plse.dtype == torch.float64
    assert all(t.is_contiguous() and t.numel() == M * k for t in out)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    check(_lib.lib().lvc_keypoint_loss(ptr(low), ptr(target), ptr(valid), ptr(num_valid), M, k, S,
                                       0.0 if normalizer is None else float(normalizer), float(loss_weight),
                                       ptr(term), ptr(pmax), ptr(plse), ptr(loss), ptr(total), ptr(count), ptr(status), _stream(low)),
          "lvc_keypoint_loss")
    return loss, total, count, term, pmax, plse


def keypoint_loss_grad(low, target, valid, pmax, plse, count, upstream, num_valid=None, normalizer=None, loss_weight=1.0, out=None):
    """dlow of `keypoint_loss`: the adjoint of the bilinear x2 applied to (softmax - onehot) * upstream / normaliser * loss_weight
    (csrc/keypoint_train.hip).  pmax / plse / count: `keypoint_loss`'s; upstream: fp32 [1] ON THE DEVICE.  -> dlow, CHANNELS-LAST
    [M,2S,2S,Kc] with Kc = `keypoint_dlow_channels(K)` (padding channels zero; rows past num_valid are not written)."""
    _req_cuda(low, target, valid, pmax, plse, count, upstream, num_valid)
    M, k, S = _keypoint_entry_args(low, target, valid, num_valid)
    assert pmax.dtype == torch.float32 and plse.dtype == torch.float64 and pmax.numel() == M * k and plse.numel() == M * k
    assert count.dtype == torch.int64 and count.numel() == 1 and upstream.dtype == torch.float32 and upstream.numel() == 1
    kc = keypoint_dlow_channels(k)
    if out is None:
        out = torch.empty(M, 2 * S, 2 * S, kc, dtype=torch.float32, device=low.device)
    assert out.shape == (M, 2 * S, 2 * S, kc) and out.is_contiguous() and out.dtype == torch.float32
    check(_lib.lib().lvc_keypoint_loss_grad(ptr(low), ptr(target), ptr(valid), ptr(pmax), ptr(plse), ptr(count), ptr(upstream),
                                            ptr(num_valid), M, k, S,
                                            0.0 if normalizer is None else float(normalizer), float(loss_weight),
                                            ptr(out), _stream(low)), "lvc_keypoint_loss_grad")
    return out


def pack_keypoint_deconv_dx(weight):
    """ConvTranspose2d weight [Cin, K, 4, 4] -> the weight operand of `keypoint_deconv_dx`: [Cin][16*Kc], column (ky*4+kx)*Kc + k."""
    _req_cuda(weight)
    cin, k = weight.shape[0], weight.shape[1]
    keypoint_deconv_check(cin, k)
    assert tuple(weight.shape[2:]) == (4, 4), weight.shape
    w = weight.detach().contiguous().float()
    packed = torch.empty(cin, 16 * keypoint_dlow_channels(k), device=w.device, dtype=torch.float32)
    check(_lib.lib().lvc_keypoint_deconv_dx_pack(ptr(w), ptr(packed), cin, k, _stream(w)), "lvc_keypoint_deconv_dx_pack")
    return packed


def unpack_keypoint_deconv_dx(packed, k):
    """The packing of `pack_keypoint_deconv_dx` back to the parameter's [Cin, K, 4, 4] (a layout change of dW, 16*K*Cin floats)."""
    cin, kc = packed.shape[0], keypoint_dlow_channels(k)
    return packed.view(cin, 16, kc)[:, :, :k].permute(0, 2, 1).reshape(cin, k, 4, 4).contiguous()


def keypoint_deconv_dx(dlow, packed, num_keypoints, num_valid=None, out=None):
    """The backward of `keypoint_deconv` into its input on fp32 MFMA (csrc/keypoint_train.hip): dlow channels-last [M,2S,2S,Kc];
    packed: `pack_keypoint_deconv_dx`.  -> dx [M,S,S,Cin] (`out` when given, else zeros: rows past num_valid are not written)."""
    _req_cuda(dlow, packed, num_valid, out)
    k = int(num_keypoints)
    kc = keypoint_dlow_channels(k)
    M, P, P_, kc_ = dlow.shape
    cin = packed.shape[0]
    keypoint_deconv_check(cin, k)
    assert P == P_ and P % 2 == 0 and kc_ == kc and dlow.is_contiguous() and dlow.dtype == torch.float32, dlow.shape
    assert packed.shape == (cin, 16 * kc) and packed.is_contiguous() and packed.dtype == torch.float32
    _check_num_valid(num_valid)
    S = P // 2
    if out is None:
        out = torch.zeros(M, S, S, cin, device=dlow.device, dtype=torch.float32)
    assert out.shape == (M, S, S, cin) and out.is_contiguous() and out.dtype == torch.float32
    check(_lib.lib().lvc_keypoint_deconv_dx(ptr(dlow), ptr(packed), ptr(num_valid), ptr(out), M, S, cin, k,
                                            _stream(dlow)), "lvc_keypoint_deconv_dx")
    return out


def keypoint_deconv_wgrad(x, dlow, num_keypoints, num_valid=None):
    """The backward of `keypoint_deconv` into weight and bias on fp32 MFMA, ordered slices (csrc/keypoint_train.hip).  x [M,S,S,Cin];
    dlow channels-last [M,2S,2S,Kc].  -> (dW [Cin,K,4,4], db [K]); bit-identical between runs."""
    _req_cuda(x, dlow, num_valid)
    k = int(num_keypoints)
    kc = keypoint_dlow_channels(k)
    M, S, S_, cin = x.shape
    keypoint_deconv_check(cin, k)
    assert S == S_ and x.is_contiguous() and x.dtype == torch.float32
    assert dlow.shape == (M, 2 * S, 2 * S, kc) and dlow.is_contiguous() and dlow.dtype == torch.float32, dlow.shape
    _check_num_valid(num_valid)
    lib = _lib.lib()
    nbytes = _lib.size_query("lvc_keypoint_deconv_wgrad_workspace_bytes", M, S, cin, k)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
    dw = torch.empty(cin, 16 * kc, dtype=torch.float32, device=x.device)
    db = torch.empty(k, dtype=torch.float32, device=x.device)
    check(lib.lvc_keypoint_deconv_wgrad(ptr(x), ptr(dlow), ptr(num_valid), ptr(dw), ptr(db), M, S, cin, k,
                                        ptr(ws), ws.numel() * 8, _stream(x)), "lvc_keypoint_deconv_wgrad")
    return unpack_keypoint_deconv_dx(dw, k), db


# --------------------------------------------------------------------------- semantic head and panoptic combine (csrc/sem_seg.hip)
# The entries of include/lvc_amd_seg.h.
SEG_POST_FIELDS = 9          # int64 words per job of lvcseg_sem_seg_postprocess
SEG_COMBINE_FIELDS = 9       # int64 words per image of lvcseg_panoptic_combine
SEG_SEGMENT_FIELDS = 8       # int32 words per row of its segment table
SEG_MAX_INSTANCES = 1024
SEG_MAX_LABELS = 4096


def upsample2_bilinear_nhwc(x, acc=None, out=None):
    """nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) on NHWC fp32 in one launch: up2(x), or acc + up2(x) with
    the accumulator added last (`out` may be `acc`).  x [N,H,W,C], C % 4 == 0 -> [N,2H,2W,C]."""
    _req_cuda(x, acc, out)
    assert x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()
    N, H, W, C = x.shape
    if out is None:
        out = torch.empty(N, 2 * H, 2 * W, C, device=x.device, dtype=torch.float32)
    for t in (acc, out):
        assert t is None or (t.shape == (N, 2 * H, 2 * W, C) and t.dtype == torch.float32 and t.is_contiguous())
    check(_lib.lib().lvcseg_upsample2_bilinear_nhwc(ptr(x), ptr(acc), ptr(out), N, H, W, C, _stream(x)),
          "lvcseg_upsample2_bilinear_nhwc")
    return out


def sem_seg_jobs(low_sizes, image_sizes, out_sizes, num_classes, ld, low_offsets=None):
    """The host job table of `sem_seg_postprocess`, one row per image: low_sizes [(h, w)] of the low-resolution logits, image_sizes
    [(h, w)] the crop of the upsampled map, out_sizes [(h, w)].  The images' logits follow each other in one buffer (low_offsets: their
    offsets in floats, default packed [h, w, ld] blocks), their soft planes [K, out_h, out_w] and label maps [out_h, out_w] are packed
    in this order.  -> (int64 numpy [n, SEG_POST_FIELDS], soft_numel, labels_numel)."""
    import numpy as np

    n = len(low_sizes)
    jobs = np.zeros((n, SEG_POST_FIELDS), dtype=np.int64)
    low = soft = lab = 0
    for i in range(n):
        (h, w), (ih, iw), (oh, ow) = low_sizes[i], image_sizes[i], out_sizes[i]
        jobs[i] = [low if low_offsets is None else low_offsets[i], h, w, ih, iw, oh, ow, soft, lab]
        low += h * w * ld
        soft += num_classes * oh * ow
        lab += oh * ow
    return jobs, soft, lab


def sem_seg_postprocess(logits, jobs, num_classes, scale, soft_numel, labels_numel, want_soft=True, want_labels=True, soft=None,
                        labels=None, ld=None):
    """F.interpolate(scale_factor=scale) -> crop -> F.interpolate(size=output) -> argmax for a batch in one launch, without the
    intermediate maps.  logits: fp32, `ld` floats per pixel (default: its last dimension), only the first num_classes are read; jobs:
    `sem_seg_jobs`' table.  -> (soft fp32 [soft_numel] or None, labels uint8 (int32 above 256 classes) [labels_numel] or None);
    elements outside the jobs' planes are not written."""
    import numpy as np

    _req_cuda(logits, soft, labels)
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    assert want_soft or want_labels
    K, ld = int(num_classes), int(logits.shape[-1] if ld is None else ld)
    jobs = np.ascontiguousarray(jobs, dtype=np.int64).reshape(-1, SEG_POST_FIELDS)
    label_dtype = torch.uint8 if K <= 256 else torch.int32
    if want_soft and soft is None:
        soft = torch.empty(int(soft_numel), device=logits.device, dtype=torch.float32)
    if want_labels and labels is None:
        labels = torch.empty(int(labels_numel), device=logits.device, dtype=label_dtype)
    assert soft is None or (soft.dtype == torch.float32 and soft.is_contiguous())
    assert labels is None or (labels.dtype in (torch.uint8, torch.int32) and labels.is_contiguous())
    if jobs.shape[0] == 0:
        return soft, labels
    d_jobs = _upload_table(jobs, logits.device)
    check(_lib.lib().lvcseg_sem_seg_postprocess(ptr(logits), logits.numel(), c_void_p(jobs.ctypes.data), ptr(d_jobs), jobs.shape[0],
                                                K, ld, int(scale), ptr(soft), 0 if soft is None else soft.numel(), ptr(labels),
                                                0 if labels is None else labels.numel(),
                                                4 if labels is not None and labels.dtype == torch.int32 else 1, _stream(logits)),
          "lvcseg_sem_seg_postprocess")
    return soft, labels


def panoptic_combine(planes, plane_jobs, counts, sizes, scores, classes, score_offsets, labels, label_offsets, num_labels,
                     overlap_thresh, stuff_area_limit, instances_thresh, use_boxes=True):
    """combine_semantic_and_instance_outputs for a batch in one launch (one workgroup per image), nothing read back.
    planes: uint8 buffer of 0 / 1 planes [h, w]; plane_jobs: their `paste_jobs` table (image after image; counts [B] instances per
    image); sizes [(h, w)]; scores fp32 / classes int32 device tensors, score_offsets [B] the index of each image's first instance in
    them; labels uint8 / int32 buffer with each image's [h, w] map at label_offsets [B]; use_boxes: scan a plane inside its job's box
    only (planes of `paste_masks` with a positive threshold are zero outside it).
    -> (panoptic int32 [sum h*w], image after image; segments int32 [rows, SEG_SEGMENT_FIELDS]; seg_counts int32 [B]; pan_offsets,
    seg_offsets: host lists)."""
    import numpy as np

    _req_cuda(planes, scores, classes, labels)
    B = len(sizes)
    plane_jobs = np.ascontiguousarray(plane_jobs, dtype=np.int64).reshape(-1, PASTE_FIELDS)
    assert labels.dtype in (torch.uint8, torch.int32) and labels.is_contiguous()
    assert scores.dtype == torch.float32 and classes.dtype == torch.int32 and scores.is_contiguous() and classes.is_contiguous()
    assert planes is None or (planes.dtype == torch.uint8 and planes.is_contiguous())
    images = np.zeros((B, SEG_COMBINE_FIELDS), dtype=np.int64)
    first = pan = rows = 0
    pan_offsets, seg_offsets = [], []
    for i, (h, w) in enumerate(sizes):
        n = int(counts[i])
        if n > SEG_MAX_INSTANCES:
            raise NotImplementedError("panoptic_combine: {} instances in one image, the kernel takes {} "
                                      "(TEST.DETECTIONS_PER_IMAGE)".format(n, SEG_MAX_INSTANCES))
        assert int(score_offsets[i]) + n <= scores.numel()
        images[i] = [first, n, h, w, label_offsets[i], pan, rows, n + num_labels, score_offsets[i]]
        pan_offsets.append(pan)
        seg_offsets.append(rows)
        first += n
        pan += h * w
        rows += n + num_labels
    dev = labels.device
    panoptic = torch.empty(pan, device=dev, dtype=torch.int32)
    segments = torch.empty(max(rows, 1), SEG_SEGMENT_FIELDS, device=dev, dtype=torch.int32)
    seg_counts = torch.empty(max(B, 1), device=dev, dtype=torch.int32)
    if B == 0:
        return panoptic, segments, seg_counts, pan_offsets, seg_offsets
    d_images = _upload_table(images, dev)
    d_planes = _upload_table(plane_jobs, dev) if plane_jobs.shape[0] else None
    check(_lib.lib().lvcseg_panoptic_combine(ptr(planes), 0 if planes is None else planes.numel(), c_void_p(plane_jobs.ctypes.data),
                                             ptr(d_planes), plane_jobs.shape[0], 1 if use_boxes else 0, ptr(scores), ptr(classes),
                                             ptr(labels), labels.numel(), 4 if labels.dtype == torch.int32 else 1, int(num_labels),
                                             c_void_p(images.ctypes.data), ptr(d_images), B, float(overlap_thresh),
                                             float(stuff_area_limit), float(instances_thresh), ptr(panoptic), panoptic.numel(),
                                             ptr(segments), rows, ptr(seg_counts), _stream(labels)),
          "lvcseg_panoptic_combine")
    return panoptic, segments, seg_counts, pan_offsets, seg_offsets


def segments_info(rows):
    """The reference's `segments_info` of one image from the rows of its segment table (host int32 numpy [count, SEG_SEGMENT_FIELDS])."""
    import numpy as np

    out = []
    for r in np.asarray(rows, dtype=np.int32):
        if r[1]:
            out.append({"id": int(r[0]), "isthing": True, "score": float(r[4:5].view(np.float32)[0]), "category_id": int(r[2]),
                        "instance_id": int(r[3])})
        else:
            out.append({"id": int(r[0]), "isthing": False, "category_id": int(r[2]), "area": int(r[5])})
    return out


# --------------------------------------------------------------------------- training the semantic branch (csrc/sem_seg_train.hip)
# The entries of include/lvc_amd_segtrain.h.
SEGTRAIN_LOSS_FIELDS = 3               # int64 words per image of the loss entries' job table
SEGTRAIN_STATUS_LABEL_RANGE = 1        # bit of the loss's status word: a label neither ignored nor in [0, K)


def upsample2_bilinear_bwd_nhwc(dy, out=None):
    """The adjoint of `upsample2_bilinear_nhwc` without accumulator: dy [N,2H,2W,C] -> dx [N,H,W,C], one gather launch, no atomics
    (two runs give the same bits)."""
    _req_cuda(dy, out)
    assert dy.dim() == 4 and dy.dtype == torch.float32 and dy.is_contiguous()
    N, H2, W2, C = dy.shape
    assert H2 % 2 == 0 and W2 % 2 == 0, dy.shape
    if out is None:
        out = torch.empty(N, H2 // 2, W2 // 2, C, device=dy.device, dtype=torch.float32)
    assert out.shape == (N, H2 // 2, W2 // 2, C) and out.dtype == torch.float32 and out.is_contiguous()
    check(_lib.lib().lvcst_upsample2_bilinear_bwd_nhwc(ptr(dy), ptr(out), N, H2 // 2, W2 // 2, C, _stream(dy)),
          "lvcst_upsample2_bilinear_bwd_nhwc")
    return out


def sem_seg_loss_jobs(label_sizes, offsets=None):
    """The host job table of the semantic loss, one row per image: label_sizes [(h, w)] of each image's own label map; the maps follow
    each other in one buffer (offsets: in elements, default packed).  -> (int64 numpy [n, SEGTRAIN_LOSS_FIELDS], labels_numel)."""
    import numpy as np

    jobs = np.zeros((len(label_sizes), SEGTRAIN_LOSS_FIELDS), dtype=np.int64)
    at = 0
    for i, (h, w) in enumerate(label_sizes):
        jobs[i] = [at if offsets is None else offsets[i], h, w]
        at += h * w
    return jobs, at


def _loss_labels_checked(labels, ignore_value):
    assert labels.dtype in (torch.uint8, torch.int64) and labels.is_contiguous(), "labels: a contiguous uint8 or int64 buffer"
    if labels.dtype == torch.uint8 and not 0 <= int(ignore_value) <= 255:
        raise ValueError("MODEL.SEM_SEG_HEAD.IGNORE_VALUE = {}: outside what uint8 labels hold".format(ignore_value))
    return 1 if labels.dtype == torch.uint8 else 8


def sem_seg_loss_fwd(logits, labels, jobs, num_classes, scale, ignore_value, status, ld=None, lse=None, d_jobs=None, maps=None):
    """F.cross_entropy(F.interpolate(logits, scale_factor=scale, bilinear), labels, "mean", ignore_index) without the interpolated
    tensor.  logits [N,h,w,ld] fp32 (the first num_classes channels are read); labels: one uint8 / int64 buffer that holds every image's
    own map where `jobs` (`sem_seg_loss_jobs`) says; status: an int32 [1] word the kernel ORs SEGTRAIN_STATUS_LABEL_RANGE into; lse: an
    fp32 [N,scale*h,scale*w] buffer for the per-pixel log-sum-exp, or None (the backward takes its two parts, `maps`).
    -> (loss fp32 [1], maps = (max, log-sum) fp32 [N,scale*h,scale*w] each, sum fp64 [1], count int64 [1], d_jobs); nothing is read back."""
    import numpy as np

    _req_cuda(logits, labels, status, lse)
    assert logits.dim() == 4 and logits.dtype == torch.float32 and logits.is_contiguous()
    N, h, w, last = logits.shape
    Kc, ld, scale = int(num_classes), int(last if ld is None else ld), int(scale)
    assert ld == last, "logits rows of ld floats"
    label_bytes = _loss_labels_checked(labels, ignore_value)
    jobs = np.ascontiguousarray(jobs, dtype=np.int64).reshape(-1, SEGTRAIN_LOSS_FIELDS)
    assert jobs.shape[0] == N and status.dtype == torch.int32 and status.numel() >= 1
    dev = logits.device
    if maps is None:
        maps = (torch.empty(N, scale * h, scale * w, device=dev, dtype=torch.float32),
                torch.empty(N, scale * h, scale * w, device=dev, dtype=torch.float32))
    for t in tuple(maps) + (lse,):
        assert t is None or (t.shape == (N, scale * h, scale * w) and t.dtype == torch.float32 and t.is_contiguous())
    nbytes = _lib.size_query("lvcst_sem_seg_loss_workspace_bytes", N, h, w, Kc, scale)
    ws = torch.empty(max(nbytes // 8, 1), device=dev, dtype=torch.float64)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    total = torch.empty(1, device=dev, dtype=torch.float64)
    count = torch.empty(1, device=dev, dtype=torch.int64)
    if d_jobs is None:
        d_jobs = _upload_table(jobs, dev) if N else None
    check(_lib.lib().lvcst_sem_seg_loss_fwd(ptr(logits), N, h, w, Kc, ld, scale, ptr(labels), labels.numel(), label_bytes,
                                            int(ignore_value), c_void_p(jobs.ctypes.data), ptr(d_jobs), ptr(maps[0]), ptr(maps[1]), ptr(lse),
                                            ptr(ws), ws.numel() * 8, ptr(loss), ptr(total), ptr(count), ptr(status), _stream(logits)),
          "lvcst_sem_seg_loss_fwd")
    return loss, tuple(maps), total, count, d_jobs


def sem_seg_loss_bwd(logits, labels, jobs, d_jobs, num_classes, scale, ignore_value, maps, g, count, out=None):
    """The gradient of `sem_seg_loss_fwd`'s loss times the device scalar g with respect to the logits: [N,h,w,ld], channels past
    num_classes zero.  maps, count: the forward's.  No atomics: two runs give the same bits."""
    import numpy as np

    mmax, lsum = maps
    _req_cuda(logits, labels, mmax, lsum, g, count, out)
    N, h, w, ld = logits.shape
    label_bytes = _loss_labels_checked(labels, ignore_value)
    jobs = np.ascontiguousarray(jobs, dtype=np.int64).reshape(-1, SEGTRAIN_LOSS_FIELDS)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and jobs.shape[0] == N
    for t in (mmax, lsum):
        assert t.shape == (N, int(scale) * h, int(scale) * w) and t.dtype == torch.float32 and t.is_contiguous()
    assert g.dtype == torch.float32 and g.numel() == 1 and count.dtype == torch.int64 and count.numel() == 1
    if out is None:
        out = torch.empty_like(logits)
    assert out.shape == logits.shape and out.dtype == torch.float32 and out.is_contiguous()
    check(_lib.lib().lvcst_sem_seg_loss_bwd(ptr(logits), N, h, w, int(num_classes), ld, int(scale), ptr(labels), labels.numel(),
                                            label_bytes, int(ignore_value), c_void_p(jobs.ctypes.data), ptr(d_jobs), ptr(mmax), ptr(lsum),
                                            ptr(g), ptr(count), ptr(out), _stream(logits)),
          "lvcst_sem_seg_loss_bwd")
    return out
