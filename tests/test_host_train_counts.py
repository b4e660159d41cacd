"""The counts a training step reads back, by name (roi_heads.pack_step_counts / unpack_step_counts), and the size-query helper of the
library loader (_lib.size_query).  No GPU: CPU tensors, and the `*_workspace_bytes` entries are host code."""
import ctypes

import pytest
import torch


def _parts(kind, B):
    """Distinct values per part, with the dtypes the step queues: the box counts, the loss kernels' counts and the valid count int64; the
    row counts and the status words int32."""
    box = torch.tensor([11, 12, 13, 14])
    if kind == "box":
        return {"box": box}, [box]
    status = torch.tensor([5], dtype=torch.int32)
    if kind == "mask":
        pixels, rows = torch.tensor([21, 22, 23]), torch.tensor([31], dtype=torch.int32)
        return ({"box": box, "mask.pixels": pixels, "mask.rows": rows, "mask.status": status},
                [box, pixels, rows.long(), status.long()])      # today's torch.cat([stats, mcounts, total.long(), status.long()])
    valid = torch.tensor([41])
    selected = torch.arange(B, dtype=torch.int32) + 50
    fg = torch.arange(B, dtype=torch.int32) + 60
    return ({"box": box, "keypoint.valid": valid, "keypoint.selected": selected, "keypoint.fg": fg, "keypoint.status": status},
            [box, valid, selected.long(), fg.long(), status.long()])      # torch.cat([stats, vcount, sel_count.long(), fg.long(), status.long()])


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("kind", ["box", "mask", "keypoint"])
def test_pack_and_unpack_step_counts(kind, B):
    from lvc_amd.modeling.roi_heads.roi_heads import pack_step_counts, unpack_step_counts

    parts, order = _parts(kind, B)
    vec, layout = pack_step_counts(parts)
    assert vec.dtype == torch.int64 and torch.equal(vec, torch.cat(order))
    assert layout == tuple((k, v.numel()) for k, v in parts.items())
    assert sum(n for _k, n in layout) == {"box": 4, "mask": 9, "keypoint": 4 + 2 * B + 2}[kind]
    named = unpack_step_counts(vec.tolist(), layout)
    assert list(named) == list(parts)
    for k, v in parts.items():
        assert named[k] == v.tolist() and len(named[k]) == v.numel(), k
    for wrong in (vec.tolist()[:-1], vec.tolist() + [0]):
        with pytest.raises(ValueError, match="unpack_step_counts"):
            unpack_step_counts(wrong, layout)


def test_a_single_part_is_not_copied():
    """A box-only model queues its four counts as they are: no concatenation launch."""
    from lvc_amd.modeling.roi_heads.roi_heads import pack_step_counts

    box = torch.tensor([1, 2, 3, 4])
    assert pack_step_counts({"box": box})[0].data_ptr() == box.data_ptr()


def test_size_query_returns_sizes_beyond_32_bits_and_refuses_negative_answers():
    from lvc_amd import _lib

    c_int = ctypes.c_int
    M, S, Cin, K = 1 << 20, 64, 4096, 64
    # csrc/keypoint_train.hip: slices * 16 * Kc * Cin * 4 bytes of tile partials + chunks * Kc * 8 bytes of bias partials, with
    # Kc = K rounded up to 4; rows = M S^2 cut into slices of 2048 unless that makes more than 64 -- then 64 slices; chunks of 512
    # low-resolution pixels (4 S^2 per row)
    rows = M * S * S
    assert (rows + 2047) // 2048 > 64
    slices, kc = 64, (K + 3) // 4 * 4
    chunks = (M * 4 * S * S + 511) // 512
    want = slices * 16 * kc * Cin * 4 + chunks * kc * 8
    assert want > 1 << 31
    got = _lib.size_query("lvc_keypoint_deconv_wgrad_workspace_bytes", c_int(M), c_int(S), c_int(Cin), c_int(K))
    assert type(got) is int and got == want
    with pytest.raises(_lib.LvcNativeError, match="lvc_keypoint_deconv_wgrad_workspace_bytes"):
        _lib.size_query("lvc_keypoint_deconv_wgrad_workspace_bytes", c_int(-1), c_int(S), c_int(Cin), c_int(K))
