"""Times the semantic half of Panoptic FPN on one MI355X and writes profiles/panoptic_bench.json.

8 images of 800 x 1333 (padded batch 800 x 1344, stride-4 maps 200 x 336), R50-FPN, 80 thing and 54 stuff classes, conditioned
synthetic weights.  Every figure is the median of REPS device-event timings; the legs of a group alternate inside one process, so
they share the machine's state.  Legs:

  head                 SemSegFPNHead.forward_nhwc: 9 conv + GN + ReLU blocks, 6 upsamples (3 of them adding into the level sum), predictor
  upsample_add         the six x2 upsample launches alone, on the head's shapes
  predictor            the padded 128 -> 64 pointwise conv alone
  post_labels / post_both      lvcseg_sem_seg_postprocess, labels only / soft logits + labels, output size = image size
  post_torch           the same work through PyTorch-ROCm: F.interpolate(x4) -> crop -> argmax per image (the yardstick; at equal sizes
                       the reference's second interpolate is the identity, and it is left out of the yardstick too)
  combine / combine_torch      lvcseg_panoptic_combine on the model's own planes and labels / the reference's loop on the same device tensors
  forward_panoptic / forward_mask    PanopticFPN.forward / the same model's Mask R-CNN forward (GeneralizedRCNN, no semantic branch)

    python scripts/bench_panoptic.py [--out profiles/panoptic_bench.json] [--reps 20] [--batch 8]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

COPY_RATE = 6.3e12      # bytes / s: the chip's measured copy rate the byte counts are held against


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def alternate(legs, reps):
    """{name: fn} -> {name: [ms]}: one timing of every leg per round, REPS rounds."""
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            out[name] += timed(fn, 1, warmup=0)
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def combine_torch(instances, labels, overlap, limit, conf):
    """The reference's combine_semantic_and_instance_outputs, statement for statement, on device tensors (detectron2
    panoptic_fpn.py:133-218)."""
    pan = torch.zeros_like(labels, dtype=torch.int32)
    order = torch.argsort(-instances.scores)
    cur, info = 0, []
    masks = instances.pred_masks.to(dtype=torch.bool, device=pan.device)
    for j in order:
        score = instances.scores[j].item()
        if score < conf:
            break
        mask = masks[j]
        area = mask.sum().item()
        if area == 0:
            continue
        inter = ((mask > 0) & (pan > 0)).sum().item()
        if inter * 1.0 / area > overlap:
            continue
        if inter > 0:
            mask = mask & (pan == 0)
        cur += 1
        pan[mask] = cur
        info.append({"id": cur, "isthing": True, "category_id": instances.pred_classes[j].item()})
    for label in torch.unique(labels).cpu().tolist():
        if label == 0:
            continue
        mask = (labels == label) & (pan == 0)
        area = mask.sum().item()
        if area < limit:
            continue
        cur += 1
        pan[mask] = cur
        info.append({"id": cur, "isthing": False, "category_id": label})
    return pan, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panoptic_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_panoptic.py measures on the GPU; there is no CPU path"

    from lvc_amd import kernels as K
    from lvc_amd.config.presets import panoptic_fpn
    from lvc_amd.modeling import build_model
    from lvc_amd.utils import synthetic as syn

    B, H, W = args.batch, args.height, args.width
    model = syn.conditioned_panoptic_(build_model(panoptic_fpn()).eval())
    head = model.sem_seg_head
    Kc, ld, scale = head.num_classes, head.logits_ld, head.common_stride
    inputs = [{"image": syn.synthetic_image(1 + i, H, W).cuda()} for i in range(B)]
    res = {"batch": B, "image": [H, W], "classes": Kc, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        x4, sizes = model.preprocess_nhwc(inputs)
        feats = model.backbone.forward_nhwc(x4)
        logits = head.forward_nhwc(feats)
        N, h, w, _ = logits.shape
        res["logits"] = [N, h, w, ld]

        # ---- head, its upsamples, its predictor
        ups = []      # (x, acc) of the six upsample launches, on the head's shapes
        for f, seq in zip(head.in_features, head.scale_heads):
            n_up = sum(type(m).__name__ == "Upsample2" for m in seq)
            fh, fw = feats[f].shape[1:3]
            for k in range(n_up):
                x = torch.randn(N, fh << k, fw << k, 128, device="cuda")
                acc = torch.randn(N, fh << (k + 1), fw << (k + 1), 128, device="cuda") if k == n_up - 1 else None
                ups.append((x, acc))
        summed = torch.randn(N, h, w, 128, device="cuda")
        pc = head.packed_predictor()
        legs = {"head": lambda: head.forward_nhwc(feats),
                "upsample_add": lambda: [K.upsample2_bilinear_nhwc(x, acc=a, out=a) for x, a in ups],
                "predictor": lambda: K.conv2d_nhwc(summed, pc, relu=False)}
        t = alternate(legs, args.reps)
        res.update({k: summary(v) for k, v in t.items()})
        up_bytes = sum(4 * (x.numel() + (2 if a is not None else 1) * 4 * x.numel()) for x, a in ups)
        res["upsample_add"]["bytes"] = up_bytes
        res["upsample_add"]["share_of_copy_rate"] = up_bytes / COPY_RATE / (res["upsample_add"]["median_ms"] * 1e-3)

        # ---- postprocess
        out_sizes = [tuple(s) for s in sizes]
        jobs, soft_numel, labels_numel = K.sem_seg_jobs([(h, w)] * N, out_sizes, out_sizes, Kc, ld)
        soft = torch.empty(soft_numel, device="cuda")
        labels = torch.empty(labels_numel, device="cuda", dtype=torch.uint8)

        def post_torch():
            out = []
            for i, (ih, iw) in enumerate(out_sizes):
                x = logits[i, :, :, :Kc].permute(2, 0, 1)[None]
                out.append(F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False)[0, :, :ih, :iw].argmax(0))
            return out

        legs = {"post_labels": lambda: K.sem_seg_postprocess(logits, jobs, Kc, scale, 0, labels_numel, want_soft=False, labels=labels),
                "post_both": lambda: K.sem_seg_postprocess(logits, jobs, Kc, scale, soft_numel, labels_numel, soft=soft, labels=labels),
                "post_torch": post_torch}
        t = alternate(legs, args.reps)
        res.update({k: summary(v) for k, v in t.items()})
        read = N * h * w * Kc * 4
        for name, written in (("post_labels", labels_numel), ("post_both", labels_numel + 4 * soft_numel)):
            res[name]["bytes_read"], res[name]["bytes_written"] = read, written
            res[name]["share_of_copy_rate"] = (read + written) / COPY_RATE / (res[name]["median_ms"] * 1e-3)
        want = post_torch()
        K.sem_seg_postprocess(logits, jobs, Kc, scale, 0, labels_numel, want_soft=False, labels=labels)
        differ = sum(int((labels[int(jobs[i, 8]): int(jobs[i, 8]) + ih * iw].view(ih, iw).long() != want[i]).sum())
                     for i, (ih, iw) in enumerate(out_sizes))
        res["post_labels"]["pixels_differing_from_torch"] = differ
        res["post_labels"]["pixels"] = labels_numel

        # ---- combine, on the model's own planes and labels
        model.__dict__.pop("_semantic", None)
        insts, planes = model._masks_and_planes(inputs, True)
        sem, lab, lab_off = model.__dict__.pop("_semantic")
        T = planes["scores"].shape[1]
        args_c = (planes["buffer"], planes["jobs"], planes["counts"], out_sizes, planes["scores"], planes["classes"], [i * T for i in range(B)],
                  lab, lab_off, Kc, model.combine_overlap_threshold, model.combine_stuff_area_limit,
                  model.combine_instances_confidence_threshold)
        label_maps = [lab[o: o + ih * iw].view(ih, iw).long() for o, (ih, iw) in zip(lab_off, out_sizes)]

        def combine_ours():
            pan, seg, cnt, _, _ = K.panoptic_combine(*args_c)
            return torch.cat([cnt[:B], seg.view(-1)]).cpu()      # with its read, as the yardstick's loop reads

        legs = {"combine": combine_ours,
                "combine_torch": lambda: [combine_torch(r, l, *args_c[-3:]) for r, l in zip(insts, label_maps)]}
        t = alternate(legs, args.reps)
        res.update({k: summary(v) for k, v in t.items()})
        res["combine"]["instances"] = [int(c) for c in planes["counts"]]
        pan, seg, cnt, pan_off, seg_off = K.panoptic_combine(*args_c)
        ref = [combine_torch(r, l, *args_c[-3:]) for r, l in zip(insts, label_maps)]
        res["combine"]["equal_to_torch_loop"] = all(
            torch.equal(pan[o: o + ih * iw].view(ih, iw), p) for o, (ih, iw), (p, _) in zip(pan_off, out_sizes, ref))
        res["combine"]["segments"] = [int(c) for c in cnt[:B].tolist()]

        # ---- the whole forward with and without the semantic branch
        legs = {"forward_panoptic": lambda: model(inputs),
                "forward_mask": lambda: mask_forward(model, inputs)}
        t = alternate(legs, args.reps)
        res.update({k: summary(v) for k, v in t.items()})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


def mask_forward(model, inputs):
    """The Mask R-CNN forward of the same model: `_inference_masks` with the semantic hook switched off."""
    hook = type(model)._on_features
    type(model)._on_features = lambda self, *a: None
    try:
        return model._inference_masks(inputs, True)
    finally:
        type(model)._on_features = hook


if __name__ == "__main__":
    main()
