"""FrozenBatchNorm2d and GroupNorm, and `get_norm`.

FrozenBatchNorm2d: buffer-only per-channel affine (reference detectron2/layers/batch_norm.py:14-125).

y = x * (weight * rsqrt(running_var + eps)) + (bias - running_mean * weight * rsqrt(running_var + eps)).
Every shipped config uses it for the whole backbone (`RESNETS.NORM = FrozenBN`, reference
detectron2/config/defaults.py:471), in training too, so `lvc_amd.layers.Conv2d` folds it into the
epilogue of the conv kernel; this module only owns the four buffers (state_dict names `weight`,
`bias`, `running_mean`, `running_var`) and is never launched on its own inside the trunk.
"""
import torch
from torch import nn


class FrozenBatchNorm2d(nn.Module):
    _version = 3

    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features) - eps)

    def affine(self):
        """(scale, shift) in fp32."""
        scale = self.weight * (self.running_var + self.eps).rsqrt()
        return scale, self.bias - self.running_mean * scale

    def forward(self, x):
        # stand-alone use (outside Conv2d) is not on the hot path; plain broadcast arithmetic.
        scale, shift = self.affine()
        return x * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:
            # pre-v2 checkpoints carry no running stats (reference batch_norm.py:67-89)
            if prefix + "running_mean" not in state_dict:
                state_dict[prefix + "running_mean"] = torch.zeros_like(self.running_mean)
            if prefix + "running_var" not in state_dict:
                state_dict[prefix + "running_var"] = torch.ones_like(self.running_var)
        if version is not None and version < 3:
            state_dict[prefix + "running_var"] -= self.eps
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def __repr__(self):
        return "FrozenBatchNorm2d(num_features={}, eps={})".format(self.num_features, self.eps)


class _GroupNormFn(torch.autograd.Function):
    """y = act(GN(x)) (+ residual | + up2(residual)) as lvc_group_norm_fwd_nhwc; backward: lvc_group_norm_bwd_nhwc (dx, dgamma,
    dbeta; the ReLU mask is rebuilt from x), and for the residual dy itself (res_mode 1) or its 2x2 down-sum (res_mode 2)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, num_groups, eps, relu, res_mode):
        from .. import kernels as K

        y, mean, rstd = K.group_norm_nhwc(x, weight, bias, num_groups, eps, relu=relu, residual=residual, res_mode=res_mode)
        ctx.save_for_backward(x, mean, rstd, weight, bias)
        ctx.num_groups, ctx.relu, ctx.res_mode = num_groups, relu, res_mode
        ctx.res_shape = residual.shape if residual is not None else None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from .. import kernels as K

        x, mean, rstd, weight, bias = ctx.saved_tensors
        dy = dy.contiguous()
        dx, dw, db = K.group_norm_backward_nhwc(dy, x, mean, rstd, weight, bias, ctx.num_groups, relu=ctx.relu)
        dres = None
        if ctx.res_shape is not None and ctx.needs_input_grad[3]:
            dres = dy if ctx.res_mode == 1 else K.upsample2_residual_grad(dy, ctx.res_shape)
        return (dx if ctx.needs_input_grad[0] else None, dw if ctx.needs_input_grad[1] else None,
                db if ctx.needs_input_grad[2] else None, dres, None, None, None, None)


class GroupNorm(nn.GroupNorm):
    """torch.nn.GroupNorm's parameters (state_dict names `weight`, `bias`; `isinstance(m, torch.nn.GroupNorm)` holds for the
    solver's WEIGHT_DECAY_NORM groups) with the forward and backward on csrc/group_norm.hip.  `lvc_amd.layers.Conv2d` calls
    `forward_nhwc` on its conv's output: conv -> GN -> ReLU | (+ upsample-add), the reference's order (wrappers.py:83-99, fpn.py:125-133)."""

    def __init__(self, num_groups, num_channels, eps=1e-5):
        super().__init__(num_groups, num_channels, eps=eps, affine=True)

    def forward_nhwc(self, x, relu=False, residual=None, res_mode=0):
        """x [N,H,W,C] contiguous.  residual: res_mode 1 the output's shape, 2 the coarser map that is nearest-x2-upsampled."""
        from .. import kernels as K

        if residual is None:
            res_mode = 0
        elif res_mode == 0:
            res_mode = 1
        if torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad or self.bias.requires_grad
                                        or (residual is not None and residual.requires_grad)):
            return _GroupNormFn.apply(x, self.weight, self.bias, residual, self.num_groups, self.eps, bool(relu), res_mode)
        return K.group_norm_nhwc(x, self.weight, self.bias, self.num_groups, self.eps, relu=relu, residual=residual, res_mode=res_mode)[0]

    def forward(self, x):
        """NCHW drop-in of nn.GroupNorm.forward on the device."""
        from .layout import require_device, to_nchw_view, to_nhwc

        require_device(x, "GroupNorm")
        return to_nchw_view(self.forward_nhwc(to_nhwc(x)))


def get_norm(norm, out_channels):
    """reference batch_norm.py:127-150: "" -> None, "FrozenBN", "GN" (32 groups).  The batch-statistics norms ("BN", "SyncBN",
    "nnSyncBN", "naiveSyncBN") are not implemented."""
    if isinstance(norm, str):
        if len(norm) == 0:
            return None
        if norm == "GN":
            return GroupNorm(32, out_channels)
        if norm != "FrozenBN":
            raise NotImplementedError(
                "lvc_amd implements NORM='', 'FrozenBN' and 'GN'; got '{}'".format(norm))
        return FrozenBatchNorm2d(out_channels)
    return norm(out_channels)
