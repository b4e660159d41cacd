"""What the mask and the keypoint head share on their reference-signature training path: `Tail`, the stand-in for the logits neither
head forms, and the skeleton of `mask_rcnn_loss` / `keypoint_rcnn_loss`."""
import torch

from ... import kernels as K


class Tail:
    """What the head's `layers` returns in the reference -- the logits [M, maps, side, side] -- as the operands they would be computed
    from: `x` [M, S, S, C] (channels-last, after the head's 3x3 convs) and the head that owns the layers behind them."""

    def __init__(self, x, head):
        self.x, self.head = x, head

    @property
    def shape(self):
        M, S = self.x.shape[0], self.x.shape[1]
        return (M, self.head.num_maps, self.head.map_scale * S, self.head.map_scale * S)

    def size(self, dim):
        return self.shape[dim]


def tail_loss_of_instances(what, tail, instances, per_image, tail_loss):
    """`what`_rcnn_loss on a `Tail` whose rows correspond 1:1 to the concatenated `instances`: per_image(instances_i, side) -> the
    per-row target tensors of one image; tail_loss(the same tensors of all images, status) -> (loss, counts: int64 device tensor).
    -> (loss, the host values of counts and the status word from ONE read), or (0 with the graph of x, None) without an instance."""
    dev = tail.x.device
    rows = [per_image(p, tail.shape[2]) for p in instances if len(p) > 0]
    if len(rows) == 0:
        return tail.x.sum() * 0, None
    rows = [torch.cat(r, dim=0).to(dev).contiguous() for r in zip(*rows)]
    assert rows[-1].shape[0] == tail.x.shape[0], "{}_rcnn_loss: {} rows of features, {} instances".format(what, tail.x.shape[0], rows[-1].shape[0])
    status = K.new_status(dev)
    loss, counts = tail_loss(rows, status)
    return loss, torch.cat([counts, status.long()]).tolist()
