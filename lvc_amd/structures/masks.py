"""`BitMasks`: the ground-truth segmentation masks of one image as bitmaps (reference detectron2/structures/masks.py:84-222).

`tensor` is bool [N, H, W].  `crop_and_resize(boxes, mask_size)` -- the Mask R-CNN training targets -- runs on the target kernel
(csrc/mask_targets.hip): the planes are read as the bytes they are, never converted to fp32.  `PolygonMasks` is not built (its
rasterisation is pycocotools' frPoly): a dataset that stores polygons is read with INPUT.MASK_FORMAT "bitmask"."""
import torch


class BitMasks:
    def __init__(self, tensor):
        device = tensor.device if isinstance(tensor, torch.Tensor) else torch.device("cpu")
        tensor = torch.as_tensor(tensor, dtype=torch.bool, device=device)
        assert tensor.dim() == 3, tensor.size()
        self.image_size = tensor.shape[1:]
        self.tensor = tensor

    def to(self, *args, **kwargs):
        return BitMasks(self.tensor.to(*args, **kwargs))

    @property
    def device(self):
        return self.tensor.device

    def __getitem__(self, item):
        if isinstance(item, int):
            return BitMasks(self.tensor[item][None])
        m = self.tensor[item]
        assert m.dim() == 3, "Indexing on BitMasks with {} returns a tensor with shape {}!".format(item, m.shape)
        return BitMasks(m)

    def __iter__(self):
        yield from self.tensor

    def __repr__(self):
        return "{}(num_instances={})".format(self.__class__.__name__, len(self.tensor))

    def __len__(self):
        return self.tensor.shape[0]

    def nonempty(self):
        return self.tensor.flatten(1).any(dim=1)

    @staticmethod
    def from_polygon_masks(polygon_masks, height, width):
        raise NotImplementedError("BitMasks.from_polygon_masks: polygon rasterisation is not built; read the dataset with "
                                  "INPUT.MASK_FORMAT \"bitmask\"")

    def crop_and_resize(self, boxes, mask_size):
        """boxes [N, 4], one per mask -> bool [N, mask_size, mask_size]: ROIAlign((mask_size, mask_size), 1.0, 0, aligned=True) of each
        plane, >= 0.5 (one launch of lvc_mask_targets, nothing read back)."""
        from .. import kernels as K

        assert len(boxes) == len(self), "{} != {}".format(len(boxes), len(self))
        n = len(self)
        dev = self.tensor.device
        if n == 0:
            return torch.zeros(0, mask_size, mask_size, dtype=torch.bool, device=dev)
        boxes = boxes.to(device=dev, dtype=torch.float32).reshape(1, n, 4).contiguous()
        matched = torch.arange(n, device=dev, dtype=torch.int64).view(1, n)
        count = torch.full((1,), n, dtype=torch.int32, device=dev)
        out = K.mask_targets(boxes, matched, count, [self.tensor.contiguous()], mask_size)
        return out.view(torch.bool)

    def get_bounding_boxes(self):
        raise NotImplementedError

    @staticmethod
    def cat(bitmasks_list):
        assert isinstance(bitmasks_list, (list, tuple))
        assert len(bitmasks_list) > 0
        assert all(isinstance(b, BitMasks) for b in bitmasks_list)
        return type(bitmasks_list[0])(torch.cat([b.tensor for b in bitmasks_list], dim=0))
