"""Training-sample transforms on the GPU, behind PyMIC's transform interface.

Mirrors the classes FPL+'s configs name (config_dual/data_vs/vs_t1s_g.cfg:21-23:
train_transform = [NormalizeWithMeanStd, Pad, RandomCrop, RandomFlip, LabelToProbability]) and the geometric augmentation
a user of the reference adds first (RandomRotate, Rescale, RandomRescale: rotate.py, rescale.py) and the intensity family
(min-max / percentile normalisation, thresholding, gamma correction, Gaussian noise: normalize.py, threshold.py, intensity.py)
and the crop, bounding-box and label family (CenterCrop, CropWithBoundingBox, RandomResizedCrop, LabelConvert,
LabelConvertNonzero, PartialLabelToProbability, ReduceLabelDim, GrayscaleToRGB: crop.py, label_convert.py) - all 23 names of
the reference's TransformDict:
same class names, same lower-cased parameter keys (PyMIC/pymic/transform/*.py), same `__call__(sample) -> sample`
contract and the same `<Name>_Param` json strings in the sample, so `TransformDict[name](params)` drops in for
PyMIC/pymic/transform/trans_dict.py:42.  The difference is where the volumes live: `sample['image']` (float32
[C,D,H,W]), `sample['label']` (uint8 [1,D,H,W]) and `sample['pixel_weight']` (float32 [1,D,H,W]) are device tensors
and every gather / reduction / interpolation is a HIP kernel (csrc/sample.hip, csrc/resample.hip, csrc/intensity.hip, csrc/crop_label.hip).  The random decisions
are drawn on the host from Python's `random` (RandomRotate: numpy's global generator) in exactly the reference's order,
so a seeded run picks the same crops, flips, angles and ratios as the reference.
"""
import json
import math
import random
from fractions import Fraction

import numpy as np

import torch

from . import ops

_SPATIAL_KEYS = ("label", "pixel_weight", "image1")


class AbstractTransform(object):
    """PyMIC/pymic/transform/abstract_transform.py:4-27"""

    def __init__(self, params):
        self.task = params['task']

    def __call__(self, sample):
        return sample

    def inverse_transform_for_prediction(self, sample):
        raise ValueError("not implemented")

    def _others(self, sample):
        if self.task != 'segmentation':
            return []
        return [k for k in _SPATIAL_KEYS if k in sample]


def _check_volume(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 4):
        raise ValueError("fplx.transform: sample['{0:}'] must be a [C,D,H,W] device tensor".format(name))
    return t.contiguous()


class NormalizeWithMeanStd(AbstractTransform):
    """normalize.py:34-68.  mean/std None -> each channel's own float32 mean and population std."""

    def __init__(self, params):
        super(NormalizeWithMeanStd, self).__init__(params)
        self.chns = params['normalizewithmeanstd_channels']
        self.mean = params.get('normalizewithmeanstd_mean', None)
        self.std = params.get('normalizewithmeanstd_std', None)
        self.ignore_np = params.get('normalizewithmeanstd_ignore_non_positive', False)
        self.inverse = params.get('normalizewithmeanstd_inverse', False)

    def __call__(self, sample):
        image = _check_volume(sample['image'], 'image')
        chns = self.chns if self.chns is not None else range(image.shape[0])
        if self.mean is None:
            self.mean = [None] * len(chns)
            self.std = [None] * len(chns)
        for i, chn in enumerate(chns):
            ms = None if self.mean[i] is None else (self.mean[i], self.std[i])
            if self.ignore_np:
                # normalize.py:55-66: moments over the positive voxels (only when none are given), the others replaced by
                # numpy.random.normal(0, 1) - drawn on the host from numpy's global generator for the WHOLE channel, as the
                # reference does, so that a seeded run reproduces its numbers
                noise = torch.from_numpy(np.random.normal(0, 1, size=tuple(image[chn].shape)).astype(np.float32))
                noise = noise.to(image.device)
                if ms is None:
                    ops.normalize_positive(image[chn], noise, out=image[chn])
                else:
                    keep = ~(image[chn] <= 0)
                    ops.normalize_mean_std(image[chn], ms, out=image[chn])
                    image[chn] = torch.where(keep, image[chn], noise)
                continue
            ops.normalize_mean_std(image[chn], ms, out=image[chn])      # in place, like the reference
        sample['image'] = image
        return sample


class Pad(AbstractTransform):
    """pad.py:117-191: reflect padding to max(image_size, output_size), lower margin int(margin / 2)."""

    def __init__(self, params):
        super(Pad, self).__init__(params)
        self.output_size = params['pad_output_size']
        self.ceil_mode = params.get('pad_ceil_mode', False)
        self.inverse = params.get('pad_inverse', True)

    def __call__(self, sample):
        image = _check_volume(sample['image'], 'image')
        shape = image.shape
        assert len(self.output_size) == 3
        if self.ceil_mode:
            out = [int(math.ceil(float(shape[1 + i]) / self.output_size[i])) * self.output_size[i] for i in range(3)]
        else:
            out = self.output_size
        margin = [max(0, out[i] - shape[1 + i]) for i in range(3)]
        lower = [int(margin[i] / 2) for i in range(3)]
        upper = [margin[i] - lower[i] for i in range(3)]
        sample['Pad_Param'] = json.dumps((lower, upper))
        if max(margin) == 0:
            return sample
        size = [shape[1 + i] + margin[i] for i in range(3)]
        sample['image'] = ops.pad_reflect(image, lower, size)
        for k in self._others(sample):
            sample[k] = ops.pad_reflect(_check_volume(sample[k], k), lower, size)
        return sample

    def inverse_transform_for_prediction(self, sample):
        p = sample['Pad_Param']
        lower, upper = json.loads(p[0] if isinstance(p, (list, tuple)) else p)

        def crop(pred):                                  # [N,C,D,H,W]
            n, c = pred.shape[:2]
            size = [pred.shape[2 + i] - lower[i] - upper[i] for i in range(3)]
            flat = pred.contiguous().view(n * c, *pred.shape[2:])
            return ops.crop_flip(flat, lower, size).view(n, c, *size)

        predict = sample['predict']
        sample['predict'] = [crop(q) for q in predict] if isinstance(predict, (tuple, list)) else crop(predict)
        return sample


def _check_tensor(t, name):
    """the rank-free form of _check_volume, for the classes that also take 2-D samples [C,H,W]"""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError("fplx.transform: sample['{0:}'] must be a device tensor".format(name))
    return t.contiguous()


class CenterCrop(AbstractTransform):
    """crop.py:13-108.  centercrop_output_size [D, H, W] (D None: the depth is kept); lower corner int(margin / 2).  Crops
    'image', 'label', 'pixel_weight' and 'image1'.  The inverse pastes a prediction (or each one of a list) back into
    zeros of the recorded shape; CropWithBoundingBox, RandomCrop and RandomResizedCrop derive from this class as in the
    reference, and the first two inherit the inverse.  An output size beyond the volume - the reference then slices from
    a negative start and returns a strip from the far end - is refused."""
    _name = 'CenterCrop'

    def __init__(self, params):
        super(CenterCrop, self).__init__(params)
        self.output_size = params['centercrop_output_size']
        self.inverse = params.get('centercrop_inverse', True)

    def _get_crop_param(self, sample):
        """-> sample (with the <Name>_Param string), lower corner [3], extent [3] of the block that is gathered"""
        shape = list(sample['image'].shape)
        assert len(self.output_size) == 3
        size = list(self.output_size)
        if size[0] is None:
            size[0] = shape[1]
        margin = [shape[i + 1] - size[i] for i in range(3)]
        if min(margin) < 0:
            raise ValueError("fplx.transform: CenterCrop output size {0:} exceeds the volume {1:}".format(size, shape[1:]))
        crop_min = [int(m / 2) for m in margin]
        crop_max = [crop_min[i] + size[i] for i in range(3)]
        sample['CenterCrop_Param'] = json.dumps((shape, [0] + crop_min, shape[0:1] + crop_max))
        return sample, crop_min, size

    def __call__(self, sample):
        image = _check_volume(sample['image'], 'image')
        sample, crop_min, size = self._get_crop_param(sample)
        sample['image'] = ops.crop_flip(image, crop_min, size)
        for k in self._others(sample):
            sample[k] = ops.crop_flip(_check_volume(sample[k], k), crop_min, size)
        return sample

    def inverse_transform_for_prediction(self, sample):
        origin_shape, crop_min, _ = _json_param(sample[self._name + '_Param'])
        # the block's extent is the prediction's own: a box that ran past the volume was truncated on the way in
        return _on_prediction(sample, lambda p: ops.paste_roi(p, crop_min[1:], origin_shape[1:]))


class CropWithBoundingBox(CenterCrop):
    """crop.py:110-167.  The box of the image's non-zero voxels over all channels (numpy.nonzero: a NaN counts, -0.0 does
    not) decides the crop: start None and output_size None -> the box itself; start None -> output_size centred on the
    box, clamped at 0; both given -> start and output_size as they are.  A box past the volume is truncated as a numpy
    slice is, while <Name>_Param keeps the untruncated numbers.  Refused: start with output_size None (the reference
    fails on len(None)) and an all-zero image (the reference fails on the minimum of an empty array)."""
    _name = 'CropWithBoundingBox'

    def __init__(self, params):
        self.start = params['cropwithboundingbox_start']
        self.output_size = params['cropwithboundingbox_output_size']
        self.inverse = params.get('cropwithboundingbox_inverse', True)
        self.task = params['task']
        if self.start is not None and self.output_size is None:
            raise ValueError("fplx.transform: CropWithBoundingBox_start needs CropWithBoundingBox_output_size")

    def _get_crop_param(self, sample):
        image = sample['image']
        shape = list(image.shape)
        count, bb_min, bb_max = ops.nonzero_bbox(image)
        if count == 0:
            raise ValueError("fplx.transform: CropWithBoundingBox on an all-zero image")
        bb_min, bb_max = bb_min[1:], bb_max[1:]
        if self.start is None:
            if self.output_size is None:
                crop_min, crop_max = bb_min, bb_max
            else:
                assert len(self.output_size) == 3
                crop_min = [int((bb_min[i] + bb_max[i] + 1) / 2) - int(self.output_size[i] / 2) for i in range(3)]
                crop_min = [max(0, crop_min[i]) for i in range(3)]
                crop_max = [crop_min[i] + self.output_size[i] for i in range(3)]
        else:
            assert len(self.start) == 3
            crop_min = list(self.start)
            crop_max = [crop_min[i] + self.output_size[i] for i in range(3)]
        sample['CropWithBoundingBox_Param'] = json.dumps((shape, [0] + crop_min, shape[0:1] + crop_max))
        size = [min(crop_max[i], shape[i + 1]) - crop_min[i] for i in range(3)]
        return sample, crop_min, size


class RandomCrop(CenterCrop):
    """crop.py:165-245.  Draw order: one randint per axis with a margin, then random() for the foreground focus,
    then one randint per axis inside the label's bounding box.  The inverse is CenterCrop's."""
    _name = 'RandomCrop'

    def __init__(self, params):
        self.output_size = params['randomcrop_output_size']
        self.fg_focus = params.get('randomcrop_foreground_focus', False)
        self.fg_ratio = params.get('randomcrop_foreground_ratio', 0.5)
        self.mask_label = params.get('randomcrop_mask_label', [1])
        self.inverse = params.get('randomcrop_inverse', True)
        self.task = params['task']
        assert isinstance(self.output_size, (list, tuple))
        if self.mask_label is not None:
            assert isinstance(self.mask_label, (list, tuple))

    def _get_crop_param(self, sample):
        shape = list(sample['image'].shape)
        assert len(self.output_size) == 3
        size = list(self.output_size)
        if size[0] is None:
            size[0] = shape[1]
        margin = [shape[i + 1] - size[i] for i in range(3)]
        crop_min = [0 if m == 0 else random.randint(0, m) for m in margin]
        if self.fg_focus and random.random() < self.fg_ratio:
            count, bb_min, bb_max = ops.label_bbox(_check_volume(sample['label'], 'label'), self.mask_label)
            if count == 0:
                bb_min, bb_max = [0] * 4, list(sample['label'].shape)
            bb_min, bb_max = bb_min[1:], bb_max[1:]
            crop_min = [random.randint(bb_min[i], bb_max[i]) - int(size[i] / 2) for i in range(3)]
            crop_min = [max(0, v) for v in crop_min]
            crop_min = [min(crop_min[i], shape[i + 1] - size[i]) for i in range(3)]
        crop_max = [crop_min[i] + size[i] for i in range(3)]
        sample['RandomCrop_Param'] = json.dumps((shape, [0] + crop_min, shape[0:1] + crop_max))
        return sample, crop_min, size


class RandomResizedCrop(CenterCrop):
    """crop.py:246-320, 2-D samples [C,H,W] only (the reference asserts it).  Draw order: random() for the scale, random()
    for the aspect ratio, then one randint per axis.  The crop is zoomed to randomresizedcrop_output_size with
    scipy.ndimage.zoom's rules (image and pixel weight order 1, label order 0) by ops.resample_affine on the plane as a
    depth-1 volume; 'image1' is left alone and there is no inverse, as in the reference."""
    _name = 'RandomResizedCrop'

    def __init__(self, params):
        self.output_size = params['randomresizedcrop_output_size']
        self.scale = params['randomresizedcrop_scale']
        self.ratio = params['randomresizedcrop_ratio']
        self.inverse = params.get('randomresizedcrop_inverse', False)
        self.task = params['task']
        assert isinstance(self.output_size, (list, tuple))
        assert isinstance(self.scale, (list, tuple))
        assert isinstance(self.ratio, (list, tuple))

    def _get_crop_param(self, sample):
        shape = list(sample['image'].shape)
        input_dim = len(shape) - 1
        assert input_dim == 2
        assert input_dim == len(self.output_size)
        scale = self.scale[0] + random.random() * (self.scale[1] - self.scale[0])
        ratio = self.ratio[0] + random.random() * (self.ratio[1] - self.ratio[0])
        crop_w = shape[-1] * scale
        crop_h = crop_w * ratio
        crop_h = min(crop_h, shape[-2])
        size = [int(crop_h), int(crop_w)]
        margin = [shape[i + 1] - size[i] for i in range(2)]
        crop_min = [random.randint(0, m) for m in margin]
        crop_max = [crop_min[i] + size[i] for i in range(2)]
        sample['RandomResizedCrop_Param'] = json.dumps((shape, [0] + crop_min, shape[0:1] + crop_max))
        return sample, crop_min, size

    def __call__(self, sample):
        image = _check_tensor(sample['image'], 'image')
        sample, crop_min, size = self._get_crop_param(sample)
        zoom = [1.0] + [(self.output_size[i] + 0.0) / size[i] for i in range(2)]

        def crop_zoom(t, order):                         # [C,H,W] -> [C,1,H,W] -> crop -> zoom -> [C,H',W']
            crop = ops.crop_flip(t.unsqueeze(1), [0] + crop_min, [1] + size)
            return _zoom(crop, zoom, _order_for(crop, order)).squeeze(1)

        sample['image'] = crop_zoom(image, 1)
        if 'label' in sample and self.task == 'segmentation':
            sample['label'] = crop_zoom(_check_tensor(sample['label'], 'label'), 0)
        if 'pixel_weight' in sample and self.task == 'segmentation':
            sample['pixel_weight'] = crop_zoom(_check_tensor(sample['pixel_weight'], 'pixel_weight'), 1)
        return sample

    def inverse_transform_for_prediction(self, sample):
        raise ValueError("not implemented")


class RandomFlip(AbstractTransform):
    """flip.py:14-62: one draw per enabled axis in the order width, height, depth; flip when the draw is > 0.5."""

    def __init__(self, params):
        super(RandomFlip, self).__init__(params)
        self.flip_depth = params['randomflip_flip_depth']
        self.flip_height = params['randomflip_flip_height']
        self.flip_width = params['randomflip_flip_width']
        self.inverse = params.get('randomflip_inverse', True)

    def __call__(self, sample):
        image = _check_volume(sample['image'], 'image')
        flip_axis = []
        if self.flip_width and random.random() > 0.5:
            flip_axis.append(-1)
        if self.flip_height and random.random() > 0.5:
            flip_axis.append(-2)
        if self.flip_depth and random.random() > 0.5:
            flip_axis.append(-3)
        sample['RandomFlip_Param'] = json.dumps(flip_axis)
        if flip_axis:
            mask = sum(1 << (-a - 1) for a in flip_axis)
            sample['image'] = ops.crop_flip(image, (0, 0, 0), image.shape[1:], mask)
            for k in self._others(sample):
                t = _check_volume(sample[k], k)
                sample[k] = ops.crop_flip(t, (0, 0, 0), t.shape[1:], mask)
        return sample

    def inverse_transform_for_prediction(self, sample):
        p = sample['RandomFlip_Param']
        flip_axis = json.loads(p[0] if isinstance(p, (list, tuple)) else p)
        if flip_axis:
            mask = sum(1 << (-a - 1) for a in flip_axis)
            pred = sample['predict']
            n, c = pred.shape[:2]
            flat = pred.contiguous().view(n * c, *pred.shape[2:])
            sample['predict'] = ops.crop_flip(flat, (0, 0, 0), pred.shape[2:], mask).view_as(pred)
        return sample


class LabelToProbability(AbstractTransform):
    """label_convert.py:64-101 (segmentation): one-hot fp32 [class_num, D, H, W] in sample['label_prob']."""

    def __init__(self, params):
        super(LabelToProbability, self).__init__(params)
        self.class_num = params['labeltoprobability_class_num']
        self.inverse = params.get('labeltoprobability_inverse', False)

    def __call__(self, sample):
        if self.task != 'segmentation':
            raise ValueError("fplx.transform: LabelToProbability supports the segmentation task only")
        label = _check_volume(sample['label'], 'label')
        if label.dtype != torch.uint8:
            raise ValueError("fplx.transform: sample['label'] must be uint8")
        sample['label_prob'] = ops.label_to_probability(label[0], self.class_num)
        return sample


def _check_label(sample):
    label = _check_tensor(sample['label'], 'label')
    if label.dtype != torch.uint8:
        raise ValueError("fplx.transform: sample['label'] must be uint8")
    return label


class ReduceLabelDim(AbstractTransform):
    """label_convert.py:13-25: the label loses its channel axis (a view; nothing is moved)"""

    def __init__(self, params):
        super(ReduceLabelDim, self).__init__(params)
        self.inverse = params.get('reducelabeldim_inverse', False)

    def __call__(self, sample):
        sample['label'] = sample['label'][0]
        return sample


class LabelConvert(AbstractTransform):
    """label_convert.py:27-50 on uint8 labels, one table look-up per voxel.  The table restates convert_label
    (util/image_process.py:194-208): labels that are not listed become 0, a source listed twice adds its targets modulo
    256.  Sources or targets outside 0..255 - an OverflowError or a silent no-match in the reference - are refused."""

    def __init__(self, params):
        super(LabelConvert, self).__init__(params)
        self.source_list = params['labelconvert_source_list']
        self.target_list = params['labelconvert_target_list']
        self.inverse = params.get('labelconvert_inverse', False)
        assert len(self.source_list) == len(self.target_list)
        self._lut = ops.label_lut_table(self.source_list, self.target_list)

    def __call__(self, sample):
        sample['label'] = ops.label_lut(_check_label(sample), self._lut)
        return sample


class LabelConvertNonzero(AbstractTransform):
    """label_convert.py:52-64: every nonzero label becomes 1 (the table 0, 1, 1, ...)"""

    def __init__(self, params):
        super(LabelConvertNonzero, self).__init__(params)
        self.inverse = params.get('labelconvertnonzero_inverse', False)
        self._lut = [0] + [1] * 255

    def __call__(self, sample):
        sample['label'] = ops.label_lut(_check_label(sample), self._lut)
        return sample


class PartialLabelToProbability(AbstractTransform):
    """label_convert.py:97-130: labels 0 .. class_num - 1 are classes, class_num marks unlabelled voxels.  One pass writes
    the one-hot 'label_prob' [class_num, ...] and 'pixel_weight' [1, ...] = 1 - (label == class_num), replacing a pixel
    weight the sample had, and finds the largest label: beyond class_num it is the reference's AssertionError."""

    def __init__(self, params):
        super(PartialLabelToProbability, self).__init__(params)
        self.class_num = params['partiallabeltoprobability_class_num']
        self.inverse = params.get('partiallabeltoprobability_inverse', False)

    def __call__(self, sample):
        label = _check_label(sample)[0]
        prob, weight, top = ops.partial_label_to_probability(label, self.class_num)
        assert top <= self.class_num
        sample['label_prob'] = prob
        sample['pixel_weight'] = weight.unsqueeze(0)
        return sample


class GrayscaleToRGB(AbstractTransform):
    """intensity.py:88-101 on [C,H,W] or [C,D,H,W]: one channel becomes three copies, three channels stay"""

    def __init__(self, params):
        super(GrayscaleToRGB, self).__init__(params)
        self.inverse = params.get('grayscaletorgb_inverse', False)

    def __call__(self, sample):
        image = _check_tensor(sample['image'], 'image')
        if image.dim() not in (3, 4):
            raise ValueError("fplx.transform: sample['image'] must be a [C,H,W] or [C,D,H,W] device tensor")
        assert image.shape[0] == 1 or image.shape[0] == 3
        if image.shape[0] == 1:
            size = ([1] * (4 - image.dim())) + list(image.shape[1:])
            src = image.view(1, *size)
            rgb = torch.empty([3] + size, dtype=image.dtype, device=image.device)
            for k in range(3):
                ops.crop_flip(src, (0, 0, 0), size, out=rgb[k:k + 1])
            sample['image'] = rgb.view(3, *image.shape[1:])
        return sample


# ---- geometric augmentation: RandomRotate, Rescale, RandomRescale.  One hot path, ops.resample_affine (csrc/resample.hip),
# which restates scipy.ndimage's affine resampling (mode='constant', cval=0, orders 0 and 1) operation for operation; the
# host below builds the fp64 matrix and offset scipy.ndimage.rotate / zoom would build.  Like the reference's rotate.py and
# rescale.py these three touch 'image', 'label' and 'pixel_weight' only ('image1' is left as it is).

def _fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic; a handful of calls per sample)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _cos_sin_deg(angle):
    """cos and sin of an angle in degrees, exact (0, +-1) at the multiples of 90 degrees as scipy.special.cosdg / sindg are:
    math.cos(math.radians(180)) is not -1 to the last bit of its partner, and a whole border of the volume falls outside"""
    r = math.fmod(float(angle), 360.0)
    if math.fmod(r, 90.0) == 0.0:
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(r // 90.0) % 4]
    a = math.radians(float(angle))
    return math.cos(a), math.sin(a)


def _rotate_affine(shape, angle, axes):
    """matrix and offset of scipy.ndimage.rotate(angle, axes, reshape=False) on a [D,H,W] volume: scipy sorts the two axes,
    R = [[cos, sin], [-sin, cos]] in that order, offset = (n - 1) / 2 - R (n - 1) / 2.  scipy forms R (n - 1) / 2 with a BLAS
    matrix-vector product, which on every FMA-capable x86 rounds row i as fma(R[i][0], v_0, R[i][1] * v_1): the same here,
    since one ulp of the offset can move a voxel on the border."""
    a, b = sorted(ax % 3 for ax in axes)
    c, s = _cos_sin_deg(angle)
    m = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    m[a][a], m[a][b], m[b][a], m[b][b] = c, s, -s, c
    va, vb = (shape[a] - 1) / 2.0, (shape[b] - 1) / 2.0
    t = [0.0, 0.0, 0.0]
    t[a] = va - _fma(c, va, s * vb)
    t[b] = vb - _fma(-s, va, c * vb)
    return m, t


def _zoom(x, zoom, order):
    """scipy.ndimage.zoom(x, [1] + zoom, order) of a [C,D,H,W] volume: extents int(round(n * zoom)) (Python's round), the
    coordinate step (n - 1) / (out - 1) - not 1 / zoom - and 1.0 where out == 1, offset 0"""
    shape = x.shape[1:]
    out = [int(round(shape[i] * zoom[i])) for i in range(3)]
    step = [(shape[i] - 1.0) / (out[i] - 1.0) if out[i] > 1 else 1.0 for i in range(3)]
    m = [[step[i] if i == j else 0.0 for j in range(3)] for i in range(3)]
    return ops.resample_affine(x, m, (0.0, 0.0, 0.0), out, order)


def _order_for(t, order):
    if order == 1 and t.dtype != torch.float32:
        raise ValueError("fplx.transform: linear interpolation takes float32 volumes, got {0:}".format(t.dtype))
    return order


def _on_prediction(sample, fn):
    """apply fn([M,D,H,W]) -> [M,D',H',W'] to sample['predict'] ([N,C,D,H,W], or a list of those)"""
    def one(pred):
        n, c = pred.shape[:2]
        out = fn(pred.contiguous().view(n * c, *pred.shape[2:]))
        return out.view(n, c, *out.shape[1:])

    predict = sample['predict']
    sample['predict'] = [one(q) for q in predict] if isinstance(predict, (tuple, list)) else one(predict)
    return sample


def _json_param(p):
    return json.loads(p[0] if isinstance(p, (list, tuple)) else p)


class RandomRotate(AbstractTransform):
    """rotate.py:14-92.  One np.random.uniform draw per plane whose range is not None, in the order d (axes -1, -2),
    h (-1, -3), w (-2, -3); every rotation is a resampling pass of its own, as in the reference (interpolating three times
    is not interpolating once).  Image and pixel weight: order 1, label: order 0."""

    def __init__(self, params):
        super(RandomRotate, self).__init__(params)
        self.angle_range_d = params['randomrotate_angle_range_d']
        self.angle_range_h = params['randomrotate_angle_range_h']
        self.angle_range_w = params['randomrotate_angle_range_w']
        self.inverse = params.get('randomrotate_inverse', True)

    @staticmethod
    def _apply(x, transform_param_list, order):
        _order_for(x, order)
        for angle, axes in transform_param_list:
            m, t = _rotate_affine(x.shape[1:], angle, axes)
            x = ops.resample_affine(x, m, t, x.shape[1:], order)
        return x

    def __call__(self, sample):
        image = _check_volume(sample['image'], 'image')
        transform_param_list = []
        for rng, axes in ((self.angle_range_d, (-1, -2)), (self.angle_range_h, (-1, -3)), (self.angle_range_w, (-2, -3))):
            if rng is not None:
                transform_param_list.append([np.random.uniform(rng[0], rng[1]), axes])
        assert len(transform_param_list) > 0
        sample['RandomRotate_Param'] = json.dumps(transform_param_list)
        sample['image'] = self._apply(image, transform_param_list, 1)
        if 'label' in sample and self.task == 'segmentation':
            sample['label'] = self._apply(_check_volume(sample['label'], 'label'), transform_param_list, 0)
        if 'pixel_weight' in sample and self.task == 'segmentation':
            sample['pixel_weight'] = self._apply(_check_volume(sample['pixel_weight'], 'pixel_weight'),
                                                 transform_param_list, 1)
        return sample

    def inverse_transform_for_prediction(self, sample):
        transform_param_list = _json_param(sample['RandomRotate_Param'])
        transform_param_list.reverse()
        inverse = [[-angle, axes] for angle, axes in transform_param_list]
        return _on_prediction(sample, lambda p: self._apply(p, inverse, 1))


class _RescaleBase(AbstractTransform):
    _name = None

    def _forward(self, sample, zoom):
        image = _check_volume(sample['image'], 'image')
        sample[self._name + '_origin_shape'] = json.dumps(list(image.shape))
        sample['image'] = _zoom(image, zoom, _order_for(image, 1))
        if 'label' in sample and self.task == 'segmentation':
            sample['label'] = _zoom(_check_volume(sample['label'], 'label'), zoom, 0)
        if 'pixel_weight' in sample and self.task == 'segmentation':
            weight = _check_volume(sample['pixel_weight'], 'pixel_weight')
            sample['pixel_weight'] = _zoom(weight, zoom, _order_for(weight, 1))
        return sample

    def inverse_transform_for_prediction(self, sample):
        origin_shape = _json_param(sample[self._name + '_origin_shape'])

        def back(p):                                     # [N*C, D, H, W]
            zoom = [(origin_shape[1:][i] + 0.0) / p.shape[1 + i] for i in range(3)]
            return _zoom(p, zoom, _order_for(p, 1))

        return _on_prediction(sample, back)


class Rescale(_RescaleBase):
    """rescale.py:14-79.  rescale_output_size: [D, H, W] (D None: keep the depth) or an int (the smallest edge is matched,
    the aspect ratio kept).  The inverse zooms the prediction back to the recorded shape with order 1."""
    _name = 'Rescale'

    def __init__(self, params):
        super(Rescale, self).__init__(params)
        self.output_size = params['rescale_output_size']
        self.inverse = params.get('rescale_inverse', True)
        assert isinstance(self.output_size, (int, list, tuple))

    def __call__(self, sample):
        shape = _check_volume(sample['image'], 'image').shape
        if isinstance(self.output_size, (list, tuple)):
            output_size = list(self.output_size)
            if output_size[0] is None:
                output_size[0] = shape[1]
            assert len(output_size) == 3
        else:
            min_edge = min(shape[1:])
            output_size = [self.output_size * shape[i + 1] / min_edge for i in range(3)]
        return self._forward(sample, [(output_size[i] + 0.0) / shape[1:][i] for i in range(3)])


class RandomRescale(_RescaleBase):
    """rescale.py:81-153: one random.random() per axis, ratio = lower + draw * (upper - lower)."""
    _name = 'RandomRescale'

    def __init__(self, params):
        super(RandomRescale, self).__init__(params)
        self.ratio0 = params['randomrescale_lower_bound']
        self.ratio1 = params['randomrescale_upper_bound']
        self.inverse = params.get('randomrescale_inverse', True)
        assert isinstance(self.ratio0, (float, list, tuple))
        assert isinstance(self.ratio1, (float, list, tuple))

    def __call__(self, sample):
        _check_volume(sample['image'], 'image')
        if isinstance(self.ratio0, (list, tuple)):
            assert len(self.ratio0) == 3
            for i in range(3):
                assert self.ratio0[i] <= self.ratio1[i]
            zoom = [self.ratio0[i] + random.random() * (self.ratio1[i] - self.ratio0[i]) for i in range(3)]
        else:
            zoom = [self.ratio0 + random.random() * (self.ratio1 - self.ratio0) for i in range(3)]
        return self._forward(sample, zoom)


# ---- intensity transforms: NormalizeWithMinMax, NormalizeWithPercentiles, ChannelWiseThreshold,
# ChannelWiseThresholdWithNormalize, GammaCorrection, GaussianNoise, NormalizeWithMeanStd_dual (normalize.py, threshold.py,
# intensity.py).  They touch sample['image'] only, channel by channel and in place, like the reference.  The kernels
# (csrc/intensity.hip) restate numpy's float32 arithmetic under NumPy 2: a Python-float parameter next to a float32 array
# takes part as float32, while two Python floats combine in double first (v1 - v0 of two given thresholds).

def _entry(values, i):
    return None if values is None else values[i]


def _scalar(x, v):
    return torch.full((1,), float(np.float32(v)), dtype=torch.float32, device=x.device)


class NormalizeWithMeanStd_dual(NormalizeWithMeanStd):
    """normalize.py:70-152: NormalizeWithMeanStd on 'image', then on 'image1', with the same parameter keys.  mean / std
    are filled on first use and shared by both, as in the reference."""

    def __call__(self, sample):
        _check_volume(sample['image1'], 'image1')
        sample = super(NormalizeWithMeanStd_dual, self).__call__(sample)
        other = super(NormalizeWithMeanStd_dual, self).__call__({'image': sample['image1']})
        sample['image1'] = other['image']
        return sample


class NormalizeWithMinMax(AbstractTransform):
    """normalize.py:155-197: clip to [v0, v1] and map to [0, 1]; v0 / v1 are the channel's min / max unless a threshold is
    given (per entry).  A constant channel gives 0 / 0 = NaN, as in the reference."""

    def __init__(self, params):
        super(NormalizeWithMinMax, self).__init__(params)
        self.chns = params['normalizewithminmax_channels']
        self.thred_lower = params['normalizewithminmax_threshold_lower']
        self.thred_upper = params['normalizewithminmax_threshold_upper']
        self.inverse = params.get('normalizewithminmax_inverse', False)

    def __call__(self, sample):
        image = _check_volume(sample['image'], 'image')
        chns = self.chns if self.chns is not None else range(image.shape[0])
        for i, chn in enumerate(chns):
            x = image[chn]
            lo, hi = _entry(self.thred_lower, i), _entry(self.thred_upper, i)
            if lo is not None and hi is not None:
                ops.clip_affine(x, lo, hi, lo, hi - lo, out=x)            # hi - lo: two host numbers, rounded once
                continue
            mm = ops.channel_minmax(x)                                    # stays on the device: no synchronisation
            v0 = mm[0:1] if lo is None else _scalar(x, lo)
            v1 = mm[1:2] if hi is None else _scalar(x, hi)
            ops.clip_affine_dev(x, v0, v1, v0, v1, out=x)
        sample['image'] = image
        return sample


class NormalizeWithPercentiles(AbstractTransform):
    """normalize.py:199-237: v0 / v1 = numpy.percentile(channel, q) - exact order statistics selected on the device,
    numpy's linear interpolation between the two neighbours on the host - then clip and map to [0, 1]."""

    def __init__(self, params):
        super(NormalizeWithPercentiles, self).__init__(params)
        self.chns = params['normalizewithpercentiles_channels']
        self.percent_lower = params['normalizewithpercentiles_percentile_lower']
        self.percent_upper = params['normalizewithpercentiles_percentile_upper']
        self.inverse = params.get('normalizewithpercentiles_inverse', False)

    def __call__(self, sample):
        image = _check_volume(sample['image'], 'image')
        chns = self.chns if self.chns is not None else range(image.shape[0])
        for chn in chns:
            x = image[chn]
            v0, v1 = ops.percentiles(x, [self.percent_lower, self.percent_upper])
            with np.errstate(invalid="ignore", over="ignore"):
                ops.clip_affine(x, v0, v1, v0, v1 - v0, out=x)            # numpy.float32 - numpy.float32
        sample['image'] = image
        return sample


class ChannelWiseThreshold(AbstractTransform):
    """threshold.py:14-63: values below the lower threshold, then values above the upper one, are replaced (by the
    threshold itself unless a replacement is given); every list is indexed by the position in `channels`."""

    def __init__(self, params):
        super(ChannelWiseThreshold, self).__init__(params)
        self.channels = params['channelwisethreshold_channels']
        self.threshold_lower = params['channelwisethreshold_threshold_lower']
        self.threshold_upper = params['channelwisethreshold_threshold_upper']
        self.replace_lower = params['channelwisethreshold_replace_lower']
        self.replace_upper = params['channelwisethreshold_replace_upper']
        self.inverse = params.get('channelwisethreshold_inverse', False)

    def __call__(self, sample):
        image = _check_volume(sample['image'], 'image')
        channels = range(image.shape[0]) if self.channels is None else self.channels
        for i, chn in enumerate(channels):
            t_lower, t_upper = _entry(self.threshold_lower, i), _entry(self.threshold_upper, i)
            r_lower, r_upper = t_lower, t_upper
            if t_lower is not None and _entry(self.replace_lower, i) is not None:
                r_lower = self.replace_lower[i]
            if t_upper is not None and _entry(self.replace_upper, i) is not None:
                r_upper = self.replace_upper[i]
            if t_lower is not None or t_upper is not None:
                ops.threshold_replace(image[chn], t_lower, r_lower, t_upper, r_upper, out=image[chn])
        sample['image'] = image
        return sample


class ChannelWiseThresholdWithNormalize(AbstractTransform):
    """threshold.py:65-132.  The thresholds are indexed by the CHANNEL NUMBER, not by the position in `channels` - the
    reference's indexing, kept.  mean_std_mode: moments of the voxels strictly inside (v0, v1), the others replaced by a
    numpy.random.normal(0, 1) draw made on the host for the whole channel.  Otherwise: clip and divide by (max - min),
    where min is v0 or the channel's min and max is the channel's max AFTER clipping."""

    def __init__(self, params):
        super(ChannelWiseThresholdWithNormalize, self).__init__(params)
        self.channels = params['channelwisethresholdwithnormalize_channels']
        self.threshold_lower = params['channelwisethresholdwithnormalize_threshold_lower']
        self.threshold_upper = params['channelwisethresholdwithnormalize_threshold_upper']
        self.mean_std_mode = params['channelwisethresholdwithnormalize_mean_std_mode']
        self.inverse = params.get('channelwisethresholdwithnormalize_inverse', False)

    def __call__(self, sample):
        image = _check_volume(sample['image'], 'image')
        channels = range(image.shape[0]) if self.channels is None else self.channels
        for chn in channels:
            x = image[chn]
            v0, v1 = self.threshold_lower[chn], self.threshold_upper[chn]
            if self.mean_std_mode == True:                                # noqa: E712 (the reference's test)
                noise = torch.from_numpy(np.random.normal(0, 1, size=tuple(x.shape)).astype(np.float32)).to(x.device)
                ops.normalize_range(x, noise, v0, v1, out=x)
                continue
            mm = ops.channel_minmax(x, v0, v1)
            lo = mm[0:1] if v0 is None else _scalar(x, v0)
            hi = mm[1:2] if v1 is None else _scalar(x, v1)                # clipping at the channel's own max is no clipping
            ops.clip_affine_dev(x, lo, hi, lo, mm[3:4], out=x)
        sample['image'] = image
        return sample


class GammaCorrection(AbstractTransform):
    """intensity.py:14-51.  Draw order: numpy.random.uniform() for the probability gate, then one random.random() per
    listed channel.  The power is the correctly rounded one; numpy's float32 power is within 1 ulp of it."""

    def __init__(self, params):
        super(GammaCorrection, self).__init__(params)
        self.channels = params['gammacorrection_channels']
        self.gamma_min = params['gammacorrection_gamma_min']
        self.gamma_max = params['gammacorrection_gamma_max']
        self.prob = params.get('gammacorrection_probability', 0.5)
        self.inverse = params.get('gammacorrection_inverse', False)

    def __call__(self, sample):
        image = _check_volume(sample['image'], 'image')
        if np.random.uniform() > self.prob:
            return sample
        self.last_gammas = []
        for chn in self.channels:
            gamma_c = random.random() * (self.gamma_max - self.gamma_min) + self.gamma_min
            self.last_gammas.append(gamma_c)
            mm = ops.channel_minmax(image[chn])
            ops.gamma_correct(image[chn], mm[0:1], mm[1:2], gamma_c, out=image[chn])
        sample['image'] = image
        return sample


class GaussianNoise(AbstractTransform):
    """intensity.py:53-86.  Draw order: numpy.random.uniform() for the gate, then numpy.random.normal(mean, std, shape) per
    listed channel - drawn on the host in float64 and uploaded, so that a seeded run adds the reference's noise.
    `gaussiannoise_device_rng` (fplx only, default False; no reference counterpart, no parity with numpy's generator): the
    noise is generated on the device from Philox4x32-10 keyed by one random.getrandbits(64) draw per firing call and the
    channel number, and never exists on the host."""

    def __init__(self, params):
        super(GaussianNoise, self).__init__(params)
        self.channels = params['gaussiannoise_channels']
        self.mean = params['gaussiannoise_mean']
        self.std = params['gaussiannoise_std']
        self.prob = params.get('gaussiannoise_probability', 0.5)
        self.inverse = params.get('gaussiannoise_inverse', False)
        self.device_rng = params.get('gaussiannoise_device_rng', False)
        self.last_seed = None

    def __call__(self, sample):
        image = _check_volume(sample['image'], 'image')
        if np.random.uniform() > self.prob:
            return sample
        if self.device_rng:
            self.last_seed = random.getrandbits(64)
        for chn in self.channels:
            x = image[chn]
            if self.device_rng:
                ops.add_noise_philox(x, self.last_seed, chn, self.mean, self.std, out=x)
            else:
                noise = torch.from_numpy(np.random.normal(self.mean, self.std, tuple(x.shape))).to(x.device)
                ops.add_noise_f64(x, noise, out=x)
        sample['image'] = image
        return sample


TransformDict = {
    'NormalizeWithMeanStd': NormalizeWithMeanStd,
    'Pad': Pad,
    'RandomCrop': RandomCrop,
    'RandomFlip': RandomFlip,
    'LabelToProbability': LabelToProbability,
    'RandomRotate': RandomRotate,
    'Rescale': Rescale,
    'RandomRescale': RandomRescale,
    'NormalizeWithMeanStd_dual': NormalizeWithMeanStd_dual,
    'NormalizeWithMinMax': NormalizeWithMinMax,
    'NormalizeWithPercentiles': NormalizeWithPercentiles,
    'ChannelWiseThreshold': ChannelWiseThreshold,
    'ChannelWiseThresholdWithNormalize': ChannelWiseThresholdWithNormalize,
    'GammaCorrection': GammaCorrection,
    'GaussianNoise': GaussianNoise,
    'CenterCrop': CenterCrop,
    'CropWithBoundingBox': CropWithBoundingBox,
    'RandomResizedCrop': RandomResizedCrop,
    'LabelConvert': LabelConvert,
    'LabelConvertNonzero': LabelConvertNonzero,
    'PartialLabelToProbability': PartialLabelToProbability,
    'ReduceLabelDim': ReduceLabelDim,
    'GrayscaleToRGB': GrayscaleToRGB,
}


def build_transforms(names, params):
    """The list PyMIC/pymic/net_run/agent_seg.py:48-61 builds from `<stage>_transform`: unknown names raise."""
    out = []
    for name in names:
        if name not in TransformDict:
            raise ValueError("Undefined transform {0:}".format(name))
        out.append(TransformDict[name](params))
    return out


def apply_transforms(transforms, sample):
    for t in transforms:
        sample = t(sample)
    return sample


class Compose(object):
    """torchvision.transforms.Compose as the reference uses it (agent_seg.py:61): a callable chain"""

    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, sample):
        return apply_transforms(self.transforms, sample)
