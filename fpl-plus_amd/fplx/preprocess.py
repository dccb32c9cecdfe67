"""Dataset preparation on the device: the step between the public vestibular-schwannoma (VS) volumes and
`python -m fplx.net_run train <cfg>`.

 - get_transform_list / preprocess_with_transform: PyMIC/pymic/util/preprocess.py - a transform list from a .cfg run over one
   image (and its label), over fplx.nifti and fplx.TransformDict, the sample on the device.
 - vs_source_crop / vs_target_crop / source_image_crop / target_image_crop: data/preprocess_vs.py:61-135 - the fixed
   bounding boxes of the two VS domains, and the target's resampling to 256 x 256 in plane with
   scipy.ndimage.zoom(img_sub, [1, 256 / Hs, 256 / Ws]) at its default spline order 3, here fplx.resample.zoom.

Where this differs from the reference: directories are arguments, not constants to edit; file names are matched without
regard to case ("t1", "t2.nii.gz": the reference's lower-case test finds none of the public `*_ceT1.nii.gz` / `*_hrT2.nii.gz`
names, which its own replace("ceT1", "Label") expects); integer-typed files are converted
to float32 before resampling and written as float32 (the reference keeps the file's type, scipy rounding the spline back to
integers); preprocess_with_transform writes the input file's own geometry (the reference hands SimpleITK the spacing in the
(z, y, x) order its loader produced).

    python -m fplx.preprocess transform <cfg> <img_in> <img_out> [<lab_in> <lab_out>]
    python -m fplx.preprocess vs-source <in_dir> <out_dir>
    python -m fplx.preprocess vs-target <in_dir> <out_dir>
"""
import argparse
import os
import sys

import numpy as np
import torch

from . import nifti, resample
from .config import parse_config
from .transform import TransformDict

VS_TARGET_SPACING_XY = 0.4102           # preprocess_vs.py:129, written whatever the zoom was
VS_TARGET_SIZE = 256.0


def get_transform_list(trans_config_file):
    """util/preprocess.py:8-24: the transforms named by [dataset] transform, built with [dataset] as their parameters"""
    config = parse_config(trans_config_file)
    transform_param = config['dataset']
    transform_param['task'] = 'segmentation'
    transform_list = []
    for name in config['dataset']['transform']:
        if name not in TransformDict:
            raise ValueError("Undefined transform {0:}".format(name))
        transform_list.append(TransformDict[name](transform_param))
    return transform_list


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("fplx.preprocess: no GPU (HIP path only, no CPU fallback)")
    return torch.device("cuda:0")


def _upload(a, dtype, device):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(device)


def _label_u8(lab, name):
    if lab.min() < 0 or lab.max() > 255:
        raise ValueError("fplx.preprocess: label values outside [0, 255] in {0:}".format(name))
    return np.asarray(lab, np.uint8)


def preprocess_with_transform(transforms, img_in_name, img_out_name, lab_in_name=None, lab_out_name=None):
    """util/preprocess.py:26-59: load, run the transforms on the device, write the image (float32) and, when both label
    names are given, the label (uint8), with the input image's spacing, origin and direction.  No transform of TransformDict
    updates sample['spacing'] (nor does the reference's), so after a transform that changes the voxel grid - Rescale,
    RandomRescale - the written spacing is still the input's and no longer describes the grid, as in the reference."""
    device = _device()
    image_dict = nifti.load_image_as_nd_array(img_in_name)
    spacing = tuple(image_dict['spacing'][::-1])           # the loader's (z, y, x) back to the file's (x, y, z)
    origin, direction = image_dict['origin'], image_dict['direction']
    sample = {'image': _upload(image_dict['data_array'], np.float32, device), 'origin': image_dict['origin'],
              'spacing': image_dict['spacing'], 'direction': image_dict['direction']}
    if lab_in_name is not None:
        lab = nifti.load_image_as_nd_array(lab_in_name)['data_array']
        sample['label'] = _upload(_label_u8(lab, lab_in_name), np.uint8, device)
    for transform in transforms:
        sample = transform(sample)
    nifti.write_nifti(img_out_name, sample['image'][0].cpu().numpy(), spacing, origin, direction)
    if lab_in_name is not None and lab_out_name is not None:
        nifti.write_nifti(lab_out_name, sample['label'][0].cpu().numpy(), spacing, origin, direction)
    return sample


# ---- the VS boxes (data/preprocess_vs.py)

def vs_source_box(shape, spacing):
    """preprocess_vs.py:75-81: (d0, d1, h0, h1, w0, w1) of a source (ceT1) volume [D,H,W] with spacing (x, y, z)"""
    D = shape[0]
    d0 = int(D - 153 / spacing[2])
    d1 = int(D - 93 / spacing[2])
    return d0, d1, 190, 350, 120, 392


def vs_target_box(shape, spacing):
    """preprocess_vs.py:107-121: (d0, d1, h0, h1, w0, w1) of a target (hrT2) volume [D,H,W] with spacing (x, y, z)"""
    D, H, W = shape
    if D < 50:
        d0, d1 = 5, D - 5
    elif spacing[2] == 1.0:
        d0, d1 = 8, 48
    elif spacing[2] == 1.5:
        d0, d1 = 8, 48
    else:
        raise ValueError("undefined case")
    h0, h1 = 120, 376
    w0, w1 = 120, 376
    h0, h1 = int(h0 * H / 512), int(h1 * H / 512)
    w0, w1 = int(w0 * W / 512), int(w1 * W / 512)
    return d0, d1, h0, h1, w0, w1


def vs_source_crop(img, lab, spacing):
    """crop a source image and its label ([D,H,W] arrays or tensors) to the source box; no label voxel may be cut"""
    d0, d1, h0, h1, w0, w1 = vs_source_box(img.shape, spacing)
    img_sub = img[d0:d1, h0:h1, w0:w1]
    lab_sub = lab[d0:d1, h0:h1, w0:w1]
    assert int(lab_sub.sum()) == int(lab.sum())
    return img_sub, lab_sub


def vs_target_crop(img, spacing):
    """crop a target image ([D,H,W] float32 device tensor) to the target box and resample it to 256 x 256 in plane at spline
    order 3 on the device -> ([Ds,256,256] device tensor, spacing [0.4102, 0.4102, sz])"""
    if not (torch.is_tensor(img) and img.dim() == 3):
        raise ValueError("fplx.preprocess.vs_target_crop takes a [D,H,W] device tensor")
    d0, d1, h0, h1, w0, w1 = vs_target_box(img.shape, spacing)
    img_sub = img[d0:d1, h0:h1, w0:w1]
    Ds, Hs, Ws = img_sub.shape
    zoom = [1.0, VS_TARGET_SIZE / Hs, VS_TARGET_SIZE / Ws]
    out = resample.zoom(img_sub.to(torch.float32).contiguous()[None], zoom, 3)[0]
    return out, [VS_TARGET_SPACING_XY, VS_TARGET_SPACING_XY, spacing[2]]


def source_image_crop(img_dir, out_dir):
    """preprocess_vs.py:61-97 over a directory: every file with "t1" in its name and its "Label" partner; files keep their
    names, types, spacing, origin and direction"""
    names = sorted(item for item in os.listdir(img_dir) if "t1" in item.lower())
    for img_name in names:
        lab_name = img_name.replace("ceT1", "Label")
        if lab_name == img_name:
            raise ValueError("fplx.preprocess: {0:} has no \"ceT1\" to replace by \"Label\": the image would be read as its "
                             "own label".format(img_name))
        img, spacing, origin, direction = nifti.read_nifti(os.path.join(img_dir, img_name))
        lab = nifti.read_nifti(os.path.join(img_dir, lab_name))[0]
        img_sub, lab_sub = vs_source_crop(img, lab, spacing)
        nifti.write_nifti(os.path.join(out_dir, img_name), img_sub, spacing, origin, direction)
        nifti.write_nifti(os.path.join(out_dir, lab_name), lab_sub, spacing, origin, direction)
    return names


def target_image_crop(img_dir, out_dir):
    """preprocess_vs.py:99-135 over a directory: every file with "t2.nii.gz" in its name, written as float32"""
    device = _device()
    names = sorted(item for item in os.listdir(img_dir) if "t2.nii.gz" in item.lower())
    for img_name in names:
        img, spacing, origin, direction = nifti.read_nifti(os.path.join(img_dir, img_name))
        out, new_spacing = vs_target_crop(_upload(img, np.float32, device), spacing)
        nifti.write_nifti(os.path.join(out_dir, img_name), out.cpu().numpy(), new_spacing, origin, direction)
    return names


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m fplx.preprocess", description="dataset preparation on the device")
    sub = parser.add_subparsers(dest="command")
    sub.required = True
    p = sub.add_parser("transform", help="run the [dataset] transform list of a .cfg over one image (and its label)")
    p.add_argument("cfg")
    p.add_argument("img_in")
    p.add_argument("img_out")
    p.add_argument("lab_in", nargs="?", default=None)
    p.add_argument("lab_out", nargs="?", default=None)
    for name, text in (("vs-source", "crop the VS source (ceT1) volumes and labels of a directory"),
                       ("vs-target", "crop the VS target (hrT2) volumes of a directory and resample them to 256 x 256")):
        p = sub.add_parser(name, help=text)
        p.add_argument("in_dir")
        p.add_argument("out_dir")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.command == "transform":
        if (args.lab_in is None) != (args.lab_out is None):
            parser.error("transform takes <lab_in> and <lab_out> together")
        preprocess_with_transform(get_transform_list(args.cfg), args.img_in, args.img_out, args.lab_in, args.lab_out)
    elif args.command == "vs-source":
        names = source_image_crop(args.in_dir, args.out_dir)
        print("vs-source: {0:} volumes".format(len(names)))
    else:
        names = target_image_crop(args.in_dir, args.out_dir)
        print("vs-target: {0:} volumes".format(len(names)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
