"""Generates tests/golden/edt.npz by RUNNING the reference's get_euclidean_distance (the reference's
PyMIC/pymic/util/image_process.py:165-192), imported with the stub modules of _ref_import.py and scipy.  Build-container
only; the GPU box reads the fixture.

Inputs: detdata-seeded blob masks (make_golden_postprocess.blob_mask, one class) at odd shapes of at most about 20 000
voxels, an all-zero volume and an all-one volume (each of them makes one of the two transforms run on a mask without any
background element).  Per input the fixture holds
  <name>.image    uint8, the input
  <name>.signed   float64, what the reference returned: edt(image <= 0.5) - edt(image > 0.5)
  <name>.sq_fg    int64, the squared distances behind edt(image > 0.5)  - round(edt^2), checked below to be the exact
  <name>.sq_bg    int64, the same for edt(image <= 0.5)                   integers of an all-pairs search, so that sqrt of
                         them is scipy's map bit for bit
Data only."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "fpl-plus_amd"))
import _ref_import  # noqa: E402

_ref_import.install()
from scipy import ndimage  # noqa: E402
from pymic.util.image_process import get_euclidean_distance  # noqa: E402
import edtoracle as O  # noqa: E402
from make_golden_postprocess import blob_mask  # noqa: E402

CASES = [("edt_a", (17, 23, 41)), ("edt_b", (7, 45, 61)), ("edt_c", (29, 19, 33)), ("edt_d", (3, 5, 301)), ("edt_e", (33, 1, 27))]


def main():
    inputs = [(n, np.asarray(blob_mask(n, s, 1) > 0, np.uint8)) for n, s in CASES]
    inputs += [("edt_zeros", np.zeros((5, 7, 9), np.uint8)), ("edt_ones", np.ones((6, 4, 11), np.uint8))]
    out = {}
    for name, img in inputs:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)          # the reference spells it ndimage.morphology.*
            signed = get_euclidean_distance(img)
        fg, bg = ndimage.distance_transform_edt(img > 0.5), ndimage.distance_transform_edt(img <= 0.5)
        assert signed.dtype == np.float64 and np.array_equal(signed, bg - fg), name
        sq_fg, sq_bg = np.rint(fg * fg).astype(np.int64), np.rint(bg * bg).astype(np.int64)
        assert np.array_equal(sq_fg, O.brute_sq_int(img > 0.5)) and np.array_equal(sq_bg, O.brute_sq_int(img <= 0.5)), name
        assert np.array_equal(np.sqrt(sq_fg.astype(np.float64)), fg) and np.array_equal(np.sqrt(sq_bg.astype(np.float64)), bg), name
        out[name + ".image"], out[name + ".signed"], out[name + ".sq_fg"], out[name + ".sq_bg"] = img, signed, sq_fg, sq_bg
        print(name, img.shape, int(img.sum()), float(signed.min()), float(signed.max()))
    out["names"] = np.array([n for n, _ in inputs])
    np.savez_compressed(os.path.join(HERE, "edt.npz"), **out)


if __name__ == "__main__":
    main()
