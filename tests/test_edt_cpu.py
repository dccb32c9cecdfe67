"""CPU tests of the exact Euclidean distance transform:
 - tests/edtoracle.py, the numpy restatement of csrc/edt.hip's three passes, against scipy.ndimage.distance_transform_edt
   itself, bit for bit, and against an all-pairs search with scipy's expression on small masks - the mask without any
   background element (scipy's phantom at index (-1, 0, 0)) in 2D and 3D, with and without sampling, included;
 - the index validator against scipy's own feature transform, and against a wrong one;
 - the C ABI: the symbols are declared, and every refusal runs before any launch;
 - the argument errors of fplx.distance_transform_edt and fplx.get_euclidean_distance, raised before any GPU call;
 - the committed fixture tests/golden/edt.npz against the oracle."""
import ctypes
import os

import numpy as np
import pytest

import detdata
import edtoracle as O

SAMPLINGS = [None, (1.5, .41, .41), (2, .5, .25), (.7, 1.3, .9)]
DENSITIES = [0.02, 0.2, 0.6]                     # share of background
SHAPES = [(9, 21, 25), (13, 16, 20)]


def random_mask(name, shape, background):
    return np.asarray(detdata.uniform(name, shape) >= background, np.uint8)


def _scipy_edt(mask, sampling, **kw):
    from scipy import ndimage
    return ndimage.distance_transform_edt(mask, sampling=sampling, **kw)


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_oracle_equals_scipy_bit_for_bit(sampling):
    total = differing = 0
    for shape in SHAPES:
        for bgd in DENSITIES:
            mask = random_mask("edt.cpu.%s.%g" % (shape, bgd), shape, bgd)
            assert 0 < mask.sum() < mask.size
            got, ref = np.sqrt(O.separable_sq(mask, sampling)), _scipy_edt(mask, sampling)
            total += got.size
            differing += int((got != ref).sum())
    print("separable minimum vs scipy, sampling %s: %d outputs, %d not identical" % (sampling, total, differing))
    assert total >= 25000 and differing == 0


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("shape", [(5, 7, 9), (6, 11), (1, 1, 4), (3, 1), (1, 1)])
def test_oracle_equals_brute_force_and_scipy_without_background(shape, sampling):
    s = None if sampling is None else sampling[-len(shape):]
    for name, mask in (("ones", np.ones(shape, np.uint8)), ("sparse", random_mask("edt.cpu.bf%s" % (shape,), shape, 0.1)),
                       ("zeros", np.zeros(shape, np.uint8))):
        sep = O.separable_sq(mask, s)
        assert np.array_equal(sep, O.brute_sq(mask, s)), (name, shape, s)
        if s is None:
            assert np.array_equal(sep, O.brute_sq_int(mask).astype(np.float64)), (name, shape)
        ref, ind = _scipy_edt(mask, s, return_indices=True)
        assert np.array_equal(np.sqrt(sep), ref), (name, shape, s)
        O.check_indices(mask, s, sep, ind.astype(np.int32))                 # scipy's own indices pass the validator
        if mask.all():
            assert (ind.reshape(len(shape), -1) == np.array([-1] + [0] * (len(shape) - 1))[:, None]).all()


def test_index_validator_refuses_wrong_indices():
    mask = random_mask("edt.cpu.val", (4, 6, 7), 0.3)
    sq = O.separable_sq(mask, (2, .5, .25))
    _, ind = _scipy_edt(mask, (2, .5, .25), return_indices=True)
    ind = ind.astype(np.int32)
    O.check_indices(mask, (2, .5, .25), sq, ind)
    fg = tuple(np.argwhere(mask)[0])
    bad = ind.copy()
    bad[(slice(None),) + fg] = fg                                       # names a foreground element (itself)
    with pytest.raises(AssertionError):
        O.check_indices(mask, (2, .5, .25), sq, bad)
    far = ind.copy()
    bg = np.argwhere(mask == 0)
    at = tuple(bg[0])
    other = [b for b in bg if tuple(b) != at][0]
    far[(slice(None),) + at] = other                                    # a background element, but not at distance 0
    with pytest.raises(AssertionError):
        O.check_indices(mask, (2, .5, .25), sq, far)
    with pytest.raises(AssertionError):
        O.check_indices(mask, (2, .5, .25), sq, ind.astype(np.int64))


def test_ulp_distance():
    a = np.array([1.0, 2.0, np.inf, 0.0])
    assert np.array_equal(O.ulp_distance(a, a), np.zeros(4))
    assert O.ulp_distance(np.nextafter(3.0, 4.0), 3.0) == 1.0 and O.ulp_distance(np.nextafter(3.0, 0.0), 3.0) == 1.0
    assert O.ulp_distance(3.0 + 4 * np.spacing(3.0), 3.0) == 4.0


def test_symbols_declared_and_constants_mirror_the_header():
    from fplx import _lib, ops
    assert {"fplx_edt_squared", "fplx_edt_pass", "fplx_edt_finish"} <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert lib.fplx_edt_squared and lib.fplx_edt_finish
    header = open(_lib.HEADER).read()
    assert "#define FPLX_EDT_MAX_EXTENT %d\n" % ops.EDT_MAX_EXTENT in header
    src = open(os.path.join(os.path.dirname(_lib.HEADER), "..", "fpl-plus_amd", "csrc", "edt.hip")).read()
    assert "constexpr int EDT_LINES = %d;" % ops.EDT_LINES in src
    # the tile of the longest line fills the 160 KiB of a CU's LDS and one more element would not fit
    row = (ops.EDT_LINES + 1) * 8
    assert ops.EDT_MAX_EXTENT * row <= 160 * 1024 < (ops.EDT_MAX_EXTENT + 1) * row and ops.EDT_MAX_EXTENT >= 512


def test_c_abi_refusals_run_before_any_launch():
    """on host memory and without a GPU: a call that got past its checks would fail with FPLX_E_HIP (-4) or fault"""
    from fplx import _lib, ops
    lib = _lib.lib()
    mask = (ctypes.c_uint8 * 64)()
    sq = (ctypes.c_double * 64)()
    idx = (ctypes.c_int * 192)()
    ws = (ctypes.c_int * 128)()
    s = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    f = lib.fplx_edt_squared
    assert f(None, 1, 4, 4, 4, 3, s, None, sq, None, None, 0, None) == -5
    assert f(mask, 1, 4, 4, 4, 3, None, None, sq, None, None, 0, None) == -5
    assert f(mask, 1, 4, 4, 4, 3, s, None, None, None, None, 0, None) == -5 and "edt_squared" in _lib.last_error()
    assert f(mask, 1, 4, 4, 4, 3, s, None, sq, idx, None, 0, None) == -5                       # indices need the workspace
    assert f(mask, 1, 4, 4, 4, 3, s, None, sq, idx, ws, 2 * 64 * 4 - 1, None) == -3
    for n, d, h, w in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0), (1 << 12, 512, 512, 2), (1 << 30, 600, 600, 600)):
        assert f(mask, n, d, h, w, 3, s, None, sq, None, None, 0, None) == -1, (n, d, h, w)
    big = ops.EDT_MAX_EXTENT + 1
    for d, h, w in ((big, 2, 2), (2, big, 2), (2, 2, big), (1 << 20, 1, 1)):
        assert f(mask, 1, d, h, w, 3, s, None, sq, None, None, 0, None) == -1, (d, h, w)
        assert "limit of %d" % ops.EDT_MAX_EXTENT in _lib.last_error()
    assert f(mask, 1, 1, big, 2, 2, s, None, sq, None, None, 0, None) == -1
    for ndim, d in ((1, 1), (4, 1), (2, 2), (0, 1)):
        assert f(mask, 1, d, 4, 4, ndim, s, None, sq, None, None, 0, None) == -1, (ndim, d)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for a in range(3):
            v = [1.0, 1.0, 1.0]
            v[a] = bad
            assert f(mask, 1, 4, 4, 4, 3, (ctypes.c_double * 3)(*v), None, sq, None, None, 0, None) == -1, (a, bad)
    with pytest.raises(ValueError, match="limit of %d" % ops.EDT_MAX_EXTENT):
        _lib.check(f(mask, 1, big, 2, 2, 3, s, None, sq, None, None, 0, None))
    p = lib.fplx_edt_pass
    assert p(None, 1, 4, 4, 4, 0, 1.0, None) == -5 and "edt_pass" in _lib.last_error()
    for n, d, h, w in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0), (1 << 12, 512, 512, 2), (1 << 30, 1 << 30, 4, 4)):
        assert p(sq, n, d, h, w, 1, 1.0, None) == -1, (n, d, h, w)
    for axis in (-1, 3):
        assert p(sq, 1, 4, 4, 4, axis, 1.0, None) == -1, axis
    for axis in range(3):
        shape = [2, 2, 2]
        shape[axis] = big
        assert p(sq, 1, shape[0], shape[1], shape[2], axis, 1.0, None) == -1 and "limit of %d" % ops.EDT_MAX_EXTENT in _lib.last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert p(sq, 1, 4, 4, 4, 2, bad, None) == -1, bad
    g = lib.fplx_edt_finish
    assert g(None, None, sq, 64, None) == -5 and g(sq, None, None, 64, None) == -5 and "edt_finish" in _lib.last_error()
    for count in (0, -1, 1 << 31):
        assert g(sq, None, sq, count, None) == -1, count


def test_argument_errors_come_before_any_gpu_call():
    """none of these may reach the device: on a machine without one a GPU call would raise something else"""
    import torch
    import fplx
    from fplx import image_process as P, ops
    assert fplx.distance_transform_edt is P.distance_transform_edt and fplx.get_euclidean_distance is P.get_euclidean_distance
    for shape in ((5,), (2, 3, 4, 5), ()):
        with pytest.raises(ValueError, match="2D or 3D"):
            P.distance_transform_edt(np.ones(shape, np.uint8))
    with pytest.raises(ValueError, match="2D or 3D"):
        P.distance_transform_edt(torch.ones(2, 2, 2, 2))
    for shape, sampling in (((4, 5), (1, 2, 3)), ((3, 4, 5), (1, 2)), ((3, 4, 5), (1, 2, 3, 4)), ((4, 5), ())):
        with pytest.raises(ValueError, match="sampling has %d entries" % len(sampling)):
            P.distance_transform_edt(np.ones(shape), sampling=sampling)
    with pytest.raises(RuntimeError, match="at least one of"):
        P.distance_transform_edt(np.ones((4, 5)), return_distances=False)
    assert ops.edt_sampling(None, 3) == [1.0, 1.0, 1.0] and ops.edt_sampling(2, 2) == [2.0, 2.0]
    assert ops.edt_sampling(np.float32(0.5), 3) == [0.5] * 3 and ops.edt_sampling([1.5, .41, .41], 3) == [1.5, .41, .41]
    # get_euclidean_distance: the reference's errors with the reference's messages
    vol = np.zeros((3, 4, 5), np.uint8)
    for bad in (np.zeros((4, 5)), np.zeros((2, 3, 4, 5)), torch.zeros(4, 5)):
        with pytest.raises(ValueError, match="^Not implemented for %dD image$" % bad.ndim):
            P.get_euclidean_distance(bad)
    with pytest.raises(ValueError, match="^Not implemented for 3D image$"):
        P.get_euclidean_distance(vol, dim=2)
    for dim in (1, 4, 0):
        with pytest.raises(ValueError, match="^Not implemented for %dD distance$" % dim):
            P.get_euclidean_distance(vol, dim=dim)
    # host tensors are refused: there is no CPU path
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        P.distance_transform_edt(torch.ones(4, 5))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.edt_squared(torch.ones(4, 5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.edt_finish(torch.ones(4, 5, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.edt_pass(torch.ones(1, 3, 4, 5, dtype=torch.float64), 0)


def test_fixture_holds_the_references_maps_and_the_oracle_reproduces_them(golden_dir):
    z = np.load(os.path.join(golden_dir, "edt.npz"))
    names = [str(n) for n in z["names"]]
    assert "edt_zeros" in names and "edt_ones" in names and len(names) >= 5
    for name in names:
        img, signed = z[name + ".image"], z[name + ".signed"]
        assert img.dtype == np.uint8 and img.ndim == 3 and img.size <= 21000 and signed.dtype == np.float64
        sq_fg, sq_bg = O.separable_sq(img > 0.5), O.separable_sq(img <= 0.5)
        assert np.array_equal(sq_fg, z[name + ".sq_fg"].astype(np.float64)), name
        assert np.array_equal(sq_bg, z[name + ".sq_bg"].astype(np.float64)), name
        assert np.array_equal(np.sqrt(sq_bg) - np.sqrt(sq_fg), signed), name
    assert not z["edt_zeros.image"].any() and z["edt_ones.image"].all()
