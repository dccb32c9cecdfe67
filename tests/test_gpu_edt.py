"""-m gpu tests of the exact Euclidean distance transform (csrc/edt.hip through fplx.ops.edt_squared / edt_finish and
fplx.image_process) against tests/edtoracle.py and scipy.ndimage.distance_transform_edt itself.

Criteria.  The squared map equals the oracle's separable float64 minimum in EVERY element - derived, not measured: the same
products, squares and sums in the same order, and a minimum has no order.  With sampling=None the values are integers and
equal an int64 all-pairs search (run where voxels x background elements <= BRUTE_PAIRS; larger masks are held to the oracle,
which tests/test_edt_cpu.py holds to scipy).  The distance map lies within 1 ulp of scipy's float64 in every element - one
faithfully rounded sqrt of an identical argument; the number of elements not identical to scipy's is printed per check
(0 if the device's sqrt is correctly rounded).  The feature transform passes the oracle's validator: every index names a
background element (or the phantom (-1, 0, 0) of a mask without one) at which scipy's expression reproduces the squared
distance bit for bit; equality with scipy's indices is not asserted, ties may resolve differently."""
import functools
import os

import numpy as np
import pytest
import torch

import detdata
import edtoracle as O

pytestmark = pytest.mark.gpu

LINES = 32                # EDT_LINES of csrc/edt.hip: the lines a block stages in LDS
MAX_EXTENT = 620          # FPLX_EDT_MAX_EXTENT: the longest line, whose tile fills the LDS
BRUTE_PAIRS = 6e7

SAMPLINGS = [None, (2, .5, .25), (1.5, .41, .41), (.7, 1.3, .9)]
LINE_COUNTS = [LINES - 1, LINES, LINES + 1, 2 * LINES + 5]


def test_constants_mirror_the_kernel():
    from fplx import ops
    assert (LINES, MAX_EXTENT) == (ops.EDT_LINES, ops.EDT_MAX_EXTENT)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def random_mask(name, shape, background):
    return np.asarray(detdata.uniform(name, shape) >= background, np.uint8)


def _scipy_edt(mask, sampling):
    from scipy import ndimage
    return ndimage.distance_transform_edt(mask, sampling=sampling)


def _check(mask, sampling, what):
    """the whole criterion for one mask and sampling; returns the device's squared map"""
    from fplx import ops
    s = None if sampling is None else tuple(sampling[-mask.ndim:])
    sq, idx = ops.edt_squared(_dev(mask), s, return_indices=True)
    assert sq.dtype == torch.float64 and sq.is_cuda and tuple(sq.shape) == mask.shape
    assert idx.dtype == torch.int32 and idx.is_cuda and tuple(idx.shape) == (mask.ndim,) + mask.shape
    alone = ops.edt_squared(_dev(mask), s)                                # without the feature transform: the same map
    dist = ops.edt_finish(sq)
    got, gi, gd = sq.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(alone.cpu().numpy(), got), what
    want = O.separable_sq(mask, s)
    bad = int((got != want).sum())
    assert bad == 0, (what, "squared map differs from the oracle in %d of %d elements" % (bad, got.size))
    assert np.isfinite(got).all() and not got[mask == 0].any(), what
    if s is None:
        assert np.array_equal(got, np.rint(got)), what
        nbg = max(1, int((mask == 0).sum()))
        if mask.size * nbg <= BRUTE_PAIRS:
            assert np.array_equal(got.astype(np.int64), O.brute_sq_int(mask)), what
    ref = _scipy_edt(mask, s)
    ulp = O.ulp_distance(gd, ref)
    print("%s: %d elements, %d not identical to scipy's distance, largest distance %.2f ulp" % (
        what, gd.size, int((gd != ref).sum()), float(ulp.max())))
    assert float(ulp.max()) <= 1.0, (what, float(ulp.max()))
    O.check_indices(mask, s, got, gi)
    return got


@pytest.mark.parametrize("sampling", [None, (1.5, .41, .41)])
@pytest.mark.parametrize("shape", [(1, 37, 29), (7, 1, 23), (11, 19, 1), (2, 3, 2), (5, 5, 5), (3, 2, 1), (1, 1, 1)])
def test_line_lengths(shape, sampling):
    """extents 1, 2, 3 and 5 along each axis; each shape as a sparse, a dense and a foreground-only mask"""
    for bgd in (0.1, 0.7, 0.0):
        _check(random_mask("edt.gpu.len%s" % (shape,), shape, bgd), sampling, ("lengths", shape, bgd, sampling))


@pytest.mark.parametrize("k", LINE_COUNTS)
def test_d_pass_line_tiles(k):
    """H x W = k lines in the D pass: one less than a block's tile of lines, exactly a tile, one more, two tiles and five"""
    _check(random_mask("edt.gpu.dl", (9, 1, k), 0.08), (.7, 1.3, .9), ("D lines", k))


@pytest.mark.parametrize("k", LINE_COUNTS)
def test_h_pass_line_tiles(k):
    """D x W = k lines in the H pass"""
    _check(random_mask("edt.gpu.hl", (1, 9, k), 0.08), (.7, 1.3, .9), ("H lines", k))


@pytest.mark.parametrize("k", LINE_COUNTS)
def test_w_pass_line_tiles(k):
    """D x H = k lines in the W pass, and lines of length k in it"""
    _check(random_mask("edt.gpu.wl", (1, k, 9), 0.08), (.7, 1.3, .9), ("W lines", k))
    _check(random_mask("edt.gpu.wn", (1, 3, k), 0.08), (.7, 1.3, .9), ("W length", k))


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("n", [MAX_EXTENT - 1, MAX_EXTENT])
def test_longest_lines(axis, n):
    """the tile of the longest line takes the whole LDS of a CU; two background elements at its far ends and one near the
    middle make the search run the full length"""
    shape = [2, 3, 34]
    shape[axis] = n
    mask = np.ones(shape, np.uint8)
    mask[0, 0, 0] = mask[-1, -1, -1] = 0
    mask[tuple(v // 2 for v in shape)] = 0
    _check(mask, (1.5, .41, .41), ("longest", axis, n))
    _check(np.ones(shape, np.uint8), None, ("longest, no background", axis, n))


def test_an_extent_above_the_limit_is_refused():
    from fplx import image_process as P, ops
    for shape in ((MAX_EXTENT + 1, 2, 2), (2, MAX_EXTENT + 1, 2), (2, 2, MAX_EXTENT + 1), (MAX_EXTENT + 1, 2), (2, MAX_EXTENT + 1)):
        with pytest.raises(ValueError, match="limit of %d" % MAX_EXTENT):
            ops.edt_squared(torch.zeros(shape, dtype=torch.uint8, device="cuda:0"))
        with pytest.raises(ValueError, match="limit of %d" % MAX_EXTENT):
            P.distance_transform_edt(np.zeros(shape, np.uint8))
    with pytest.raises(ValueError, match="limit of %d" % MAX_EXTENT):
        P.get_euclidean_distance(np.zeros((2, MAX_EXTENT + 1, 2), np.uint8))


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("shape", [(37, 45), (1, 9), (9, 1), (2 * LINES + 5, 33)])
def test_2d(shape, sampling):
    for bgd in (0.05, 0.5, 0.0):
        _check(random_mask("edt.gpu.2d%s" % (shape,), shape, bgd), sampling, ("2D", shape, bgd, sampling))


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("background", [0.02, 0.5, 0.98])
def test_several_blocks_per_pass(background, sampling):
    shape = (40, 64, 64)
    _check(random_mask("edt.gpu.blocks.%g" % background, shape, background), sampling, ("blocks", background, sampling))


def _content_masks():
    shape = (11, 14, 37)
    corners = np.ones(shape, np.uint8)
    corners[0, 0, 0] = corners[-1, -1, -1] = 0
    one_fg = np.zeros(shape, np.uint8)
    one_fg[5, 7, 20] = 1
    checker = (np.indices(shape).sum(axis=0) % 2).astype(np.uint8)
    out = {"corners": corners, "single foreground": one_fg, "checkerboard": checker, "all background": np.zeros(shape, np.uint8),
           "all foreground": np.ones(shape, np.uint8), "all foreground 2D": np.ones((14, 37), np.uint8)}
    for a in range(3):
        plane = np.ones(shape, np.uint8)
        plane[tuple(slice(None) if k != a else shape[a] // 3 for k in range(3))] = 0
        out["plane %d" % a] = plane
    return out


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("name", sorted(_content_masks()))
def test_mask_content(name, sampling):
    mask = _content_masks()[name]
    got = _check(mask, sampling, (name, sampling))
    if name == "all background":
        assert not got.any()
    if name.startswith("all foreground"):                               # the phantom at (-1, 0, 0): the exact expression
        s = O.sampling_of(None if sampling is None else sampling[-mask.ndim:], mask.ndim)
        delta = np.moveaxis(np.indices(mask.shape).astype(np.float64), 0, -1)
        delta[..., 0] += 1.0
        assert np.array_equal(got, O.expression(delta, s))


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edt.npz"))
    return {k: z[k] for k in z.files}


def _signed_bound(sq_fg, sq_bg):
    """1 ulp of each of the two roots"""
    return np.spacing(np.sqrt(sq_fg.astype(np.float64))) + np.spacing(np.sqrt(sq_bg.astype(np.float64)))


@pytest.mark.parametrize("name", ["edt_a", "edt_b", "edt_c", "edt_d", "edt_e", "edt_zeros", "edt_ones"])
def test_get_euclidean_distance_against_the_reference(name):
    from fplx import image_process as P, ops
    z = _golden()
    assert name in [str(n) for n in z["names"]]
    img, signed = z[name + ".image"], z[name + ".signed"]
    both = _dev(np.stack([img > 0.5, img <= 0.5]).astype(np.uint8))
    sq = ops.edt_squared(both, batched=True).cpu().numpy()
    assert np.array_equal(sq[0], z[name + ".sq_fg"].astype(np.float64)), name
    assert np.array_equal(sq[1], z[name + ".sq_bg"].astype(np.float64)), name
    got = P.get_euclidean_distance(img)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == img.shape
    err = np.abs(got - signed)
    print("%s: %d of %d elements of the signed map not identical to the reference's" % (name, int((got != signed).sum()), got.size))
    assert (err <= _signed_bound(z[name + ".sq_fg"], z[name + ".sq_bg"])).all(), (name, float(err.max()))
    # spacing is accepted and ignored, as in the reference; float and device inputs give the same map
    assert np.array_equal(P.get_euclidean_distance(img.astype(np.float32), 3, [2.0, 0.5, 0.5]), got)
    dev = P.get_euclidean_distance(_dev(img))
    assert dev.is_cuda and dev.dtype == torch.float64 and np.array_equal(dev.cpu().numpy(), got)


def test_get_euclidean_distance_on_the_shipped_label_volume(golden_dir):
    from scipy import ndimage
    from fplx import image_process as P
    from fplx.nifti import load_nifty_volume_as_4d_array
    lab = load_nifty_volume_as_4d_array(os.path.join(golden_dir, "nifti", "vs_gk_98_t2_lab.nii.gz"))["data_array"][0]
    fg, bg = ndimage.distance_transform_edt(lab > 0.5), ndimage.distance_transform_edt(lab <= 0.5)
    got = P.get_euclidean_distance(lab)
    assert got.dtype == np.float64 and got.shape == lab.shape
    ref = bg - fg
    print("label volume %s: %d of %d elements of the signed map not identical to scipy's" % (
        lab.shape, int((got != ref).sum()), got.size))
    assert (np.abs(got - ref) <= np.spacing(fg) + np.spacing(bg)).all()
    d, ind = P.distance_transform_edt(lab, sampling=(1.5, .41, .41), return_indices=True)
    want = ndimage.distance_transform_edt(lab, sampling=(1.5, .41, .41))
    assert float(O.ulp_distance(d, want).max()) <= 1.0
    O.check_indices(lab, (1.5, .41, .41), O.separable_sq(lab, (1.5, .41, .41)), ind)


def test_device_in_device_out_and_batches():
    from fplx import image_process as P, ops
    masks = np.stack([random_mask("edt.gpu.batch%d" % i, (9, 35, 41), b) for i, b in enumerate((0.03, 0.5, 0.0, 1.0))])
    dev = _dev(masks)
    for s in (None, (1.5, .41, .41)):
        sq, idx = ops.edt_squared(dev, s, return_indices=True, batched=True)
        assert tuple(sq.shape) == masks.shape and tuple(idx.shape) == (4, 3, 9, 35, 41)
        for i in range(4):
            one_sq, one_idx = ops.edt_squared(dev[i].contiguous(), s, return_indices=True)
            assert torch.equal(sq[i], one_sq) and torch.equal(idx[i], one_idx), (i, s)
            d, di = P.distance_transform_edt(dev[i], sampling=s, return_indices=True)
            assert d.is_cuda and di.is_cuda and d.dtype == torch.float64 and di.dtype == torch.int32
            assert torch.equal(d, ops.edt_finish(one_sq)) and torch.equal(di, one_idx)
    two = _dev(masks[0, 0])
    sq2, idx2 = ops.edt_squared(_dev(masks[:, 0]), (.41, .41), return_indices=True, batched=True)
    assert tuple(idx2.shape) == (4, 2, 35, 41) and torch.equal(sq2[0], ops.edt_squared(two, (.41, .41)))
    assert torch.equal(ops.edt_finish(sq[0], sq[1]), ops.edt_finish(sq[1]) - ops.edt_finish(sq[0]))


@pytest.mark.parametrize("shape", [(2, 9, 35, 41), (1, 1, 2 * LINES + 5, 33), (3, 5, 1, 7)])
def test_single_passes_compose_the_transform(shape):
    """fplx_edt_pass along axes 0, 1, 2 on g0 = 0 / +inf is the squared transform; one pass alone is the oracle's line minimum"""
    from fplx import ops
    masks = np.stack([random_mask("edt.gpu.pass%d" % i, shape[1:], 0.05) for i in range(shape[0])])
    masks[(slice(None),) + tuple(v // 2 for v in shape[1:])] = 0        # every mask has background: no phantom in this test
    s = (.7, 1.3, .9)
    g0 = np.where(masks != 0, np.inf, 0.0)
    g = _dev(g0)
    for axis in range(3):
        assert ops.edt_pass(g, axis, s[axis]) is g
    assert torch.equal(g, ops.edt_squared(_dev(masks), s, batched=True))
    for axis in range(3):                                   # one pass on the raw map: +inf lines stay +inf
        one = ops.edt_pass(_dev(g0), axis, s[axis]).cpu().numpy()
        pos = np.arange(shape[1 + axis], dtype=np.float64)
        t = (pos[:, None] - pos[None, :]) * s[axis]
        want = (np.moveaxis(g0, 1 + axis, -1)[..., None, :] + t * t).min(axis=-1)
        assert np.array_equal(one, np.moveaxis(want, -1, 1 + axis)), axis


def test_numpy_in_numpy_out_and_any_dtype():
    from fplx import image_process as P
    mask = random_mask("edt.gpu.np", (6, 17, 33), 0.1)
    d, ind = P.distance_transform_edt(mask, return_indices=True)
    assert isinstance(d, np.ndarray) and d.dtype == np.float64 and d.shape == mask.shape
    assert isinstance(ind, np.ndarray) and ind.dtype == np.int32 and ind.shape == (3,) + mask.shape
    only = P.distance_transform_edt(mask, return_distances=False, return_indices=True)
    assert isinstance(only, np.ndarray) and np.array_equal(only, ind)
    values = detdata.normal("edt.gpu.np.v", mask.shape) * mask                      # nonzero = foreground, of any dtype and sign
    for a in (values, values.astype(np.float32), mask.astype(bool), mask.astype(np.int64) * -3, mask[::1].astype(np.float64)):
        assert np.array_equal(P.distance_transform_edt(a), d), a.dtype
    assert np.array_equal(P.distance_transform_edt(mask, sampling=2), P.distance_transform_edt(mask, sampling=(2, 2, 2)))
    assert np.array_equal(P.distance_transform_edt(_dev(values)).cpu().numpy(), d)
    assert np.array_equal(P.distance_transform_edt(np.asfortranarray(mask)), d)    # a strided input is made contiguous


def test_two_runs_are_bitwise_equal():
    from fplx import ops
    dev = _dev(random_mask("edt.gpu.twice", (40, 64, 64), 0.01))
    a, ai = ops.edt_squared(dev, (.7, 1.3, .9), return_indices=True)
    b, bi = ops.edt_squared(dev, (.7, 1.3, .9), return_indices=True)
    assert torch.equal(a, b) and torch.equal(ai, bi) and torch.equal(ops.edt_finish(a), ops.edt_finish(b))
