"""numpy restatement of the crop, bounding-box and label feature: the four kernels of csrc/crop_label.hip (plus the plain
crop they are combined with) and the eight transforms built on them (fplx.transform.CenterCrop, CropWithBoundingBox,
RandomResizedCrop, LabelConvert, LabelConvertNonzero, PartialLabelToProbability, ReduceLabelDim, GrayscaleToRGB, and
RandomCrop with the inverse it gained), on numpy samples.  It states the RULES - which voxels count as non-zero, how a
box that runs past the volume is truncated, what the table of a label conversion holds, in which order the draws are
made - independently of the product code; tests/test_crop_label_cpu.py holds it against the reference's own results
(tests/golden/crop_label.npz) bit for bit, and the GPU tests hold the kernels against it.

Also here, shared by the fixture generator and the tests: the deterministic inputs and the table of fixture cases."""
import json
import random

import numpy as np

import detdata
import resample_ref as R

INT_MAX = 0x7fffffff
VOL = (9, 20, 23)
PLANE = (37, 41)


# ---- the kernels

def nonzero_bbox(x):
    """-> (count, lo[4], hi[4]) of the float32 volume's non-zero voxels: every bit pattern but +0.0 / -0.0 counts (NaN does);
    hi is the largest index + 1; count 0 -> lo = INT_MAX, hi = 0 (what the kernel leaves)"""
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 4
    hit = (x.view(np.uint32) & np.uint32(0x7fffffff)) != 0
    idx = np.nonzero(hit)
    if idx[0].size == 0:
        return 0, [INT_MAX] * 4, [0] * 4
    return int(idx[0].size), [int(i.min()) for i in idx], [int(i.max()) + 1 for i in idx]


def lut_table(sources, targets):
    """table of a label conversion on uint8: entry v = sum of the targets whose source is v, modulo 256"""
    assert len(sources) == len(targets)
    return [sum(t for s, t in zip(sources, targets) if s == v) % 256 for v in range(256)]


def label_lut(label, lut):
    assert label.dtype == np.uint8 and len(lut) == 256
    return np.asarray(lut, np.uint8)[label]


def partial_label(label, class_num):
    """-> one-hot fp32 [class_num, *shape], weight fp32 [*shape] (0 where the label is class_num), the largest label"""
    assert label.dtype == np.uint8
    prob = np.stack([(label == k) for k in range(class_num)]).astype(np.float32)
    weight = np.where(label == class_num, np.float32(0), np.float32(1)).astype(np.float32)
    return prob, weight, int(label.max())


def paste_roi(sub, lower, out_size):
    """zeros [C, *out_size] with sub [C,d,h,w] at `lower`; the box must lie inside"""
    c, sd, sh, sw = sub.shape
    for lo, s, o in zip(lower, (sd, sh, sw), out_size):
        if lo < 0 or lo + s > o:
            raise ValueError("paste_roi: box outside the output volume")
    out = np.zeros((c,) + tuple(int(v) for v in out_size), sub.dtype)
    out[:, lower[0]:lower[0] + sd, lower[1]:lower[1] + sh, lower[2]:lower[2] + sw] = sub
    return out


def crop(x, lower, size):
    """fplx_crop_flip without a flip: the box must lie inside the volume"""
    for lo, s, n in zip(lower, size, x.shape[1:]):
        if lo < 0 or s <= 0 or lo + s > n:
            raise ValueError("crop: box outside the volume")
    return np.ascontiguousarray(x[:, lower[0]:lower[0] + size[0], lower[1]:lower[1] + size[1], lower[2]:lower[2] + size[2]])


def zoom_plane(x, out_hw, order):
    """scipy.ndimage.zoom of a [C,h,w] array to [C,*out_hw] (channel zoom 1) through the resampling restatement, the plane
    as a depth-1 volume"""
    vol = x[:, None]
    out = [1, int(out_hw[0]), int(out_hw[1])]
    m, t = R.zoom_affine(vol.shape[1:], out)
    return R.resample_affine(vol, m, t, out, order)[:, 0]


# ---- the transforms (numpy samples; `p`: the lower-cased parameter dictionary)

SPATIAL = ("label", "pixel_weight", "image1")


class _Crop(object):
    name = None

    def __init__(self, p):
        self.p = p

    def box(self, sample):
        """-> lower corner [3] and untruncated upper corner [3]; subclasses draw / measure here"""
        raise NotImplementedError

    def __call__(self, sample):
        shape = list(sample["image"].shape)
        lo, hi = self.box(sample)
        sample[self.name + "_Param"] = json.dumps([shape, [0] + lo, [shape[0]] + hi])
        size = [min(hi[i], shape[1 + i]) - lo[i] for i in range(3)]
        for k in ("image",) + SPATIAL:
            if k in sample:
                sample[k] = crop(sample[k], lo, size)
        return sample

    def inverse(self, sample):
        p = sample[self.name + "_Param"]
        shape, lo, _ = json.loads(p[0] if isinstance(p, (list, tuple)) else p)

        def one(q):
            n, c = q.shape[:2]
            return paste_roi(q.reshape((n * c,) + q.shape[2:]), lo[1:], shape[1:]).reshape((n, c) + tuple(shape[1:]))

        q = sample["predict"]
        sample["predict"] = [one(v) for v in q] if isinstance(q, (list, tuple)) else one(q)
        return sample

    inverse_transform_for_prediction = inverse


class CenterCrop(_Crop):
    name = "CenterCrop"

    def box(self, sample):
        shape = sample["image"].shape[1:]
        size = [shape[0] if self.p["centercrop_output_size"][0] is None else self.p["centercrop_output_size"][0]]
        size += list(self.p["centercrop_output_size"][1:])
        if any(s > n for s, n in zip(size, shape)):
            raise ValueError("CenterCrop: output size exceeds the volume")
        lo = [int((n - s) / 2) for n, s in zip(shape, size)]
        return lo, [a + s for a, s in zip(lo, size)]


class CropWithBoundingBox(_Crop):
    name = "CropWithBoundingBox"

    def __init__(self, p):
        super(CropWithBoundingBox, self).__init__(p)
        if p["cropwithboundingbox_start"] is not None and p["cropwithboundingbox_output_size"] is None:
            raise ValueError("CropWithBoundingBox: a start needs an output size")

    def box(self, sample):
        start, size = self.p["cropwithboundingbox_start"], self.p["cropwithboundingbox_output_size"]
        count, b0, b1 = nonzero_bbox(sample["image"])
        if count == 0:
            raise ValueError("CropWithBoundingBox: all-zero image")
        b0, b1 = b0[1:], b1[1:]
        if start is not None:
            lo = list(start)
        elif size is None:
            return b0, b1
        else:
            lo = [max(0, int((b0[i] + b1[i] + 1) / 2) - int(size[i] / 2)) for i in range(3)]
        return lo, [lo[i] + size[i] for i in range(3)]


class RandomCrop(_Crop):
    name = "RandomCrop"

    def box(self, sample):
        shape = sample["image"].shape[1:]
        size = list(self.p["randomcrop_output_size"])
        if size[0] is None:
            size[0] = shape[0]
        lo = [random.randint(0, n - s) if n != s else 0 for n, s in zip(shape, size)]
        if self.p.get("randomcrop_foreground_focus", False) and random.random() < self.p.get("randomcrop_foreground_ratio", 0.5):
            mask = np.isin(sample["label"], list(self.p.get("randomcrop_mask_label", [1])))
            idx = np.nonzero(mask)
            if idx[0].size:
                b0, b1 = [int(i.min()) for i in idx][1:], [int(i.max()) + 1 for i in idx][1:]
            else:
                b0, b1 = [0, 0, 0], list(shape)
            lo = [random.randint(b0[i], b1[i]) - int(size[i] / 2) for i in range(3)]
            lo = [min(max(0, lo[i]), shape[i] - size[i]) for i in range(3)]
        return lo, [a + s for a, s in zip(lo, size)]


class RandomResizedCrop(object):
    def __init__(self, p):
        self.p = p

    def __call__(self, sample):
        shape = list(sample["image"].shape)
        assert len(shape) == 3
        out, sc, ra = (self.p["randomresizedcrop_" + k] for k in ("output_size", "scale", "ratio"))
        assert len(out) == 2
        scale = sc[0] + random.random() * (sc[1] - sc[0])
        ratio = ra[0] + random.random() * (ra[1] - ra[0])
        w = shape[2] * scale
        h = min(w * ratio, shape[1])
        size = [int(h), int(w)]
        lo = [random.randint(0, shape[1 + i] - size[i]) for i in range(2)]
        sample["RandomResizedCrop_Param"] = json.dumps([shape, [0] + lo, [shape[0]] + [lo[i] + size[i] for i in range(2)]])
        for k, order in (("image", 1), ("label", 0), ("pixel_weight", 1)):
            if k in sample:
                c = sample[k][:, lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1]]
                sample[k] = zoom_plane(np.ascontiguousarray(c), out, order)
        return sample


class LabelConvert(object):
    def __init__(self, p):
        s, t = p["labelconvert_source_list"], p["labelconvert_target_list"]
        if any(not 0 <= v <= 255 for v in list(s) + list(t)):
            raise ValueError("LabelConvert: labels outside 0..255")
        self.lut = lut_table(s, t)

    def __call__(self, sample):
        sample["label"] = label_lut(sample["label"], self.lut)
        return sample


class LabelConvertNonzero(object):
    def __init__(self, p):
        pass

    def __call__(self, sample):
        sample["label"] = label_lut(sample["label"], [0] + [1] * 255)
        return sample


class PartialLabelToProbability(object):
    def __init__(self, p):
        self.class_num = p["partiallabeltoprobability_class_num"]

    def __call__(self, sample):
        prob, weight, top = partial_label(sample["label"][0], self.class_num)
        assert top <= self.class_num
        sample["label_prob"], sample["pixel_weight"] = prob, weight[None]
        return sample


class LabelToProbability(object):
    def __init__(self, p):
        self.class_num = p["labeltoprobability_class_num"]

    def __call__(self, sample):
        sample["label_prob"] = partial_label(sample["label"][0], self.class_num)[0]
        return sample


class ReduceLabelDim(object):
    def __init__(self, p):
        pass

    def __call__(self, sample):
        sample["label"] = sample["label"][0]
        return sample


class GrayscaleToRGB(object):
    def __init__(self, p):
        pass

    def __call__(self, sample):
        c = sample["image"].shape[0]
        assert c in (1, 3)
        if c == 1:
            sample["image"] = np.repeat(sample["image"], 3, axis=0)
        return sample


TRANSFORMS = {c.__name__: c for c in (CenterCrop, CropWithBoundingBox, RandomCrop, RandomResizedCrop, LabelConvert,
                                      LabelConvertNonzero, PartialLabelToProbability, LabelToProbability, ReduceLabelDim,
                                      GrayscaleToRGB)}
NEW_NAMES = ("CenterCrop", "CropWithBoundingBox", "RandomResizedCrop", "LabelConvert", "LabelConvertNonzero",
             "PartialLabelToProbability", "ReduceLabelDim", "GrayscaleToRGB")


# ---- deterministic inputs and the fixture cases

def inputs():
    """image_a: two channels, zero outside an inner block each, a NaN in the last voxel and a -0.0 in the first row: the box
    of its non-zero voxels is [0,2,5,4]..[2,9,20,23].  image_b / image_c: one non-zero voxel, the first / the last."""
    d, h, w = VOL
    a = np.zeros((2,) + VOL, np.float32)
    a[0, 2:7, 5:16, 4:19] = detdata.normal("cl.image_a0", (5, 11, 15)) * 37.0 + 210.0
    a[1, 3:6, 8:12, 9:15] = detdata.normal("cl.image_a1", (3, 4, 6)) * 37.0 + 210.0
    a[1, d - 1, h - 1, w - 1] = np.nan
    a[0, 0, 0, 3] = -0.0
    b = np.zeros((2,) + VOL, np.float32)
    b[0, 0, 0, 0] = 3.5
    c = np.zeros((2,) + VOL, np.float32)
    c[1, d - 1, h - 1, w - 1] = -2.25
    label = np.minimum(detdata.uniform("cl.label", (1,) + VOL) * 5.0, 4.0).astype(np.uint8)
    plane_label = np.minimum(detdata.uniform("cl.plane_label", (1,) + PLANE) * 5.0, 4.0).astype(np.uint8)
    return {
        "image_a": a, "image_b": b, "image_c": c, "label": label,
        "pixel_weight": (detdata.uniform("cl.pw", (1,) + VOL) > 0.3).astype(np.float32) * np.float32(0.73),
        "image1": (detdata.normal("cl.image1", (2,) + VOL) * 11.0 + 3.0).astype(np.float32),
        "volume1": (detdata.normal("cl.volume1", (1,) + VOL) * 37.0 + 210.0).astype(np.float32),
        "plane": (detdata.normal("cl.plane", (3,) + PLANE) * 37.0 + 210.0).astype(np.float32),
        "plane1": (detdata.normal("cl.plane1", (1,) + PLANE) * 37.0 + 210.0).astype(np.float32),
        "plane_label": plane_label,
        "plane_weight": detdata.uniform("cl.plane_pw", (1,) + PLANE),
    }


def prediction(name, shape):
    return (detdata.normal(name, shape) * 3.0).astype(np.float32)


def _cwb(start, size):
    return {"cropwithboundingbox_start": start, "cropwithboundingbox_output_size": size}


_FULL = {"image": "image_a", "label": "label", "pixel_weight": "pixel_weight", "image1": "image1"}
_PLANE = {"image": "plane", "label": "plane_label", "pixel_weight": "plane_weight"}
_LABEL = {"image": "image_a", "label": "label", "pixel_weight": "pixel_weight"}
_RRC = {"randomresizedcrop_output_size": [24, 20], "randomresizedcrop_scale": [0.3, 1.0],
        "randomresizedcrop_ratio": [0.75, 1.33]}
_CHAIN = dict(_cwb(None, None), labelconvert_source_list=[0, 1, 2, 4], labelconvert_target_list=[0, 1, 2, 3],
              randomcrop_output_size=[4, 8, 9], randomcrop_foreground_focus=True, randomcrop_foreground_ratio=0.5,
              randomcrop_mask_label=[1, 2], labeltoprobability_class_num=4)
_CHAIN_NAMES = ["CropWithBoundingBox", "LabelConvert", "RandomCrop", "LabelToProbability"]


def _inv(of, channels=3, count=1, collated=False):
    return {"of": of, "channels": channels, "count": count, "collated": collated}


CASES = {
    "cwb_box": dict(names=["CropWithBoundingBox"], params=_cwb(None, None), sample=_FULL, inverse=_inv("CropWithBoundingBox")),
    "cwb_size": dict(names=["CropWithBoundingBox"], params=_cwb(None, [4, 8, 30]), sample=_FULL,
                     inverse=_inv("CropWithBoundingBox", count=2)),
    "cwb_start": dict(names=["CropWithBoundingBox"], params=_cwb([1, 2, 3], [4, 8, 9]), sample=_FULL,
                      inverse=_inv("CropWithBoundingBox", collated=True)),
    "cwb_far": dict(names=["CropWithBoundingBox"], params=_cwb([7, 15, 20], [4, 8, 9]), sample=_FULL,
                    inverse=_inv("CropWithBoundingBox")),
    "cwb_first": dict(names=["CropWithBoundingBox"], params=_cwb(None, None), sample={"image": "image_b"},
                      inverse=_inv("CropWithBoundingBox")),
    "cwb_last": dict(names=["CropWithBoundingBox"], params=_cwb(None, None), sample={"image": "image_c"},
                     inverse=_inv("CropWithBoundingBox")),
    "cc_keep": dict(names=["CenterCrop"], params={"centercrop_output_size": [None, 8, 9]}, sample=_FULL,
                    inverse=_inv("CenterCrop")),
    "cc_all": dict(names=["CenterCrop"], params={"centercrop_output_size": [5, 8, 9]}, sample=_FULL,
                   inverse=_inv("CenterCrop", count=2, collated=True)),
    "rrc_seed1": dict(names=["RandomResizedCrop"], params=_RRC, sample=_PLANE, seed=1),
    "rrc_seed2": dict(names=["RandomResizedCrop"], params=_RRC, sample=_PLANE, seed=2),
    "rrc_seed3": dict(names=["RandomResizedCrop"], params=_RRC, sample=_PLANE, seed=3),
    "lc_dup": dict(names=["LabelConvert"], sample=_LABEL,
                   params={"labelconvert_source_list": [1, 2, 4, 4], "labelconvert_target_list": [3, 1, 200, 100]}),
    "lc_brats": dict(names=["LabelConvert"], sample=_LABEL,
                     params={"labelconvert_source_list": [0, 1, 2, 4], "labelconvert_target_list": [0, 1, 2, 3]}),
    "lcn": dict(names=["LabelConvertNonzero"], params={}, sample=_LABEL),
    "pl2p": dict(names=["PartialLabelToProbability"], params={"partiallabeltoprobability_class_num": 4}, sample=_LABEL),
    "rld": dict(names=["ReduceLabelDim"], params={}, sample=_LABEL),
    "rgb_plane1": dict(names=["GrayscaleToRGB"], params={}, sample={"image": "plane1"}),
    "rgb_plane3": dict(names=["GrayscaleToRGB"], params={}, sample={"image": "plane"}),
    "rgb_volume1": dict(names=["GrayscaleToRGB"], params={}, sample={"image": "volume1"}),
    "chain_seed1": dict(names=_CHAIN_NAMES, params=_CHAIN, sample=_FULL, seed=1, inverse=_inv("RandomCrop", channels=4)),
    "chain_seed2": dict(names=_CHAIN_NAMES, params=_CHAIN, sample=_FULL, seed=2, inverse=_inv("RandomCrop", channels=4)),
}
SAMPLE_KEYS = ("image", "label", "pixel_weight", "image1", "label_prob")


def run_case(case, transforms, inp, to_sample=lambda a: a.copy(), seed_fn=None):
    """runs one fixture case with the classes of the mapping `transforms` (this module's TRANSFORMS, or the product's
    TransformDict) -> (transform objects, final sample); to_sample converts an input array to what the classes take"""
    c = CASES[case]
    if "seed" in c:
        random.seed(c["seed"])
        np.random.seed(c["seed"])
    ts = [transforms[n](dict(c["params"], task="segmentation")) for n in c["names"]]
    sample = {k: to_sample(inp[v]) for k, v in c["sample"].items()}
    for t in ts:
        sample = t(sample)
    return ts, sample


# ---- holding a run against the fixture: equality, nothing else

def assert_same(got, want, what):
    """same shape, same dtype, NaNs in the same places and every other element bit for bit (so -0.0 is not 0.0)"""
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype != np.float32:
        assert np.array_equal(got, want), what
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    a, b = np.ascontiguousarray(got)[~nan], np.ascontiguousarray(want)[~nan]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def check_case(g, case, transforms, inp, to_sample=lambda a: a.copy(), to_numpy=lambda t: t):
    """one fixture case through the classes of `transforms`: outputs, parameter strings, the position of Python's generator
    after the draws, and the inverse on the stored prediction(s) - all equal to what the reference left in the fixture g"""
    c = CASES[case]
    ts, s = run_case(case, transforms, inp, to_sample)
    for k in SAMPLE_KEYS:
        key = "%s_%s" % (case, k)
        assert (k in s) == (key in g.files), (case, k)
        if k in s:
            assert_same(to_numpy(s[k]), g[key], key)
    params = [k for k in g.files if k.startswith(case + "_") and k.endswith("_Param")]
    assert len(params) == sum(1 for n in c["names"] if n in ("CenterCrop", "CropWithBoundingBox", "RandomCrop", "RandomResizedCrop"))
    for key in params:
        assert s[key[len(case) + 1:]] == str(g[key]), key                    # the very string
    if "seed" in c:
        assert random.random() == float(g[case + "_next_random"]), case
    inv = c.get("inverse")
    if not inv:
        return s
    t = ts[c["names"].index(inv["of"])]
    preds = [g["%s_predict%s" % (case, "" if i == 0 else i)] for i in range(inv["count"])]
    for i, p in enumerate(preds):                                            # the stored predictions are the named ones
        assert np.array_equal(p, prediction("%s.predict%d" % (case, i), p.shape))
    pk = inv["of"] + "_Param"
    q = {pk: [str(g[case + "_" + pk])] if inv["collated"] else str(g[case + "_" + pk]),
         "predict": [to_sample(p) for p in preds] if inv["count"] > 1 else to_sample(preds[0])}
    q = t.inverse_transform_for_prediction(q)
    assert isinstance(q["predict"], list) == (inv["count"] > 1), case
    got = q["predict"] if inv["count"] > 1 else [q["predict"]]
    for i, v in enumerate(got):
        assert_same(to_numpy(v), g["%s_inverse%s" % (case, "" if i == 0 else i)], (case, "inverse", i))
    return s
