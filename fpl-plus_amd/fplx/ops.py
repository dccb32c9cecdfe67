"""Tensor-level wrappers over the C ABI (include/fplx.h).  PyTorch is only plumbing here:
device memory, the current HIP stream and dtype tags.  Activations are 2-D views
[voxels, ld] of NDHWC tensors; a column slice `buf[:, a:b]` is a channel slice.
"""
import ctypes
import math

import numpy as np
import torch
from . import _lib
from ._lib import F32, BF16, call

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dt_of(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise ValueError("fplx: unsupported activation dtype {0:}".format(t.dtype))


def ptr(t):
    return 0 if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def require_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("fplx: tensors must live on the GPU (HIP path only, no CPU fallback)")


def cl_strides(D, H, W, ld):
    """element strides (n,d,h,w,c) of an NDHWC tensor with voxel stride ld"""
    return (D * H * W * ld, H * W * ld, W * ld, ld, 1)


def planar_strides(C, D, H, W):
    """element strides (n,d,h,w,c) of a contiguous NCDHW tensor"""
    return (C * D * H * W, H * W, W, 1, D * H * W)


def ld_of(t2d):
    assert t2d.dim() == 2 and t2d.stride(1) == 1
    return t2d.stride(0)


def pack_conv_weight(w, act_dtype, want_wb=True):
    co, ci, kd, kh, kw = w.shape
    wf = torch.empty((kd * kh * kw, co, ci), dtype=act_dtype, device=w.device)
    wb = torch.empty((kd * kh * kw, ci, co), dtype=act_dtype, device=w.device) if want_wb else None
    call("fplx_pack_conv_weight", ptr(w), ptr(wf), ptr(wb), co, ci, kd, kh, kw, _DT[act_dtype], stream())
    return wf, wb


def pack_stamp_floats(cout, cin):
    """floats of a layer's stamp buffer (include/fplx.h, fplx_pack_conv_weights_batched): 32 per 16 x 32-channel pack tile"""
    return (cout // 16) * (cin // 32) * 32


def pack_conv_weights_batched(ws, act_dtype, want_wb, into=None, stamps=None, verify=False):
    """pack_conv_weight for a list of 3x3x3 weights in one launch -> list of (wf, wb).
    into: optional list of existing (wf, wb) destinations (None entries: allocate) - the engine's persistent pack buffers
    stamps: optional list of per-layer fp32 stamp buffers (pack_stamp_floats; None entries: none) that record which master values
    each pack tile was made from; verify=True: `into` and `stamps` hold an earlier pack - only the tiles whose masters changed
    since are packed again (one cheap launch when nothing changed)"""
    import ctypes
    n = len(ws)
    outs = []
    for i, (w, wantb) in enumerate(zip(ws, want_wb)):
        co, ci = w.shape[0], w.shape[1]
        assert tuple(w.shape[2:]) == (3, 3, 3) and w.dtype == torch.float32 and w.is_contiguous()
        if into is not None and into[i] is not None:
            outs.append(into[i])
            continue
        assert not verify, "verify needs the earlier pack (into)"
        wf = torch.empty((27, co, ci), dtype=act_dtype, device=w.device)
        wb = torch.empty((27, ci, co), dtype=act_dtype, device=w.device) if wantb else None
        outs.append((wf, wb))
    vp = ctypes.c_void_p * n
    ip = ctypes.c_int * n
    st = None
    if stamps is not None:
        for w, s_ in zip(ws, stamps):
            assert s_ is None or (s_.dtype == torch.float32 and s_.numel() >= pack_stamp_floats(w.shape[0], w.shape[1]))
        st = vp(*[ptr(s_) or None for s_ in stamps])
    call("fplx_pack_conv_weights_batched", n, vp(*[ptr(w) for w in ws]), vp(*[ptr(o[0]) for o in outs]),
         vp(*[ptr(o[1]) or None for o in outs]), ip(*[w.shape[0] for w in ws]), ip(*[w.shape[1] for w in ws]),
         _DT[act_dtype], st, 1 if verify else 0, stream())
    return outs


def pack_weights_multi(jobs):
    """jobs: [(kind, w fp32 contiguous, wf or None, wb or None, a, b, taps)] (kind 0: conv weight [a = Cout][b = Cin][taps];
    1: transposed conv [a = Cin][b = Cout][taps]) - all of them in ONE launch (fplx_pack_weights_multi)"""
    import ctypes
    n = len(jobs)
    vp, ip = ctypes.c_void_p * n, ctypes.c_int * n
    dts = [_DT[(j[2] if j[2] is not None else j[3]).dtype] for j in jobs]
    call("fplx_pack_weights_multi", n, ip(*[j[0] for j in jobs]), vp(*[ptr(j[1]) for j in jobs]), vp(*[ptr(j[2]) or None for j in jobs]),
         vp(*[ptr(j[3]) or None for j in jobs]), ip(*[j[4] for j in jobs]), ip(*[j[5] for j in jobs]), ip(*[j[6] for j in jobs]),
         ip(*dts), stream())


def pack_deconv_weight(w, act_dtype):
    """ConvTranspose3d weight [Cin,Cout,2,2,2] (8 taps) or ConvTranspose2d weight [Cin,Cout,2,2] (4 taps)"""
    ci, co = w.shape[0], w.shape[1]
    taps = 8 if w.dim() == 5 else 4
    wf = torch.empty((taps, co, ci), dtype=act_dtype, device=w.device)
    wb = torch.empty((taps, ci, co), dtype=act_dtype, device=w.device)
    call("fplx_pack_deconv_weight" if taps == 8 else "fplx_pack_deconv122_weight", ptr(w), ptr(wf), ptr(wb), ci, co,
         _DT[act_dtype], stream())
    return wf, wb


def pack_conv2d_weight(w, act_dtype, want_wb=True):
    """Conv2d weight [Cout,Cin,3,3] -> the 27-tap layouts of pack_conv_weight with the 9 taps in the middle depth plane"""
    co, ci = w.shape[0], w.shape[1]
    wf = torch.empty((27, co, ci), dtype=act_dtype, device=w.device)
    wb = torch.empty((27, ci, co), dtype=act_dtype, device=w.device) if want_wb else None
    call("fplx_pack_conv2d_weight", ptr(w), ptr(wf), ptr(wb), co, ci, _DT[act_dtype], stream())
    return wf, wb


def conv3d_stats_rows(dims, cin, cout, k, x_dt, y_dt, mid=False):
    """mid: the pack is a Conv2d in the middle depth plane (pack_conv2d_weight) - the fplx_conv2d_* form"""
    n, d, h, w = dims
    if mid:
        return _lib.lib().fplx_conv2d_stats_rows(n, d, h, w, cin, cout, x_dt, y_dt)
    return _lib.lib().fplx_conv3d_stats_rows(n, d, h, w, cin, cout, k[0], k[1], k[2], x_dt, y_dt)


def conv3d_fwd_ws_bytes(dims, cin, cout, k, x_dt, y_dt, mid=False):
    n, d, h, w = dims
    if mid:
        return _lib.lib().fplx_conv2d_fwd_ws_bytes(n, d, h, w, cin, cout, x_dt, y_dt)
    return _lib.lib().fplx_conv3d_fwd_ws_bytes(n, d, h, w, cin, cout, k[0], k[1], k[2], x_dt, y_dt)


_fwd_ws = {}


def _fwd_scratch(need, device):
    """scratch of `need` bytes for the split-K forward kernels (None for 0), per (device, stream): launches on one stream are
    ordered and may share it, launches on different streams (the engine runs two) may not"""
    if not need:
        return None
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    if key not in _fwd_ws or _fwd_ws[key].numel() < need:
        _fwd_ws[key] = torch.empty(int(need), dtype=torch.uint8, device=device)
    return _fwd_ws[key]


def conv3d_fwd(x, xs, x_dt, wp, bias, y, ys, y_dt, dims, cin, cout, k, stats=None, ws=None, mid=False):
    n, d, h, w = dims
    if ws is None:
        ws = _fwd_scratch(conv3d_fwd_ws_bytes(dims, cin, cout, k, x_dt, y_dt, mid), y.device)
    nws = 0 if ws is None else ws.numel() * ws.element_size()
    if mid:
        assert tuple(k) == (3, 3, 3)
        call("fplx_conv2d_fwd", ptr(x), x_dt, xs[0], xs[1], xs[2], xs[3], xs[4], ptr(wp), ptr(bias),
             ptr(y), y_dt, ys[0], ys[1], ys[2], ys[3], ys[4], n, d, h, w, cin, cout, ptr(stats), ptr(ws), nws, stream())
        return
    call("fplx_conv3d_fwd", ptr(x), x_dt, xs[0], xs[1], xs[2], xs[3], xs[4], ptr(wp), ptr(bias),
         ptr(y), y_dt, ys[0], ys[1], ys[2], ys[3], ys[4], n, d, h, w, cin, cout, k[0], k[1], k[2],
         ptr(stats), ptr(ws), nws, stream())


def conv3d_wgrad_ws_bytes(dims, cin, cout, k):
    n, d, h, w = dims
    return _lib.lib().fplx_conv3d_wgrad_ws_bytes(n, d, h, w, cin, cout, k[0], k[1], k[2])


def conv3d_wgrad(x, xs, x_dt, dy, ys, dy_dt, dw, db, dims, cin, cout, k, ws):
    n, d, h, w = dims
    call("fplx_conv3d_wgrad", ptr(x), x_dt, xs[0], xs[1], xs[2], xs[3], xs[4],
         ptr(dy), dy_dt, ys[0], ys[1], ys[2], ys[3], ys[4], ptr(dw), ptr(db), n, d, h, w, cin, cout,
         k[0], k[1], k[2], ptr(ws), ws.numel() * ws.element_size(), stream())


def conv2d_wgrad_ws_bytes(dims, cin, cout):
    n, d, h, w = dims
    return _lib.lib().fplx_conv2d_wgrad_ws_bytes(n, d, h, w, cin, cout)


def conv2d_wgrad(x, xs, x_dt, dy, ys, dy_dt, dw9, db, dims, cin, cout, ws):
    """weight gradient of a Conv2d(3x3) per depth slice: dw9 fp32 [Cout, Cin, 3, 3] (9 of 27 taps on the MFMA path)"""
    n, d, h, w = dims
    call("fplx_conv2d_wgrad", ptr(x), x_dt, xs[0], xs[1], xs[2], xs[3], xs[4], ptr(dy), dy_dt, ys[0], ys[1], ys[2], ys[3],
         ys[4], ptr(dw9), ptr(db), n, d, h, w, cin, cout, ptr(ws), ws.numel() * ws.element_size(), stream())


def conv3d_cat2_ok(dims, cin, cout):
    """True if the 3x3x3 convolution on cat([x0, x1], channel) of two cin/2-channel bf16 tensors has the split fast
    path (level 0 of the 32-base network): the concatenation is then never materialised."""
    n, d, h, w = dims
    return _lib.lib().fplx_conv3d_cat2_ok(n, d, h, w, cin, cout) == 1


def conv3d_fwd_cat2(x0, x1, wp, bias, y, dims, cin, cout, stats=None, mid=False):
    n, d, h, w = dims
    assert ld_of(x0) == ld_of(x1)
    call("fplx_conv2d_fwd_cat2" if mid else "fplx_conv3d_fwd_cat2", ptr(x0), ptr(x1), ld_of(x0), ptr(wp), ptr(bias), ptr(y), ld_of(y), n, d, h, w, cin,
         cout, ptr(stats), stream())


def conv3d_dgrad_split2(dy, wb, dx0, dx1, dims, cin, cout, mid=False):
    n, d, h, w = dims
    assert ld_of(dx0) == ld_of(dx1)
    call("fplx_conv2d_dgrad_split2" if mid else "fplx_conv3d_dgrad_split2", ptr(dy), ld_of(dy), ptr(wb), ptr(dx0), ptr(dx1), ld_of(dx0), n, d, h, w, cin,
         cout, stream())


def conv3d_wgrad_cat2(x0, x1, dy, dw, dims, cin, cout, ws, mid=False):
    """mid: dw is the 9-tap Conv2d gradient [Cout, Cin, 3, 3]"""
    n, d, h, w = dims
    assert ld_of(x0) == ld_of(x1)
    call("fplx_conv2d_wgrad_cat2" if mid else "fplx_conv3d_wgrad_cat2", ptr(x0), ptr(x1), ld_of(x0), ptr(dy), ld_of(dy),
         ptr(dw), n, d, h, w, cin, cout, ptr(ws), ws.numel() * ws.element_size(), stream())


def conv3d_fwd_act_ok(dims, cin, cout, mid=False, cat2=False):
    """True if the layer's forward kernel has the fused (folded eval-mode BatchNorm) + PReLU write-out"""
    n, d, h, w = dims
    return _lib.lib().fplx_conv3d_fwd_act_ok(n, d, h, w, cin, cout, 1 if mid else 0, 1 if cat2 else 0) == 1


def conv3d_fwd_act(x0, x1, wp, bias, slope, y, dims, cin, cout, mid=False, n_x0=0):
    """inference: y = PReLU(conv(x; wp) + bias) with the eval-mode BatchNorm already folded into wp / bias; x1: the second half
    of a channel concatenation (or None); n_x0: x0 holds that many samples, read modulo (0 = all).  bf16 NDHWC 2-D views."""
    n, d, h, w = dims
    ws = _fwd_scratch(conv3d_fwd_ws_bytes(dims, cin, cout, (3, 3, 3), BF16, BF16, mid), y.device)
    if x1 is not None:
        assert ld_of(x0) == ld_of(x1)
    call("fplx_conv3d_fwd_act", ptr(x0), ptr(x1), ld_of(x0), ptr(wp), ptr(bias), ptr(slope), ptr(y), ld_of(y), n, d, h, w, cin,
         cout, 1 if mid else 0, int(n_x0), ptr(ws), 0 if ws is None else ws.numel(), stream())


def _dc(sd):
    return "fplx_deconv2_" if sd == 2 else "fplx_deconv122_"


def deconv2_fwd(x, wf, bias, y, dims, cin, cout, sd=2):
    """sd = 2: ConvTranspose3d(2,2); sd = 1: ConvTranspose2d(2,2) on every depth slice (dims = INPUT dims)"""
    n, d, h, w = dims
    call(_dc(sd) + "fwd", ptr(x), ld_of(x), ptr(wf), ptr(bias), ptr(y), ld_of(y), n, d, h, w, cin, cout,
         dt_of(x), stream())


def deconv2_dgrad(dy, wb, dx, dims, cin, cout, sd=2):
    n, d, h, w = dims
    call(_dc(sd) + "dgrad", ptr(dy), ld_of(dy), ptr(wb), ptr(dx), ld_of(dx), n, d, h, w, cin, cout,
         dt_of(dy), stream())


def deconv2_wgrad_ws_bytes(dims, cin, cout, sd=2):
    n, d, h, w = dims
    return getattr(_lib.lib(), _dc(sd) + "wgrad_ws_bytes")(n, d, h, w, cin, cout)


def deconv2_wgrad(x, dy, dw, db, dims, cin, cout, ws, sd=2):
    n, d, h, w = dims
    call(_dc(sd) + "wgrad", ptr(x), ld_of(x), ptr(dy), ld_of(dy), ptr(dw), ptr(db), n, d, h, w, cin, cout,
         dt_of(x), ptr(ws), ws.numel() * ws.element_size(), stream())


def upsample2_fwd(x, y, dims, c, sd=2):
    """(tri / bi)linear x2 upsampling, align_corners = True; dims = INPUT dims, sd = 1: H and W only (2.5D levels)"""
    n, d, h, w = dims
    call("fplx_upsample2_fwd", ptr(x), ld_of(x), ptr(y), ld_of(y), n, d, h, w, c, dt_of(x), sd, stream())


def upsample2_bwd(dy, dx, dims, c, sd=2):
    n, d, h, w = dims
    call("fplx_upsample2_bwd", ptr(dy), ld_of(dy), ptr(dx), ld_of(dx), n, d, h, w, c, dt_of(dy), sd, stream())


def bn_train_finalize(stats, rows, c, count, gamma, beta, rm, rv, nbt, bnbuf, momentum=0.1, eps=1e-5):
    """bnbuf: fp32 [4, C] -> rows mean, rstd, scale, shift"""
    call("fplx_bn_train_finalize", ptr(stats), rows, c, count, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt),
         momentum, eps, ptr(bnbuf[0]), ptr(bnbuf[1]), ptr(bnbuf[2]), ptr(bnbuf[3]), stream())


def bn_eval_prepare(gamma, beta, rm, rv, bnbuf, eps=1e-5):
    c = gamma.numel()
    call("fplx_bn_eval_prepare", ptr(gamma), ptr(beta), ptr(rm), ptr(rv), eps, c, ptr(bnbuf[2]), ptr(bnbuf[3]),
         stream())


def bn_act_fwd(y, out, bnbuf, slope, p, seed, sid, c):
    call("fplx_bn_act_fwd", ptr(y), ld_of(y), ptr(out), ld_of(out), ptr(bnbuf[2]), ptr(bnbuf[3]), ptr(slope),
         float(p), int(seed), int(sid), y.shape[0], c, dt_of(y), stream())


def num_partials(voxels):
    return _lib.lib().fplx_num_partials(voxels)


def outconv_bn_rows(dims, c0=32, ncls=2):
    """partial rows of the fused out_conv backward (fplx_outconv_bn_rows); 0 where the fused forms do not apply"""
    n, d, h, w = dims
    return _lib.lib().fplx_outconv_bn_rows(n, d, h, w, int(c0), int(ncls))


def outconv_bn_ok(dims, c0, ncls):
    """True if out_conv can be fused with the BatchNorm + PReLU passes of the site in front of it (fplx_outconv_fwd_bn,
    fplx_outconv_dgrad_bn_reduce / _apply: bf16, C0 = 32, classes <= 4)"""
    return outconv_bn_rows(dims, c0, ncls) > 0


def outconv_fwd_bn(y, bnbuf, slope, a, wf, bias, logits, dims, c0, ncls):
    """a = PReLU(BN(y)) (bnbuf rows 2 / 3 = scale / shift) and logits = out_conv(a) in one pass over y.  a = None: the
    activation is not written (allowed where outconv_wgrad_bn_ws_bytes(...) > 0: backward then takes everything from y)"""
    n, d, h, w = dims
    call("fplx_outconv_fwd_bn", ptr(y), ld_of(y), ptr(bnbuf[2]), ptr(bnbuf[3]), ptr(slope), ptr(a), int(c0) if a is None else ld_of(a),
         ptr(wf), ptr(bias), ptr(logits), n, d, h, w, int(c0), int(ncls), stream())


def outconv_wgrad_bn_ws_bytes(dims, c0, ncls):
    """workspace of outconv_wgrad_bn; 0 where that form is not available (the stored activation + conv3d_wgrad are needed)"""
    n, d, h, w = dims
    return int(_lib.lib().fplx_outconv_wgrad_bn_ws_bytes(n, d, h, w, int(c0), int(ncls)))


def outconv_wgrad_bn(y, bnbuf, slope, dlogits, dw, db, dims, c0, ncls, ws):
    """out_conv's weight (and bias, db may be None) gradient from the PRE-BatchNorm tensor y of the site in front of it: the
    activation is formed on the way in (fplx_outconv_wgrad_bn), so the forward never has to store it"""
    n, d, h, w = dims
    call("fplx_outconv_wgrad_bn", ptr(y), ld_of(y), ptr(bnbuf[2]), ptr(bnbuf[3]), ptr(slope), ptr(dlogits), ptr(dw), ptr(db),
         n, d, h, w, int(c0), int(ncls), ptr(ws), ws.numel() * ws.element_size(), stream())


def outconv_dgrad_bn_bwd(dlogits, wb, y, bnbuf, slope, train, dgamma, dbeta, dslope, part, coef, dy, dims, c0, ncls):
    """backward of [BN + PReLU -> out_conv] without ever storing out_conv's data gradient: reduction (recomputing it from
    dlogits), the usual finalize, apply (recomputing it again) -> dy.  part must hold outconv_bn_rows(dims, c0, ncls) x (2 c0 + 1) floats."""
    n, d, h, w = dims
    rows = outconv_bn_rows(dims, c0, ncls)
    if part.numel() < rows * (2 * c0 + 1):
        raise ValueError("fplx: partial-row buffer too small for the fused out_conv backward (%d < %d floats)" % (part.numel(), rows * (2 * c0 + 1)))
    bn = [ptr(bnbuf[0]), ptr(bnbuf[1]), ptr(bnbuf[2]), ptr(bnbuf[3])]
    call("fplx_outconv_dgrad_bn_reduce", ptr(dlogits), ptr(wb), ptr(y), ld_of(y), bn[0], bn[1], bn[2], bn[3], ptr(slope), ptr(part),
         n, d, h, w, int(c0), int(ncls), stream())
    call("fplx_bn_act_bwd_finalize", ptr(part), rows, int(c0), y.shape[0], 1 if train else 0, ptr(dgamma), ptr(dbeta), ptr(dslope),
         ptr(coef), stream())
    call("fplx_outconv_dgrad_bn_apply", ptr(dlogits), ptr(wb), ptr(y), ld_of(y), bn[0], bn[1], bn[2], bn[3], ptr(slope), ptr(coef),
         ptr(dy), ld_of(dy), n, d, h, w, int(c0), int(ncls), stream())


def bn_pool_fused_ok(c, dtype):
    return _lib.lib().fplx_bn_pool_fused_ok(int(c), _DT[dtype]) == 1


def bn_act_pool_fwd(y, out, pooled, bnbuf, slope, dims, c, pd=2):
    """tail of a DownBlock in one pass: out = PReLU(BN(y)) (the skip tensor) and pooled = MaxPool(out)"""
    n, d, h, w = dims
    call("fplx_bn_act_pool_fwd", ptr(y), ld_of(y), ptr(out), ld_of(out), ptr(pooled), ld_of(pooled), ptr(bnbuf[2]), ptr(bnbuf[3]),
         ptr(slope), n, d, h, w, c, dt_of(y), pd, stream())


def pool_bwd_bn_reduce(y, dy, dskip, dx, bnbuf, slope, dims, c, part, pd=2):
    """dx = dskip + unpooled(dy) (= d of the DownBlock's output) and the partial rows of bn_act_bwd's reduction over it"""
    n, d, h, w = dims
    call("fplx_pool_bwd_bn_reduce", ptr(y), ld_of(y), ptr(dy), ld_of(dy), ptr(dskip), 0 if dskip is None else ld_of(dskip), ptr(dx),
         ld_of(dx), ptr(bnbuf[0]), ptr(bnbuf[1]), ptr(bnbuf[2]), ptr(bnbuf[3]), ptr(slope), n, d, h, w, c, dt_of(y), pd, ptr(part),
         stream())


def bn_act_bwd(y, dout, dy, bnbuf, slope, p, seed, sid, c, train, dgamma, dbeta, dslope, part, coef, reduced=False, apply=True):
    """three-stage backward of the fused BN-apply + PReLU + dropout pass; dy may alias dout.
    reduced: `part` already holds the partial rows (pool_bwd_bn_reduce wrote them while it formed dout)
    apply=False: reduction + finalize only - `coef` is left for a consumer that forms dy itself (stem_wgrad_bn)"""
    v = y.shape[0]
    rows = num_partials(v)
    if not reduced:
        call("fplx_bn_act_bwd_reduce", ptr(y), ld_of(y), ptr(dout), ld_of(dout), ptr(bnbuf[0]), ptr(bnbuf[1]),
             ptr(bnbuf[2]), ptr(bnbuf[3]), ptr(slope), float(p), int(seed), int(sid), v, c, dt_of(y), ptr(part), stream())
    call("fplx_bn_act_bwd_finalize", ptr(part), rows, c, v, 1 if train else 0, ptr(dgamma), ptr(dbeta), ptr(dslope),
         ptr(coef), stream())
    if not apply:
        return
    call("fplx_bn_act_bwd_apply", ptr(y), ld_of(y), ptr(dout), ld_of(dout), ptr(dy), ld_of(dy), ptr(bnbuf[0]),
         ptr(bnbuf[1]), ptr(bnbuf[2]), ptr(bnbuf[3]), ptr(slope), ptr(coef), float(p), int(seed), int(sid), v, c,
         dt_of(y), stream())


def stem_wgrad_bn_ok(dims, cin, cout):
    """True if the stem site's weight gradient can take y and d(a) and form dy itself (fplx_stem_wgrad_bn): the layers
    fplx_conv3d_plan_query gives to the MFMA stem kernels (fp32 NCDHW input of 1 | 4 channels, C0 % 32 == 0)"""
    import ctypes
    n, d, h, w = dims
    kern, g, ks, r = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().fplx_conv3d_plan_query(n, d, h, w, int(cin), int(cout), 3, 3, 3, F32, BF16, ctypes.byref(kern),
                                                 ctypes.byref(g), ctypes.byref(ks), ctypes.byref(r)))
    return kern.value == 6                               # FPLX_KERNEL_STEM


def stem_wgrad_bn(x, y, dout, bnbuf, slope, coef, dw, dims, cin, cout, ws):
    """weight gradient of the stem convolution from y (its stored output) and dout = gradient w.r.t. the site's OUTPUT: the apply
    pass of the site's BatchNorm + PReLU backward runs on the pieces the kernel stages; dy is never stored"""
    n, d, h, w = dims
    call("fplx_stem_wgrad_bn", ptr(x), ptr(y), ld_of(y), ptr(dout), ld_of(dout), ptr(bnbuf[0]), ptr(bnbuf[1]), ptr(bnbuf[2]),
         ptr(bnbuf[3]), ptr(slope), ptr(coef), ptr(dw), n, d, h, w, int(cin), int(cout), ptr(ws), ws.numel() * ws.element_size(),
         stream())


def maxpool2_fwd(x, y, dims, c, pd=2):
    """pd = 2: MaxPool3d(2); pd = 1: MaxPool2d(2) on every depth slice"""
    n, d, h, w = dims
    call("fplx_maxpool2_fwd" if pd == 2 else "fplx_maxpool122_fwd", ptr(x), ld_of(x), ptr(y), ld_of(y), n, d, h, w, c, dt_of(x), stream())


def maxpool2_bwd(x, dy, dskip, dx, dims, c, pd=2):
    n, d, h, w = dims
    call("fplx_maxpool2_bwd" if pd == 2 else "fplx_maxpool122_bwd", ptr(x), ld_of(x), ptr(dy), ld_of(dy), ptr(dskip), 0 if dskip is None else ld_of(dskip),
         ptr(dx), ld_of(dx), n, d, h, w, c, dt_of(x), stream())


def head_fwd(a, w, bias, logits, n, v, c, ncls):
    """1x1x1 classification head (fplx_head_fwd): a NDHWC 2-D view [n * v, ld] (fp32 | bf16), w fp32 [ncls, c(, 1, 1, 1)],
    logits fp32 planar [n, ncls, v] (contiguous)"""
    call("fplx_head_fwd", ptr(a), ld_of(a), dt_of(a), ptr(w), ptr(bias), ptr(logits), int(n), int(v), int(c), int(ncls), stream())


def head_dgrad(dlogits, w, da, n, v, c, ncls, accumulate=False):
    """da = w^T dlogits in da's dtype; accumulate: added into da in place (the second consumer of a decoder level's output)"""
    call("fplx_head_dgrad", ptr(dlogits), ptr(w), ptr(da), ld_of(da), dt_of(da), int(n), int(v), int(c), int(ncls),
         1 if accumulate else 0, stream())


def head_wgrad_ws_bytes(n, v, c, ncls):
    return int(_lib.lib().fplx_head_wgrad_ws_bytes(int(n), int(v), int(c), int(ncls)))


def head_wgrad(a, dlogits, dw, db, n, v, c, ncls, ws):
    """dw fp32 [ncls, c], db fp32 [ncls] (or None) through ws (uint8, head_wgrad_ws_bytes)"""
    call("fplx_head_wgrad", ptr(a), ld_of(a), dt_of(a), ptr(dlogits), ptr(dw), ptr(db), int(n), int(v), int(c), int(ncls),
         ptr(ws), 0 if ws is None else ws.numel() * ws.element_size(), stream())


def interp_fwd(x, y, nc, dims, f):
    """trilinear interpolation by f in {2, 4, 8}, align_corners = False: fp32 planar [nc, d, h, w] -> [nc, f d, f h, f w]"""
    d, h, w = dims
    call("fplx_interp_fwd", ptr(x), ptr(y), int(nc), int(d), int(h), int(w), int(f), stream())


def interp_bwd(dy, dx, nc, dims, f):
    """the transpose of interp_fwd: dy [nc, f d, f h, f w] -> dx [nc, d, h, w] (dims = the COARSE extents)"""
    d, h, w = dims
    call("fplx_interp_bwd", ptr(dy), ptr(dx), int(nc), int(d), int(h), int(w), int(f), stream())


def loss_rows(v):
    return _lib.lib().fplx_loss_rows(v)


def loss_k(c):
    return 6 * c + 3


def _ncv(logits):
    return logits.shape[0], logits.shape[1], logits[0, 0].numel()


def seg_loss_fwd(logits, label, pw, iw, weights, softmax, part, out, coef):
    n, c, v = _ncv(logits)
    call("fplx_seg_loss_fwd", ptr(logits), ptr(label), ptr(pw), ptr(iw), n, c, v, weights[0], weights[1], weights[2],
         weights[3], 1 if softmax else 0, ptr(part), ptr(out), ptr(coef), stream())


def _seg_loss_sums(logits, label, pw, weights, softmax, part, sums, totals):
    n, c, v = _ncv(logits)                                   # the sums do not depend on the weights
    call("fplx_seg_loss_sums", ptr(logits), ptr(label), ptr(pw), n, c, v, 1 if softmax else 0, ptr(part), ptr(sums), ptr(totals),
         stream())


def _seg_loss_from_sums(sums, totals, iw, n, n_global, c, v, has_pw, weights, out, coef):
    call("fplx_seg_loss_from_sums", ptr(sums), ptr(totals), ptr(iw), n, n_global, c, v, 1 if has_pw else 0, weights[0], weights[1],
         weights[2], weights[3], ptr(out), ptr(coef), stream())


def _fwd_dist(sums_fn, from_sums_fn, k, logits, label, pw, iw, how, softmax, part, out, coef, group):
    """a forward under data parallelism: the sums over the local samples are all-reduced over `group` between the reduction
    and the evaluation, so loss, metric and backward coefficients are those of the FULL batch (what the reference's
    nn.DataParallel computes on its gathered logits, agent_seg.py:692-698; every sum of either family is additive over the
    ranks).  All ranks must hold the same number of samples.  how: the family's weights or cfg."""
    import torch.distributed as dist
    n, c, v = _ncv(logits)
    sums = torch.empty((n + 1, k), dtype=torch.float64, device=logits.device)
    sums_fn(logits, label, pw, how, softmax, part, sums[:n], sums[n])
    dist.all_reduce(sums[n], op=dist.ReduceOp.SUM, group=group)
    from_sums_fn(sums[:n], sums[n], iw, n, n * dist.get_world_size(group), c, v, pw is not None, how, out, coef)


def seg_loss_fwd_dist(logits, label, pw, iw, weights, softmax, part, out, coef, group):
    """seg_loss_fwd over the full batch of all ranks (_fwd_dist)"""
    _fwd_dist(_seg_loss_sums, _seg_loss_from_sums, loss_k(logits.shape[1]), logits, label, pw, iw, weights, softmax, part, out, coef,
              group)


def seg_loss_bwd(logits, label, pw, coef, gscale, weights, softmax, dlogits):
    n, c, v = _ncv(logits)
    call("fplx_seg_loss_bwd", ptr(logits), ptr(label), ptr(pw), ptr(coef), ptr(gscale), n, c, v, weights[0],
         weights[1], weights[2], weights[3], 1 if softmax else 0, ptr(dlogits), stream())


# ---- second loss family (include/fplx.h, "segmentation loss, second family")
LOSS_EXT_TERMS = ("focal", "noise_robust", "explog", "gce", "mae", "mse", "slsr")        # order of cfg[4..10] and of out[4 + C ..]
LOSS_EXT_PARAMS = ("beta", "gamma_nr", "w_dice_el", "gamma_el", "q", "epsilon", "use_pixel_weight", "class_weight")
LOSS_EXT_DEFAULTS = (1.0, 1.0, 0.5, 1.0, 0.5, 0.25, False, None)


def loss_ext_k(c):
    return 10 * c + 7


def loss_ext_nout(c):
    return 4 + c + 7


def loss_ext_ncoef(n, c):
    return n * c * 2 + 2 + 4 * c + 4


def loss_ext_cfg(terms, ext, c):
    """the host array `cfg` of the fplx_seg_loss_ext_* calls: terms = the four weights of the first family, ext = (the seven
    weights in LOSS_EXT_TERMS order, the parameters in LOSS_EXT_PARAMS order); class_weight None = all ones"""
    w, prm = ext
    if len(terms) != 4 or len(w) != len(LOSS_EXT_TERMS) or len(prm) != len(LOSS_EXT_PARAMS):
        raise ValueError("fplx loss: malformed term description")
    cw = prm[7]
    if cw is None:
        cw = (1.0,) * c
    if len(cw) != c:
        raise ValueError("fplx loss: loss_class_weight has {0:} entries for {1:} classes".format(len(cw), c))
    vals = [float(t) for t in terms] + [float(t) for t in w] + [float(t) for t in prm[:6]] + [1.0 if prm[6] else 0.0]
    vals += [float(t) for t in cw]
    return (ctypes.c_float * len(vals))(*vals)


def seg_loss_ext_fwd(logits, label, pw, iw, cfg, softmax, part, out, coef):
    n, c, v = _ncv(logits)
    call("fplx_seg_loss_ext_fwd", ptr(logits), ptr(label), ptr(pw), ptr(iw), n, c, v, cfg, 1 if softmax else 0, ptr(part),
         ptr(out), ptr(coef), stream())


def seg_loss_ext_sums(logits, label, pw, cfg, softmax, part, sums, totals):
    n, c, v = _ncv(logits)
    call("fplx_seg_loss_ext_sums", ptr(logits), ptr(label), ptr(pw), n, c, v, cfg, 1 if softmax else 0, ptr(part), ptr(sums),
         ptr(totals), stream())


def seg_loss_ext_from_sums(sums, totals, iw, n, n_global, c, v, has_pw, cfg, out, coef):
    call("fplx_seg_loss_ext_from_sums", ptr(sums), ptr(totals), ptr(iw), n, n_global, c, v, 1 if has_pw else 0, cfg, ptr(out),
         ptr(coef), stream())


def seg_loss_ext_fwd_dist(logits, label, pw, iw, cfg, softmax, part, out, coef, group):
    """seg_loss_ext_fwd over the full batch of all ranks (_fwd_dist)"""
    _fwd_dist(seg_loss_ext_sums, seg_loss_ext_from_sums, loss_ext_k(logits.shape[1]), logits, label, pw, iw, cfg, softmax, part, out,
              coef, group)


def seg_loss_ext_bwd(logits, label, pw, coef, gscale, cfg, softmax, dlogits):
    n, c, v = _ncv(logits)
    call("fplx_seg_loss_ext_bwd", ptr(logits), ptr(label), ptr(pw), ptr(coef), ptr(gscale), n, c, v, cfg, 1 if softmax else 0,
         ptr(dlogits), stream())


class LossPass(object):
    """One fused loss pass: the first family's (ext None: terms = the weights of Dice, CE, image-weighted Dice, entropy) or, with
    ext = (weights, parameters) of the second family's terms (AbstractSegLoss.ext_spec()), the pass that evaluates all eleven.
    The only place the two families' buffer sizes and entry points are chosen between; the entry points are looked up on this
    module at the time of the call."""

    def __init__(self, terms, ext, softmax):
        self.terms, self.ext, self.softmax = tuple(float(t) for t in terms), ext, bool(softmax)
        self._cfg = {}

    def sizes(self, n, c):
        """partial-row width k, floats of `out`, floats of `coef`"""
        if self.ext is None:
            return loss_k(c), 4 + c, n * c * 2 + 2
        return loss_ext_k(c), loss_ext_nout(c), loss_ext_ncoef(n, c)

    def _args(self, c):
        """what the family's entry points take behind the tensors: the four weights, or cfg (built once per class count)"""
        if self.ext is None:
            return self.terms
        if c not in self._cfg:
            self._cfg[c] = loss_ext_cfg(self.terms, self.ext, c)
        return self._cfg[c]

    def forward(self, logits, label, pw, iw, part, out, coef, group=None, dist=False):
        """dist: over the full batch of the ranks of `group` (None: the default group)"""
        how = self._args(logits.shape[1])
        if dist:
            (seg_loss_fwd_dist if self.ext is None else seg_loss_ext_fwd_dist)(logits, label, pw, iw, how, self.softmax, part, out,
                                                                               coef, group)
        else:
            (seg_loss_fwd if self.ext is None else seg_loss_ext_fwd)(logits, label, pw, iw, how, self.softmax, part, out, coef)

    def backward(self, logits, label, pw, coef, gscale, dlogits):
        (seg_loss_bwd if self.ext is None else seg_loss_ext_bwd)(logits, label, pw, coef, gscale, self._args(logits.shape[1]),
                                                                 self.softmax, dlogits)


def adam_pack_ok(cout, cin):
    return _lib.lib().fplx_adam_pack_ok(int(cout), int(cin)) == 1


OPTIM_KINDS = ("SGD", "Adadelta", "Adagrad", "Adamax", "ASGD", "RMSprop", "Rprop", "Adam")      # FPLX_OPT_* in include/fplx.h


def _optim_args(kind, p, g, s0, s1, hp, step, grad_scale):
    k = OPTIM_KINDS.index(kind) if isinstance(kind, str) else int(kind)
    return (k, ptr(p), ptr(g), ptr(s0) or None, ptr(s1) or None, p.numel(), (ctypes.c_float * len(hp))(*map(float, hp)), len(hp),
            int(step), grad_scale)


def _pack_layer_args(layers):
    """layers: [(element offset in p, cout, cin, wf, wb[, stamp])] ascending by offset (stamp: pack_conv_weights_batched)
    -> nl, off, cout, cin, wf, wb, stamp of fplx_optim_pack_step"""
    n = len(layers)
    vp, ip, lp = ctypes.c_void_p * n, ctypes.c_int * n, ctypes.c_int64 * n
    off, cout, cin, wf, wb, stamp = zip(*[l if len(l) > 5 else tuple(l) + (None,) for l in layers])
    dev = lambda ts: vp(*[None if t is None else t.data_ptr() for t in ts])       # one pass per column: this runs every step
    return (n, lp(*map(int, off)), ip(*map(int, cout)), ip(*map(int, cin)), dev(wf), dev(wb), dev(stamp))


def optim_step(kind, p, g, s0, s1, hp, step, grad_scale=1.0):
    """fplx_optim_step: one step of `kind` (a name of OPTIM_KINDS or its FPLX_OPT_* number) over the flat fp32 segment p.
    s0 / s1: the kind's state streams or None; hp: the kind's hyper-parameters in the order include/fplx.h documents."""
    call("fplx_optim_step", *(_optim_args(kind, p, g, s0, s1, hp, step, grad_scale) + (stream(),)))


def optim_pack_step(kind, p, g, s0, s1, hp, step, grad_scale, layers):
    """fplx_optim_step AND the bf16 packs of the 3x3x3 weights inside p in one launch; layers: see _pack_layer_args"""
    call("fplx_optim_pack_step", *(_optim_args(kind, p, g, s0, s1, hp, step, grad_scale) + _pack_layer_args(layers) + (stream(),)))


# Adam under its own two names (kind "Adam" of the above): a kernel timer that wraps ops by name reads these positional arguments
def adam_step(p, g, m, v, lr, step, weight_decay, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8):
    optim_step("Adam", p, g, m, v, (lr, betas[0], betas[1], eps, weight_decay), step, grad_scale)


def adam_pack_step(p, g, m, v, lr, step, weight_decay, grad_scale, betas, eps, layers):
    optim_pack_step("Adam", p, g, m, v, (lr, betas[0], betas[1], eps, weight_decay), step, grad_scale, layers)


def mc_filter(logits_tcv, thr=0.01, want_hards=True, want_maps=False):
    """logits_tcv: fp32 [T, C, ...volume...] on the GPU -> dict (device tensors, no sync)"""
    require_gpu(logits_tcv)
    t, c = logits_tcv.shape[0], logits_tcv.shape[1]
    vol = tuple(logits_tcv.shape[2:])
    v = logits_tcv[0, 0].numel()
    dev = logits_tcv.device
    lg = logits_tcv.contiguous()
    hards = torch.empty((t,) + vol, dtype=torch.uint8, device=dev) if want_hards else None
    mean = torch.empty(vol, dtype=torch.float32, device=dev) if want_maps else None
    unc = torch.empty(vol, dtype=torch.float32, device=dev) if want_maps else None
    part = torch.empty((num_partials(v), 2), dtype=torch.float64, device=dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    call("fplx_mc_filter", ptr(lg), t, c, v, thr, ptr(hards), ptr(mean), ptr(unc), ptr(part), ptr(out), stream())
    return dict(hards=hards, means=mean, uncertainty=unc, stats=out)


def hard_label(logits):
    """save_outputs (reference agent_seg.py:1049-1050): [N,C,...] fp32 -> uint8 [N,...]"""
    require_gpu(logits)
    n, c = logits.shape[0], logits.shape[1]
    lg = logits.contiguous()
    out = torch.empty((n,) + tuple(logits.shape[2:]), dtype=torch.uint8, device=logits.device)
    call("fplx_hard_label", ptr(lg), n, c, lg[0, 0].numel(), ptr(out), stream())
    return out


def pixel_weight(mask_a, mask_b, image_weight=None):
    """reference data/get_pixel_weight.py:21-26 (+ NiftyDataset.set_weight_ when image_weight is given)"""
    require_gpu(mask_a, mask_b)
    if mask_a.shape != mask_b.shape:
        raise ValueError("fplx: mask shapes differ")        # get_pixel_weight.py:19 asserts the same
    a = mask_a.contiguous()
    b = mask_b.contiguous()
    out = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    call("fplx_pixel_weight", ptr(a), ptr(b), a.numel(), 0 if image_weight is None else 1,
         0.0 if image_weight is None else float(image_weight), ptr(out), stream())
    return out


# ---------------------------------------------------------------- training-sample transforms (csrc/sample.hip)
_ELEM = {torch.float32: 4, torch.uint8: 1}


def _elem_bytes(t):
    try:
        return _ELEM[t.dtype]
    except KeyError:
        raise ValueError("fplx: transforms take float32 or uint8 volumes, got {0:}".format(t.dtype))


def normalize_mean_std(x, mean_std=None, out=None, want_moments=False):
    """(x - mean) / std of one channel volume (fp32, contiguous); mean_std None -> x's own float32 mean / population std"""
    require_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty_like(x) if out is None else out
    ms = None if mean_std is None else torch.tensor(list(mean_std), dtype=torch.float32, device=x.device)
    nb = _lib.lib().fplx_normalize_ws_bytes()
    ws = torch.empty(nb // 8, dtype=torch.float64, device=x.device)
    got = torch.empty(2, dtype=torch.float32, device=x.device) if want_moments else None
    call("fplx_normalize_mean_std", ptr(x), ptr(out), x.numel(), ptr(ms), ptr(ws), nb, ptr(got), stream())
    return (out, got) if want_moments else out


def normalize_positive(x, noise, out=None, want_moments=False):
    """NormalizeWithMeanStd_ignore_non_positive: (x - mean) / std with the moments of the voxels > 0; noise elsewhere"""
    require_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and noise.dtype == torch.float32 and noise.is_contiguous()
    assert noise.numel() == x.numel()
    out = torch.empty_like(x) if out is None else out
    nb = _lib.lib().fplx_normalize_ws_bytes()
    ws = torch.empty(nb // 8, dtype=torch.float64, device=x.device)
    got = torch.empty(2, dtype=torch.float32, device=x.device) if want_moments else None
    call("fplx_normalize_positive", ptr(x), ptr(noise), ptr(out), x.numel(), ptr(ws), nb, ptr(got), stream())
    return (out, got) if want_moments else out


# ---- intensity transforms (csrc/intensity.hip): one channel volume per call, fp32, contiguous; out=x runs in place

def _chan(x, *more):
    require_gpu(x, *more)
    if not (x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0):
        raise ValueError("fplx: intensity ops take a non-empty contiguous float32 volume")
    return x


def _f32(v):
    """a host number as the float32 numpy makes of it next to a float32 array (NumPy 2: Python scalars are weak)"""
    return float(np.float32(v))


def channel_minmax(x, lower=None, upper=None):
    """-> device float32[4] = [min, max, min and max of x clipped to lower / upper (each optional)]; NaN propagates"""
    _chan(x)
    ws = torch.empty(4, dtype=torch.int32, device=x.device)
    out = torch.empty(4, dtype=torch.float32, device=x.device)
    call("fplx_channel_minmax", ptr(x), x.numel(), 0.0 if lower is None else _f32(lower), int(lower is not None),
         0.0 if upper is None else _f32(upper), int(upper is not None), ptr(ws), 16, ptr(out), stream())
    return out


def select_kth(x, ranks):
    """exact order statistics: device float32 [len(ranks), 2] = (s[k], s[min(k + 1, n - 1)]) of the sorted values, 1..4 ranks"""
    _chan(x)
    ranks = [int(k) for k in ranks]
    nb = _lib.lib().fplx_select_ws_bytes()
    ws = torch.empty(nb // 4, dtype=torch.int32, device=x.device)
    out = torch.empty((len(ranks), 2), dtype=torch.float32, device=x.device)
    call("fplx_select_kth", ptr(x), x.numel(), (ctypes.c_int64 * max(len(ranks), 1))(*ranks), len(ranks), ptr(out), ptr(ws),
         nb, stream())
    return out


def percentile_index(n, q):
    """where numpy.percentile(x, q) (method 'linear') looks in the sorted float32 array of n values -> (lo, g): the result
    interpolates s[lo] and s[min(lo + 1, n - 1)] with the weight g.  numpy does this in FLOAT32 when the data are float32
    and q is a Python number: quantile = float32(q) / float32(100), index v = float32(n - 1) * quantile, each
    rounded to float32, lo = floor(v), g = v - lo; v >= n - 1 reads the last element twice (g = v + 1
    then, which multiplies a zero difference).  For n beyond 2^24 / 100 the index itself is rounded: numpy's choice, kept."""
    f = np.float32
    qq = f(q) / f(100)
    v = f(n - 1) * qq
    if v >= f(n - 1):
        return n - 1, v + f(1)
    lo = f(np.floor(v))
    return int(lo), v - lo


def percentile_lerp(a, b, g):
    """numpy's _lerp on float32 scalars: a + (b - a) g below g = 0.5, else b - (b - a) (1 - g)"""
    a, b, g = np.float32(a), np.float32(b), np.float32(g)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return a + d * g if g < 0.5 else b - d * (np.float32(1) - g)


def percentiles(x, qs):
    """numpy.percentile(x, q) for each q (at most 3): one selection on the device, one device->host copy of the order
    statistics, numpy's interpolation on the host -> list of numpy.float32.  The largest element rides along: a NaN
    anywhere in x sorts last and makes every percentile NaN, as in numpy."""
    n = x.numel()
    for q in qs:
        if not 0 <= q <= 100:
            raise ValueError("Percentiles must be in the range [0, 100]")
    idx = [percentile_index(n, q) for q in qs]
    s = select_kth(x, [lo for lo, _ in idx] + [n - 1]).cpu().numpy()
    if np.isnan(s[-1, 0]):
        return [np.float32(np.nan) for _ in qs]
    return [percentile_lerp(s[j, 0], s[j, 1], g) for j, (_, g) in enumerate(idx)]


def clip_affine(x, v0, v1, a, b, out=None):
    """(clip(x, v0, v1) - a) / b with host float32 numbers"""
    _chan(x)
    out = torch.empty_like(x) if out is None else out
    call("fplx_clip_affine", ptr(x), ptr(out), x.numel(), _f32(v0), _f32(v1), _f32(a), _f32(b), stream())
    return out


def clip_affine_dev(x, v0, v1, a, hi, out=None):
    """(clip(x, v0, v1) - a) / (hi - a) with v0, v1, a, hi one-element float32 device tensors (no host synchronisation)"""
    _chan(x, v0, v1, a, hi)
    for t in (v0, v1, a, hi):
        assert t.dtype == torch.float32 and t.numel() >= 1
    out = torch.empty_like(x) if out is None else out
    call("fplx_clip_affine_dev", ptr(x), ptr(out), x.numel(), ptr(v0), ptr(v1), ptr(a), ptr(hi), stream())
    return out


def threshold_replace(x, t_lower, r_lower, t_upper, r_upper, out=None):
    """x < t_lower -> r_lower, then > t_upper -> r_upper; a threshold of None switches its side off"""
    _chan(x)
    out = torch.empty_like(x) if out is None else out
    call("fplx_threshold_replace", ptr(x), ptr(out), x.numel(), 0.0 if t_lower is None else _f32(t_lower),
         0.0 if t_lower is None else _f32(r_lower), int(t_lower is not None), 0.0 if t_upper is None else _f32(t_upper),
         0.0 if t_upper is None else _f32(r_upper), int(t_upper is not None), stream())
    return out


def normalize_range(x, noise, lower=None, upper=None, out=None, want_moments=False):
    """(x - mean) / std with the moments of the voxels lower < x < upper (each bound optional); noise elsewhere"""
    _chan(x, noise)
    assert noise.dtype == torch.float32 and noise.is_contiguous() and noise.numel() == x.numel()
    out = torch.empty_like(x) if out is None else out
    nb = _lib.lib().fplx_normalize_ws_bytes()
    ws = torch.empty(nb // 8, dtype=torch.float64, device=x.device)
    got = torch.empty(2, dtype=torch.float32, device=x.device) if want_moments else None
    call("fplx_normalize_range", ptr(x), ptr(noise), ptr(out), x.numel(), 0.0 if lower is None else _f32(lower),
         int(lower is not None), 0.0 if upper is None else _f32(upper), int(upper is not None), ptr(ws), nb, ptr(got), stream())
    return (out, got) if want_moments else out


def gamma_correct(x, vmin, vmax, gamma, out=None):
    """float32(((x - vmin) / (vmax - vmin)) ** float32(gamma)) * (vmax - vmin) + vmin; vmin, vmax: device scalars"""
    _chan(x, vmin, vmax)
    out = torch.empty_like(x) if out is None else out
    call("fplx_gamma", ptr(x), ptr(out), x.numel(), ptr(vmin), ptr(vmax), _f32(gamma), stream())
    return out


def add_noise_f64(x, noise, out=None):
    """float32(double(x) + noise) for a float64 device volume of the same size"""
    _chan(x, noise)
    assert noise.dtype == torch.float64 and noise.is_contiguous() and noise.numel() == x.numel()
    out = torch.empty_like(x) if out is None else out
    call("fplx_add_noise_f64", ptr(x), ptr(noise), ptr(out), x.numel(), stream())
    return out


def add_noise_philox(x, seed, stream_id, mean, std, out=None, want_uniforms=False):
    """Gaussian noise generated on the device (Philox4x32-10 + Box-Muller in fp64, see include/fplx.h)"""
    _chan(x)
    out = torch.empty_like(x) if out is None else out
    u = torch.empty((x.numel(), 2), dtype=torch.float64, device=x.device) if want_uniforms else None
    call("fplx_add_noise_philox", ptr(x), ptr(out), x.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF,
         float(mean), float(std), ptr(u), stream())
    return (out, u) if want_uniforms else out


def pad_reflect(x, lower, out_size):
    """numpy.pad(x, mode='reflect') of a [C,D,H,W] volume to out_size (D,H,W) with lower margins `lower`"""
    require_gpu(x)
    assert x.dim() == 4 and x.is_contiguous()
    c, d, h, w = x.shape
    y = torch.empty((c,) + tuple(out_size), dtype=x.dtype, device=x.device)
    call("fplx_pad_reflect", ptr(x), ptr(y), _elem_bytes(x), c, d, h, w, lower[0], lower[1], lower[2], out_size[0],
         out_size[1], out_size[2], stream())
    return y


def crop_flip(x, crop_min, out_size, flip_mask=0, out=None):
    """crop box [crop_min, crop_min + out_size) of a [C,D,H,W] volume, then flip (bit0 W, bit1 H, bit2 D); out: an
    existing contiguous [C,*out_size] destination of x's dtype"""
    require_gpu(x)
    assert x.dim() == 4 and x.is_contiguous()
    c, d, h, w = x.shape
    if out is not None:
        assert out.is_cuda and out.is_contiguous() and out.dtype == x.dtype and tuple(out.shape) == (c,) + tuple(out_size)
    y = torch.empty((c,) + tuple(out_size), dtype=x.dtype, device=x.device) if out is None else out
    call("fplx_crop_flip", ptr(x), ptr(y), _elem_bytes(x), c, d, h, w, crop_min[0], crop_min[1], crop_min[2], out_size[0],
         out_size[1], out_size[2], int(flip_mask), stream())
    return y


def resample_affine(x, matrix, offset, out_size, order):
    """y[c][o] = interp(x[c], matrix o + offset) for a [C,D,H,W] volume -> [C,*out_size]: scipy.ndimage's affine resampling
    (mode='constant', cval=0) for order 0 (float32 or uint8) and order 1 (float32).  matrix (3x3) and offset (3) are host
    numbers, taken as fp64."""
    require_gpu(x)
    if not (x.dim() == 4 and x.is_contiguous()):
        raise ValueError("fplx: resample_affine takes a contiguous [C,D,H,W] volume")
    m = [float(v) for row in matrix for v in row]
    t = [float(v) for v in offset]
    if len(m) != 9 or len(t) != 3 or len(out_size) != 3:
        raise ValueError("fplx: resample_affine takes a 3x3 matrix, a 3-vector offset and a 3D output size")
    c, d, h, w = x.shape
    od, oh, ow = (int(v) for v in out_size)
    y = torch.empty((c, max(od, 0), max(oh, 0), max(ow, 0)), dtype=x.dtype, device=x.device)
    call("fplx_resample_affine", ptr(x), ptr(y), _elem_bytes(x), int(order), c, d, h, w, od, oh, ow,
         (ctypes.c_double * 9)(*m), (ctypes.c_double * 3)(*t), stream())
    return y


SPLINE_ORDERS = (3,)          # the spline orders csrc/spline.hip builds (its table has one row per order)


def _check_spline_volume(x, who, order):
    require_gpu(x)
    if not (x.dim() == 4 and x.is_contiguous()):
        raise ValueError("fplx: {0:} takes a contiguous [C,D,H,W] volume".format(who))
    if x.dtype != torch.float32:
        raise ValueError("fplx: {0:} takes float32 volumes, got {1:}".format(who, x.dtype))
    if int(order) not in SPLINE_ORDERS:
        raise ValueError("fplx: {0:}: spline order {1:} is not built (built: {2:})".format(
            who, order, ", ".join(str(o) for o in SPLINE_ORDERS)))


def spline_prefilter(x, order=3):
    """B-spline coefficients (float64 [C,D,H,W]) of a float32 [C,D,H,W] volume under scipy's mirror boundary:
    scipy.ndimage.spline_filter(x, order, output=float64, mode='mirror') along D, H and W"""
    _check_spline_volume(x, "spline_prefilter", order)
    c, d, h, w = x.shape
    coef = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    call("fplx_spline_prefilter", ptr(x), ptr(coef), c, d, h, w, int(order), stream())
    return coef


def resample_spline(x, matrix, offset, out_size, order=3):
    """y[c][o] = spline(x[c], matrix o + offset) for a float32 [C,D,H,W] volume -> [C,*out_size]: scipy.ndimage's affine
    resampling at spline order 3 (mode='constant', cval=0): the prefilter, then the 64-tap interpolation.  matrix (3x3) and
    offset (3) are host numbers, taken as fp64."""
    _check_spline_volume(x, "resample_spline", order)
    m = [float(v) for row in matrix for v in row]
    t = [float(v) for v in offset]
    if len(m) != 9 or len(t) != 3 or len(out_size) != 3:
        raise ValueError("fplx: resample_spline takes a 3x3 matrix, a 3-vector offset and a 3D output size")
    c, d, h, w = x.shape
    od, oh, ow = (int(v) for v in out_size)
    y = torch.empty((c, max(od, 0), max(oh, 0), max(ow, 0)), dtype=torch.float32, device=x.device)
    if min(c, d, h, w) > 0 and min(od, oh, ow) > 0:
        coef = spline_prefilter(x, order)
    else:
        coef = torch.empty(x.shape, dtype=torch.float64, device=x.device)      # the library refuses the extents below
    call("fplx_resample_spline", ptr(coef), ptr(y), c, d, h, w, od, oh, ow, (ctypes.c_double * 9)(*m),
         (ctypes.c_double * 3)(*t), int(order), stream())
    return y


EDT_LINES = 32                # EDT_LINES of csrc/edt.hip: the lines a block stages in LDS
EDT_MAX_EXTENT = 620          # FPLX_EDT_MAX_EXTENT of include/fplx.h: the longest line whose tile fits the 160 KiB of LDS


def edt_sampling(sampling, ndim):
    """scipy's `sampling` argument -> ndim floats: None is 1 per axis, a scalar is repeated, a sequence needs ndim entries"""
    if sampling is None:
        return [1.0] * ndim
    s = [float(v) for v in np.atleast_1d(np.asarray(sampling, np.float64)).ravel()]
    if len(s) == 1:
        s = s * ndim
    if len(s) != ndim:
        raise ValueError("fplx: sampling has {0:} entries for a {1:}D input".format(len(s), ndim))
    return s


def edt_squared(mask, sampling=None, return_indices=False, batched=False):
    """squared Euclidean distance (float64, mask's shape) of every voxel of a uint8 mask [D,H,W] or [H,W] (batched=True: a
    leading batch dimension in front) to the nearest zero voxel under `sampling`: scipy.ndimage.distance_transform_edt
    before its square root, bit for bit.  A mask without a zero gets scipy's result, the distance to index (-1, 0, 0).
    return_indices: also int32 [ndim, ...] ([N, ndim, ...] when batched), the coordinates of a zero voxel at that distance"""
    require_gpu(mask)
    nd = mask.dim() - (1 if batched else 0)
    if nd not in (2, 3):
        raise ValueError("fplx: edt_squared takes a 2D or 3D mask, got {0:}D".format(nd))
    if not (mask.dtype == torch.uint8 and mask.is_contiguous()):
        raise ValueError("fplx: edt_squared takes a contiguous uint8 mask")
    s = edt_sampling(sampling, nd)
    n = mask.shape[0] if batched else 1
    d, h, w = ((1,) if nd == 2 else ()) + tuple(mask.shape[-nd:])
    if min(n, d, h, w) > 0:
        phantom = (mask.reshape(n, -1).amin(dim=1) != 0).to(torch.uint8)      # a device flag per mask: no host round trip
    else:
        phantom = None                                                          # the library refuses the extents below
    sq = torch.empty(mask.shape, dtype=torch.float64, device=mask.device)
    idx = ws = None
    if return_indices:
        lead = (n,) if batched else ()
        idx = torch.empty(lead + (nd,) + tuple(mask.shape[-nd:]), dtype=torch.int32, device=mask.device)
        ws = torch.empty(2 * mask.numel(), dtype=torch.int32, device=mask.device)
    call("fplx_edt_squared", ptr(mask), n, d, h, w, nd, (ctypes.c_double * 3)(*([1.0] * (3 - nd) + s)), ptr(phantom), ptr(sq),
         ptr(idx), ptr(ws), 0 if ws is None else ws.numel() * 4, stream())
    return (sq, idx) if return_indices else sq


def edt_pass(g, axis, sampling=1.0):
    """one pass of the transform IN PLACE on a float64 map [N,D,H,W] along axis 0 (D), 1 (H) or 2 (W):
    g[j] = min_i (g[i] + ((j - i) * sampling)^2) on every line (+inf allowed); returns g"""
    require_gpu(g)
    if not (g.dim() == 4 and g.dtype == torch.float64 and g.is_contiguous()):
        raise ValueError("fplx: edt_pass takes a contiguous float64 [N,D,H,W] map")
    n, d, h, w = g.shape
    call("fplx_edt_pass", ptr(g), n, d, h, w, int(axis), float(sampling), stream())
    return g


def edt_finish(sq_a, sq_b=None):
    """sqrt(sq_a), or with sq_b the signed map sqrt(sq_b) - sqrt(sq_a) of get_euclidean_distance; float64 in and out"""
    require_gpu(sq_a, sq_b)
    for t in (sq_a, sq_b):
        if t is not None and not (t.dtype == torch.float64 and t.is_contiguous() and t.shape == sq_a.shape):
            raise ValueError("fplx: edt_finish takes contiguous float64 maps of one shape")
    out = torch.empty_like(sq_a)
    call("fplx_edt_finish", ptr(sq_a), ptr(sq_b), ptr(out), sq_a.numel(), stream())
    return out


def label_bbox(label, mask_labels):
    """-> (count, bb_min[4], bb_max[4]) of {label in mask_labels} on a uint8 [C,D,H,W] label (one device->host copy)"""
    require_gpu(label)
    assert label.dtype == torch.uint8 and label.dim() == 4 and label.is_contiguous()
    c, d, h, w = label.shape
    ml = torch.tensor([int(v) for v in mask_labels], dtype=torch.int32, device=label.device)
    out = torch.empty(9, dtype=torch.int32, device=label.device)
    call("fplx_label_bbox", ptr(label), c, d, h, w, ptr(ml), ml.numel(), ptr(out), stream())
    o = out.tolist()
    return o[0], o[1:5], o[5:9]


def nonzero_bbox(x):
    """-> (count, bb_min[4], bb_max[4]) of {x != 0} on a float32 [C,D,H,W] volume, numpy.nonzero's test (a NaN counts, -0.0
    does not); one device->host copy.  count == 0: bb_min / bb_max are meaningless"""
    require_gpu(x)
    if not (x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("fplx: nonzero_bbox takes a contiguous float32 [C,D,H,W] volume")
    c, d, h, w = x.shape
    out = torch.empty(9, dtype=torch.int32, device=x.device)
    call("fplx_nonzero_bbox", ptr(x), c, d, h, w, ptr(out), stream())
    o = out.tolist()
    return o[0], o[1:5], o[5:9]


def label_lut_table(source_list, target_list):
    """the 256-entry table of convert_label (util/image_process.py:194-208) on uint8 labels: lut[v] = sum of the targets of
    every source equal to v, mod 256 - a source listed twice adds its targets and wraps, labels not listed map to 0"""
    if len(source_list) != len(target_list):
        raise ValueError("fplx: label conversion takes as many targets as sources")
    lut = [0] * 256
    for s, t in zip(source_list, target_list):
        if not (isinstance(s, (int, np.integer)) and isinstance(t, (int, np.integer)) and 0 <= s <= 255 and 0 <= t <= 255):
            raise ValueError("fplx: label conversion takes integer labels in 0..255, got {0!r} -> {1!r}".format(s, t))
        lut[int(s)] = (lut[int(s)] + int(t)) % 256
    return lut


def label_lut(label, lut, out=None):
    """out = lut[label] on a uint8 volume of any shape; lut: 256 integers in 0..255 (a list, or a uint8 device tensor)"""
    require_gpu(label)
    if not (label.dtype == torch.uint8 and label.is_contiguous() and label.numel() > 0):
        raise ValueError("fplx: label_lut takes a non-empty contiguous uint8 volume")
    if not torch.is_tensor(lut):
        lut = torch.tensor([int(v) for v in lut], dtype=torch.uint8, device=label.device)
    require_gpu(lut)
    if not (lut.dtype == torch.uint8 and lut.numel() == 256 and lut.is_contiguous()):
        raise ValueError("fplx: label_lut takes a table of 256 uint8 entries")
    out = torch.empty_like(label) if out is None else out
    call("fplx_label_lut", ptr(label), ptr(out), label.numel(), ptr(lut), stream())
    return out


def partial_label_to_probability(label, class_num):
    """uint8 label [D,H,W] (or any shape) with `class_num` marking unlabelled voxels -> (fp32 one-hot [class_num, *shape],
    fp32 weight [*shape] = 1 - (label == class_num), largest label as a python int: one device->host copy)"""
    require_gpu(label)
    if not (label.dtype == torch.uint8 and label.is_contiguous() and label.numel() > 0):
        raise ValueError("fplx: partial_label_to_probability takes a non-empty contiguous uint8 volume")
    prob = torch.empty((class_num,) + tuple(label.shape), dtype=torch.float32, device=label.device)
    weight = torch.empty(tuple(label.shape), dtype=torch.float32, device=label.device)
    top = torch.empty(1, dtype=torch.int32, device=label.device)
    call("fplx_partial_label_to_probability", ptr(label), ptr(prob), ptr(weight), int(class_num), label.numel(), ptr(top),
         stream())
    return prob, weight, int(top.item())


def paste_roi(sub, lower, out_size):
    """zeros of [C,*out_size] with the [C,d,h,w] volume `sub` at `lower`: the inverse of a crop, every element written once"""
    require_gpu(sub)
    if not (sub.dim() == 4 and sub.is_contiguous()):
        raise ValueError("fplx: paste_roi takes a contiguous [C,D,H,W] volume")
    c, sd, sh, sw = sub.shape
    od, oh, ow = (int(v) for v in out_size)
    out = torch.empty((c, max(od, 0), max(oh, 0), max(ow, 0)), dtype=sub.dtype, device=sub.device)
    call("fplx_paste_roi", ptr(sub), ptr(out), _elem_bytes(sub), c, sd, sh, sw, od, oh, ow, int(lower[0]), int(lower[1]),
         int(lower[2]), stream())
    return out


def label_to_probability(label, class_num):
    """uint8 label [D,H,W] (or any shape) -> fp32 one-hot [class_num, *shape]"""
    require_gpu(label)
    assert label.dtype == torch.uint8 and label.is_contiguous()
    prob = torch.empty((class_num,) + tuple(label.shape), dtype=torch.float32, device=label.device)
    call("fplx_label_to_probability", ptr(label), ptr(prob), class_num, label.numel(), stream())
    return prob


def set_weight_(pixel_weight, image_weight):
    """NiftyDataset.set_weight_ in place on a fp32 device volume"""
    require_gpu(pixel_weight)
    assert pixel_weight.dtype == torch.float32 and pixel_weight.is_contiguous()
    call("fplx_set_weight", ptr(pixel_weight), pixel_weight.numel(), float(image_weight), stream())
    return pixel_weight


def overlap_counts(seg, gt, labels, fuse=False, on_device=False):
    """exact voxel counts [rows, 3] = (|seg==l & gt==l|, |seg==l|, |gt==l|) as python ints (one device->host copy), or with
    on_device the int64 device tensor (no copy: a training loop that reads the host once per round)"""
    require_gpu(seg, gt)
    if seg.shape != gt.shape:
        raise ValueError("fplx: segmentation and ground truth shapes differ")
    assert seg.dtype == torch.uint8 and gt.dtype == torch.uint8
    s, g = seg.contiguous(), gt.contiguous()
    lab = torch.tensor([int(v) for v in labels], dtype=torch.int32, device=s.device)
    rows = 1 if fuse else lab.numel()
    out = torch.empty((rows, 3), dtype=torch.int64, device=s.device)
    call("fplx_overlap_counts", ptr(s), ptr(g), s.numel(), ptr(lab), lab.numel(), 1 if fuse else 0, ptr(out), stream())
    return out if on_device else out.tolist()


def edge_points(mask):
    """get_edge_points of a binary uint8 device volume [D, H, W] ([H, W]: the 2D form) -> uint8 edge map"""
    require_gpu(mask)
    assert mask.dtype == torch.uint8 and mask.dim() in (2, 3)
    m = mask.contiguous()
    d, h, w = (1,) + tuple(m.shape) if m.dim() == 2 else tuple(m.shape)
    edge = torch.empty_like(m)
    call("fplx_surface_edge_points", ptr(m), d, h, w, ptr(edge), stream())
    return edge


def surface_min_dist(query_zyx, seed_zyx, spacing):
    """distance (GeodisTK raster-scan metric on a constant image) from each int32 (z, y, x) query row to the nearest
    seed row -> fp32 [nq]; 1e10 everywhere when there is no seed"""
    require_gpu(query_zyx)
    assert query_zyx.dtype == torch.int32 and query_zyx.dim() == 2 and query_zyx.shape[1] == 3
    assert seed_zyx.dtype == torch.int32 and seed_zyx.dim() == 2 and seed_zyx.shape[1] == 3
    q, sd = query_zyx.contiguous(), seed_zyx.contiguous()
    out = torch.empty((q.shape[0],), dtype=torch.float32, device=q.device)
    if q.shape[0] == 0:
        return out
    call("fplx_surface_min_dist", ptr(q), q.shape[0], ptr(sd) if sd.shape[0] else 0, sd.shape[0], float(spacing[0]),
         float(spacing[1]), float(spacing[2]), ptr(out), stream())
    return out


# ---------------------------------------------------------------- prediction post-processing (csrc/postprocess.hip)
_CC_HEAD = 320          # ints in front of the per-voxel workspace (include/fplx.h FPLX_CC_LABEL_WS_BYTES / FPLX_KLC_WS_BYTES)


def _cc_volume(seg):
    require_gpu(seg)
    if seg.dtype != torch.uint8 or seg.dim() not in (2, 3):
        raise ValueError("fplx: connected components take a uint8 volume [D, H, W] or [H, W], got {0:} {1:}".format(
            seg.dtype, tuple(seg.shape)))
    s = seg.contiguous()
    d, h, w = (1,) + tuple(s.shape) if s.dim() == 2 else tuple(s.shape)
    return s, d, h, w


def _cc_check(ws):
    err = int(ws[0].item())
    if err:
        raise _lib.FplxError("fplx: connected components: a union-find loop reached its iteration cap (error word %d)" % err)


def connected_components(seg, per_class=False):
    """6-connected components of a uint8 device volume [D, H, W] ([H, W]: 4-connected) -> int32 labels of the same shape:
    the C-order linear index of the component's first voxel, -1 for background.  per_class: neighbours join only when
    their values are equal (every class labelled in one pass); otherwise whenever both are nonzero.  Synchronises once
    (error word)."""
    s, d, h, w = _cc_volume(seg)
    labels = torch.empty(s.shape, dtype=torch.int32, device=s.device)
    ws = torch.empty(_CC_HEAD, dtype=torch.int32, device=s.device)
    call("fplx_cc_label", ptr(s), d, h, w, 1 if per_class else 0, ptr(labels), ptr(ws), ws.numel() * 4, stream())
    _cc_check(ws)
    return labels


def keep_largest_component(seg, mode=1):
    """PostKeepLargestComponent on a uint8 device volume [D, H, W] or [H, W]: mode 1 keeps the largest component of the
    foreground, mode 2 the largest component of every foreground class; every component of the largest size is kept.
    Synchronises once (error word)."""
    if mode not in (1, 2):
        raise ValueError("fplx: keep_largest_component mode must be 1 or 2, got {0!r}".format(mode))
    s, d, h, w = _cc_volume(seg)
    out = torch.empty_like(s)
    ws = torch.empty(_CC_HEAD + 2 * s.numel(), dtype=torch.int32, device=s.device)
    call("fplx_keep_largest_component", ptr(s), d, h, w, 1 if mode == 2 else 0, ptr(out), ptr(ws), ws.numel() * 4,
         stream())
    _cc_check(ws)
    return out


# ---- semi-supervised learning (include/fplx.h, "semi-supervised learning"; csrc/ssl.hip)
def _ssl_f32(*ts):
    require_gpu(*ts)
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("fplx ssl: tensors must be contiguous fp32")


def ssl_perturb(x, noise=None, reps=1, sigma=0.1, clip=0.2, seed=0, stream_id=0, out=None):
    """-> y [reps, *x.shape] = x + clamp(sigma z, -clip, clip) per repetition (ssl_mt.py:79, ssl_uamt.py:83-85); z = `noise`
    ([reps, *x.shape] fp32, torch's CPU result bit for bit) or, with noise None, drawn on the device from (seed, stream_id)"""
    _ssl_f32(x, noise, out)
    n = x.numel()
    if noise is not None and noise.numel() != reps * n:
        raise ValueError("fplx ssl_perturb: noise has {0:} elements for {1:} x {2:}".format(noise.numel(), reps, n))
    out = torch.empty((reps,) + tuple(x.shape), dtype=torch.float32, device=x.device) if out is None else out
    if out.numel() != reps * n:
        raise ValueError("fplx ssl_perturb: out has {0:} elements for {1:} x {2:}".format(out.numel(), reps, n))
    call("fplx_ssl_perturb", ptr(x), ptr(noise), ptr(out), n, int(reps), float(sigma), float(clip),
         int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF, stream())
    return out


def ssl_part(logits, k):
    """the fp32 partial-row workspace of a consistency (k = 2) or entropy (k = 1) forward over `logits`"""
    n, _, v = _ncv(logits)
    return torch.empty((n, loss_rows(v), k), dtype=torch.float32, device=logits.device)


def ssl_consistency_fwd(student, teacher, mc=None, thr=0.0, softmax=True, part=None, out=None, mask=None):
    """student, teacher [N, C, ...]; mc [T, N, C, ...] or None (MeanTeacher) -> (out double [4]: masked sum of squares, kept
    voxels, loss, 0; mask uint8 [N, ...] or None)"""
    _ssl_f32(student, teacher, mc)
    n, c, v = _ncv(student)
    if teacher.shape != student.shape:
        raise ValueError("fplx ssl: teacher {0:} and student {1:} differ in shape".format(tuple(teacher.shape), tuple(student.shape)))
    t = 0 if mc is None else int(mc.shape[0])
    if mc is not None and tuple(mc.shape[1:]) != tuple(student.shape):
        raise ValueError("fplx ssl: mc must be [T] + the student's shape, got {0:}".format(tuple(mc.shape)))
    dev = student.device
    part = ssl_part(student, 2) if part is None else part
    out = torch.empty(4, dtype=torch.float64, device=dev) if out is None else out
    if t > 0 and mask is None:
        mask = torch.empty((n,) + tuple(student.shape[2:]), dtype=torch.uint8, device=dev)
    call("fplx_ssl_consistency_fwd", ptr(student), ptr(teacher), ptr(mc), t, n, c, v, float(thr), 1 if softmax else 0,
         ptr(mask) if t > 0 else 0, ptr(part), ptr(out), stream())
    return out, (mask if t > 0 else None)


def ssl_consistency_bwd(student, teacher, mask, out, gscale, t, softmax=True, dstudent=None):
    """-> dstudent = gscale[0] dLoss/dstudent of the forward that wrote `out` and `mask` (t: its number of MC passes)"""
    _ssl_f32(student, teacher, gscale)
    n, c, v = _ncv(student)
    dstudent = torch.empty_like(student) if dstudent is None else dstudent
    call("fplx_ssl_consistency_bwd", ptr(student), ptr(teacher), ptr(mask), ptr(out), ptr(gscale), n, c, v, int(t),
         1 if softmax else 0, ptr(dstudent), stream())
    return dstudent


def ssl_entropy_fwd(logits, softmax=True, part=None, out=None):
    """EntropyLoss (loss/seg/ssl.py:32-44) -> out double [4]: sum of -sum_c p' ln p', N V, loss, 0"""
    _ssl_f32(logits)
    n, c, v = _ncv(logits)
    part = ssl_part(logits, 1) if part is None else part
    out = torch.empty(4, dtype=torch.float64, device=logits.device) if out is None else out
    call("fplx_ssl_entropy_fwd", ptr(logits), n, c, v, 1 if softmax else 0, ptr(part), ptr(out), stream())
    return out


def ssl_entropy_bwd(logits, gscale, softmax=True, dlogits=None):
    _ssl_f32(logits, gscale)
    n, c, v = _ncv(logits)
    dlogits = torch.empty_like(logits) if dlogits is None else dlogits
    call("fplx_ssl_entropy_bwd", ptr(logits), ptr(gscale), n, c, v, 1 if softmax else 0, ptr(dlogits), stream())
    return dlogits


def ema_step(ema, p, alpha):
    """ema = alpha ema + (1 - alpha) p in place over two flat fp32 buffers of the same length (ssl_mt.py:112-113)"""
    _ssl_f32(ema, p)
    if ema.numel() != p.numel():
        raise ValueError("fplx ema_step: {0:} and {1:} elements".format(ema.numel(), p.numel()))
    call("fplx_ema_step", ptr(ema), ptr(p), ema.numel(), float(alpha), stream())
    return ema


def _ssl_table(ts, what, lo, hi):
    """K contiguous fp32 tensors of one shape -> (list, n, c, v)"""
    ts = list(ts)
    if not lo <= len(ts) <= hi:
        raise ValueError("fplx ssl: {0:} takes {1:} to {2:} logit tensors, got {3:}".format(what, lo, hi, len(ts)))
    _ssl_f32(*ts)
    for t in ts[1:]:
        if t.shape != ts[0].shape:
            raise ValueError("fplx ssl: {0:}: the logit tensors differ in shape: {1:} and {2:}".format(
                what, tuple(ts[0].shape), tuple(t.shape)))
    return (ts,) + _ncv(ts[0])


def ssl_pyramid_fwd(logits_list, part=None, out=None):
    """URPC's regulariser (ssl_urpc.py:76-91) over K = 2..4 logit tensors [N, C, ...] (the unlabelled rows) -> out double
    [4 K + 2]: per scale A_k, B_k, V_k, L_k; then loss_reg and 0 (include/fplx.h)"""
    ls, n, c, v = _ssl_table(logits_list, "ssl_pyramid_fwd", 2, 4)
    k = len(ls)
    part = ssl_part(ls[0], 3 * k) if part is None else part
    out = torch.empty(4 * k + 2, dtype=torch.float64, device=ls[0].device) if out is None else out
    call("fplx_ssl_pyramid_fwd", _ptrs(ls), k, n, c, v, ptr(part), ptr(out), stream())
    return out


def ssl_pyramid_bwd(logits_list, out, gscale, dlogits=None):
    """-> K tensors dlogits_j = gscale[0] d loss_reg / d logits_j of the forward that wrote `out`, in one launch"""
    ls, n, c, v = _ssl_table(logits_list, "ssl_pyramid_bwd", 2, 4)
    _ssl_f32(gscale)
    require_gpu(out)
    dlogits = [torch.empty_like(t) for t in ls] if dlogits is None else list(dlogits)
    if len(dlogits) != len(ls):
        raise ValueError("fplx ssl_pyramid_bwd: {0:} gradient tensors for {1:} logit tensors".format(len(dlogits), len(ls)))
    _ssl_f32(*dlogits)
    call("fplx_ssl_pyramid_bwd", _ptrs(ls), ptr(out), ptr(gscale), len(ls), n, c, v, _ptrs(dlogits), stream())
    return dlogits


def ssl_pseudo_onehot(logits_list, onehot=None):
    """K = 1..3 logit tensors [N, C, ...] -> K fp32 one-hot tensors of the first maximum over C (ssl_cps.py:103-106), one launch"""
    ls, n, c, v = _ssl_table(logits_list, "ssl_pseudo_onehot", 1, 3)
    onehot = [torch.empty_like(t) for t in ls] if onehot is None else list(onehot)
    if len(onehot) != len(ls):
        raise ValueError("fplx ssl_pseudo_onehot: {0:} outputs for {1:} logit tensors".format(len(onehot), len(ls)))
    _ssl_f32(*onehot)
    call("fplx_ssl_pseudo_onehot", _ptrs(ls), len(ls), n, c, v, _ptrs(onehot), stream())
    return onehot


# ---- weakly-supervised learning (include/fplx.h, "weakly-supervised learning"; csrc/wsl.hip)
_CRF_TILE = 16


def _wsl_dims(logits, image=None):
    """logits [N, C, D, H, W] (and the image [N, Ci, D, H, W] of the same spatial shape) -> (n, c, ci, d, h, w)"""
    if logits.dim() != 5:
        raise ValueError("fplx wsl: logits must be [N, C, D, H, W], got {0:}D".format(logits.dim()))
    n, c, d, h, w = (int(s) for s in logits.shape)
    ci = 0
    if image is not None:
        if image.dim() != 5 or image.shape[0] != n or tuple(image.shape[2:]) != (d, h, w):
            raise ValueError("fplx wsl: image {0:} does not match logits {1:}".format(tuple(image.shape), tuple(logits.shape)))
        ci = int(image.shape[1])
    return n, c, ci, d, h, w


def wsl_gatedcrf_fwd(logits, image, desc, radius, softmax=True, kp=None, part=None, out=None):
    """GatedCRFLoss.forward (loss/seg/gatedcrf.py:18-110, Potts, no masks) over the slices of logits [N, C, D, H, W] and image
    [N, Ci, D, H, W]; desc: [(weight, sigma_xy, sigma_rgb)] with 0 for an absent modality -> (out double [4]: the sum, 0, the
    loss, N D H W; kp fp32, the shape of the logits)"""
    _ssl_f32(logits, image, kp, part)
    n, c, ci, d, h, w = _wsl_dims(logits, image)
    flat = [float(x) for row in desc for x in row]
    if len(flat) != 3 * len(desc):
        raise ValueError("fplx wsl: a kernel descriptor is (weight, sigma_xy, sigma_rgb)")
    arr = (ctypes.c_float * max(len(flat), 1))(*flat)
    dev = logits.device
    kp = torch.empty_like(logits) if kp is None else kp
    rows = n * d * ((h + _CRF_TILE - 1) // _CRF_TILE) * ((w + _CRF_TILE - 1) // _CRF_TILE)
    part = torch.empty(rows, dtype=torch.float32, device=dev) if part is None else part
    if part.numel() < rows:
        raise ValueError("fplx wsl: part has {0:} elements, {1:} needed".format(part.numel(), rows))
    out = torch.empty(4, dtype=torch.float64, device=dev) if out is None else out
    call("fplx_wsl_gatedcrf_fwd", ptr(logits), ptr(image), n, c, ci, d, h, w, ctypes.cast(arr, ctypes.c_void_p), len(desc),
         int(radius), 1 if softmax else 0, ptr(kp), ptr(part), ptr(out), stream())
    return out, kp


def wsl_gatedcrf_bwd(logits, kp, gscale, softmax=True, dlogits=None):
    """-> dlogits = gscale[0] dLoss/dlogits of the forward that wrote `kp`"""
    _ssl_f32(logits, kp, gscale, dlogits)
    n, c, _, d, h, w = _wsl_dims(logits)
    dlogits = torch.empty_like(logits) if dlogits is None else dlogits
    call("fplx_wsl_gatedcrf_bwd", ptr(logits), ptr(kp), ptr(gscale), n, c, d, h, w, 1 if softmax else 0, ptr(dlogits), stream())
    return dlogits


def wsl_tv_fwd(logits, softmax=True, count=None, ws=None, part=None, out=None):
    """TotalVariationLoss.forward (loss/seg/ssl.py:68-86) for logits [N, C, D, H, W] -> (out double [4]: sum of contour, 0,
    the loss, N C D H W; count int32, the shape of the logits)"""
    _ssl_f32(logits, part)
    n, c, _, d, h, w = _wsl_dims(logits)
    dev = logits.device
    e = logits.numel()
    count = torch.empty(logits.shape, dtype=torch.int32, device=dev) if count is None else count
    ws = torch.empty(3 * e, dtype=torch.int32, device=dev) if ws is None else ws
    part = torch.empty(n * c * loss_rows(d * h * w), dtype=torch.float32, device=dev) if part is None else part
    out = torch.empty(4, dtype=torch.float64, device=dev) if out is None else out
    require_gpu(count, ws)
    if count.dtype != torch.int32 or count.numel() != e or not count.is_contiguous():
        raise ValueError("fplx wsl: count must be contiguous int32 of the logits' shape")
    call("fplx_wsl_tv_fwd", ptr(logits), n, c, d, h, w, 1 if softmax else 0, ptr(count), ptr(ws), ws.numel() * ws.element_size(),
         ptr(part), ptr(out), stream())
    return out, count


def wsl_tv_bwd(logits, count, gscale, softmax=True, dlogits=None):
    _ssl_f32(logits, gscale, dlogits)
    n, c, _, d, h, w = _wsl_dims(logits)
    dlogits = torch.empty_like(logits) if dlogits is None else dlogits
    call("fplx_wsl_tv_bwd", ptr(logits), ptr(count), ptr(gscale), n, c, d, h, w, 1 if softmax else 0, ptr(dlogits), stream())
    return dlogits


def wsl_mumford_shah_fwd(logits, image, penalty=1, lam=1.0, softmax=True, cen=None, part=None, out=None):
    """MumfordShahLoss.forward (loss/seg/mumford_shah.py:62-95) -> (out double [4]: the level-set sum, the gradient sum, the
    loss, N C D H W; cen fp32 [N, D, Ci, C], the per-slice centroids)"""
    _ssl_f32(logits, image, cen, part)
    n, c, ci, d, h, w = _wsl_dims(logits, image)
    dev = logits.device
    cen = torch.empty((n, d, ci, c), dtype=torch.float32, device=dev) if cen is None else cen
    part = torch.empty(n * d * loss_rows(h * w) * c * (1 + ci), dtype=torch.float32, device=dev) if part is None else part
    out = torch.empty(4, dtype=torch.float64, device=dev) if out is None else out
    call("fplx_wsl_mumford_shah_fwd", ptr(logits), ptr(image), n, c, ci, d, h, w, int(penalty), float(lam), 1 if softmax else 0,
         ptr(cen), ptr(part), ptr(out), stream())
    return out, cen


def wsl_mumford_shah_bwd(logits, image, cen, gscale, penalty=1, lam=1.0, softmax=True, dlogits=None):
    _ssl_f32(logits, image, cen, gscale, dlogits)
    n, c, ci, d, h, w = _wsl_dims(logits, image)
    dlogits = torch.empty_like(logits) if dlogits is None else dlogits
    call("fplx_wsl_mumford_shah_bwd", ptr(logits), ptr(image), ptr(cen), ptr(gscale), n, c, ci, d, h, w, int(penalty), float(lam),
         1 if softmax else 0, ptr(dlogits), stream())
    return dlogits


# ---- noisy-label learning (include/fplx.h, "noisy-label learning"; csrc/nll.hip)
NLL_RANK, NLL_BELOW = 0, 1                          # FPLX_NLL_RANK / FPLX_NLL_BELOW
NLL_USES = {"CoTeaching": (2, 1), "TriNet": (6, 5, 3)}       # bit i of uses[j]: mask i gates network j


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _nll_list(ts, what):
    ts = list(ts)
    if not 1 <= len(ts) <= 3:
        raise ValueError("fplx nll: {0:} takes 1 to 3 tensors, got {1:}".format(what, len(ts)))
    for t in ts[1:]:
        if t.shape != ts[0].shape:
            raise ValueError("fplx nll: {0:} differ in shape: {1:} and {2:}".format(what, tuple(ts[0].shape), tuple(t.shape)))
    return ts


def nll_quantile_rank(q, n):
    """where torch.quantile(x, q) looks in the sorted float32 array of n values -> (k, w): the result is torch's lerp of s[k] and
    s[k + 1] with the weight w.  torch makes q a tensor of the input's dtype, so pos = float32(q) * float32(n - 1) is rounded
    to float32 (beyond n = 2^24 the rank itself is rounded: torch's choice, kept); k = floor(pos), w = pos - k.  A pos that
    float32(n - 1) rounded past the last element reads the last element."""
    if not 0.0 <= q <= 1.0:
        raise ValueError("quantile() q values must be in the range [0, 1]")
    pos = np.float32(q) * np.float32(n - 1)
    k = np.floor(pos)
    if k >= n - 1:
        return n - 1, 0.0
    return int(k), float(np.float32(pos - k))


def nll_voxel_ce_fwd(logits_list, label, loss=None, part=None):
    """K logit tensors [N, C, ...] and one soft label of that shape -> (loss: list of K fp32 [N V], the per-voxel cross entropy
    -sum_c y_c ln(0.999 p_c + 5e-4) in reshape_tensor_to_2D's voxel order; part fp32 [K, N, fplx_nll_ce_rows(V)], the partials of
    their sums)"""
    ls = _nll_list(logits_list, "logits")
    _ssl_f32(label, *ls)
    n, c, v = _ncv(ls[0])
    if label.shape != ls[0].shape:
        raise ValueError("fplx nll: label {0:} and logits {1:} differ in shape".format(tuple(label.shape), tuple(ls[0].shape)))
    dev = label.device
    loss = [torch.empty(n * v, dtype=torch.float32, device=dev) for _ in ls] if loss is None else loss
    part = torch.empty((len(ls), n, _lib.lib().fplx_nll_ce_rows(v)), dtype=torch.float32, device=dev) if part is None else part
    call("fplx_nll_voxel_ce_fwd", _ptrs(ls), len(ls), ptr(label), n, c, v, _ptrs(loss), ptr(part), stream())
    return loss, part


def nll_select_mask(loss, mode, num_remb=0, q=None, mask=None):
    """loss fp32 [n] -> mask uint8 [n].  NLL_RANK: the first num_remb entries of a stable ascending argsort (CoTeaching's
    ind_sorted[:num_remb]); NLL_BELOW: loss < torch.quantile(loss, q) (TriNet).  The order statistics come from select_kth
    and stay on the device."""
    _chan(loss)
    n = loss.numel()
    mask = torch.empty(n, dtype=torch.uint8, device=loss.device) if mask is None else mask
    if mode == NLL_RANK:
        num_remb = int(num_remb)
        if not 0 <= num_remb <= n:
            raise ValueError("fplx nll_select_mask: num_remb = {0:} outside [0, {1:}]".format(num_remb, n))
        sk = ws = None
        nb = _lib.lib().fplx_nll_mask_ws_bytes()
        if num_remb > 0:
            sk = select_kth(loss, [num_remb - 1])
            ws = torch.empty(nb // 4, dtype=torch.int32, device=loss.device)
        call("fplx_nll_select_mask", ptr(loss), n, NLL_RANK, num_remb, 0.0, ptr(sk), 0, ptr(mask), ptr(ws), nb, stream())
    elif mode == NLL_BELOW:
        k, w = nll_quantile_rank(q, n)
        sk = select_kth(loss, [k, n - 1])                   # the largest rides along: NaN sorts last
        call("fplx_nll_select_mask", ptr(loss), n, NLL_BELOW, 0, w, ptr(sk), sk[1].data_ptr(), ptr(mask), 0, 0, stream())
    else:
        raise ValueError("fplx nll_select_mask: mode {0:} (NLL_RANK, NLL_BELOW)".format(mode))
    return mask


def nll_select_fwd(loss, masks, uses, part, out=None):
    """K losses [n], K masks [n], uses[j] = bit set of the masks that gate network j, part = nll_voxel_ce_fwd's -> out double
    [K, 4]: sum of the kept loss_j, number kept, their mean (NaN for an empty selection), sum of all loss_j"""
    loss, masks = _nll_list(loss, "losses"), list(masks)
    require_gpu(part, *(loss + masks))
    k, n = len(loss), loss[0].numel()
    if len(masks) != k or len(uses) != k or any(m.numel() != n or m.dtype != torch.uint8 for m in masks):
        raise ValueError("fplx nll_select_fwd: {0:} losses need {0:} uint8 masks of {1:} elements and {0:} uses".format(k, n))
    if part.numel() % k:
        raise ValueError("fplx nll_select_fwd: part has {0:} elements for {1:} networks".format(part.numel(), k))
    dev = loss[0].device
    out = torch.empty((k, 4), dtype=torch.float64, device=dev) if out is None else out
    nb = _lib.lib().fplx_nll_select_ws_bytes()
    ws = torch.empty(nb // 4, dtype=torch.int32, device=dev)
    call("fplx_nll_select_fwd", _ptrs(loss), _ptrs(masks), (ctypes.c_int * k)(*[int(u) for u in uses]), k, n, ptr(part),
         part.numel() // k, ptr(out), ptr(ws), nb, stream())
    return out


def nll_select_bwd(logits_list, label, masks, uses, out, gscale, wj, dlogits=None):
    """-> K tensors dlogits_j = gscale[0] wj d(mean of the kept loss_j) / dlogits_j of the forward that wrote `out`"""
    ls, masks = _nll_list(logits_list, "logits"), list(masks)
    _ssl_f32(label, gscale, *ls)
    require_gpu(out, *masks)
    n, c, v = _ncv(ls[0])
    k = len(ls)
    if len(masks) != k or len(uses) != k or any(m.numel() != n * v or m.dtype != torch.uint8 for m in masks):
        raise ValueError("fplx nll_select_bwd: {0:} logits need {0:} uint8 masks of {1:} elements and {0:} uses".format(k, n * v))
    dlogits = [torch.empty_like(t) for t in ls] if dlogits is None else dlogits
    call("fplx_nll_select_bwd", _ptrs(ls), ptr(label), _ptrs(masks), (ctypes.c_int * k)(*[int(u) for u in uses]), k, ptr(out),
         ptr(gscale), float(wj), n, c, v, _ptrs(dlogits), stream())
    return dlogits


# ---- confident learning (csrc/cl.hip): psx fp32 planar [C, M], s uint8 [M]; every cut stays on the device

CL_BY_CLASS, CL_BY_NOISE_RATE, CL_BOTH = 0, 1, 2


def _cl_planar(psx, s=None, what="psx"):
    """-> (c, m) of a planar [C, M] float32 tensor whose class planes are contiguous and follow each other (a view at an
    offset is fine: the kernels fall back to one voxel per lane where a base is not 16-byte aligned)"""
    require_gpu(psx, s)
    if not (psx.dtype == torch.float32 and psx.dim() == 2 and psx.numel() > 0 and psx.is_contiguous()):
        raise ValueError("fplx cl: {0:} must be a non-empty contiguous float32 tensor [C, M]".format(what))
    c, m = int(psx.shape[0]), int(psx.shape[1])
    if s is not None and not (s.dtype == torch.uint8 and s.dim() == 1 and s.numel() == m and s.is_contiguous()):
        raise ValueError("fplx cl: the labels must be a contiguous uint8 tensor of {0:} elements".format(m))
    return c, m


def cl_softmax(x, out=None):
    """logits fp32 planar [C, M] -> psx of that shape, the max-subtracted fp32 softmax over the classes, written once"""
    c, m = _cl_planar(x, what="the logits")
    out = torch.empty_like(x) if out is None else out
    if _cl_planar(out, what="out") != (c, m):
        raise ValueError("fplx cl_softmax: out has another shape than the logits")
    call("fplx_cl_softmax", ptr(x), c, m, ptr(out), stream())
    return out


def cl_class_stats(psx, s):
    """-> (sums float64 [C], counts int64 [C + 2], thr float64 [C]) on the device: counts[k] = #{s == k}, counts[C] = #{s >= C},
    counts[C + 1] = #{voxels with a NaN}; sums[k] = the float64 sum of psx[k] over s == k; thr = sums / counts"""
    c, m = _cl_planar(psx, s)
    dev = psx.device
    nb = _lib.lib().fplx_cl_stats_ws_bytes()
    ws = torch.empty((nb + 7) // 8, dtype=torch.int64, device=dev)
    sums = torch.empty(c, dtype=torch.float64, device=dev)
    thr = torch.empty(c, dtype=torch.float64, device=dev)
    counts = torch.empty(c + 2, dtype=torch.int64, device=dev)
    call("fplx_cl_class_stats", ptr(psx), ptr(s), c, m, ptr(ws), ws.numel() * 8, ptr(sums), ptr(counts), ptr(thr), stream())
    return sums, counts, thr


def cl_confident_joint(psx, s, thr):
    """-> joint int64 [C, C] on the device: joint[s][guess] over the voxels with a confident class (thr: device float64 [C])"""
    c, m = _cl_planar(psx, s)
    require_gpu(thr)
    if not (thr.dtype == torch.float64 and thr.numel() == c and thr.is_contiguous()):
        raise ValueError("fplx cl_confident_joint: thr must be a contiguous float64 tensor of {0:} elements".format(c))
    joint = torch.empty((c, c), dtype=torch.int64, device=psx.device)
    call("fplx_cl_confident_joint", ptr(psx), ptr(s), c, m, ptr(thr), ptr(joint), stream())
    return joint


def cl_select_keys(psx, s, k, j=-1, out=None):
    """-> keys fp32 [M] for select_kth: psx[k] (j < 0) or -(psx[j] - psx[k]) where s == k, NaN elsewhere"""
    c, m = _cl_planar(psx, s)
    out = torch.empty(m, dtype=torch.float32, device=psx.device) if out is None else _chan(out)
    if out.numel() != m:
        raise ValueError("fplx cl_select_keys: out has {0:} elements for {1:} voxels".format(out.numel(), m))
    call("fplx_cl_select_keys", ptr(psx), ptr(s), c, m, int(k), int(j), ptr(out), stream())
    return out


def cl_noise_mask(psx, s, method, class_cut=None, pair_cut=None, pair_active=None):
    """-> (mask uint8 [M], count int64 [1]) on the device.  class_cut fp32 [C] and pair_cut fp32 [C, C] are device tensors,
    pair_active a host array [C, C] (pair_cut[k, j] is read where pair_active[k, j])"""
    c, m = _cl_planar(psx, s)
    require_gpu(class_cut, pair_cut)
    for t, n, what in ((class_cut, c, "class_cut"), (pair_cut, c * c, "pair_cut")):
        if t is not None and not (t.dtype == torch.float32 and t.numel() == n and t.is_contiguous()):
            raise ValueError("fplx cl_noise_mask: {0:} must be a contiguous float32 tensor of {1:} elements".format(what, n))
    act = None
    if pair_active is not None:
        act = np.ascontiguousarray(np.asarray(pair_active) != 0, np.uint8)
        if act.shape != (c, c):
            raise ValueError("fplx cl_noise_mask: pair_active must be [{0:}, {0:}]".format(c))
    mask = torch.empty(m, dtype=torch.uint8, device=psx.device)
    count = torch.empty(1, dtype=torch.int64, device=psx.device)
    call("fplx_cl_noise_mask", ptr(psx), ptr(s), c, m, int(method), ptr(class_cut), ptr(pair_cut),
         None if act is None else act.ctypes.data, ptr(mask), ptr(count), stream())
    return mask, count
