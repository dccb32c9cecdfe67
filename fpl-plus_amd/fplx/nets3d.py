"""UNet2D5 and UNet3D - drop-ins for the reference's dense 3D networks behind PyMIC's SegNetDict
(reference: PyMIC/pymic/net/net3d/unet2d5.py:144-211, PyMIC/pymic/net/net3d/unet3d.py:81-160, registry
PyMIC/pymic/net/net_dict_seg.py).

Same constructor (`params` dict), same state_dict keys and shapes (`block0.conv.conv_conv.0.weight`,
`in_conv.conv_conv.{0,1,4,5}.*`, `down1.maxpool_conv.1.conv_conv.*`, `up1.conv1x1.*` / `up1.up.*`, `out_conv{,1,2,3}.*`): a
checkpoint written by the reference loads with strict=True and the other way round.  torch.nn modules are parameter
containers only; all arithmetic runs in the HIP kernels of libfplx.so.  There is no CPU path.

The two networks share ONE forward / backward schedule, `Schedule3D` below, built from fplx.ops - plain launches on the
current stream, no fusion beyond the DownBlock tail, no second stream, weight packs rebuilt by every forward.  fplx.engine
(the benchmarked UNet2D5_dsbn path) is not touched.  What differs between the two is data:
  UNet2D5   five levels, conv_dims per level (2: Conv2d / MaxPool2d / ConvTranspose2d per depth slice), PReLU, (1,3,3) out_conv
  UNet3D    four or five levels, all 3D, LeakyReLU(0.01) (the BatchNorm + activation kernels read the slope from a device
            float; its gradient lands in scratch), 1x1x1 out_conv through fplx_head_*, optional deep supervision: 1x1x1
            heads on the decoder outputs of levels 1-3, brought to full size by fplx_interp_* - forward returns a list of four.

Differences, on purpose:
  * params['precision'] = 'fp32' (default, parity mode) | 'bf16', as for UNet2D5_dsbn.
  * forward(x, domain_label=None): domain_label is accepted and ignored (the DSBN agent passes it to every network).
  * UNet3D: feature_chns must be multiples of 8 (at most 512) and class_num at most 8 - the head kernels' limits.
"""
import torch
import torch.nn as nn

from . import ops
from ._lib import F32


# ---------------------------------------------------------------------------------------------- parameter containers
class ConvBlock(nn.Module):
    """`conv_conv`: conv, BatchNorm, activation, Dropout, conv, BatchNorm, activation - the member indices are the state_dict
    keys (0, 1, 4, 5; with PReLU also 2 and 6)"""

    def __init__(self, in_channels, out_channels, dropout_p, dim=3, prelu=False):
        super(ConvBlock, self).__init__()
        conv, bn = (nn.Conv3d, nn.BatchNorm3d) if dim == 3 else (nn.Conv2d, nn.BatchNorm2d)
        act = nn.PReLU if prelu else nn.LeakyReLU
        self.dim = dim
        self.dropout_p = float(dropout_p)
        self.conv_conv = nn.Sequential(conv(in_channels, out_channels, kernel_size=3, padding=1), bn(out_channels), act(),
                                       nn.Dropout(dropout_p),
                                       conv(out_channels, out_channels, kernel_size=3, padding=1), bn(out_channels), act())

    @property
    def dropout(self):
        return self.conv_conv[3]


class _Down3D(nn.Module):
    def __init__(self, in_channels, out_channels, dropout_p):
        super(_Down3D, self).__init__()
        self.maxpool_conv = nn.Sequential(nn.MaxPool3d(2), ConvBlock(in_channels, out_channels, dropout_p))


class _Up3D(nn.Module):
    def __init__(self, in_channels1, in_channels2, out_channels, dropout_p, trilinear):
        super(_Up3D, self).__init__()
        self.trilinear = bool(trilinear)
        if self.trilinear:
            self.conv1x1 = nn.Conv3d(in_channels1, in_channels2, kernel_size=1)
            self.up = nn.Upsample(scale_factor=2, mode='trilinear', align_corners=True)
        else:
            self.up = nn.ConvTranspose3d(in_channels1, in_channels2, kernel_size=2, stride=2)
        self.conv = ConvBlock(in_channels2 * 2, out_channels, dropout_p)


class _Down25(nn.Module):
    def __init__(self, in_channels, out_channels, dim, dropout_p, downsample):
        super(_Down25, self).__init__()
        self.dim = dim
        self.conv = ConvBlock(in_channels, out_channels, dropout_p, dim, prelu=True)
        if downsample:
            self.down_layer = (nn.MaxPool2d if dim == 2 else nn.MaxPool3d)(kernel_size=2, stride=2)


class _Up25(nn.Module):
    def __init__(self, in_channels1, in_channels2, out_channels, dim, dropout_p, bilinear):
        super(_Up25, self).__init__()
        self.dim, self.bilinear = dim, bool(bilinear)
        if self.bilinear:
            conv = nn.Conv2d if dim == 2 else nn.Conv3d
            self.up = nn.Sequential(conv(in_channels1, in_channels2, kernel_size=1),
                                    nn.Upsample(scale_factor=2, mode='bilinear' if dim == 2 else 'trilinear', align_corners=True))
        else:
            self.up = (nn.ConvTranspose2d if dim == 2 else nn.ConvTranspose3d)(in_channels1, in_channels2, kernel_size=2, stride=2)
        self.conv = ConvBlock(in_channels2 * 2, out_channels, dropout_p, dim, prelu=True)


# ---------------------------------------------------------------------------------------------- the schedule
class _Saved(object):
    __slots__ = ("x", "dims", "train", "seed", "step", "blocks", "skips", "packs", "xd")


class Schedule3D(object):
    """forward / backward of a `_Net3D` as a fixed sequence of fplx.ops launches on the current stream.  Activations are NDHWC
    2-D views [voxels, channels] in the network's act_dtype; the skip / up concat of a decoder level is one [voxels, 2 C] buffer
    that the encoder and the up-sampling write into.  Block b of the dropout stream: encoder level i -> i, decoder level l -> 8 - l."""

    def __init__(self, net):
        self.net = net
        self.ws = None

    def invalidate(self):
        """nothing is cached between forwards (the packs are rebuilt every time): kept for the optimisers' interface"""

    def _workspace(self, nbytes, dev):
        nbytes = max(int(nbytes), 16)
        if self.ws is None or self.ws.numel() < nbytes or self.ws.device != dev:
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self.ws

    def _pack(self, adt):
        net, packs = self.net, {}
        first = net._blocks[0]
        for blk in net._blocks:
            for i in (0, 4):
                conv = blk["cc"][i]
                want_wb = not (blk is first and i == 0)              # no data gradient w.r.t. the network input
                pack = ops.pack_conv2d_weight if conv.weight.dim() == 4 else ops.pack_conv_weight
                packs[id(conv)] = pack(conv.weight, adt, want_wb)
        for up in net._ups:
            w = up["mod"].weight
            if up["linear"]:                                         # kernel-1 convolution in front of the x2 upsampling
                packs[id(up["mod"])] = ops.pack_conv_weight(w.reshape(w.shape[0], w.shape[1], 1, 1, 1), adt, True)
            else:
                packs[id(up["mod"])] = ops.pack_deconv_weight(w, adt)
        if not net._head_out:                                        # (1,3,3) out_conv -> fp32 planar logits
            oc = net.out_conv
            packs["out_conv"] = (ops.pack_conv_weight(oc.weight, torch.float32, False)[0], ops.pack_conv_weight(oc.weight, adt, True)[1])
        return packs

    # ------------------------------------------------------------------ forward
    def forward(self, x, train, drop_on, seed, step, keep):
        """x fp32 [N, Cin, D, H, W] on the GPU -> ([logits fp32 [N, classes, D, H, W], ...], saved state or None)"""
        net = self.net
        ops.require_gpu(x)
        if x.dim() != 5:
            raise ValueError('expected 5D input (got {}D input)'.format(x.dim()))
        x = x.float().contiguous()
        N, Cin, D, H, W = x.shape
        if Cin != net.in_chns:
            raise ValueError("fplx: input has {0:} channels, network expects {1:}".format(Cin, net.in_chns))
        L, ft = net.levels, net.ft_chns
        pds = [2 if net.dims[l] == 3 else 1 for l in range(L - 1)]      # depth factor of the pooling after level l
        dfac = 1
        for f in pds:
            dfac *= f
        hw = 1 << (L - 1)
        if (D % dfac) or (H % hw) or (W % hw):
            raise ValueError("fplx: H, W must be multiples of %d and D of %d (%d 2x poolings, depth only at the 3D levels), "
                             "got %dx%dx%d" % (hw, dfac, L - 1, D, H, W))
        dev, adt = x.device, net.act_dtype
        a_dt = ops._DT[adt]
        dims = [(N, D, H, W)]
        for l in range(L - 1):
            dims.append((N, dims[l][1] // pds[l], dims[l][2] // 2, dims[l][3] // 2))
        vox = [n * d * h * w for (n, d, h, w) in dims]
        packs = self._pack(adt)
        sv = _Saved()
        sv.x, sv.dims, sv.train, sv.seed, sv.step, sv.packs, sv.blocks = x, dims, train, seed, step, packs, {}

        def empty(v, c):
            return torch.empty((v, c), dtype=adt, device=dev)

        cats = [empty(vox[l], 2 * ft[l]) for l in range(L - 1)]
        skips = [cats[l][:, :ft[l]] for l in range(L - 1)]
        ups = [cats[l][:, ft[l]:] for l in range(L - 1)]
        sv.skips = skips

        def conv_site(xin, xs, x_dt, cin, conv, bn, slope, l, out_view, p, sid, pool=None):
            cout = conv.weight.shape[0]
            mid = conv.weight.dim() == 4              # Conv2d of a 2.5D level: its pack lives in the middle depth plane
            y = empty(vox[l], cout)
            bnbuf = torch.empty((4, cout), dtype=torch.float32, device=dev)
            stats, rows = None, 0
            if train:
                rows = ops.conv3d_stats_rows(dims[l], cin, cout, (3, 3, 3), x_dt, a_dt, mid)
                stats = torch.empty((rows, 2, cout), dtype=torch.float32, device=dev)
            ops.conv3d_fwd(xin, xs, x_dt, packs[id(conv)][0], conv.bias, y, ops.cl_strides(*dims[l][1:], cout), a_dt, dims[l], cin,
                           cout, (3, 3, 3), stats, mid=mid)
            if train:
                ops.bn_train_finalize(stats, rows, cout, vox[l], bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                      bn.num_batches_tracked, bnbuf, bn.momentum, bn.eps)
            else:
                ops.bn_eval_prepare(bn.weight, bn.bias, bn.running_mean, bn.running_var, bnbuf, bn.eps)
            if pool is not None:
                ops.bn_act_pool_fwd(y, out_view, pool[0], bnbuf, slope, dims[l], cout, pool[1])
            else:
                ops.bn_act_fwd(y, out_view, bnbuf, slope, p, seed, sid, cout)
            return y, bnbuf

        def conv_block(blk, xin, xs, x_dt, cin, out_view, pool=None):
            l, b, cc = blk["level"], blk["b"], blk["cc"]
            c = ft[l]
            a1 = empty(vox[l], c)
            sid = step * 16 + b
            p1 = blk["mod"].dropout_p if drop_on[b] else 0.0
            s1, s2 = net._slopes(blk)
            y1, bn1 = conv_site(xin, xs, x_dt, cin, cc[0], cc[1], s1, l, a1, p1, sid)
            y2, bn2 = conv_site(a1, ops.cl_strides(*dims[l][1:], c), a_dt, c, cc[4], cc[5], s2, l, out_view, 0.0, 0, pool)
            sv.blocks[b] = dict(xin=xin, xs=xs, x_dt=x_dt, cin=cin, y1=y1, bn1=bn1, p1=p1, sid=sid, a1=a1, y2=y2, bn2=bn2,
                                out=out_view)

        # ---- encoder
        cur, cur_s, cur_dt, cur_c = x, ops.planar_strides(Cin, D, H, W), F32, Cin
        for i in range(L):
            blk = net._blocks[i]
            last = i == L - 1
            out_view = empty(vox[i], ft[i]) if last else skips[i]
            pooled = None if last else empty(vox[i + 1], ft[i])
            fused = not last and ops.bn_pool_fused_ok(ft[i], adt)
            conv_block(blk, cur, cur_s, cur_dt, cur_c, out_view, (pooled, pds[i]) if fused else None)
            if last:
                cur = out_view
            else:
                if not fused:
                    ops.maxpool2_fwd(out_view, pooled, dims[i], ft[i], pds[i])
                cur, cur_s, cur_dt, cur_c = pooled, ops.cl_strides(*dims[i + 1][1:], ft[i]), a_dt, ft[i]
        xd = {L - 1: cur}                              # decoder outputs by level (the deepest encoder output below them)
        # ---- decoder
        for l in range(L - 2, -1, -1):
            up = net._ups[l]
            if up["linear"]:
                low = empty(vox[l + 1], ft[l])
                ops.conv3d_fwd(cur, ops.cl_strides(*dims[l + 1][1:], ft[l + 1]), a_dt, packs[id(up["mod"])][0], up["mod"].bias, low,
                               ops.cl_strides(*dims[l + 1][1:], ft[l]), a_dt, dims[l + 1], ft[l + 1], ft[l], (1, 1, 1), None)
                ops.upsample2_fwd(low, ups[l], dims[l + 1], ft[l], pds[l])
            else:
                ops.deconv2_fwd(cur, packs[id(up["mod"])][0], up["mod"].bias, ups[l], dims[l + 1], ft[l + 1], ft[l], pds[l])
            out = empty(vox[l], ft[l])
            conv_block(net._blocks[L + (L - 2 - l)], cats[l], ops.cl_strides(*dims[l][1:], 2 * ft[l]), a_dt, 2 * ft[l], out)
            cur = out
            xd[l] = out
        sv.xd = xd
        # ---- output heads -> fp32 planar logits
        ncls = net.n_class
        logits = torch.empty((N, ncls, D, H, W), dtype=torch.float32, device=dev)
        if net._head_out:
            ops.head_fwd(cur, net.out_conv.weight, net.out_conv.bias, logits, N, vox[0] // N, ft[0], ncls)
        else:
            ops.conv3d_fwd(cur, ops.cl_strides(D, H, W, ft[0]), a_dt, packs["out_conv"][0], net.out_conv.bias, logits,
                           ops.planar_strides(ncls, D, H, W), F32, dims[0], ft[0], ncls, (1, 3, 3), None)
        outs = [logits]
        for l, head in net._deep_heads:
            coarse = torch.empty((N, ncls) + tuple(dims[l][1:]), dtype=torch.float32, device=dev)
            ops.head_fwd(xd[l], head.weight, head.bias, coarse, N, vox[l] // N, ft[l], ncls)
            full = torch.empty_like(logits)
            ops.interp_fwd(coarse, full, N * ncls, dims[l][1:], 1 << l)
            outs.append(full)
        return outs, (sv if keep else None)

    # ------------------------------------------------------------------ backward
    def backward(self, sv, douts, gflat):
        """douts: one fp32 [N, classes, D, H, W] gradient (or None) per output of forward; gflat: flat fp32 gradient buffer laid
        out like net.flat_params"""
        net = self.net
        dims, packs, train = sv.dims, sv.packs, sv.train
        L, ft, ncls = net.levels, net.ft_chns, net.n_class
        N, D, H, W = dims[0]
        dev, adt = gflat.device, net.act_dtype
        a_dt = ops._DT[adt]
        vox = [n * d * h * w for (n, d, h, w) in dims]
        pds = [2 if net.dims[l] == 3 else 1 for l in range(L - 1)]
        gflat.zero_()                  # BatchNorm affine / PReLU gradients are accumulated by their finalize kernels
        gv = net.grad_views(gflat)
        name_of = net._name_of

        def g(t):
            return gv[name_of[id(t)]]

        def empty(v, c):
            return torch.empty((v, c), dtype=adt, device=dev)

        need = 16
        for b, blk in sv.blocks.items():
            l = net._block_by_b[b]["level"]
            two_d = net._block_by_b[b]["mod"].dim == 2
            for cin in (blk["cin"], ft[l]):
                need = max(need, ops.conv2d_wgrad_ws_bytes(dims[l], cin, ft[l]) if two_d else
                           ops.conv3d_wgrad_ws_bytes(dims[l], cin, ft[l], (3, 3, 3)))
        for l in range(L - 1):
            if net._ups[l]["linear"]:
                need = max(need, ops.conv3d_wgrad_ws_bytes(dims[l + 1], ft[l + 1], ft[l], (1, 1, 1)))
            else:
                need = max(need, ops.deconv2_wgrad_ws_bytes(dims[l + 1], ft[l + 1], ft[l], pds[l]))
        if net._head_out:
            need = max(need, ops.head_wgrad_ws_bytes(N, vox[0] // N, ft[0], ncls))
        else:
            need = max(need, ops.conv3d_wgrad_ws_bytes(dims[0], ft[0], ncls, (1, 3, 3)))
        for l, _ in net._deep_heads:
            need = max(need, ops.head_wgrad_ws_bytes(N, vox[l] // N, ft[l], ncls))
        ws = self._workspace(need, dev)
        maxc = max(ft) * 2
        part = torch.empty(ops.num_partials(vox[0]) * (2 * maxc + 1), dtype=torch.float32, device=dev)
        coef = torch.empty((2, maxc), dtype=torch.float32, device=dev)
        scratch = torch.zeros(4, dtype=torch.float32, device=dev)       # where LeakyReLU's slope "gradient" goes

        # ---- the deep-supervision heads: their logits' gradients back to the coarse grids, their weight gradients
        dcoarse = {}
        for (l, head), dfull in zip(net._deep_heads, douts[1:]):
            if dfull is None:
                continue
            dc = torch.empty((N, ncls) + tuple(dims[l][1:]), dtype=torch.float32, device=dev)
            ops.interp_bwd(dfull.float().contiguous(), dc, N * ncls, dims[l][1:], 1 << l)
            ops.head_wgrad(sv.xd[l], dc, g(head.weight), g(head.bias), N, vox[l] // N, ft[l], ncls, ws)
            dcoarse[l] = (dc, head)
        # ---- out_conv
        d0 = douts[0]
        d0 = torch.zeros((N, ncls, D, H, W), dtype=torch.float32, device=dev) if d0 is None else d0.float().contiguous()
        last = sv.xd[0]
        d_cur = empty(vox[0], ft[0])
        oc = net.out_conv
        if net._head_out:
            ops.head_dgrad(d0, oc.weight, d_cur, N, vox[0] // N, ft[0], ncls, False)
            ops.head_wgrad(last, d0, g(oc.weight), g(oc.bias), N, vox[0] // N, ft[0], ncls, ws)
        else:
            ops.conv3d_fwd(d0, ops.planar_strides(ncls, D, H, W), F32, packs["out_conv"][1], None, d_cur,
                           ops.cl_strides(D, H, W, ft[0]), a_dt, dims[0], ncls, ft[0], (1, 3, 3), None)
            ops.conv3d_wgrad(last, ops.cl_strides(D, H, W, ft[0]), a_dt, d0, ops.planar_strides(ncls, D, H, W), F32, g(oc.weight),
                             g(oc.bias), dims[0], ft[0], ncls, (1, 3, 3), ws)

        def site_bwd(conv, bn, slope, y, bnbuf, p, sid, d_out, xin, xs, x_dt, cin, l, want_dx, dx_view, reduced=False):
            """backward of conv -> BatchNorm -> activation -> dropout; d_out is overwritten with dy"""
            c = ft[l]
            dslope = gv[name_of[id(slope)]] if id(slope) in name_of else scratch
            ops.bn_act_bwd(y, d_out, d_out, bnbuf, slope, p, sv.seed, sid, c, train, g(bn.weight), g(bn.bias), dslope, part, coef,
                           reduced)
            db = None if train else g(conv.bias)   # conv bias in front of train-mode BatchNorm: d/d bias = sum of dy = 0 exactly
            gw = g(conv.weight)
            two_d = gw.dim() == 4
            ys = ops.cl_strides(*dims[l][1:], c)
            if want_dx:
                ops.conv3d_fwd(d_out, ys, a_dt, packs[id(conv)][1], None, dx_view,
                               ops.cl_strides(*dims[l][1:], ops.ld_of(dx_view)), a_dt, dims[l], c, cin, (3, 3, 3), None, mid=two_d)
            if two_d:
                ops.conv2d_wgrad(xin, xs, x_dt, d_out, ys, a_dt, gw, db, dims[l], cin, c, ws)
            else:
                ops.conv3d_wgrad(xin, xs, x_dt, d_out, ys, a_dt, gw, db, dims[l], cin, c, (3, 3, 3), ws)

        def block_bwd(meta, d_out, want_dx, reduced=False):
            """d_out: gradient w.r.t. the block output [V, C] (overwritten) -> d(block input) or None"""
            blk, cc, l = sv.blocks[meta["b"]], meta["cc"], meta["level"]
            c, cin = ft[l], blk["cin"]
            s1, s2 = net._slopes(meta)
            d_a1 = empty(vox[l], c)
            site_bwd(cc[4], cc[5], s2, blk["y2"], blk["bn2"], 0.0, 0, d_out, blk["a1"], ops.cl_strides(*dims[l][1:], c), a_dt, c, l,
                     True, d_a1, reduced)
            d_in = empty(vox[l], cin) if want_dx else None
            site_bwd(cc[0], cc[1], s1, blk["y1"], blk["bn1"], blk["p1"], blk["sid"], d_a1, blk["xin"], blk["xs"], blk["x_dt"], cin,
                     l, want_dx, d_in)
            return d_in

        # ---- decoder, level 0 upwards
        d_skips = [None] * (L - 1)
        for l in range(L - 1):
            d_cat = block_bwd(net._blocks[L + (L - 2 - l)], d_cur, True)                 # [V_l, 2 ft_l]
            d_skips[l], d_up = d_cat[:, :ft[l]], d_cat[:, ft[l]:]
            up = net._ups[l]
            mod, xin = up["mod"], sv.xd[l + 1]
            d_cur = empty(vox[l + 1], ft[l + 1])
            if up["linear"]:
                d_low = empty(vox[l + 1], ft[l])
                ops.upsample2_bwd(d_up, d_low, dims[l + 1], ft[l], pds[l])
                lows, highs = ops.cl_strides(*dims[l + 1][1:], ft[l]), ops.cl_strides(*dims[l + 1][1:], ft[l + 1])
                ops.conv3d_fwd(d_low, lows, a_dt, packs[id(mod)][1], None, d_cur, highs, a_dt, dims[l + 1], ft[l], ft[l + 1],
                               (1, 1, 1), None)
                ops.conv3d_wgrad(xin, highs, a_dt, d_low, lows, a_dt, g(mod.weight), g(mod.bias), dims[l + 1], ft[l + 1], ft[l],
                                 (1, 1, 1), ws)
            else:
                ops.deconv2_dgrad(d_up, packs[id(mod)][1], d_cur, dims[l + 1], ft[l + 1], ft[l], pds[l])
                ops.deconv2_wgrad(xin, d_up, g(mod.weight), g(mod.bias), dims[l + 1], ft[l + 1], ft[l], ws, pds[l])
            if (l + 1) in dcoarse:                   # the level's output has a second consumer: its deep-supervision head
                dc, head = dcoarse[l + 1]
                ops.head_dgrad(dc, head.weight, d_cur, N, vox[l + 1] // N, ft[l + 1], ncls, True)
        # ---- encoder, deepest level upwards
        d_pool = block_bwd(net._blocks[L - 1], d_cur, True)
        for i in range(L - 2, -1, -1):
            meta = net._blocks[i]
            blk = sv.blocks[i]
            d_a2 = empty(vox[i], ft[i])
            fused = ops.bn_pool_fused_ok(ft[i], adt)
            if fused:          # pooling gradient + skip gradient and the BatchNorm reduction over the result, in one pass
                ops.pool_bwd_bn_reduce(blk["y2"], d_pool, d_skips[i], d_a2, blk["bn2"], net._slopes(meta)[1], dims[i], ft[i], part,
                                       pds[i])
            else:
                ops.maxpool2_bwd(sv.skips[i], d_pool, d_skips[i], d_a2, dims[i], ft[i], pds[i])
            d_pool = block_bwd(meta, d_a2, i > 0, fused)
        return gflat


class _Net3DFunction(torch.autograd.Function):
    """One autograd node for the whole network: forward / backward are Schedule3D's."""

    @staticmethod
    def forward(ctx, x, net, train, drop_on, seed, step, keep, *params):
        outs, sv = net.engine.forward(x, train, drop_on, seed, step, keep)
        ctx.net, ctx.sv = net, sv
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        net, sv = ctx.net, ctx.sv
        if sv is None:
            raise RuntimeError("fplx: backward through a forward that ran under no_grad")
        gflat = torch.empty_like(net.flat_params)
        net.engine.backward(sv, douts, gflat)
        ctx.sv = None
        gv = net.grad_views(gflat)
        return (None,) * 7 + tuple(gv[name] for name in net._order)


# ---------------------------------------------------------------------------------------------- the networks
class _Net3D(nn.Module):
    """what UNet2D5 and UNet3D share: the flat parameter buffer (the fused optimisers' interface: _ensure_flat, _order,
    _layout, segments, get_param, engine.invalidate) and the call"""
    num_domains = 1            # one BatchNorm statistics set

    def _init_common(self, params):
        prec = params.get('precision', 'fp32')
        if prec not in ('fp32', 'bf16'):
            raise ValueError("fplx {0:}: precision must be fp32 or bf16 (got {1:})".format(type(self).__name__, prec))
        self.act_dtype = torch.float32 if prec == 'fp32' else torch.bfloat16
        self.dropout_seed = int(params.get('dropout_seed', 1))
        self._fwd_counter = 0
        self.flat_params = None
        self._layout = None

    def _finish(self):
        """after the members exist: per-block tables for the schedule"""
        self._block_by_b = {blk["b"]: blk for blk in self._blocks}
        self.block_modules = [blk["mod"] for blk in self._blocks]
        self.engine = Schedule3D(self)

    def _slopes(self, blk):
        cc = blk["cc"]
        if isinstance(cc[2], nn.PReLU):
            return cc[2].weight, cc[6].weight
        return self.leaky_slope, self.leaky_slope

    # ------------------------------------------------------------------ parameter bookkeeping
    def _ensure_flat(self):
        """all parameters as views of ONE flat fp32 buffer, in named_parameters() order - the reference's net.parameters()
        order, so optimiser states translate index by index (fplx.checkpoint); every parameter starts on a 16-byte boundary"""
        named = dict(self.named_parameters())
        first = next(iter(named.values()))
        fp = self.flat_params
        ok = fp is not None and fp.device == first.device
        if ok:
            base, end = fp.data_ptr(), fp.data_ptr() + fp.numel() * 4
            ok = all(base <= p.data_ptr() < end for p in named.values())
        if ok:
            return
        order = list(named.keys())
        total = sum((named[k].numel() + 3) // 4 * 4 for k in order)
        flat = torch.zeros(total, dtype=torch.float32, device=first.device)
        layout, off = {}, 0
        for k in order:
            p = named[k]
            n = p.numel()
            flat[off:off + n].copy_(p.data.reshape(-1).float())
            p.data = flat[off:off + n].view(p.shape)
            layout[k] = (off, n, tuple(p.shape))
            off += (n + 3) // 4 * 4
        self.flat_params, self._layout, self._order, self._named = flat, layout, order, named
        self._name_of = {id(p): k for k, p in named.items()}
        self.engine.invalidate()

    def get_param(self, name):
        return self._named[name]

    def grad_views(self, gflat):
        return {k: gflat[o:o + n].view(shp) for k, (o, n, shp) in self._layout.items()}

    def segments(self):
        """-> (shared (start, end), []): one segment, there are no per-domain BatchNorm sets"""
        return (0, self.flat_params.numel()), []

    def reference_param_names(self):
        """net.parameters() order of the reference class (same members in the same definition order)"""
        return [k for k, _ in self.named_parameters()]

    # ------------------------------------------------------------------ nn.Module surface
    def _apply(self, fn, recurse=True):
        r = super(_Net3D, self)._apply(fn, recurse)
        self.flat_params = None          # parameters were re-created: re-flatten lazily
        return r

    def load_state_dict(self, state_dict, strict=True, **kw):
        r = super(_Net3D, self).load_state_dict(state_dict, strict=strict, **kw)
        self.engine.invalidate()
        return r

    def parameters_changed(self):
        self.engine.invalidate()

    def dropout_active(self):
        """by block id of the dropout stream: the nn.Dropout child's own training flag decides (what the reference's
        test-time dropout flips, agent_seg.py:845-852)"""
        on = [False] * 9
        for blk in self._blocks:
            on[blk["b"]] = bool(blk["mod"].dropout.training and blk["mod"].dropout_p > 0)
        return on

    def forward(self, x, domain_label=None):
        if not x.is_cuda:
            raise RuntimeError("fplx {0:} runs on the GPU only (libfplx.so HIP kernels); got a CPU tensor".format(
                type(self).__name__))
        self._ensure_flat()
        params = [self._named[k] for k in self._order]
        step = self._fwd_counter
        self._fwd_counter += 1
        outs = _Net3DFunction.apply(x, self, self.training, self.dropout_active(), self.dropout_seed, step,
                                    torch.is_grad_enabled(), *params)
        return list(outs) if len(outs) > 1 else outs[0]


class UNet2D5(_Net3D):
    def __init__(self, params):
        super(UNet2D5, self).__init__()
        self.params = params
        self.in_chns = params['in_chns']
        self.ft_chns = list(params['feature_chns'])
        self.dropout = list(params['dropout'])
        self.dims = list(params['conv_dims'])
        self.n_class = params['class_num']
        self.bilinear = params['bilinear']
        assert (len(self.ft_chns) == 5)                                     # unet2d5.py:180
        if len(self.dims) != 5 or any(d not in (2, 3) for d in self.dims):
            raise ValueError("fplx UNet2D5: conv_dims must be five values out of {{2, 3}} (got {0:})".format(self.dims))
        self._init_common(params)
        ft, dp, dm = self.ft_chns, self.dropout, self.dims
        self.levels = 5
        self.block0 = _Down25(self.in_chns, ft[0], dm[0], dp[0], True)
        self.block1 = _Down25(ft[0], ft[1], dm[1], dp[1], True)
        self.block2 = _Down25(ft[1], ft[2], dm[2], dp[2], True)
        self.block3 = _Down25(ft[2], ft[3], dm[3], dp[3], True)
        self.block4 = _Down25(ft[3], ft[4], dm[4], dp[4], False)
        self.up1 = _Up25(ft[4], ft[3], ft[3], dm[3], dp[3], self.bilinear)
        self.up2 = _Up25(ft[3], ft[2], ft[2], dm[2], dp[2], self.bilinear)
        self.up3 = _Up25(ft[2], ft[1], ft[1], dm[1], dp[1], self.bilinear)
        self.up4 = _Up25(ft[1], ft[0], ft[0], dm[0], dp[0], self.bilinear)
        self.out_conv = nn.Conv3d(ft[0], self.n_class, kernel_size=(1, 3, 3), padding=(0, 1, 1))
        downs = [self.block0, self.block1, self.block2, self.block3, self.block4]
        upm = [self.up1, self.up2, self.up3, self.up4]                       # levels 3, 2, 1, 0
        self._blocks = [dict(mod=d.conv, cc=d.conv.conv_conv, level=i, b=i) for i, d in enumerate(downs)]
        self._blocks += [dict(mod=u.conv, cc=u.conv.conv_conv, level=3 - j, b=5 + j) for j, u in enumerate(upm)]
        self._ups = [None] * 4
        for j, u in enumerate(upm):
            self._ups[3 - j] = dict(mod=u.up[0] if self.bilinear else u.up, linear=bool(self.bilinear))
        self._head_out = False
        self._deep_heads = []
        self._finish()


class UNet3D(_Net3D):
    def __init__(self, params):
        super(UNet3D, self).__init__()
        self.params = params
        self.in_chns = params['in_chns']
        self.ft_chns = list(params['feature_chns'])
        self.dropout = list(params['dropout'])
        self.n_class = params['class_num']
        self.trilinear = params['trilinear']
        self.deep_sup = params['deep_supervise']
        assert (len(self.ft_chns) == 5 or len(self.ft_chns) == 4)           # unet3d.py:114
        if any(c % 8 or c > 512 for c in self.ft_chns) or not 1 <= self.n_class <= 8:
            raise ValueError("fplx UNet3D: feature_chns must be multiples of 8 up to 512 and class_num at most 8 (the 1x1x1 "
                             "head kernels), got {0:} / {1:}".format(self.ft_chns, self.n_class))
        self._init_common(params)
        ft, dp = self.ft_chns, self.dropout
        L = self.levels = len(ft)
        self.dims = [3] * L
        self.in_conv = ConvBlock(self.in_chns, ft[0], dp[0])
        self.down1 = _Down3D(ft[0], ft[1], dp[1])
        self.down2 = _Down3D(ft[1], ft[2], dp[2])
        self.down3 = _Down3D(ft[2], ft[3], dp[3])
        if L == 5:
            self.down4 = _Down3D(ft[3], ft[4], dp[4])
            self.up1 = _Up3D(ft[4], ft[3], ft[3], dp[3], self.trilinear)
        self.up2 = _Up3D(ft[3], ft[2], ft[2], dp[2], self.trilinear)
        self.up3 = _Up3D(ft[2], ft[1], ft[1], dp[1], self.trilinear)
        self.up4 = _Up3D(ft[1], ft[0], ft[0], dp[0], self.trilinear)
        self.out_conv = nn.Conv3d(ft[0], self.n_class, kernel_size=1)
        if self.deep_sup:
            self.out_conv1 = nn.Conv3d(ft[1], self.n_class, kernel_size=1)
            self.out_conv2 = nn.Conv3d(ft[2], self.n_class, kernel_size=1)
            self.out_conv3 = nn.Conv3d(ft[3], self.n_class, kernel_size=1)
        # LeakyReLU's slope where the BatchNorm + activation kernels read it: a device float (not a parameter, not saved)
        self.register_buffer("leaky_slope", torch.full((1,), 0.01, dtype=torch.float32), persistent=False)
        enc = [self.in_conv] + [getattr(self, "down%d" % i).maxpool_conv[1] for i in range(1, L)]
        self._blocks = [dict(mod=m, cc=m.conv_conv, level=i, b=i) for i, m in enumerate(enc)]
        self._ups = [None] * (L - 1)
        for l in range(L - 2, -1, -1):                                       # up(4 - l) works at level l
            u = getattr(self, "up%d" % (4 - l))
            self._blocks.append(dict(mod=u.conv, cc=u.conv.conv_conv, level=l, b=8 - l))
            self._ups[l] = dict(mod=u.conv1x1 if self.trilinear else u.up, linear=bool(self.trilinear))
        self._head_out = True
        self._deep_heads = [(1, self.out_conv1), (2, self.out_conv2), (3, self.out_conv3)] if self.deep_sup else []
        self._finish()
