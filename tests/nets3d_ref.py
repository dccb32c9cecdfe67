"""CPU restatement (test infrastructure, NOT product code) of the dense 3D networks UNet2D5 and UNet3D and of
DeepSuperviseLoss, over a state dict with the reference's keys: the same ATen CPU operators the reference calls, arranged by
our own code, pinned against fixtures produced by running the reference itself (tests/golden/make_golden_nets3d.py ->
nets3d_*.npz; tests/test_nets3d_cpu.py).  Citations are reference paths under PyMIC/pymic/.

act_dtype = torch.bfloat16 rounds to bf16 where the HIP schedule (fplx/nets3d.py) stores bf16 tensors: packed convolution
weights, every convolution output, every activation; the 1x1x1 heads keep fp32 weights and write fp32 logits.
"""
import torch
import torch.nn.functional as F

from oracle.torch_ref import quant, split_state, prelu, fold_depth, unfold_depth, dice_loss, BN_EPS, BN_MOMENTUM  # noqa: F401
from oracle.torch_ref import tap, act, pool


def batch_norm(x, sd, key, train, unrounded=None):
    """nn.BatchNorm2d / 3d through the operator the reference's module calls: batch statistics in train mode (and the running
    update, momentum 0.1, unbiased variance), running statistics otherwise.
    unrounded: the convolution output before it was rounded to its bf16 storage - the convolution kernels form the statistics
    from their fp32 accumulators (include/fplx.h, fplx_conv3d_fwd: `stats` ... of the (unrounded) outputs) and the BatchNorm pass
    applies them to the stored tensor x"""
    if train:
        sd[key + ".num_batches_tracked"] += 1
    rm, rv = sd[key + ".running_mean"], sd[key + ".running_var"]
    if unrounded is None or not train:
        return F.batch_norm(x, rm, rv, sd[key + ".weight"], sd[key + ".bias"], train, BN_MOMENTUM, BN_EPS)
    red = (0,) + tuple(range(2, x.dim()))
    mean, var = unrounded.mean(red), unrounded.var(red, unbiased=False)
    n = x.numel() / x.shape[1]
    with torch.no_grad():
        rm.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * mean.detach())
        rv.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * var.detach() * n / (n - 1))
    sh = (1, -1) + (1,) * (x.dim() - 2)
    return (x - mean.view(sh)) * torch.rsqrt(var.view(sh) + BN_EPS) * sd[key + ".weight"].view(sh) + sd[key + ".bias"].view(sh)


def conv_block(x, sd, key, train, act_dtype, leaky, tape=None):
    """`conv_conv` (unet3d.py:20-28 with LeakyReLU, unet2d5.py:22-40 with PReLU; dropout 0): 2D when the weights are"""
    conv = F.conv2d if sd[key + ".0.weight"].dim() == 4 else F.conv3d
    rounding = act_dtype is not None and act_dtype != torch.float32
    for c, b, a in ((0, 1, 2), (4, 5, 6)):
        y = conv(x, quant(sd["%s.%d.weight" % (key, c)], act_dtype), sd["%s.%d.bias" % (key, c)], padding=1)
        x = batch_norm(tap(tape, "conv", quant(y, act_dtype)), sd, "%s.%d" % (key, b), train, y if rounding else None)
        x = act(tape, x, 0.01 if leaky else sd["%s.%d.weight" % (key, a)])
        x = quant(x, act_dtype)
    return x


def unet3d_forward(sd, params, x, train=True, act_dtype=None, round_input=True, tape=None):
    """UNet3D.forward (unet3d.py:137-160) -> tensor, or the list of four with deep supervision"""
    L = len(params["feature_chns"])
    x = quant(x, act_dtype) if round_input else x
    xs = [conv_block(x, sd, "in_conv.conv_conv", train, act_dtype, True, tape)]
    for i in range(1, L):
        xs.append(conv_block(pool(tape, xs[-1]), sd, "down%d.maxpool_conv.1.conv_conv" % i, train, act_dtype, True, tape))
    h = xs[-1]
    xd = {L - 1: h}
    for l in range(L - 2, -1, -1):
        key = "up%d" % (4 - l)
        if params["trilinear"]:
            up = quant(F.conv3d(h, quant(sd[key + ".conv1x1.weight"], act_dtype), sd[key + ".conv1x1.bias"]), act_dtype)
            up = quant(F.interpolate(up, scale_factor=2, mode="trilinear", align_corners=True), act_dtype)
        else:
            up = quant(F.conv_transpose3d(h, quant(sd[key + ".up.weight"], act_dtype), sd[key + ".up.bias"], stride=2), act_dtype)
        h = conv_block(torch.cat([tap(tape, "skip", xs[l]), tap(tape, "up", up)], dim=1), sd, key + ".conv.conv_conv", train, act_dtype,
                       True, tape)
        xd[l] = h
    out = F.conv3d(xd[0], sd["out_conv.weight"], sd["out_conv.bias"])
    if not params["deep_supervise"]:
        return out
    outs = [out]
    for l in (1, 2, 3):
        o = F.conv3d(tap(tape, "head", xd[l]), sd["out_conv%d.weight" % l], sd["out_conv%d.bias" % l])
        outs.append(F.interpolate(o, list(out.shape[2:]), mode="trilinear"))
    return outs


def unet2d5_forward(sd, params, x, train=True, act_dtype=None, round_input=True, tape=None):
    """UNet2D5.forward (unet2d5.py:199-211): a conv_dims = 2 level folds the depth axis into the batch (67-88, 122-142)"""
    dims, bilinear = list(params["conv_dims"]), bool(params["bilinear"])
    n = x.shape[0]
    h = quant(x, act_dtype) if round_input else x
    skips = []
    for i in range(5):
        key = "block%d.conv.conv_conv" % i
        if dims[i] == 2:
            h2 = conv_block(fold_depth(h), sd, key, train, act_dtype, False, tape)
            h = unfold_depth(h2, n)
            if i < 4:
                skips.append(h)
                h = unfold_depth(pool(tape, h2), n)
        else:
            h = conv_block(h, sd, key, train, act_dtype, False, tape)
            if i < 4:
                skips.append(h)
                h = pool(tape, h)
    for j in range(4):
        l = 3 - j
        key = "up%d" % (j + 1)
        two = dims[l] == 2
        hin = fold_depth(h) if two else h
        if bilinear:
            conv = F.conv2d if two else F.conv3d
            up = quant(conv(hin, quant(sd[key + ".up.0.weight"], act_dtype), sd[key + ".up.0.bias"]), act_dtype)
            up = quant(F.interpolate(up, scale_factor=2, mode="bilinear" if two else "trilinear", align_corners=True), act_dtype)
        else:
            tr = F.conv_transpose2d if two else F.conv_transpose3d
            up = quant(tr(hin, quant(sd[key + ".up.weight"], act_dtype), sd[key + ".up.bias"], stride=2), act_dtype)
        skip = tap(tape, "skip", skips[l])
        skip = fold_depth(skip) if two else skip
        h = conv_block(torch.cat([skip, tap(tape, "up", up)], dim=1), sd, key + ".conv.conv_conv", train, act_dtype, False, tape)
        if two:
            h = unfold_depth(h, n)
    return F.conv3d(h, sd["out_conv.weight"], sd["out_conv.bias"], padding=(0, 1, 1))


def forward(sd, params, x, train=True, act_dtype=None, round_input=True, tape=None):
    """tape: a decision tape (tests/kinkoracle.py) for the activations, poolings, skip, up-sampled and head-input tensors; None:
    the plain operators.
    round_input: the first convolution rounds the fp32 network input to bf16 - true of the MFMA stem kernels (bf16 operands),
    not of the generic kernel that serves a stem they do not take (it reads the input as stored, fp32)"""
    fn = unet3d_forward if params["net_type"] == "UNet3D" else unet2d5_forward
    return fn(sd, params, x, train, act_dtype, round_input, tape)


def deep_supervise_loss(preds, base, weights=None):
    """DeepSuperviseLoss.forward (loss/seg/deep_sup.py:24-41): sum_i w_i base(pred_i) / sum_i w_i"""
    if not isinstance(preds, (list, tuple)):
        raise ValueError("For deep supervision, the prediction should be a list or a tuple")
    weights = [1.0] * len(preds) if weights is None else weights
    assert len(weights) == len(preds)
    loss_sum, weight_sum = 0.0, 0.0
    for p, w in zip(preds, weights):
        loss_sum = loss_sum + base(p) * w
        weight_sum += w
    return loss_sum / weight_sum


def loss_of(out, y):
    """the fixtures' loss: DiceLoss, through DeepSuperviseLoss for a list"""
    if isinstance(out, (list, tuple)):
        return deep_supervise_loss(out, lambda p: dice_loss(p, y))
    return dice_loss(out, y)
