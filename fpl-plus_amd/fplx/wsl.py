"""Weakly-supervised trainers behind the reference's third entry point `pymic_wsl`: scribble- and partial-label training
(reference: PyMIC/pymic/net_run_wsl/wsl_abstract.py:6-44 WSLSegAgent, wsl_em.py, wsl_tv.py, wsl_mumford_shah.py, wsl_gatedcrf.py,
wsl_ustm.py:17-154, wsl_main.py; loss/seg/gatedcrf.py GatedCRFLoss, loss/seg/ssl.py:46-86 TotalVariationLoss,
loss/seg/mumford_shah.py MumfordShahLoss).

The regularisers run in the kernels of csrc/wsl.hip (include/fplx.h, "weakly-supervised learning"): `TotalVariationLoss`,
`MumfordShahLoss` and `GatedCRFLoss` are autograd nodes over them, so `loss = loss_sup + regular_w * loss_reg; loss.backward()`
reads as in the reference.  The supervised term is the configured loss on `label_prob`; the all-zero label rows that
`PartialLabelToProbability` gives unannotated voxels drop out of it by themselves.

Kept: the config keys ([weakly_supervised_learning] wsl_method, regularize_w, rampup_start, rampup_end, ema_decay,
gatedcrfloss_w0 / _xy0 / _rgb / _w1 / _xy1 / _radius, ustm_mcdroput_n (sic), MumfordShahLoss_penalty / MumfordShahLoss_lambda),
the sigmoid ramp on glob_it (constant within a validation round), optimiser and scheduler step before the EMA, the returned
scalars.
Different, on purpose: TotalVariationLoss() and MumfordShahLoss() can be constructed and called (the reference's
raise under a current torch); TotalVariationLoss takes 5-D input only; the CRF radius must be integral (the reference's default
5.0 fails in its own unfold) and masks, compatibility matrices, custom downsamplers and kernel visualisation are refused; the
CRF and Mumford-Shah kernels index [N, C, D, H, W] directly where the reference transposes and copies; an odd
ustm_mcdroput_n is refused (as uamt_mcdroput_n is, fplx/ssl.py); USTM's rot_times comes from an agent-owned
random.Random(random_seed), not the global generator; DSBN networks and torch.distributed groups are refused; DMPLS is refused
(it needs the dual-branch networks).
"""
import math
import random

import numpy as np
import torch
import torch.nn as nn
from torch.optim import lr_scheduler

from . import ops
from .agent import SegmentationAgent
from .nets3d import UNet2D5, UNet3D
from .ssl import EntropyLoss, consistency_loss, ema_update, get_rampup_ratio, _logits_of, _DSBN_NAMES


def _softmax_of(loss_input_dict, own):
    return bool(loss_input_dict.get('softmax', own))


# ---------------------------------------------------------------- TotalVariationLoss

class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, softmax):
        logits = logits.float().contiguous()
        out, count = ops.wsl_tv_fwd(logits, softmax)
        ctx.save_for_backward(logits, count)
        ctx.softmax = softmax
        return out[2].float()

    @staticmethod
    def backward(ctx, g):
        logits, count = ctx.saved_tensors
        return ops.wsl_tv_bwd(logits, count, g.float().contiguous().reshape(1), ctx.softmax), None


class TotalVariationLoss(nn.Module):
    """loss/seg/ssl.py:46-86: mean of relu(dilate(erode(p')) - erode(p')) over N C D H W with 3x3x3 windows, p' = 0.999 p + 5e-4.
    Called with the reference's loss_input_dict: `prediction` (element 0 of a list) [N, C, D, H, W], `softmax` (default True;
    `loss_softmax` of `params` where the dict does not say).  Equal window values take the first in (d, h, w) scan order, as
    torch's pooling does.  Not registered in SegLossDict / SegLossDictAll, as in the reference."""

    def __init__(self, params=None):
        super(TotalVariationLoss, self).__init__()
        self.softmax = True if params is None else params.get('loss_softmax', True)

    def forward(self, loss_input_dict):
        predict = _first(loss_input_dict['prediction'])
        if predict.dim() == 4:
            raise ValueError("fplx wsl: TotalVariationLoss takes [N, C, D, H, W]; the reference's `dim == 2` compares a list with "
                             "an int, so its 2-D branch is never taken and a 4-D tensor would be pooled across classes")
        if predict.dim() != 5:
            raise ValueError("fplx wsl: TotalVariationLoss takes [N, C, D, H, W], got {0:}D".format(predict.dim()))
        ops.require_gpu(predict)
        return _TotalVariation.apply(predict, _softmax_of(loss_input_dict, self.softmax))


# ---------------------------------------------------------------- MumfordShahLoss

class _MumfordShah(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, image, penalty, lam, softmax, holder):
        logits = logits.float().contiguous()
        image = image.detach().float().contiguous()
        out, cen = ops.wsl_mumford_shah_fwd(logits, image, penalty, lam, softmax)
        ctx.save_for_backward(logits, image, cen)
        ctx.penalty, ctx.lam, ctx.softmax = penalty, lam, softmax
        if holder is not None:
            holder["out"], holder["cen"] = out, cen
        return out[2].float()

    @staticmethod
    def backward(ctx, g):
        logits, image, cen = ctx.saved_tensors
        d = ops.wsl_mumford_shah_bwd(logits, image, cen, g.float().contiguous().reshape(1), ctx.penalty, ctx.lam, ctx.softmax)
        return d, None, None, None, None, None


def _as_5d(t, what):
    if t.dim() == 4:
        return t.unsqueeze(2)                      # [N, C, H, W]: every sample is one slice
    if t.dim() != 5:
        raise ValueError("fplx wsl: {0:} must be [N, C, H, W] or [N, C, D, H, W], got {1:}D".format(what, t.dim()))
    return t


class MumfordShahLoss(nn.Module):
    """loss/seg/mumford_shah.py:7-95: per slice, class and image channel the level-set term sum (I - centroid)^2 p plus
    lambda times the l1 (or l2) forward differences of p along H and W, over numel(p).  `params` gives `MumfordShahLoss_penalty`
    ('l1' default, or 'l2') and `MumfordShahLoss_lambda` (default 1.0) with that capitalisation; a parsed .cfg lower-cases its
    keys, so from a .cfg these two are always l1 and 1.0 in the reference, and they are here too.  `softmax`: the dict's, else
    `loss_softmax` of `params`, else True.  Input [N, C, H, W] or [N, C, D, H, W]; `image` of the same spatial shape."""

    def __init__(self, params=None):
        super(MumfordShahLoss, self).__init__()
        params = {} if params is None else params
        self.penalty = params.get('MumfordShahLoss_penalty', "l1")
        self.grad_w = params.get('MumfordShahLoss_lambda', 1.0)
        self.softmax = params.get('loss_softmax', True)
        if self.penalty not in ("l1", "l2"):
            raise ValueError("fplx wsl: MumfordShahLoss_penalty is 'l1' or 'l2', got {0:}".format(self.penalty))

    def forward(self, loss_input_dict, holder=None):
        predict = _as_5d(_logits_of(loss_input_dict['prediction'], "prediction"), "prediction")
        image = loss_input_dict['image']
        ops.require_gpu(image)
        image = _as_5d(image, "image")
        return _MumfordShah.apply(predict, image, 2 if self.penalty == "l2" else 1, float(self.grad_w),
                                  _softmax_of(loss_input_dict, self.softmax), holder)


# ---------------------------------------------------------------- GatedCRFLoss

class _GatedCRF(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, image, desc, radius, softmax, holder):
        logits = logits.float().contiguous()
        image = image.detach().float().contiguous()
        out, kp = ops.wsl_gatedcrf_fwd(logits, image, desc, radius, softmax)
        ctx.save_for_backward(logits, kp)
        ctx.softmax = softmax
        if holder is not None:
            holder["out"], holder["kp"] = out, kp
        return out[2].float()

    @staticmethod
    def backward(ctx, g):
        logits, kp = ctx.saved_tensors
        d = ops.wsl_gatedcrf_bwd(logits, kp, g.float().contiguous().reshape(1), ctx.softmax)
        return d, None, None, None, None, None


def crf_descriptors(kernels_desc):
    """the reference's [{'weight': w, 'xy': s, 'rgb': s}, ...] -> [(weight, sigma_xy, sigma_rgb)], 0 for an absent modality"""
    rows = []
    for i, desc in enumerate(kernels_desc):
        other = sorted(set(desc) - {"weight", "xy", "rgb"})
        if other:
            raise ValueError("fplx wsl: GatedCRFLoss kernel {0:} names the modalities {1:}; 'xy' and 'rgb' are built".format(i, other))
        if "weight" not in desc or not ("xy" in desc or "rgb" in desc):
            raise ValueError("fplx wsl: GatedCRFLoss kernel {0:} needs a weight and at least one of 'xy', 'rgb'".format(i))
        sxy, srgb = float(desc.get("xy", 0.0)), float(desc.get("rgb", 0.0))
        if ("xy" in desc and not sxy > 0) or ("rgb" in desc and not srgb > 0):
            raise ValueError("fplx wsl: GatedCRFLoss kernel {0:}: a sigma must be positive".format(i))
        rows.append((float(desc["weight"]), sxy, srgb))
    if not 1 <= len(rows) <= 4:
        raise ValueError("fplx wsl: GatedCRFLoss takes 1 to 4 kernel descriptors, got {0:}".format(len(rows)))
    return rows


def crf_radius(kernels_radius):
    r = int(kernels_radius)
    if r != kernels_radius:
        raise ValueError("fplx wsl: GatedCRFLoss radius {0:} is not integral".format(kernels_radius))
    if not 1 <= r <= 8:
        raise ValueError("fplx wsl: GatedCRFLoss radius {0:}; 1 to 8 is built".format(r))
    return r


class GatedCRFLoss(nn.Module):
    """loss/seg/gatedcrf.py:9-110 with the Potts shortcut: sum_i sum_{j != i in the window} k_ij (1 - p(i) . p(j)) / (N H W), k the
    weighted sum of the Gaussian kernels of `kernels_desc` over pixel position ('xy') and `sample['rgb']`; window positions
    outside the image count with the zero padding's features, as in the reference.  The signature is the reference's; `softmax`
    (keyword, default False) says that y_hat_softmax holds logits; y_hat_softmax and sample['rgb'] are [N, C, H, W] or, taken
    slice by slice without a copy, [N, C, D, H, W].  Returns {'loss': ...}."""

    def forward(self, y_hat_softmax, kernels_desc, kernels_radius, sample, height_input, width_input, mask_src=None, mask_dst=None,
                compatibility=None, custom_modality_downsamplers=None, out_kernels_vis=False, softmax=False, holder=None):
        if mask_src is not None or mask_dst is not None:
            raise ValueError("fplx wsl: GatedCRFLoss source / destination masks are not built (the weakly-supervised agent "
                             "passes none)")
        if compatibility is not None:
            raise ValueError("fplx wsl: GatedCRFLoss compatibility matrices are not built (Potts model only; the reference's "
                             "branch reads `compatibility.diag.sum()` and cannot run)")
        if custom_modality_downsamplers is not None:
            raise ValueError("fplx wsl: GatedCRFLoss custom_modality_downsamplers are not built (modalities at the prediction's "
                             "resolution only)")
        if out_kernels_vis:
            raise ValueError("fplx wsl: GatedCRFLoss out_kernels_vis is not built (no kernel tensor is ever materialised)")
        desc = crf_descriptors(kernels_desc)
        radius = crf_radius(kernels_radius)
        pred = _as_5d(_first(y_hat_softmax), "y_hat_softmax")
        if (int(height_input), int(width_input)) != (pred.shape[-2], pred.shape[-1]):
            raise ValueError("fplx wsl: GatedCRFLoss at a prediction resolution {0:}x{1:} different from the input's {2:}x{3:} is "
                             "not built".format(pred.shape[-2], pred.shape[-1], height_input, width_input))
        ops.require_gpu(pred)
        if any(row[2] > 0 for row in desc):
            if "rgb" not in sample:
                raise ValueError("fplx wsl: modality rgb is listed in a kernel descriptor, but not present in the sample")
            image = sample["rgb"]
            ops.require_gpu(image)
            image = _as_5d(image, "sample['rgb']")
        else:
            image = pred.new_zeros((pred.shape[0], 1) + tuple(pred.shape[2:]))
        return {'loss': _GatedCRF.apply(pred, image, desc, radius, bool(softmax), holder)}


# ---------------------------------------------------------------- agents

_REFUSED_METHODS = ("DMPLS",)


class WSLSegAgent(SegmentationAgent):
    """wsl_abstract.py:6-44.  One training loop with three hooks: `_student_input`, `_regulariser`, `_after_step`."""
    uses_teacher = False
    uses_mc = False

    def __init__(self, config, stage='train'):
        wsl_cfg = config.get('weakly_supervised_learning', {})
        net_type = config.get('network', {}).get('net_type', None)
        if net_type in _DSBN_NAMES:
            raise ValueError("fplx wsl: {0:} is a domain-specific-BatchNorm network; the weakly-supervised agents derive from "
                             "net_run/agent_seg.py and run UNet2D5 / UNet3D only".format(net_type))
        t = wsl_cfg.get('ustm_mcdroput_n', 8)
        if self.uses_mc and (int(t) % 2 or not 2 <= int(t) <= 16):
            raise ValueError("fplx wsl: ustm_mcdroput_n = {0:}; an even number from 2 to 16 is supported (the reference fills "
                             "2 (T // 2) of its T slots and averages the empty one in as a uniform prediction)".format(t))
        config['network'].setdefault('num_domains', 1)
        super(WSLSegAgent, self).__init__(config, stage)
        if self.distributed:
            raise ValueError("fplx wsl: the weakly-supervised agents run in a single process (no torch.distributed group): the "
                             "gradients of UNet2D5 / UNet3D are not all-reduced")
        self.net_ema = None
        self.noise_source = None          # tests: callable(reps, shape) -> fp32 noise [reps, *shape] on the device
        self.rot_source = None            # tests: callable() -> rot_times in 0..3
        self._rot_rng = random.Random(self.random_seed)
        self._wsl_iter = 0

    def create_dataset(self):
        ds = self.config['dataset']
        for ours, theirs in (('1_train_csv', 'train_csv'), ('1_valid_csv', 'valid_csv')):
            if ds.get(ours, None) is None and ds.get(theirs, None) is not None:
                ds[ours] = ds[theirs]
        super(WSLSegAgent, self).create_dataset()

    def create_network(self):
        super(WSLSegAgent, self).create_network()
        if not isinstance(self.net, (UNet2D5, UNet3D)):
            raise ValueError("fplx wsl: the weakly-supervised agents run UNet2D5 / UNet3D, got {0:}".format(type(self.net).__name__))
        if self.uses_teacher and self.net_ema is None:                       # wsl_ustm.py:39-49, built as SSLMeanTeacher's
            net_name = self.config['network']['net_type']
            if net_name not in self.net_dict:
                raise ValueError("Undefined network {0:}".format(net_name))
            cfg = dict(self.config['network'])
            cfg['dropout_seed'] = int(cfg.get('dropout_seed', 1)) + 1
            self.net_ema = self.net_dict[net_name](cfg)
        if self.net_ema is not None:
            self.net_ema.float()
            self.net_ema.to(self.device)

    def create_loss_calculator(self, entropy_weight=0.0):
        """net_run/agent_seg.py: no entropy term (SSLSegAgent.create_loss_calculator says why); the argument is ignored"""
        super(WSLSegAgent, self).create_loss_calculator(0.0)

    def _ramp(self):
        wsl_cfg = self.config['weakly_supervised_learning']
        iter_max = self.config['training']['iter_max']
        return get_rampup_ratio(getattr(self, 'glob_it', 0), wsl_cfg.get('rampup_start', 0), wsl_cfg.get('rampup_end', iter_max),
                                "sigmoid")

    # ---- hooks
    def _student_input(self, x):
        return x

    def _regulariser(self, inputs, outputs, y, ramp):
        raise NotImplementedError

    def _after_step(self):
        pass

    def _train_loop(self, dual):
        class_num = self.config['network']['class_num']
        iter_valid = self.config['training']['iter_valid']
        wsl_cfg = self.config['weakly_supervised_learning']
        it = iter(self.train_loader_1)
        self.net.train()
        sums = None
        dice = []
        regular_w = 0.0
        for _ in range(iter_valid):
            data, it = self._next(it, self.train_loader_1)
            inputs = self.convert_tensor_type(data['image']).to(self.device).contiguous()
            y = self.convert_tensor_type(data['label_prob']).to(self.device)
            self.optimizer.zero_grad()
            outputs = self.net(self._student_input(inputs))
            loss_sup = self.get_loss_value(data, outputs, y)
            dice.append(self.loss_calculator.last_out[4:4 + class_num])
            ramp = self._ramp()
            regular_w = wsl_cfg.get('regularize_w', 0.1) * ramp
            loss_reg = self._regulariser(inputs, outputs, y, ramp)
            loss = loss_sup + regular_w * loss_reg
            loss.backward()
            self.optimizer.step()
            if self.scheduler is not None and not isinstance(self.scheduler, lr_scheduler.ReduceLROnPlateau):
                self.scheduler.step()
            self._after_step()
            row = torch.stack([loss.detach(), loss_sup.detach(), loss_reg.detach()])
            sums = row if sums is None else sums + row
        vals = (sums / iter_valid).cpu().numpy().astype(np.float64)          # the round's one host read
        cls = torch.stack(dice).mean(0).cpu().numpy().astype(np.float64)
        return {'loss': float(vals[0]), 'loss_sup': float(vals[1]), 'loss_reg': float(vals[2]), 'regular_w': regular_w,
                'avg_dice': float(cls.mean()), 'class_dice': cls}


def _first(outputs):
    return outputs[0] if isinstance(outputs, (list, tuple)) else outputs


class WSLEntropyMinimization(WSLSegAgent):
    """wsl_em.py: EntropyLoss over the prediction (line 66-67)"""

    def _regulariser(self, inputs, outputs, y, ramp):
        return EntropyLoss()({"prediction": outputs, 'softmax': True})


class WSLTotalVariation(WSLSegAgent):
    """wsl_tv.py: TotalVariationLoss over the prediction (line 62-63)"""

    def _regulariser(self, inputs, outputs, y, ramp):
        return TotalVariationLoss()({"prediction": outputs, 'softmax': True})


class WSLMumfordShah(WSLSegAgent):
    """wsl_mumford_shah.py: MumfordShahLoss(wsl_cfg) over the prediction and the input image (line 46, 67-68)"""

    def _regulariser(self, inputs, outputs, y, ramp):
        return MumfordShahLoss(self.config['weakly_supervised_learning'])({"prediction": outputs, 'image': inputs})


class WSLGatedCRF(WSLSegAgent):
    """wsl_gatedcrf.py:14-125: two kernels, {w0, xy0, rgb} and {w1, xy1}, over the slices of the batch; the logits go to the kernel
    as they are (softmax inside, no transposed copies)"""

    def __init__(self, config, stage='train'):
        super(WSLGatedCRF, self).__init__(config, stage)
        wsl_cfg = self.config['weakly_supervised_learning']
        w0 = wsl_cfg.get('gatedcrfloss_w0', 1.0)
        xy0 = wsl_cfg.get('gatedcrfloss_xy0', 5)
        rgb = wsl_cfg.get('gatedcrfloss_rgb', 0.1)
        w1 = wsl_cfg.get('gatedcrfloss_w1', 1.0)
        xy1 = wsl_cfg.get('gatedcrfloss_xy1', 3)
        self.kernels = [{'weight': w0, 'xy': xy0, 'rgb': rgb}, {'weight': w1, 'xy': xy1}]
        self.radius = crf_radius(wsl_cfg.get('gatedcrfloss_radius', 5))

    def _regulariser(self, inputs, outputs, y, ramp):
        out = _first(outputs)
        return GatedCRFLoss()(out, self.kernels, self.radius, {'rgb': inputs}, out.shape[-2], out.shape[-1], softmax=True)["loss"]


class WSLUSTM(WSLSegAgent):
    """wsl_ustm.py:17-154: a noisy student, a teacher on the rotated and noisy input, the Monte-Carlo entropy mask of UAMT on the
    rotated input, the EMA after the step.  torch.rot90 of the inputs and of the student's logits is plumbing (softmax is per
    voxel, so it commutes with the rotation); the consistency term is fplx.ssl's kernel."""
    uses_teacher = True
    uses_mc = True

    def _perturb(self, x, reps):
        self._wsl_iter += 1
        noise = None if self.noise_source is None else self.noise_source(reps, tuple(x.shape))
        return ops.ssl_perturb(x, noise, reps, 0.1, 0.2, self.random_seed, self._wsl_iter)

    def _teacher(self, x):
        with torch.no_grad():
            return _first(self.net_ema(x))

    def _student_input(self, x):
        return self._perturb(x, 1)[0]                                        # wsl_ustm.py:81-82

    def _regulariser(self, inputs, outputs, y, ramp):
        rot_times = self._rot_rng.randrange(0, 4) if self.rot_source is None else int(self.rot_source())
        inputs_rot = torch.rot90(inputs, rot_times, [-2, -1]).contiguous()
        teacher = self._teacher(self._perturb(inputs_rot, 1)[0])             # wsl_ustm.py:88-92
        student_rot = torch.rot90(_first(outputs), rot_times, [-2, -1])
        T = int(self.config['weakly_supervised_learning'].get("ustm_mcdroput_n", 8))
        mc = torch.empty((T,) + tuple(teacher.shape), dtype=torch.float32, device=teacher.device)
        b = inputs_rot.shape[0]
        for i in range(T // 2):                                              # wsl_ustm.py:99-107
            pair = self._perturb(inputs_rot, 2).reshape((2 * b,) + tuple(inputs_rot.shape[1:]))
            mc[2 * i:2 * i + 2] = self._teacher(pair).reshape((2,) + tuple(teacher.shape))
        threshold = (0.75 + 0.25 * ramp) * math.log(teacher.shape[1])        # wsl_ustm.py:115
        return consistency_loss(student_rot, teacher, mc, threshold)

    def _after_step(self):
        wsl_cfg = self.config['weakly_supervised_learning']
        iter_max = self.config['training']['iter_max']
        alpha = min(1 - 1 / (iter_max + 1), wsl_cfg.get('ema_decay', 0.99))  # wsl_ustm.py:129-130
        ema_update(self.net_ema, self.net, alpha)


WSLMethodDict = {'EntropyMinimization': WSLEntropyMinimization,
                 'GatedCRF': WSLGatedCRF,
                 'MumfordShah': WSLMumfordShah,
                 'TotalVariation': WSLTotalVariation,
                 'USTM': WSLUSTM}


def wsl_agent_class(name):
    """wsl_main.py: the agent class of [weakly_supervised_learning] wsl_method"""
    if name in _REFUSED_METHODS:
        raise ValueError("fplx wsl: {0:} is not built: it needs UNet2D_DualBranch / UNet3D_DualBranch, which the registry does "
                         "not hold (SegNetDict has UNet2D5, UNet3D and the DSBN networks)".format(name))
    if name not in WSLMethodDict:
        raise ValueError("Undefined weakly-supervised method {0:}".format(name))
    return WSLMethodDict[name]
