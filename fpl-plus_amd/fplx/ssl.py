"""Semi-supervised trainers behind the reference's second entry point `pymic_ssl`
(reference: PyMIC/pymic/net_run_ssl/ssl_abstract.py:16-107 SSLSegAgent, ssl_em.py:15-110 SSLEntropyMinimization,
ssl_mt.py:14-135 SSLMeanTeacher, ssl_uamt.py:13-138 SSLUncertaintyAwareMeanTeacher, ssl_main.py:16-44; util/ramps.py:13-33
get_rampup_ratio; loss/seg/ssl.py:10-44 EntropyLoss).

What an iteration adds to supervised training - the softmax pairs and the squared-difference reduction, UAMT's Monte-Carlo
entropy mask, the clamped-noise perturbation of the teacher input, the EMA of every parameter - runs in the kernels of
csrc/ssl.hip (include/fplx.h, "semi-supervised learning"), one pass each; `consistency_loss` and `EntropyLoss` are autograd
nodes over them, so `loss = loss_sup + regular_w * loss_reg; loss.backward()` reads as in the reference.

Kept: the config keys ([semi_supervised_learning] ssl_method, regularize_w, rampup_start, rampup_end, ema_decay,
uamt_mcdroput_n (sic); [dataset] train_csv_unlab, train_transform_unlab, train_batch_size_unlab), ONE forward over
cat([x0, x1]), the supervised loss on the labelled rows, the sigmoid ramp on glob_it (constant within a validation round),
optimiser and scheduler step before the EMA, alpha = min(1 - 1 / (iter_max + 1), ema_decay), the returned scalars, a teacher
that stays in train mode, takes no gradient and is not saved.
Different, on purpose: an odd uamt_mcdroput_n is refused (the reference averages an all-zero slot in);
EntropyLoss() can be constructed (the reference's cannot under a current torch) and applies softmax as ssl_em.py:76 asks;
DSBN networks and torch.distributed groups are refused.  The teacher's dropout stream is seeded with the student's
dropout_seed + 1.

CPS and URPC (ssl_cps.py:31-176, ssl_urpc.py:14-122) are registered in SSLMethodDictAll / ssl_agent_class_all;
SSLMethodDict and ssl_agent_class keep the first three methods.  URPC runs on UNet3D / UNet2D5 with [network] deep_supervise =
True (the reference's UNet2D_URPC is not in its tree): its regulariser over the K output scales is `pyramid_consistency_loss`,
ONE autograd node on fplx_ssl_pyramid_fwd / _bwd.  CPS runs a BiNet under a GroupOptimizer (fplx/netgroup.py); its pseudo
labels come from fplx_ssl_pseudo_onehot, the argmax of the LOGITS (two distinct logits that fp32 softmax rounds to one
probability keep their order here; the reference takes the first of the pair).  CCT stays refused: its auxiliary-decoder
network (pymic.net.net2d) is in neither tree.
"""
import logging
import math

import numpy as np
import torch
import torch.nn as nn
from torch.optim import lr_scheduler

from . import ops
from .agent import SegmentationAgent
from .dataset import NiftyDataset, BatchLoader
from .netgroup import BiNet, GroupOptimizer, _DSBN_NAMES
from .nets3d import UNet2D5, UNet3D
from .optim import get_optimizer
from .transform import Compose


def get_rampup_ratio(i, start, end, mode="linear"):
    """util/ramps.py:13-33"""
    i = np.clip(i, start, end)
    if mode == "linear":
        rampup = (i - start) / (end - start)
    elif mode == "sigmoid":
        phase = 1.0 - (i - start) / (end - start)
        rampup = float(np.exp(-5.0 * phase * phase))
    elif mode == "cosine":
        phase = 1.0 - (i - start) / (end - start)
        rampup = float(.5 * (np.cos(np.pi * phase) + 1))
    else:
        raise ValueError("Undefined rampup mode {0:}".format(mode))
    return rampup


def _logits_of(t, what):
    if isinstance(t, (list, tuple)):
        t = t[0]
    ops.require_gpu(t)
    if t.dim() < 3:
        raise ValueError("fplx ssl: {0:} must be [N, C, ...], got {1:}D".format(what, t.dim()))
    return t


class _Consistency(torch.autograd.Function):
    """fplx_ssl_consistency_fwd / _bwd as one autograd node; the teacher and the Monte-Carlo stack receive no gradient"""

    @staticmethod
    def forward(ctx, student, teacher, mc, thr, softmax, holder):
        student = student.float().contiguous()
        teacher = teacher.detach().float().contiguous()
        mc = None if mc is None else mc.detach().float().contiguous()
        out, mask = ops.ssl_consistency_fwd(student, teacher, mc, thr, softmax)
        ctx.save_for_backward(student, teacher, mask, out)
        ctx.t, ctx.softmax = (0 if mc is None else int(mc.shape[0])), softmax
        if holder is not None:
            holder["out"], holder["mask"] = out, mask
        return out[2].float()

    @staticmethod
    def backward(ctx, g):
        student, teacher, mask, out = ctx.saved_tensors
        d = ops.ssl_consistency_bwd(student, teacher, mask, out, g.float().contiguous().reshape(1), ctx.t, ctx.softmax)
        return d, None, None, None, None, None


def consistency_loss(student_logits, teacher_logits, mc_logits=None, threshold=None, softmax=True, holder=None):
    """MeanTeacher's regulariser torch.nn.MSELoss()(softmax(student), softmax(teacher)) (ssl_mt.py:90-100) or, with mc_logits
    [T, N, C, ...] (T even, at most 16) and a threshold, UAMT's masked one (ssl_uamt.py:77-100): the squared error summed over
    the voxels whose Monte-Carlo predictive entropy is below the threshold, over 2 x their number.  holder: an optional dict that
    receives the kernel's `out` (double [4]) and `mask`."""
    if (mc_logits is None) != (threshold is None):
        raise ValueError("fplx ssl: mc_logits and threshold go together")
    if mc_logits is not None and (mc_logits.shape[0] % 2 or mc_logits.shape[0] > 16 or mc_logits.shape[0] < 2):
        raise ValueError("fplx ssl: {0:} Monte-Carlo passes; an even number up to 16 is supported".format(mc_logits.shape[0]))
    s = _logits_of(student_logits, "student_logits")
    t = _logits_of(teacher_logits, "teacher_logits")
    return _Consistency.apply(s, t, mc_logits, 0.0 if threshold is None else float(threshold), bool(softmax), holder)


class _Entropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, softmax):
        logits = logits.float().contiguous()
        out = ops.ssl_entropy_fwd(logits, softmax)
        ctx.save_for_backward(logits)
        ctx.softmax = softmax
        return out[2].float()

    @staticmethod
    def backward(ctx, g):
        logits, = ctx.saved_tensors
        return ops.ssl_entropy_bwd(logits, g.float().contiguous().reshape(1), ctx.softmax), None


class EntropyLoss(nn.Module):
    """loss/seg/ssl.py:10-44: mean over the voxels of -sum_c p' ln p' / ln C, p' = 0.999 p + 5e-4.  Called with the reference's
    loss_input_dict: `prediction` (element 0 of a list), `softmax` (default True; `loss_softmax` of `params` where the dict
    does not say).  Not registered in SegLossDict / SegLossDictAll, as in the reference."""

    def __init__(self, params=None):
        super(EntropyLoss, self).__init__()
        self.softmax = True if params is None else params.get('loss_softmax', True)

    def forward(self, loss_input_dict):
        predict = _logits_of(loss_input_dict['prediction'], "prediction")
        return _Entropy.apply(predict, bool(loss_input_dict.get('softmax', self.softmax)))


def ema_update(net_ema, net, alpha):
    """ssl_mt.py:112-113 for all parameters in one launch: net_ema = alpha net_ema + (1 - alpha) net over the two flat
    parameter buffers.  Buffers (running statistics) are not averaged, as in the reference."""
    for m in (net_ema, net):
        if not callable(getattr(m, "_ensure_flat", None)):
            raise ValueError("fplx ssl: ema_update needs fplx networks with a flat parameter buffer, got {0:}".format(
                type(m).__name__))
        m._ensure_flat()
    if net_ema._layout != net._layout or net_ema.flat_params.numel() != net.flat_params.numel():
        raise ValueError("fplx ssl: teacher and student differ in their parameter layout")
    with torch.no_grad():
        ops.ema_step(net_ema.flat_params, net.flat_params, alpha)
    net_ema.parameters_changed()                   # the teacher's packs are rebuilt from the new values


class _Pyramid(torch.autograd.Function):
    """fplx_ssl_pyramid_fwd / _bwd as one autograd node over the K joint-batch tensors; rows < n0 receive zeros"""

    @staticmethod
    def forward(ctx, n0, holder, *outputs):
        full = [t.float().contiguous() for t in outputs]
        out = ops.ssl_pyramid_fwd([t[n0:] for t in full])           # N is outermost: the unlabelled rows are contiguous views
        ctx.save_for_backward(out, *full)
        ctx.n0 = n0
        if holder is not None:
            holder["out"] = out
        return out[4 * len(full)].float()

    @staticmethod
    def backward(ctx, g):
        out, full = ctx.saved_tensors[0], list(ctx.saved_tensors[1:])
        grads = [torch.empty_like(t) for t in full]
        for d in grads:
            d[:ctx.n0].zero_()
        ops.ssl_pyramid_bwd([t[ctx.n0:] for t in full], out, g.float().contiguous().reshape(1), [d[ctx.n0:] for d in grads])
        return (None, None) + tuple(grads)


def pyramid_consistency_loss(outputs_list, n0, holder=None):
    """URPC's regulariser (ssl_urpc.py:76-91) over the K = 2..4 full-resolution outputs [N, C, ...] of the joint batch: the
    softmax of every scale, their mean, and per scale the KL-rectified squared error mean(sq * exp(-var)) / (mean(exp(-var)) +
    1e-8) + mean(var) over the rows n0:, averaged over the scales.  The mean carries gradient, as in the reference.  holder: an
    optional dict that receives the kernel's `out` (double [4 K + 2]: A_k, B_k, V_k, L_k per scale, loss_reg, 0).  Nothing is
    read back to the host."""
    if not isinstance(outputs_list, (list, tuple)):
        raise ValueError("fplx ssl: pyramid_consistency_loss takes the LIST of a deep-supervised network's outputs "
                         "([network] deep_supervise = True), got {0:}".format(type(outputs_list).__name__))
    ts = list(outputs_list)
    if not 2 <= len(ts) <= 4:
        raise ValueError("fplx ssl: pyramid_consistency_loss takes 2 to 4 output scales, got {0:}".format(len(ts)))
    for t in ts:
        ops.require_gpu(t)
        if t.dim() < 3:
            raise ValueError("fplx ssl: every output must be [N, C, ...], got {0:}D".format(t.dim()))
        if t.shape != ts[0].shape:
            raise ValueError("fplx ssl: the output scales differ in shape ({0:} and {1:}); URPC compares full-resolution "
                             "outputs".format(tuple(ts[0].shape), tuple(t.shape)))
    n0 = int(n0)
    if not 0 <= n0 < ts[0].shape[0]:
        raise ValueError("fplx ssl: n0 = {0:} leaves no unlabelled row in a batch of {1:}".format(n0, ts[0].shape[0]))
    return _Pyramid.apply(n0, holder, *ts)


def cross_pseudo_labels(logits_list):
    """CPS's pseudo labels (ssl_cps.py:103-106) for 1 to 3 logit tensors [N, C, ...] in one launch: detached fp32 one-hot tensors
    of the first maximum of the logits over C"""
    ts = [t.detach().float().contiguous() for t in logits_list]
    with torch.no_grad():
        return ops.ssl_pseudo_onehot(ts)


_REFUSED_METHODS = ("CCT", "CPS", "URPC")


class SSLSegAgent(SegmentationAgent):
    """ssl_abstract.py:16-107.  Subclasses give `_regulariser`; MeanTeacher and UAMT also keep `net_ema`."""
    uses_teacher = False
    uses_mc = False

    def __init__(self, config, stage='train'):
        ssl_cfg = config.get('semi_supervised_learning', {})
        net_type = config.get('network', {}).get('net_type', None)
        if net_type in _DSBN_NAMES:
            raise ValueError("fplx ssl: {0:} is a domain-specific-BatchNorm network; the semi-supervised agents derive from "
                             "net_run/agent_seg.py and run UNet2D5 / UNet3D only".format(net_type))
        t = ssl_cfg.get('uamt_mcdroput_n', 8)
        if self.uses_mc and (int(t) % 2 or not 2 <= int(t) <= 16):
            raise ValueError("fplx ssl: uamt_mcdroput_n = {0:}; an even number from 2 to 16 is supported (the reference fills "
                             "2 (T // 2) of its T slots and averages the empty one in as a uniform prediction)".format(t))
        config['network'].setdefault('num_domains', 1)
        super(SSLSegAgent, self).__init__(config, stage)
        if self.distributed:
            raise ValueError("fplx ssl: the semi-supervised agents run in a single process (no torch.distributed group): the "
                             "gradients of UNet2D5 / UNet3D are not all-reduced")
        self.train_set_unlab = None
        self.train_loader_unlab = None
        self.net_ema = None
        self.noise_source = None          # tests: callable(reps, shape) -> fp32 noise [reps, *shape] on the device
        self._ssl_iter = 0

    def set_unlabeled_loader(self, loader):
        """any iterable of batch dicts with 'image', as set_loaders"""
        self.train_loader_unlab = loader

    # ---- datasets (ssl_abstract.py:34-79)
    def get_unlabeled_dataset_from_config(self):
        ds = self.config['dataset']
        transform_names = ds['train_transform_unlab']
        self.transform_list = []
        data_transform = None
        if transform_names is not None and len(transform_names) > 0:
            transform_param = ds
            transform_param['task'] = 'segmentation'
            for name in transform_names:
                if name not in self.transform_dict:
                    raise ValueError("Undefined transform {0:}".format(name))
                self.transform_list.append(self.transform_dict[name](transform_param))
            data_transform = Compose(self.transform_list)
        return NiftyDataset(root_dir=ds['root_dir'], csv_file=ds.get('train_csv_unlab', None), modal_num=ds.get('modal_num', 1),
                            with_label=False, transform=data_transform, device=self.device, cache=ds.get('cache_on_device', True))

    def create_dataset(self):
        ds = self.config['dataset']
        for ours, theirs in (('1_train_csv', 'train_csv'), ('1_valid_csv', 'valid_csv')):
            if ds.get(ours, None) is None and ds.get(theirs, None) is not None:
                ds[ours] = ds[theirs]
        super(SSLSegAgent, self).create_dataset()
        if self.stage == 'train':
            if self.train_set_unlab is None:
                self.train_set_unlab = self.get_unlabeled_dataset_from_config()
            g = torch.Generator()
            g.manual_seed(self.random_seed + 1)
            self.train_loader_unlab = BatchLoader(self.train_set_unlab, ds['train_batch_size_unlab'], True, g)

    # ---- construction
    def create_network(self):
        super(SSLSegAgent, self).create_network()
        if not isinstance(self.net, (UNet2D5, UNet3D)):
            raise ValueError("fplx ssl: the semi-supervised agents run UNet2D5 / UNet3D, got {0:}".format(type(self.net).__name__))
        if self.uses_teacher and self.net_ema is None:                       # ssl_mt.py:35-45
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
        """net_run/agent_seg.py: no entropy term - that one belongs to the DSBN agent (net_run_dsbn/agent_seg.py:352-354) and
        SegmentationAgent.train_valid asks for it when `dual` is false; the argument is ignored"""
        super(SSLSegAgent, self).create_loss_calculator(0.0)

    # ---- the iteration
    def _ramp(self):
        ssl_cfg = self.config['semi_supervised_learning']
        iter_max = self.config['training']['iter_max']
        return get_rampup_ratio(getattr(self, 'glob_it', 0), ssl_cfg.get('rampup_start', 0), ssl_cfg.get('rampup_end', iter_max),
                                "sigmoid")

    def _noise(self, reps, shape):
        return None if self.noise_source is None else self.noise_source(reps, shape)

    def _perturb(self, x1, reps):
        """[reps, *x1.shape]: x1 + clamp(0.1 z, -0.2, 0.2) per repetition; z from noise_source or the device generator keyed by
        (random_seed, iteration)"""
        self._ssl_iter += 1
        return ops.ssl_perturb(x1, self._noise(reps, tuple(x1.shape)), reps, 0.1, 0.2, self.random_seed, self._ssl_iter)

    def _regulariser(self, outputs, n0, x1, ramp):
        raise NotImplementedError

    def _after_step(self):
        pass

    def _train_loop(self, dual):
        class_num = self.config['network']['class_num']
        iter_valid = self.config['training']['iter_valid']
        ssl_cfg = self.config['semi_supervised_learning']
        if self.train_loader_unlab is None:
            raise ValueError("fplx ssl: no unlabelled loader (create_dataset or set_unlabeled_loader)")
        if getattr(self, '_unlab_iter', None) is None:
            self._unlab_iter = iter(self.train_loader_unlab)
        lab_iter = iter(self.train_loader_1)
        self.net.train()
        sums = None
        dice = []
        regular_w = 0.0
        for _ in range(iter_valid):
            data_lab, lab_iter = self._next(lab_iter, self.train_loader_1)
            data_unlab, self._unlab_iter = self._next(self._unlab_iter, self.train_loader_unlab)
            x0 = self.convert_tensor_type(data_lab['image']).to(self.device)
            y0 = self.convert_tensor_type(data_lab['label_prob']).to(self.device)
            x1 = self.convert_tensor_type(data_unlab['image']).to(self.device).contiguous()
            n0 = x0.shape[0]
            self.optimizer.zero_grad()
            outputs = self.net(torch.cat([x0, x1], dim=0))                   # ONE forward over both batches
            p0 = [o[:n0] for o in outputs] if isinstance(outputs, (list, tuple)) else outputs[:n0]
            loss_sup = self.get_loss_value(data_lab, p0, y0)
            dice.append(self.loss_calculator.last_out[4:4 + class_num])     # hard Dice of the labelled rows
            ramp = self._ramp()
            regular_w = ssl_cfg.get('regularize_w', 0.1) * ramp
            loss_reg = self._regulariser(outputs, n0, x1, ramp)
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

    def train_valid(self):
        if self.train_loader_unlab is None:
            raise ValueError("fplx ssl: no unlabelled loader (create_dataset or set_unlabeled_loader)")
        self._unlab_iter = iter(self.train_loader_unlab)                     # ssl_abstract.py:105-107
        return super(SSLSegAgent, self).train_valid()


class SSLEntropyMinimization(SSLSegAgent):
    """ssl_em.py:15-110: EntropyLoss over ALL rows of the joint forward (line 76)"""

    def _regulariser(self, outputs, n0, x1, ramp):
        return EntropyLoss()({"prediction": outputs, 'softmax': True})


class SSLMeanTeacher(SSLSegAgent):
    """ssl_mt.py:14-135"""
    uses_teacher = True

    def _teacher(self, x):
        with torch.no_grad():
            out = self.net_ema(x)
        return out[0] if isinstance(out, (list, tuple)) else out

    def _student_unlab(self, outputs, n0):
        out = outputs[0] if isinstance(outputs, (list, tuple)) else outputs
        return out[n0:]

    def _regulariser(self, outputs, n0, x1, ramp):
        inputs_ema = self._perturb(x1, 1)[0]                                 # ssl_mt.py:79
        return consistency_loss(self._student_unlab(outputs, n0), self._teacher(inputs_ema))

    def _after_step(self):
        ssl_cfg = self.config['semi_supervised_learning']
        iter_max = self.config['training']['iter_max']
        alpha = min(1 - 1 / (iter_max + 1), ssl_cfg.get('ema_decay', 0.99))  # ssl_mt.py:110-111
        ema_update(self.net_ema, self.net, alpha)


class SSLUncertaintyAwareMeanTeacher(SSLMeanTeacher):
    """ssl_uamt.py:13-138"""
    uses_mc = True

    def _regulariser(self, outputs, n0, x1, ramp):
        p1 = self._student_unlab(outputs, n0)
        teacher = self._teacher(self._perturb(x1, 1)[0])                     # ssl_uamt.py:61,75
        T = int(self.config['semi_supervised_learning'].get("uamt_mcdroput_n", 8))
        mc = torch.empty((T,) + tuple(p1.shape), dtype=torch.float32, device=p1.device)
        b = x1.shape[0]
        for i in range(T // 2):                                              # ssl_uamt.py:82-90: two noisy copies per pass
            pair = self._perturb(x1, 2).reshape((2 * b,) + tuple(x1.shape[1:]))
            mc[2 * i:2 * i + 2] = self._teacher(pair).reshape((2,) + tuple(p1.shape))
        class_num = p1.shape[1]
        threshold = (0.75 + 0.25 * ramp) * math.log(class_num)              # ssl_uamt.py:98
        return consistency_loss(p1, teacher, mc, threshold)


class SSLURPC(SSLSegAgent):
    """ssl_urpc.py:14-122 on a deep-supervised UNet3D / UNet2D5 (four full-resolution outputs); the returned scalars are
    _train_loop's: loss, loss_sup, loss_reg, regular_w, avg_dice, class_dice"""

    def __init__(self, config, stage='train'):
        if not config.get('network', {}).get('deep_supervise', False):
            raise ValueError("fplx ssl: URPC compares the output scales of one network and needs a list of outputs: set "
                             "[network] deep_supervise = True (UNet3D / UNet2D5 then return four full-resolution outputs)")
        super(SSLURPC, self).__init__(config, stage)

    def _regulariser(self, outputs, n0, x1, ramp):
        return pyramid_consistency_loss(outputs, n0)


class SSLCPS(SSLSegAgent):
    """ssl_cps.py:31-176: two networks of [network] net_type in a BiNet, each supervised on the labelled rows and on the OTHER
    one's pseudo labels of the unlabelled rows"""

    def __init__(self, config, stage='train'):
        if config.get('network', {}).get('deep_supervise', False):
            raise ValueError("fplx ssl: CPS takes one output per network; with [network] deep_supervise = True the reference's "
                             "torch.softmax(outputs1, dim=1) (ssl_cps.py:94) fails on a list - set deep_supervise = False")
        super(SSLCPS, self).__init__(config, stage)
        self.summ_writer = None           # tests / callers: an object with add_scalars(tag, dict, step), as the reference's

    def create_network(self):
        if self.net is None:
            self.net = BiNet(self.config['network'], self.net_dict)
        if self.tensor_type != 'float':
            raise ValueError("fplx: tensor_type must be float (fp32 parameters)")
        self.net.float()
        self.net.to(self.device)

    def create_optimizer(self, params=None):
        opt_params = self.config['training']
        if self.optimizer is None:
            self.optimizer = GroupOptimizer([get_optimizer(opt_params['optimizer'], m, opt_params) for m in self.net.members()])
        super(SSLCPS, self).create_optimizer(params)

    def _train_loop(self, dual):
        class_num = self.config['network']['class_num']
        iter_valid = self.config['training']['iter_valid']
        ssl_cfg = self.config['semi_supervised_learning']
        if self.train_loader_unlab is None:
            raise ValueError("fplx ssl: no unlabelled loader (create_dataset or set_unlabeled_loader)")
        if getattr(self, '_unlab_iter', None) is None:
            self._unlab_iter = iter(self.train_loader_unlab)
        lab_iter = iter(self.train_loader_1)
        self.net.train()
        sums = None
        dice = []
        regular_w = 0.0
        for _ in range(iter_valid):
            data_lab, lab_iter = self._next(lab_iter, self.train_loader_1)
            data_unlab, self._unlab_iter = self._next(self._unlab_iter, self.train_loader_unlab)
            x0 = self.convert_tensor_type(data_lab['image']).to(self.device)
            y0 = self.convert_tensor_type(data_lab['label_prob']).to(self.device)
            x1 = self.convert_tensor_type(data_unlab['image']).to(self.device).contiguous()
            n0 = x0.shape[0]
            self.optimizer.zero_grad()
            outputs1, outputs2 = self.net(torch.cat([x0, x1], dim=0))        # ONE forward over both batches, per network
            loss_sup1 = self.get_loss_value(data_lab, outputs1[:n0], y0)
            dice.append(self.loss_calculator.last_out[4:4 + class_num])     # hard Dice of net 1's labelled rows
            loss_sup2 = self.get_loss_value(data_lab, outputs2[:n0], y0)
            pse_prob1, pse_prob2 = cross_pseudo_labels([outputs1[n0:], outputs2[n0:]])
            pse_sup1 = self.get_loss_value(data_unlab, outputs1[n0:], pse_prob2)
            pse_sup2 = self.get_loss_value(data_unlab, outputs2[n0:], pse_prob1)
            regular_w = ssl_cfg.get('regularize_w', 0.1) * self._ramp()
            loss = (loss_sup1 + regular_w * pse_sup1) + (loss_sup2 + regular_w * pse_sup2)
            loss.backward()
            self.optimizer.step()
            if self.scheduler is not None and not isinstance(self.scheduler, lr_scheduler.ReduceLROnPlateau):
                self.scheduler.step()
            row = torch.stack([loss.detach(), loss_sup1.detach(), loss_sup2.detach(), pse_sup1.detach(), pse_sup2.detach()])
            sums = row if sums is None else sums + row
        vals = (sums / iter_valid).cpu().numpy().astype(np.float64)          # the round's one host read
        cls = torch.stack(dice).mean(0).cpu().numpy().astype(np.float64)
        return {'loss': float(vals[0]), 'loss_sup1': float(vals[1]), 'loss_sup2': float(vals[2]), 'loss_pse_sup1': float(vals[3]),
                'loss_pse_sup2': float(vals[4]), 'regular_w': regular_w, 'avg_dice': float(cls.mean()), 'class_dice': cls}

    def write_scalars(self, train_scalars, valid_scalars, lr_value, glob_it):
        """ssl_cps.py:152-176: the two log lines, and the same tags into `summ_writer` where one is attached"""
        w = self.summ_writer
        if w is not None:
            w.add_scalars('loss', {'train': train_scalars['loss'], 'valid': valid_scalars['loss']}, glob_it)
            w.add_scalars('loss_sup', {'net1': train_scalars['loss_sup1'], 'net2': train_scalars['loss_sup2']}, glob_it)
            w.add_scalars('loss_pseudo_sup', {'net1': train_scalars['loss_pse_sup1'], 'net2': train_scalars['loss_pse_sup2']}, glob_it)
            w.add_scalars('regular_w', {'regular_w': train_scalars['regular_w']}, glob_it)
            w.add_scalars('lr', {"lr": lr_value}, glob_it)
            w.add_scalars('dice', {'train': train_scalars['avg_dice'], 'valid': valid_scalars['avg_dice']}, glob_it)
            for c in range(self.config['network']['class_num']):
                w.add_scalars('class_{0:}_dice'.format(c), {'train': train_scalars['class_dice'][c],
                                                            'valid': valid_scalars['class_dice'][c]}, glob_it)
        for name, sc in (('train', train_scalars), ('valid', valid_scalars)):
            logging.info('{0:} loss {1:.4f}, avg dice {2:.4f} '.format(name, sc['loss'], sc['avg_dice']) + "[" +
                         ' '.join("{0:.4f}".format(x) for x in sc['class_dice']) + "]")

    def train_valid(self):
        history = super(SSLCPS, self).train_valid()
        for glob_it, lr_value, train_scalars, valid_scalars in history:
            self.write_scalars(train_scalars, valid_scalars, lr_value, glob_it)
        return history


SSLMethodDict = {'EntropyMinimization': SSLEntropyMinimization,
                 'MeanTeacher': SSLMeanTeacher,
                 'UAMT': SSLUncertaintyAwareMeanTeacher}

# the first registry stays as the earlier suite pins it; this one holds every method that is built (the SegLossDict /
# SegLossDictAll precedent)
SSLMethodDictAll = dict(SSLMethodDict, CPS=SSLCPS, URPC=SSLURPC)


def ssl_agent_class(name):
    """ssl_main.py:16-21,42-43: the agent class of [semi_supervised_learning] ssl_method among the first three methods"""
    if name in _REFUSED_METHODS:
        raise ValueError("fplx ssl: {0:} is not built: CCT, CPS and URPC need multi-decoder or two-branch networks the registry "
                         "does not hold (SegNetDict has UNet2D5, UNet3D and the DSBN networks); CPS and URPC are in "
                         "SSLMethodDictAll / ssl_agent_class_all".format(name))
    if name not in SSLMethodDict:
        raise ValueError("Undefined semi-supervised method {0:}".format(name))
    return SSLMethodDict[name]


def ssl_agent_class_all(name):
    """the agent class among all five built methods; CCT is refused"""
    if name == "CCT":
        raise ValueError("fplx ssl: CCT is not built: its network with auxiliary decoders lives in pymic.net.net2d, a package "
                         "the reference tree does not contain")
    if name not in SSLMethodDictAll:
        raise ValueError("Undefined semi-supervised method {0:}".format(name))
    return SSLMethodDictAll[name]
