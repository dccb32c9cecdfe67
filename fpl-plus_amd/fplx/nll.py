"""Noisy-label trainers behind the reference's fourth entry point `pymic_nll`
(reference: PyMIC/pymic/net_run_nll/nll_co_teaching.py:21-147 BiNet / NLLCoTeaching, nll_trinet.py:21-171 TriNet / NLLTriNet,
nll_main.py:12-41; util/ramps.py get_rampup_ratio).

What an iteration adds to supervised training - the per-voxel cross entropy of two or three networks, the selection of the
small-loss voxels (CoTeaching: the first num_remb of an argsort; TriNet: below torch.quantile) and the means over the sets the
OTHER network(s) chose - runs in the kernels of csrc/nll.hip (include/fplx.h, "noisy-label learning") on the order statistics
of fplx_select_kth: no sort, no gather, no host round trip.  `selective_ce_loss` is ONE autograd node over all logit tensors.

Kept: the config keys ([noisy_label_learning] nll_method, co_teaching_select_ratio, trinet_select_ratio, rampup_start,
rampup_end), the ramps (sigmoid for CoTeaching, linear for TriNet), num_remb = int(remb_ratio * n), the state-dict keys
net1.* / net2.* / net3.*, the returned scalars with their quirks (TriNet reports (loss1 + loss2) / 2 and no loss3), BiNet's
eval output (out1 + out2) / 3 (sic), CoTeaching's warning about loss_type.
Different, on purpose: of the voxels tied at the num_remb-th loss the first in index order are taken (the
reference's argsort is not stable and takes some of them); DAST is refused (it needs a two-branch network); DSBN networks and
torch.distributed groups are refused; the members' dropout streams are seeded dropout_seed + 0, + 1, + 2.
BiNet, TriNet and GroupOptimizer live in fplx/netgroup.py (the semi-supervised CPS agent builds on them too) and are re-exported
here unchanged.
"""
import logging

import numpy as np
import torch
from torch.optim import lr_scheduler

from . import filter as fpl_filter_mod
from . import ops
from .agent import SegmentationAgent
from .optim import get_optimizer
from .netgroup import _NetGroup, BiNet, TriNet, GroupOptimizer, _DSBN_NAMES          # noqa: F401 (re-exported)
from .ssl import get_rampup_ratio, _logits_of

NLL_MODES = ("CoTeaching", "TriNet")


class _SelectiveCE(torch.autograd.Function):
    """fplx_nll_voxel_ce_fwd, fplx_select_kth + fplx_nll_select_mask per network, fplx_nll_select_fwd / _bwd as one node"""

    @staticmethod
    def forward(ctx, labels, mode, ratio, holder, *logits):
        ls = [t.float().contiguous() for t in logits]
        y = labels.detach().float().contiguous()
        loss, part = ops.nll_voxel_ce_fwd(ls, y)
        n = loss[0].numel()
        if mode == "CoTeaching":
            num_remb = int(ratio * n)                                          # nll_co_teaching.py:112
            masks = [ops.nll_select_mask(l, ops.NLL_RANK, num_remb=num_remb) for l in loss]
        else:
            masks = [ops.nll_select_mask(l, ops.NLL_BELOW, q=ratio) for l in loss]
        uses = ops.NLL_USES[mode]
        out = ops.nll_select_fwd(loss, masks, uses, part)
        ctx.save_for_backward(y, out, *(masks + ls))
        ctx.k, ctx.uses, ctx.wj = len(ls), uses, (1.0 if mode == "CoTeaching" else 1.0 / 3.0)
        if holder is not None:
            holder["out"], holder["masks"], holder["losses"] = out, masks, loss
        total = out[:, 2].sum()
        return (total if mode == "CoTeaching" else total / 3.0).float()

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        y, out, masks, ls = saved[0], saved[1], list(saved[2:2 + ctx.k]), list(saved[2 + ctx.k:])
        d = ops.nll_select_bwd(ls, y, masks, ctx.uses, out, g.float().contiguous().reshape(1), ctx.wj)
        return (None, None, None, None) + tuple(d)


def selective_ce_loss(logits_list, labels_prob, mode, ratio, holder=None):
    """The reference's training scalar of one iteration.  mode "CoTeaching": two logit tensors, `ratio` = remb_ratio, the loss is
    loss1[ind_2_sorted[:num_remb]].mean() + loss2[ind_1_sorted[:num_remb]].mean() with num_remb = int(ratio * n)
    (nll_co_teaching.py:100-118).  mode "TriNet": three tensors, `ratio` = the quantile q, mask_k = loss_k < quantile(loss_k, q),
    the loss is the mean over k of sum(loss_k * mask_i * mask_j) / sum(mask_i * mask_j), i, j the other two (nll_trinet.py:66-
    120).  holder: an optional dict that receives `out` (double [K, 4]: kept sum, kept count, their mean, the sum of all
    loss_k), `masks` (K uint8 [n]) and `losses` (K fp32 [n]), n = N D H W voxels in reshape_tensor_to_2D's order.  Nothing is
    read back to the host."""
    if mode not in NLL_MODES:
        raise ValueError("fplx nll: mode {0:} (one of {1:})".format(mode, ", ".join(NLL_MODES)))
    ls = [_logits_of(t, "logits") for t in logits_list]
    want = len(ops.NLL_USES[mode])
    if len(ls) != want:
        raise ValueError("fplx nll: {0:} takes {1:} logit tensors, got {2:}".format(mode, want, len(ls)))
    ratio = float(ratio)
    if not 0.0 <= ratio <= 1.0:
        raise ValueError("fplx nll: ratio {0:} outside [0, 1]".format(ratio))
    ops.require_gpu(labels_prob)
    return _SelectiveCE.apply(labels_prob, mode, ratio, holder, *ls)


_REFUSED_METHODS = ("DAST",)


class NLLSegAgent(SegmentationAgent):
    """what NLLCoTeaching and NLLTriNet share.  Subclasses give `group_class`, `mode`, the ratio key and the ramp."""
    group_class = None
    mode = None
    ratio_key = None
    ramp_mode = "linear"

    def __init__(self, config, stage='train'):
        net_type = config.get('network', {}).get('net_type', None)
        if net_type in _DSBN_NAMES:
            raise ValueError("fplx nll: {0:} is a domain-specific-BatchNorm network; the noisy-label agents derive from "
                             "net_run/agent_seg.py and run UNet2D5 / UNet3D only".format(net_type))
        config['network'].setdefault('num_domains', 1)
        super(NLLSegAgent, self).__init__(config, stage)
        if self.distributed:
            raise ValueError("fplx nll: the noisy-label agents run in a single process (no torch.distributed group): the "
                             "gradients of UNet2D5 / UNet3D are not all-reduced")

    def create_dataset(self):
        ds = self.config['dataset']
        for ours, theirs in (('1_train_csv', 'train_csv'), ('1_valid_csv', 'valid_csv')):
            if ds.get(ours, None) is None and ds.get(theirs, None) is not None:
                ds[ours] = ds[theirs]
        super(NLLSegAgent, self).create_dataset()

    def create_network(self):
        if self.net is None:
            self.net = self.group_class(self.config['network'], self.net_dict)
        if self.tensor_type != 'float':
            raise ValueError("fplx: tensor_type must be float (fp32 parameters)")
        self.net.float()
        self.net.to(self.device)
        n = sum(p.numel() for p in self.net.parameters() if p.requires_grad)
        logging.info('parameter number {0:}'.format(n))

    def create_optimizer(self, params=None):
        opt_params = self.config['training']
        if self.optimizer is None:
            self.optimizer = GroupOptimizer([get_optimizer(opt_params['optimizer'], m, opt_params) for m in self.net.members()])
        super(NLLSegAgent, self).create_optimizer(params)

    def create_loss_calculator(self, entropy_weight=0.0):
        """the validation loss only (training takes selective_ce_loss); no entropy term, as in net_run/agent_seg.py"""
        super(NLLSegAgent, self).create_loss_calculator(0.0)

    def _remb_ratio(self):
        nll_cfg = self.config['noisy_label_learning']
        iter_max = self.config['training']['iter_max']
        ramp = get_rampup_ratio(getattr(self, 'glob_it', 0), nll_cfg.get('rampup_start', 0), nll_cfg.get('rampup_end', iter_max),
                                self.ramp_mode)
        return 1 - (1 - nll_cfg[self.ratio_key]) * ramp

    def training(self):
        class_num = self.config['network']['class_num']
        iter_valid = self.config['training']['iter_valid']
        it = iter(self.train_loader_1)
        self.net.train()
        sums, dice = None, []
        labels = list(range(class_num))
        remb_ratio = 1.0
        for _ in range(iter_valid):
            data, it = self._next(it, self.train_loader_1)
            inputs = self.convert_tensor_type(data['image']).to(self.device)
            labels_prob = self.convert_tensor_type(data['label_prob']).to(self.device)
            self.optimizer.zero_grad()
            outputs = self.net(inputs)
            remb_ratio = self._remb_ratio()
            holder = {}
            loss = selective_ce_loss(outputs, labels_prob, self.mode, remb_ratio, holder)
            loss.backward()
            self.optimizer.step()
            if self.scheduler is not None and not isinstance(self.scheduler, lr_scheduler.ReduceLROnPlateau):
                self.scheduler.step()
            out = holder["out"]
            n = holder["losses"][0].numel()
            # loss1, loss2 (selected means), loss_no_select1, loss_no_select2 (means over all voxels): device fp32, as the reference's
            row = torch.stack([out[0, 2], out[1, 2], out[0, 3] / n, out[1, 3] / n]).float()
            sums = row if sums is None else sums + row
            hard = fpl_filter_mod.hard_label(_logits_of(outputs[0], "outputs1"))            # argmax of outputs1, whole batch
            cnt = ops.overlap_counts(hard, fpl_filter_mod.hard_label(labels_prob), labels, on_device=True).float()
            dice.append((2.0 * cnt[:, 0] + 1e-5) / (cnt[:, 1] + cnt[:, 2] + 1e-5))          # get_classwise_dice
        vals = (sums / iter_valid).cpu().numpy().astype(np.float64)                       # the round's one host read
        cls = torch.stack(dice).mean(0).cpu().numpy().astype(np.float64)
        return {'loss': float(vals[0] + vals[1]) / 2, 'loss1': float(vals[0]), 'loss2': float(vals[1]),
                'loss_no_select1': float(vals[2]), 'loss_no_select2': float(vals[3]), 'select_ratio': remb_ratio,
                'avg_dice': float(cls.mean()), 'class_dice': cls}

    def training_all(self):
        """[training] dual selects between two supervised loops of the DSBN agent; here both names run the one NLL loop"""
        return self.training()


class NLLCoTeaching(NLLSegAgent):
    """nll_co_teaching.py:37-147"""
    group_class = BiNet
    mode = "CoTeaching"
    ratio_key = 'co_teaching_select_ratio'
    ramp_mode = "sigmoid"

    def __init__(self, config, stage='train'):
        super(NLLCoTeaching, self).__init__(config, stage)
        loss_type = config.get('training', {}).get("loss_type", None)
        if loss_type != "CrossEntropyLoss":
            logging.warning("only CrossEntropyLoss supported for coteaching, the specified loss {0:} is ingored".format(loss_type))


class NLLTriNet(NLLSegAgent):
    """nll_trinet.py:39-171"""
    group_class = TriNet
    mode = "TriNet"
    ratio_key = 'trinet_select_ratio'


NLLMethodDict = {'CoTeaching': NLLCoTeaching,
                 'TriNet': NLLTriNet}


def nll_agent_class(name):
    """nll_main.py:12-14,39-40: the agent class of [noisy_label_learning] nll_method"""
    if name in _REFUSED_METHODS:
        raise ValueError("fplx nll: {0:} is not built: DAST needs a two-branch network (`b0_pred, b1_pred = self.net(x)`, "
                         "nll_dast.py) the registry does not hold (SegNetDict has UNet2D5, UNet3D and the DSBN networks)".format(name))
    if name not in NLLMethodDict:
        raise ValueError("Undefined noisy-label method {0:}".format(name))
    return NLLMethodDict[name]
