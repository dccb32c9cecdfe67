"""The network groups of the reference's two-network trainers and the one optimiser over them: BiNet (nll_co_teaching.py:21-35,
ssl_cps.py:15-29), TriNet (nll_trinet.py:21-37), GroupOptimizer.  A module of its own because both fplx/nll.py (CoTeaching,
TriNet) and fplx/ssl.py (CPS) build on it and nll.py imports from ssl.py; fplx.nll re-exports the names unchanged."""
import torch
import torch.nn as nn
from torch.optim import Optimizer

from .agent import SegNetDict

_DSBN_NAMES = ("UNet2D5_dsbn", "UNet3D_dsbn")


class _NetGroup(nn.Module):
    """what BiNet and TriNet share: `count` networks of [network] net_type under the reference's member names"""
    count = 0

    def __init__(self, params, net_dict=None):
        super(_NetGroup, self).__init__()
        net_dict = SegNetDict if net_dict is None else net_dict
        net_name = params['net_type']
        if net_name in _DSBN_NAMES:
            raise ValueError("fplx nll: {0:} is a domain-specific-BatchNorm network; the noisy-label agents derive from "
                             "net_run/agent_seg.py and run UNet2D5 / UNet3D only".format(net_name))
        if net_name not in net_dict:
            raise ValueError("Undefined network {0:}".format(net_name))
        seed = int(params.get('dropout_seed', 1))
        for i in range(self.count):
            cfg = dict(params)
            cfg['dropout_seed'] = seed + i                 # the reference's members draw from one global stream
            setattr(self, "net{0:}".format(i + 1), net_dict[net_name](cfg))

    def members(self):
        return [getattr(self, "net{0:}".format(i + 1)) for i in range(self.count)]

    def reference_param_names(self):
        """fplx.checkpoint.reference_model_state_dict: this module's own state_dict() is the reference's"""
        return [k for k, _ in self.named_parameters()]

    def load_state_dict(self, state_dict, strict=True, **kw):
        r = super(_NetGroup, self).load_state_dict(state_dict, strict=strict, **kw)
        for m in self.members():
            if callable(getattr(m, "parameters_changed", None)):
                m.parameters_changed()                     # the members' packs are rebuilt from the new values
        return r

    def _outputs(self, x, domain_label):
        return [m(x, domain_label=domain_label) for m in self.members()]

    @staticmethod
    def _sum(outs):
        """out1 + out2 (+ out3), added in that order; deep supervision: output by output"""
        if isinstance(outs[0], (list, tuple)):
            return [_NetGroup._sum([o[i] for o in outs]) for i in range(len(outs[0]))]
        acc = outs[0]
        for o in outs[1:]:
            acc = acc + o
        return acc

    def forward(self, x, domain_label=None):
        """the tuple of the members' outputs in training; in eval mode their sum over 3 - for BiNet too"""
        outs = self._outputs(x, domain_label)
        if self.training:
            return tuple(outs)
        s = self._sum(outs)
        return [t / 3 for t in s] if isinstance(s, list) else s / 3


class BiNet(_NetGroup):
    """nll_co_teaching.py:21-35.  In eval mode the output is (out1 + out2) / 3 - the reference's literal, kept (the argmax is
    the mean's; a validation loss computed from it sees logits scaled by 2 / 3)."""
    count = 2


class TriNet(_NetGroup):
    """nll_trinet.py:21-37.  In eval mode the output is (out1 + out2 + out3) / 3."""
    count = 3


class GroupOptimizer(Optimizer):
    """ONE optimiser over the members of a BiNet / TriNet: a fused optimiser per member (each bound to its network's flat
    buffer), stepped with the hyper-parameters of this object's single param group - what lr schedulers write and
    `param_groups[0]['lr']` reads.  Every optimiser of get_optimizer is elementwise, so this is the reference's single
    optimiser over all parameters."""

    def __init__(self, members):
        self.members = list(members)
        if not self.members:
            raise ValueError("fplx nll: an optimiser group needs at least one member")
        params = [p for m in self.members for g in m.param_groups for p in g['params']]
        super(GroupOptimizer, self).__init__(params, self._hp(self.members[0]))

    @staticmethod
    def _hp(opt):
        return {k: v for k, v in opt.param_groups[0].items() if k != 'params'}

    @torch.no_grad()
    def step(self, closure=None):
        hp = self._hp(self)
        for m in self.members:
            m.param_groups[0].update({k: v for k, v in hp.items() if k in m.param_groups[0]})
            m.step()

    def state_dict(self):
        """{'members': each member's state_dict (torch.optim's layout over that network's parameters), 'param_groups': this
        object's hyper-parameters}"""
        return {'members': [m.state_dict() for m in self.members], 'param_groups': [self._hp(self)]}

    def load_state_dict(self, sd):
        if 'members' not in sd or len(sd['members']) != len(self.members):
            raise ValueError("fplx nll: the optimiser state holds {0:} members, this group {1:}".format(
                len(sd.get('members', ())), len(self.members)))
        for m, s in zip(self.members, sd['members']):
            m.load_state_dict(s)
        self.param_groups[0].update({k: v for k, v in sd['param_groups'][0].items() if k != 'params'})
