"""Fused optimisers + lr schedule with the reference's optimiser semantics
(reference: PyMIC/pymic/net_run_dsbn/get_optimizer.py:9-57: optim.<Name>(params, lr[, momentum], weight_decay=wd) with torch's
defaults for everything else; MultiStepLR(milestones, gamma, last_epoch)).

torch.optim.Optimizer is subclassed only so that torch's lr schedulers, `param_groups` and
`state_dict` plumbing keep working; the update itself is ONE HIP kernel launch per flat
segment (shared parameters, each domain's BN affine parameters): parameters whose gradient is
None are skipped entirely, exactly like torch's optimisers - with DSBN that is every BN set of
the domains that took no part in the step (dsbn.py:56).

FusedOptimizer holds what does not depend on the update rule (flat state buffers, segments and their step counts, the two
entry points, the pack plan, the launch); the eight classes behind get_optimizer's names add the rule: which kind of
fplx_optim_step, which hyper-parameters, which state.
"""
import torch
from torch.optim import Optimizer, lr_scheduler

from . import ops


def keyword_match(a, b):
    return a.lower() == b.lower()


class FusedOptimizer(Optimizer):
    """Base of the fused optimisers.  A subclass names torch's class (TORCH) and its kind of fplx_optim_step /
    fplx_optim_pack_step (KIND, a name of ops.OPTIM_KINDS), lists its per-element state under torch's key names (STATE;
    `_active_state()` where that depends on a hyper-parameter) and gives `_hp(si)`, the kind's hyper-parameters in the order
    include/fplx.h documents."""
    TORCH = None
    KIND = None
    STATE = ()
    HAS_STEP = True                      # torch keeps a `step` tensor per parameter (all but SGD)

    def __init__(self, net, defaults):
        net._ensure_flat()
        self.net = net
        super(FusedOptimizer, self).__init__([net.get_param(k) for k in net._order], defaults)
        for name in self._active_state():
            setattr(self, name, torch.zeros_like(net.flat_params))
        shared, doms = net.segments()
        self.seg_ranges = [shared] + doms
        self.seg_steps = [0] * len(self.seg_ranges)
        self.grad_scale = 1.0            # e.g. 1/world_size after an all-reduce(sum)
        # data parallelism in autograd mode (SegmentationAgent): step() all-reduces (sum) the gradients first - the loss was
        # evaluated over the full batch of all ranks (fplx.loss dist_sync), so the sum IS its gradient
        self.dist_sync, self.dist_group = False, None

    def _active_state(self):
        """names of the flat state buffers this instance reads and writes, in the order of the kernel's streams"""
        return self.STATE

    def _buffer(self, name):
        """the flat state buffer `name`, created (zero) on first use: a momentum switched on after construction"""
        b = getattr(self, name, None)
        if b is None:
            b = torch.zeros_like(self.net.flat_params)
            setattr(self, name, b)
        return b

    def _hp(self, si):
        raise NotImplementedError

    def _update(self, si, start, end, g, plan):
        """one launch over flat_params[start:end] with the gradient g (same length) at segment si's current step count;
        plan: the engine's pack plan (the launch then writes the bf16 packs too) or None"""
        st = [self._buffer(name)[start:end] for name in self._active_state()] + [None, None]
        args = (self.KIND, self.net.flat_params[start:end], g, st[0], st[1], self._hp(si), self.seg_steps[si], self.grad_scale)
        if plan:
            ops.optim_pack_step(*(args + (plan,)))
        else:
            ops.optim_step(*args)

    def _segment_stepped(self, si):
        """after segment si's launch(es) of one step: per-segment host scalars (ASGD)"""

    def _segment_grad(self, start, end):
        """flat gradient tensor covering [start, end) if every parameter's .grad is the matching
        view of ONE flat buffer; 'none' if all grads are None; else None (mixed)."""
        net = self.net
        base, any_grad, all_grad, contiguous = None, False, True, True
        for k in net._order:
            o, n, _ = net._layout[k]
            if o < start or o >= end:
                continue
            g = net.get_param(k).grad
            if g is None:
                all_grad = False
                continue
            any_grad = True
            if not g.is_contiguous() or g.dtype != torch.float32:
                contiguous = False
                continue
            b = g.data_ptr() - (o - start) * 4
            if base is None:
                base = (b, g)
            elif b != base[0]:
                contiguous = False
        if not any_grad:
            return "none"
        if all_grad and contiguous:
            # rebuild a flat view over the underlying storage (all grads are views of one buffer)
            first = None
            for k in net._order:
                o, n, _ = net._layout[k]
                if o == start:
                    first = net.get_param(k).grad
                    break
            need = (first.storage_offset() + end - start) * 4
            if first.untyped_storage().nbytes() >= need:
                return torch.as_strided(first, (end - start,), (1,), first.storage_offset())
        return None

    @torch.no_grad()
    def step(self, closure=None):
        net = self.net
        net._ensure_flat()
        net.engine.invalidate()                 # raw-pointer update below: packs and eval-mode folds are stale afterwards
        for si, (start, end) in enumerate(self.seg_ranges):
            g = self._segment_grad(start, end)
            if isinstance(g, str):
                continue                                        # whole segment has no gradient: skipped
            self.seg_steps[si] += 1
            if self.dist_sync:
                import torch.distributed as dist
                if g is not None:
                    dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.dist_group)
                else:
                    for k in net._order:
                        o, n, _ = net._layout[k]
                        p = net.get_param(k)
                        if start <= o < end and p.grad is not None:
                            dist.all_reduce(p.grad, op=dist.ReduceOp.SUM, group=self.dist_group)
            if g is not None:
                self._update(si, start, end, g, None)
            else:                                               # gradients not flat: one launch per tensor
                for k in net._order:
                    o, n, _ = net._layout[k]
                    p = net.get_param(k)
                    if o < start or o >= end or p.grad is None:
                        continue
                    self._update(si, o, o + n, p.grad.float().contiguous().view(-1), None)
            self._segment_stepped(si)
        net.engine.invalidate()

    @torch.no_grad()
    def step_flat(self, gflat, active_domains):
        """engine-mode update: gflat is laid out like net.flat_params; only the shared segment and
        the listed domains' BN segments are updated."""
        net = self.net
        net.engine.invalidate()                 # the update goes through raw pointers: packs and eval-mode folds are stale now
        self._opt_called = True                 # torch's lr schedulers check that an optimiser step preceded theirs
        fused = False
        for si, (start, end) in enumerate(self.seg_ranges):
            if si > 0 and (si - 1) not in active_domains:
                continue
            self.seg_steps[si] += 1
            plan = net.engine.adam_pack_plan() if si == 0 else None
            if plan:
                # the shared segment: the update AND the bf16 packs of its 3x3x3 weights in one launch - the next forward finds
                # them in place instead of re-reading every master weight (get_optimizer.py:13-34 + unet2d5_dsbn.py:54-55)
                assert start == 0 and all(l[0] + l[1] * l[2] * 27 <= end for l in plan)
                fused = True
            self._update(si, start, end, gflat[start:end], plan or None)
            self._segment_stepped(si)
        if fused:
            net.engine.packs_written_by_optimizer()

    def state_dict(self):
        """torch.optim.<TORCH>'s layout over the reference's parameter list (fplx/checkpoint.py): what the reference's
        agent saves as 'optimizer_state_dict' and what its create_optimizer loads back (agent_abstract.py:327-330)"""
        from .checkpoint import optimizer_to_reference
        return optimizer_to_reference(self)

    def _segment_scalars(self):
        """per-segment host scalars beyond the step count, as {name: list} (ASGD's eta and mu)"""
        return {}

    def flat_state_dict(self):
        sd = {name: self._buffer(name) for name in self._active_state()}
        sd.update({k: list(v) for k, v in self._segment_scalars().items()})
        sd.update({"seg_steps": list(self.seg_steps),
                   "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]})
        return sd

    def load_state_dict(self, sd):
        if "state" in sd:                                       # a torch.optim.<TORCH> / reference checkpoint
            from .checkpoint import optimizer_from_reference
            return optimizer_from_reference(self, sd)
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        for name in self._active_state():
            self._buffer(name).copy_(sd[name])
        self.seg_steps = list(sd["seg_steps"])
        for k in self._segment_scalars():
            setattr(self, k, list(sd[k]))


class FusedAdam(FusedOptimizer):
    """torch.optim.Adam(lr, weight_decay) (get_optimizer.py:16-17).  Its launches go through ops.adam_step / ops.adam_pack_step,
    kind "Adam" under the names a kernel timer looks for."""
    TORCH = KIND = "Adam"
    STATE = ("exp_avg", "exp_avg_sq")

    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super(FusedAdam, self).__init__(net, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _hp(self, si):
        g = self.param_groups[0]
        return (g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'])

    def _update(self, si, start, end, g, plan):
        lr, b1, b2, eps, wd = self._hp(si)
        args = (self.net.flat_params[start:end], g, self.exp_avg[start:end], self.exp_avg_sq[start:end], lr, self.seg_steps[si],
                wd, self.grad_scale, (b1, b2), eps)
        if plan:
            ops.adam_pack_step(*(args + (plan,)))
        else:
            ops.adam_step(*args)


class FusedSGD(FusedOptimizer):
    """torch.optim.SGD(lr, momentum, weight_decay) (get_optimizer.py:13-15): dampening 0, no Nesterov momentum"""
    TORCH = KIND = "SGD"
    STATE = ("momentum_buffer",)
    HAS_STEP = False

    def __init__(self, net, lr=1e-3, momentum=0.0, weight_decay=0.0):
        super(FusedSGD, self).__init__(net, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))

    def _active_state(self):
        return self.STATE if self.param_groups[0]['momentum'] != 0 else ()

    def _hp(self, si):
        g = self.param_groups[0]
        return (g['lr'], g['momentum'], g['weight_decay'])


class FusedAdadelta(FusedOptimizer):
    """torch.optim.Adadelta(lr, weight_decay) (get_optimizer.py:20-21)"""
    TORCH = KIND = "Adadelta"
    STATE = ("square_avg", "acc_delta")

    def __init__(self, net, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0.0):
        super(FusedAdadelta, self).__init__(net, dict(lr=lr, rho=rho, eps=eps, weight_decay=weight_decay))

    def _hp(self, si):
        g = self.param_groups[0]
        return (g['lr'], g['rho'], g['eps'], g['weight_decay'])


class FusedAdagrad(FusedOptimizer):
    """torch.optim.Adagrad(lr, weight_decay) (get_optimizer.py:22-23); the accumulator starts at 0"""
    TORCH = KIND = "Adagrad"
    STATE = ("sum",)

    def __init__(self, net, lr=1e-2, lr_decay=0.0, weight_decay=0.0, eps=1e-10):
        super(FusedAdagrad, self).__init__(net, dict(lr=lr, lr_decay=lr_decay, eps=eps, weight_decay=weight_decay,
                                                     initial_accumulator_value=0.0))

    def _hp(self, si):
        g = self.param_groups[0]
        return (g['lr'], g['lr_decay'], g['eps'], g['weight_decay'])


class FusedAdamax(FusedOptimizer):
    """torch.optim.Adamax(lr, weight_decay) (get_optimizer.py:24-25)"""
    TORCH = KIND = "Adamax"
    STATE = ("exp_avg", "exp_inf")

    def __init__(self, net, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super(FusedAdamax, self).__init__(net, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _hp(self, si):
        g = self.param_groups[0]
        return (g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'])


def _f32(x):
    """x as torch keeps a scalar in a float32 tensor"""
    return float(torch.tensor(float(x), dtype=torch.float32))


class FusedASGD(FusedOptimizer):
    """torch.optim.ASGD(lr, weight_decay) (get_optimizer.py:26-27).  eta and mu are per-segment host scalars (seg_eta, seg_mu),
    float32 values like torch's state tensors: a step uses the pair formed after the previous one, from the lr of that time."""
    TORCH = KIND = "ASGD"
    STATE = ("ax",)

    def __init__(self, net, lr=1e-2, lambd=1e-4, alpha=0.75, t0=1e6, weight_decay=0.0):
        super(FusedASGD, self).__init__(net, dict(lr=lr, lambd=lambd, alpha=alpha, t0=t0, weight_decay=weight_decay))
        self.seg_eta = [None] * len(self.seg_ranges)            # None: not stepped yet - the first step takes the lr of its time
        self.seg_mu = [1.0] * len(self.seg_ranges)

    def _segment_scalars(self):
        return {"seg_eta": self.seg_eta, "seg_mu": self.seg_mu}

    def _hp(self, si):
        g = self.param_groups[0]
        if self.seg_eta[si] is None:
            self.seg_eta[si] = _f32(g['lr'])
        return (self.seg_eta[si], self.seg_mu[si], g['lambd'], g['weight_decay'])

    def _segment_stepped(self, si):
        g, step = self.param_groups[0], self.seg_steps[si]
        self.seg_eta[si] = _f32(g['lr'] / ((1 + g['lambd'] * g['lr'] * step) ** g['alpha']))
        self.seg_mu[si] = _f32(1 / max(1, step - g['t0']))


class FusedRMSprop(FusedOptimizer):
    """torch.optim.RMSprop(lr, momentum, weight_decay) (get_optimizer.py:30-32): not centred"""
    TORCH = KIND = "RMSprop"
    STATE = ("square_avg", "momentum_buffer")

    def __init__(self, net, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0):
        super(FusedRMSprop, self).__init__(net, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum,
                                                     centered=False))

    def _active_state(self):
        return self.STATE if self.param_groups[0]['momentum'] > 0 else self.STATE[:1]

    def _hp(self, si):
        g = self.param_groups[0]
        return (g['lr'], g['alpha'], g['eps'], g['momentum'], g['weight_decay'])


class FusedRprop(FusedOptimizer):
    """torch.optim.Rprop(lr) (get_optimizer.py:33-34): no weight decay; a segment's step_size is filled with the lr of its
    first step (the kernel does that at step 1)"""
    TORCH = KIND = "Rprop"
    STATE = ("prev", "step_size")

    def __init__(self, net, lr=1e-2, etas=(0.5, 1.2), step_sizes=(1e-6, 50)):
        super(FusedRprop, self).__init__(net, dict(lr=lr, etas=etas, step_sizes=step_sizes))

    def _hp(self, si):
        g = self.param_groups[0]
        return (g['lr'], g['etas'][0], g['etas'][1], g['step_sizes'][0], g['step_sizes'][1])


FUSED_CLASSES = (FusedAdam, FusedSGD, FusedAdadelta, FusedAdagrad, FusedAdamax, FusedASGD, FusedRMSprop, FusedRprop)
_REFUSED = {
    "sparseadam": "SparseAdam raises on dense gradients, and the network's gradients are dense: the reference cannot train "
                  "with it either (get_optimizer.py:18-19)",
    "lbfgs": "LBFGS.step needs a closure that the reference's training loops never pass (agent_seg.py:490-494): the reference "
             "cannot train with it either (get_optimizer.py:28-29)",
}


def get_optimizer(name, net, optim_params):
    """get_optimizer (get_optimizer.py:9-36): the eight names the reference can train with, each one fused launch per segment.
    The reference reads optim_params['momentum'] before it dispatches (get_optimizer.py:11); here Adam alone tolerates a
    missing key (existing callers omit it), every other name raises ValueError naming it."""
    lr = optim_params['learning_rate']
    weight_decay = optim_params['weight_decay']
    if keyword_match(name, "Adam"):
        return FusedAdam(net, lr, weight_decay=weight_decay)
    if name.lower() in _REFUSED:
        raise ValueError("unsupported optimizer {0:}: {1:}".format(name, _REFUSED[name.lower()]))
    by_name = {c.TORCH.lower(): c for c in FUSED_CLASSES[1:]}
    if name.lower() not in by_name:
        raise ValueError("unsupported optimizer {0:}".format(name))               # get_optimizer.py:36
    if 'momentum' not in optim_params:
        raise ValueError("optimizer {0:}: the key 'momentum' is missing from the training parameters (the reference reads it "
                         "for every optimizer, get_optimizer.py:11)".format(name))
    cls = by_name[name.lower()]
    if cls in (FusedSGD, FusedRMSprop):
        return cls(net, lr, momentum=optim_params['momentum'], weight_decay=weight_decay)
    if cls is FusedRprop:
        return cls(net, lr)
    return cls(net, lr, weight_decay=weight_decay)


def get_lr_scheduler(optimizer, sched_params):
    """get_lr_scheduler (get_optimizer.py:39-57)."""
    name = sched_params["lr_scheduler"]
    if name is None:
        return None
    lr_gamma = sched_params["lr_gamma"]
    if keyword_match(name, "ReduceLROnPlateau"):
        patience = sched_params["ReduceLROnPlateau_patience".lower()] / sched_params["iter_valid"]
        return lr_scheduler.ReduceLROnPlateau(optimizer, mode="max", factor=lr_gamma, patience=patience)
    if keyword_match(name, "MultiStepLR"):
        return lr_scheduler.MultiStepLR(optimizer, sched_params["lr_milestones"], lr_gamma,
                                        sched_params["last_iter"])
    raise ValueError("unsupported lr scheduler {0:}".format(name))
