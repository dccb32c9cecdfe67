"""Decision tape for the two network restatements (test infrastructure, torch on the CPU).

A U-Net's parameter gradients are piecewise smooth in its weights: every LeakyReLU / PReLU sign and every max-pooling winner is
a decision, and two correct evaluations that decide ONE voxel differently (a pre-activation of 1e-7 that rounds to either side
of zero) differ by far more than their round-off.  The tape makes the decisions explicit.  `oracle/torch_ref.unet_forward` and
`tests/nets3d_ref.forward` send every activation and pooling through `Tape.act` / `Tape.pool` and show it the tensors around
them (`Tape.tap`).  A tape records, per site and in forward order, the decision it would take itself, the margin of that
decision and the site's tensors; run `forced`, it applies somebody else's decisions instead - the fp32 restatement's, or the
device's, read off the state a forward keeps for its backward (`device_decisions`) - and the gradients follow them.  A float64
run with the decisions of an fp32 evaluation forced is then a reference for that evaluation's ARITHMETIC alone.

Conventions
  * every recorded tensor and every decision is [N, C, D, H, W]; the depth-folded [N D, C, H, W] tensors of a 2-D level are
    unfolded, the device's NDHWC [voxels, C] views are permuted (`ncdhw`).
  * activation: decision z > 0, margin |z|.  The slopes are positive, so the sign of a stored activation is the sign of its
    pre-activation; a stored activation that is exactly 0 is undecided and takes the reference's decision.
  * pooling: decision = index of the winner inside its window, the window scanned depth, then height, then width (a 2-D
    level's window has no depth: four entries).  Ties: the FIRST maximum in that order wins - the rule of F.max_pool3d and of
    the kernels (tests/test_gpu_kernels.py::test_maxpool_fwd_bwd_first_max_wins); `device_winners` applies the same rule
    when it compares a pooled tensor with the tensor it was pooled from.  Margin: largest minus second largest of the window.
  * mutants (tests/test_kink_oracle_cpu.py): `bwd` gives a site another decision in the backward only, `cut` drops the
    gradient that flows back through one tapped tensor (a skip connection, a deep-supervision head's input).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_ref as R
from oracle.torch_ref import fold_depth, unfold_depth

# ---------------------------------------------------------------------------------------------- section "Tolerances"
MARGIN = 8.0                 # the device sums the same terms in other orders (MFMA accumulation, split-K and per-block partials);
#                              one host run samples ONE order.  The derived worst-case bounds of the project sit ~45 x above
#                              observed errors (DESIGN, the pyramid section): 8 is well inside what round-off alone can do
NEAR_TIE = 64.0              # a differing decision is a near-tie when its float64 margin <= NEAR_TIE x the site's measured error
MAX_DIFFERING = 16           # decisions per case that may differ from the free float64 run or be undecided
# a PReLU slope gradient is the cancelling sum over a whole tensor of d out * min(z, 0): its error is bounded relative to
# sum |terms|.  The bf16 tests allow SLOPE_CANCEL = 0.01 = 2.56 units of bf16 round-off (2^-8); the same count of fp32 units:
SLOPE_CANCEL_F32 = 0.01 * 2.0 ** -16


def _canon(t, n):
    return t if t.dim() == 5 else unfold_depth(t, n)


def _like(dec, x):
    return dec if x.dim() == 5 else fold_depth(dec)


def windows(x5, pd):
    """[N, C, D, H, W] -> [N, C, D / pd, H / 2, W / 2, 4 pd]: the pooling windows, entries in depth, height, width order"""
    n, c, d, h, w = x5.shape
    v = x5.reshape(n, c, d // pd, pd, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7)
    return v.reshape(n, c, d // pd, h // 2, w // 2, 4 * pd)


def first_true(eq):
    """index of the first True along the last axis; -1 where there is none"""
    k = eq.shape[-1]
    idx = torch.where(eq, torch.arange(k), torch.full((), k, dtype=torch.long)).min(-1).values
    return torch.where(idx == k, torch.full((), -1, dtype=torch.long), idx)


class _ActBwd(torch.autograd.Function):
    """activation whose backward follows another sign mask than its forward (a mutant)"""

    @staticmethod
    def forward(ctx, z, slope, fwd_mask, bwd_mask):
        ctx.save_for_backward(z, slope, bwd_mask)
        return torch.where(fwd_mask, z, z * slope)

    @staticmethod
    def backward(ctx, g):
        z, slope, m = ctx.saved_tensors
        zero = torch.zeros((), dtype=g.dtype)
        return torch.where(m, g, g * slope), torch.where(m, zero, g * z).sum().reshape(slope.shape), None, None


class _PoolBwd(torch.autograd.Function):
    """gather of the window entry `fwd_idx` whose backward scatters to `bwd_idx` (a mutant)"""

    @staticmethod
    def forward(ctx, win, fwd_idx, bwd_idx):
        ctx.save_for_backward(bwd_idx)
        ctx.shape = win.shape
        return win.gather(-1, fwd_idx.unsqueeze(-1)).squeeze(-1)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        return torch.zeros(ctx.shape, dtype=g.dtype).scatter_(-1, idx.unsqueeze(-1), g.unsqueeze(-1)), None, None


class Tape(object):
    """events: every tapped tensor and every decision site in forward order, dicts with `kind` in
         conv | act | pool | up | skip | head
       sites: the act / pool events among them.  An act event holds dec (own decision), margin, used (the decision applied),
       bn (pre-activation), out (the activation, as the graph holds it: `raw`), slope; a pool event dec, margin, used, inp, out.
       forced: None or a list of decisions aligned with `sites`;
       bwd: {site index: decision the backward follows};  cut: {(kind, k)}: the k-th tap of that kind passes no gradient."""

    def __init__(self, n, forced=None, bwd=None, cut=None):
        self.n, self.forced, self.bwd, self.cut = n, forced, bwd or {}, set(cut or ())
        self.events, self.sites, self.count = [], [], {}

    def tap(self, kind, t):
        k = self.count.get(kind, 0)
        self.count[kind] = k + 1
        self.events.append(dict(kind=kind, k=k, t=_canon(t, self.n)))
        return t.detach() if (kind, k) in self.cut else t

    def _forced(self):
        i = len(self.sites)
        return i, (None if self.forced is None else self.forced[i])

    def act(self, z, slope):
        i, f = self._forced()
        own = z > 0
        mask = own if f is None else _like(f, z)
        b = self.bwd.get(i)
        if b is not None:
            sl = slope if torch.is_tensor(slope) else torch.full((1,), slope, dtype=z.dtype)
            out = _ActBwd.apply(z, sl, mask, _like(b, z))
        elif f is None:                           # the restatements' own statements, bit for bit
            out = R.prelu(z, slope) if torch.is_tensor(slope) else F.leaky_relu(z, slope)
        else:
            out = torch.where(mask, z, z * slope)
        k = self.count.get("act", 0)
        self.count["act"] = k + 1
        ev = dict(kind="act", k=k, dec=_canon(own, self.n), used=_canon(mask, self.n), margin=_canon(z.detach().abs(), self.n),
                  bn=_canon(z, self.n), raw=out, t=_canon(out, self.n), slope=slope)
        self.events.append(ev)
        self.sites.append(ev)
        return out

    def pool(self, x):
        i, f = self._forced()
        x5 = _canon(x, self.n)
        pd = 2 if x.dim() == 5 else 1
        win = windows(x5, pd)
        wd = win.detach()
        top = torch.topk(wd, 2, dim=-1).values
        own = first_true(wd == top[..., :1])
        used = own if f is None else f
        b = self.bwd.get(i)
        if b is not None:
            out = _PoolBwd.apply(win, used, b)
        elif f is None:
            out = _canon(F.max_pool3d(x, 2, 2) if x.dim() == 5 else F.max_pool2d(x, 2, 2), self.n)
        else:
            out = win.gather(-1, used.unsqueeze(-1)).squeeze(-1)
        k = self.count.get("pool", 0)
        self.count["pool"] = k + 1
        ev = dict(kind="pool", k=k, dec=own, used=used, margin=top[..., 0] - top[..., 1], inp=x5, raw=out, t=out)
        self.events.append(ev)
        self.sites.append(ev)
        return out if x.dim() == 5 else fold_depth(out)

    def decisions(self):
        return [s["dec"] for s in self.sites]


# ---------------------------------------------------------------------------------------------- cases and CPU runs
class Case(object):
    """one network, one weight draw, one input: family 'dsbn' (oracle/torch_ref.unet_forward) or 'n3d' (tests/nets3d_ref)"""

    def __init__(self, name, family, params, weights, x, y, domain=0, loss="dice"):
        self.name, self.family, self.params, self.weights, self.x, self.y = name, family, params, weights, x, y
        self.domain, self.loss = domain, loss

    def loss_of(self, outs):
        y = self.y.to(outs[0].dtype)
        base = (lambda p: R.dice_loss(p, y)) if self.loss == "dice" else (lambda p: R.ce_loss(p, y))
        if len(outs) == 1:
            return base(outs[0])
        import nets3d_ref as R3
        return R3.deep_supervise_loss(outs, base)


def dsbn_case(name, domain):
    import detdata
    from make_golden_cfg import NETS, SHAPES, label_for
    p = NETS[name]
    return Case("%s.d%d" % (name, domain), "dsbn", p, detdata.state_dict_3d(p), torch.from_numpy(detdata.normal("x." + name, SHAPES[name])),
                torch.from_numpy(label_for(name)), domain, "dice")


def n3d_case(name, deep=None, draw=None, loss="dice"):
    """draw: None = the fixture's weights; a tag such as 'nll1': every float tensor but the running variances nudged by
    0.02 detdata.normal(tag + '.' + key) (the members of tests/test_gpu_nll.py and tests/test_gpu_ssl2.py)"""
    import detdata
    import nets3d_cfg as C
    p = dict(C.NETS[name])
    w = dict(C.weights_for(name))
    if deep is not None:
        p["deep_supervise"] = deep
        if not deep:
            w = {k: v for k, v in w.items() if not k.startswith(("out_conv1", "out_conv2", "out_conv3"))}
    if draw:
        for k, v in w.items():
            if v.dtype == np.float32 and not k.endswith("running_var"):
                w[k] = (v + 0.02 * detdata.normal("%s.%s" % (draw, k), v.shape)).astype(np.float32)
    tag = name + ("" if deep is None else (".ds" if deep else ".plain")) + ("." + draw if draw else "")
    return Case(tag, "n3d", p, w, torch.from_numpy(C.input_for(name)), torch.from_numpy(C.label_for(name)), 0, loss)


class Run(object):
    __slots__ = ("case", "dtype", "outs", "tape", "sd", "prm")


def run(case, dtype, forced=None, bwd=None, cut=None, taped=True):
    """one train-mode forward of the restatement in `dtype` -> Run (the graph is kept: `grads`)"""
    sd, prm = {}, {}
    for k, v in case.weights.items():
        t = torch.from_numpy(np.array(v))
        if t.is_floating_point():
            t = t.to(dtype)
        if k.endswith(R.PARAM_SUFFIXES):
            t.requires_grad_(True)
            prm[k] = t
        sd[k] = t
    x = case.x.to(dtype)
    tape = Tape(x.shape[0], forced, bwd, cut) if taped else None
    if case.family == "dsbn":
        outs = R.unet_forward(sd, case.params, x, case.domain, True, tape=tape)
    else:
        import nets3d_ref as R3
        outs = R3.forward(sd, case.params, x, True, tape=tape)
    r = Run()
    r.case, r.dtype, r.tape, r.sd, r.prm = case, dtype, tape, sd, prm
    r.outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
    return r


def loss_dlogits(r):
    """the loss gradient at the run's own outputs -> one tensor per output (run's dtype)"""
    leaves = [o.detach().clone().requires_grad_(True) for o in r.outs]
    return list(torch.autograd.grad(r.case.loss_of(leaves), leaves))


def dense_dlogits(case, like):
    """a dense normal draw per output, scaled to the RMS of the corresponding tensor of `like`: every voxel of every level is
    excited, not only the label ball"""
    import detdata
    out = []
    for i, a in enumerate(like):
        d = torch.from_numpy(detdata.normal("kink.dl.%s.%d" % (case.name, i), tuple(a.shape))).to(a.dtype)
        out.append(d * (a.pow(2).mean().sqrt() / d.pow(2).mean().sqrt()))
    return out


def grads(r, douts):
    """-> ({parameter key: gradient or None}, [d out per site or None]) of sum_i <outs_i, douts_i>"""
    keys = list(r.prm)
    raws = [s["raw"] for s in r.tape.sites] if r.tape is not None else []
    g = torch.autograd.grad(r.outs, [r.prm[k] for k in keys] + raws, grad_outputs=[d.to(r.dtype) for d in douts],
                            allow_unused=True, retain_graph=True)
    return dict(zip(keys, g[:len(keys)])), [None if t is None else _canon(t, r.tape.n) for t in g[len(keys):]]


# ---------------------------------------------------------------------------------------------- reports
def is_bn_fed_bias(k):
    """bias of a 3x3(x3) convolution in front of train-mode BatchNorm: the true gradient is exactly 0"""
    if not k.endswith(".bias"):
        return False
    if ".conv_conv." in k:
        return k.rsplit(".", 2)[1] in ("0", "4")
    return ".conv3d_" in k or ".conv2d_" in k


def grad_kind(k, sd):
    stem, leaf = k.rsplit(".", 1)
    if (stem + ".running_mean") in sd:
        return "bn." + leaf
    if leaf == "weight" and sd[k].dim() == 1:
        return "slope"
    return "conv." + leaf


def saved_report(r):
    """every saved tensor of a taped run in forward order -> [(name, kind, float64 tensor)]: conv outputs with their BatchNorm
    rows, activations, pooled and up-sampled tensors, the outputs, the updated running statistics"""
    rep, site = [], 0
    for ev in r.tape.events:
        kd = ev["kind"]
        if kd == "conv":
            y = ev["t"].detach().double()
            red = (0, 2, 3, 4)
            rep.append(("site%02d.conv" % site, "conv", y))
            rep.append(("site%02d.mean" % site, "mean", y.mean(red)))
            rep.append(("site%02d.rstd" % site, "rstd", torch.rsqrt(y.var(red, unbiased=False) + R.BN_EPS)))
        elif kd == "act":
            rep.append(("site%02d.act" % site, "act", ev["t"].detach().double()))
            site += 1
        elif kd == "pool":
            rep.append(("pool%d" % ev["k"], "pool", ev["t"].detach().double()))
        elif kd == "up":
            rep.append(("up%d" % ev["k"], "up", ev["t"].detach().double()))
    for i, o in enumerate(r.outs):
        rep.append(("logits%d" % i, "logits", o.detach().double()))
    for k, v in r.sd.items():
        leaf = k.rsplit(".", 1)[1]
        if leaf in ("running_mean", "running_var") and _live_stat(r, k):
            rep.append((k, leaf, v.detach().double()))
    return rep


def _live_stat(r, k):
    return r.case.family != "dsbn" or (".bns.%d." % r.case.domain) in k


def grad_report(r, g):
    """parameter gradients in backward order (out_conv first) -> [(key, kind, float64 tensor)]; no entry for the parameters
    without a gradient (the other domain's BatchNorm) and for the convolution biases in front of a train-mode BatchNorm"""
    return [(k, grad_kind(k, r.sd), g[k].detach().double()) for k in reversed(list(r.prm))
            if g[k] is not None and not is_bn_fed_bias(k)]


def slope_terms(r, douts_site):
    """{PReLU slope key: sum |d out * min(z, 0)|}, the scale its gradient's error is bounded by, from the tape"""
    name_of = {id(t): k for k, t in r.prm.items()}
    out = {}
    for s, d in zip(r.tape.sites, douts_site):
        if s["kind"] == "act" and torch.is_tensor(s["slope"]) and d is not None:
            neg = torch.where(s["used"], torch.zeros((), dtype=r.dtype), s["bn"].detach())
            k = name_of[id(s["slope"])]
            out[k] = out.get(k, 0.0) + float((d * neg).abs().sum())
    return out


def gaps(rep_a, rep_b):
    """{name: max |a - b| / max |b|} of two reports with the same entries (b: the float64 reference)"""
    assert [e[0] for e in rep_a] == [e[0] for e in rep_b]
    return {n: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300) for (n, _, a), (_, _, b) in zip(rep_a, rep_b)}


def tolerances(gap, rep):
    """{name: MARGIN max(gap, median gap of the report's tensors of the same kind)}, max-normalised"""
    by_kind = {}
    for n, kd, _ in rep:
        by_kind.setdefault(kd, []).append(gap[n])
    med = {kd: float(np.median(v)) for kd, v in by_kind.items()}
    return {n: MARGIN * max(gap[n], med[kd]) for n, kd, _ in rep}


def ratios(rep_got, rep_ref, tol, terms=None):
    """[(name, error / tolerance, error, tolerance)] in the report's order; errors and tolerances absolute.  terms: {slope key:
    sum |terms|} - those entries get SLOPE_CANCEL_F32 of it on top"""
    assert [e[0] for e in rep_got] == [e[0] for e in rep_ref]
    out = []
    for (n, _, a), (_, _, b) in zip(rep_got, rep_ref):
        assert a.shape == b.shape, (n, a.shape, b.shape)
        t = tol[n] * float(b.abs().max())
        if terms and n in terms:
            t += SLOPE_CANCEL_F32 * terms[n]
        e = float((a.double() - b).abs().max())
        out.append((n, e / max(t, 1e-300), e, t))
    return out


def worst(rs):
    return max(rs, key=lambda r: r[1])


def first_bad(rs):
    for r in rs:
        if not r[1] <= 1.0:
            return r
    return None


class Reference(object):
    """what one case needs from the CPU, computed once: the free float64 run, the fp32 restatement, the float64 run with the
    fp32 run's decisions forced, the two dlogits and section "Tolerances" for the saved tensors and for both gradient sets"""

    def __init__(self, case):
        self.case = case
        self.free = run(case, torch.float64)
        self.r32 = run(case, torch.float32)
        self.f32dec = self.r32.tape.decisions()
        self.forced32 = run(case, torch.float64, forced=self.f32dec)
        dl = loss_dlogits(self.free)
        self.douts = [[d.float() for d in dl], [d.float() for d in dense_dlogits(case, dl)]]     # what the device is fed
        self.n_differ32 = sum(int((a != b).sum()) for a, b in zip(self.f32dec, self.free.tape.decisions()))
        self.n_decisions = sum(d.numel() for d in self.f32dec)
        rep64 = saved_report(self.forced32)
        self.saved_gap = gaps(saved_report(self.r32), rep64)
        self.saved_tol = tolerances(self.saved_gap, rep64)
        self.grad_gap, self.grad_tol, self.g32, self.g64, self.site_douts, self.terms = [], [], [], [], [], []
        for d in self.douts:
            g32, _ = grads(self.r32, d)
            g64, ds = grads(self.forced32, d)
            a, b = grad_report(self.r32, g32), grad_report(self.forced32, g64)
            gp = gaps(a, b)
            self.g32.append(a)
            self.g64.append(b)
            self.site_douts.append(ds)
            self.terms.append(slope_terms(self.forced32, ds))
            self.grad_gap.append(gp)
            self.grad_tol.append(tolerances(gp, b))


# ---------------------------------------------------------------------------------------------- the device's saved state
def ncdhw(t, dims):
    """a schedule's NDHWC [voxels, C] view (any strides, any dtype) -> float64 [N, C, D, H, W] on the CPU"""
    n, d, h, w = dims
    return t.detach().float().cpu().contiguous().reshape(n, d, h, w, t.shape[1]).permute(0, 4, 1, 2, 3).double()


def _blocks(sv):
    b = sv.blocks
    return list(b.values()) if isinstance(b, dict) else list(b)


def device_tensors(sv, ref_tape):
    """the saved state of Engine.forward / Schedule3D.forward(keep=True) laid beside a tape's events -> [(event, dict)] with
    the device's conv output and BatchNorm rows / activation / pooled / up-sampled tensor of that event.  Block order is forward
    order in both schedules; the level of a decoder block follows from the number of levels; Engine keeps `sv.pooled`, for
    Schedule3D the next encoder block's input is the pooled tensor"""
    blocks, dims = _blocks(sv), sv.dims
    L = len(dims)
    level = list(range(L)) + list(range(L - 2, -1, -1))
    out, site = [], 0
    for ev in ref_tape.events:
        kd, k = ev["kind"], ev["k"]
        if kd in ("conv", "act"):
            blk, l = blocks[site // 2], level[site // 2]
            first = site % 2 == 0
            if kd == "conv":
                bn = blk["bn1" if first else "bn2"].detach().float().cpu().double()
                out.append((ev, dict(t=ncdhw(blk["y1" if first else "y2"], dims[l]), mean=bn[0], rstd=bn[1])))
            else:
                out.append((ev, dict(t=ncdhw(blk["a1" if first else "out"], dims[l]))))
                site += 1
        elif kd == "pool":
            pooled = sv.pooled[k] if hasattr(sv, "pooled") else blocks[k + 1]["xin"]
            out.append((ev, dict(t=ncdhw(pooled, dims[k + 1]), skip=ncdhw(blocks[k]["out"], dims[k]), pd=dims[k][1] // dims[k + 1][1])))
        elif kd == "up":
            blk, l = blocks[L + k], level[L + k]
            cat = blk["xin"]
            out.append((ev, dict(t=ncdhw(cat[:, cat.shape[1] // 2:], dims[l]))))
    return out


def device_winners(pooled, skip, pd):
    """winner index per window from the pooled tensor and the tensor it was pooled from: the first entry (depth, height, width
    order) equal to the pooled value - first maximum wins; -1 where no entry equals it (the pooled value is not in its window)"""
    return first_true(windows(skip, pd) == pooled.unsqueeze(-1))


def device_decisions(dt):
    """dt: device_tensors(sv, the free float64 tape) -> (decisions aligned with the tape's sites, undecided count, [problems]).  Signs from the stored activations (an exact
    0 takes the free run's decision), winners from pooled-vs-skip (first maximum wins)"""
    dec, undecided, problems = [], 0, []
    for ev, dv in dt:
        if ev["kind"] == "act":
            a = dv["t"]
            zero = a == 0
            undecided += int(zero.sum())
            dec.append(torch.where(zero, ev["dec"], a > 0))
        elif ev["kind"] == "pool":
            w = device_winners(dv["t"], dv["skip"], dv["pd"])
            if int((w < 0).sum()):
                problems.append("pool%d: %d pooled values are not in their window" % (ev["k"], int((w < 0).sum())))
                w = torch.where(w < 0, ev["dec"], w)
            dec.append(w)
    return dec, undecided, problems


def census(dt, dec):
    """dt: device_tensors(sv, the free float64 tape).  Every device decision that differs from the free float64 run's -> (count, [(site, index, margin, site error)] of the ones
    that are NOT near-ties).  The site's error is max |device - float64| of the tensor the decision is taken on (the
    pre-activation, recovered from the stored activation by the site's slope; the tensor that is pooled), over the elements
    whose decisions agree: at a differing element the difference contains the margin itself"""
    n_diff, clear, listing = 0, [], []
    sites = [(ev, dv) for ev, dv in dt if ev["kind"] in ("act", "pool")]
    for i, ((ev, dv), d) in enumerate(zip(sites, dec)):
        diff = d != ev["dec"]
        nd = int(diff.sum())
        if not nd:
            continue
        n_diff += nd
        if ev["kind"] == "act":
            slope = float(ev["slope"].detach()) if torch.is_tensor(ev["slope"]) else float(ev["slope"])
            a = dv["t"]
            z_dev = torch.where(a > 0, a, a / slope)
            err = (z_dev - ev["bn"].detach().double()).abs()
            err = float(err[~diff].max())
        else:
            err = float((dv["skip"] - ev["inp"].detach().double()).abs().max())
        for idx in diff.nonzero().tolist():
            m = float(ev["margin"][tuple(idx)])
            listing.append(("%s%d" % (ev["kind"], ev["k"]), tuple(idx), m, err))
            if not m <= NEAR_TIE * err:
                clear.append(listing[-1])
    return n_diff, clear, listing


def device_saved_report(dt, outs, net_sd, template):
    """dt: device_tensors(sv, a tape of the case) -> the device's tensors under the names and in the order of
    saved_report(template run)"""
    rep, site = [], 0
    for ev, dv in dt:
        kd = ev["kind"]
        if kd == "conv":
            rep.append(("site%02d.conv" % site, "conv", dv["t"]))
            rep.append(("site%02d.mean" % site, "mean", dv["mean"]))
            rep.append(("site%02d.rstd" % site, "rstd", dv["rstd"]))
        elif kd == "act":
            rep.append(("site%02d.act" % site, "act", dv["t"]))
            site += 1
        elif kd == "pool":
            rep.append(("pool%d" % ev["k"], "pool", dv["t"]))
        elif kd == "up":
            rep.append(("up%d" % ev["k"], "up", dv["t"]))
    for i, o in enumerate(outs):
        rep.append(("logits%d" % i, "logits", o.detach().float().cpu().double()))
    for k in template.sd:
        leaf = k.rsplit(".", 1)[1]
        if leaf in ("running_mean", "running_var") and _live_stat(template, k):
            rep.append((k, leaf, net_sd[k].detach().float().cpu().double()))
    return rep
