"""Oracles for seven of the eight optimiser kinds of fplx_optim_step (SGD, Adadelta, Adagrad, Adamax, ASGD, RMSprop, Rprop; the
eighth, Adam, has lossoracle.adam_ref and the recorded bits of tests/golden/adam_parent_digest.json), in the manner of adam_ref: one step from fp32 state, evaluated in float64, with a per-element bound for every output.

Conventions.  u = U = 2^-24: one correctly rounded fp32 operation (+, x, /, sqrt, fma) errs by at most u |result|; ETA = 2^-126
covers a result in the denormal range.  Hyper-parameters are taken as the floats that cross the C ABI (`f32`): the rounding of a
hyper-parameter changes the hyper-parameter, it is not an arithmetic error, and the tests hand torch the same rounded values.
A scalar the host forms in double and rounds once (1 - rho, Adagrad's and Adamax's step size, ASGD's 1 - lambd eta) is evaluated
the same way here and then rounded with f32: kernel, torch and oracle hold the same number.  Every bound below holds for BOTH
orders of evaluation that occur: torch's (separate roundings, addcmul / addcdiv / lerp, (value * a) / b) and the kernel's (fma,
value * (a / b)); E_x is the bound of x, capitals are sums of absolute values.

  gi = wd p + g gs          Gi = |wd p| + |g gs|;  E_gi = 2 u Gi    (product g gs, product wd p, the sum: each <= u Gi ... 2 u Gi
                            covers the fma form and torch's two-step form; gs is a power of two in the tests, so g gs is exact)
  SGD       b' = mom b + gi     E_b = E_gi + 2 u (|mom b| + Gi)                    (product, sum)
            p' = p - lr x       E_p = lr E_x + 2 u |lr x| + u |p|   + u |p'|       (x = b' or gi; product, sum)
  Adagrad   s' = s + gi^2       E_s = 2 Gi E_gi + 2 u (s + Gi^2) + ETA
            std = sqrt(s') + eps    E_sq = min(E_s / (2 sqrt s'), sqrt E_s) + u sqrt s';  E_std = E_sq + u std
            q = gi / std        E_q = E_gi / std + |gi| E_std / std^2 + u |q|
            p' = p - clr q      E_p = clr E_q + 3 u |clr q| + u (|p| + |clr q|)     (clr's own rounding, product, the other order)
  RMSprop   s' = a s + (1 - a) gi^2     E_s = (1 - a) 2 Gi E_gi + 3 u (a |s| + (1 - a) Gi^2) + ETA    (as Adam's v')
            avg = sqrt(s') + eps, q = gi / avg as Adagrad's;  momentum: b' = mom b + q, E_b = E_q + 2 u (|mom b| + |q|);
            p' = p - lr x as SGD's with x = b' or q
  Adadelta  s' as RMSprop's with rho;  v = s' + eps: E_v = E_s + u v;  std = sqrt v: E_std = min(E_v / (2 std), sqrt E_v) + u std
            a = acc + eps: E_a = u a;  dl = sqrt a: E_dl = E_a / (2 dl) + u dl       (a >= eps > 0)
            r = dl / std: E_r = E_dl / std + dl E_std / std^2 + u r;  delta = r gi: E_d = E_r |gi| + r E_gi + u |delta|
            acc' = rho acc + (1 - rho) delta^2: E_acc = (1 - rho) 2 |delta| E_d + 3 u (rho |acc| + (1 - rho) delta^2) + ETA
            p' = p - lr delta as SGD's
  Adamax    m' = b1 m + (1 - b1) gi     E_m = (1 - b1) E_gi + 4 u (|b1 m| + (1 - b1) Gi)     (torch: lerp, m + w (gi - m))
            t' = max(b2 t, |gi| + eps)  E_t = max(u b2 |t|, E_gi + u (|gi| + eps))           (max is 1-Lipschitz in each argument)
            q = m' / t': E_q = E_m / t' + |m'| E_t / t'^2 + u |q|;  p' = p - clr q as Adagrad's
  ASGD      d = f32(1 - lambd eta);  t = p d: E_t = u |t|;  p' = t - eta gi: E_p = E_t + eta E_gi + 2 u |eta gi| + u (|t| + |p'|)
            ax' = p' if mu == 1 else ax + (p' - ax) mu: E_ax = mu E_p + 2 u mu (|p'| + |ax|) + u |ax'|     (mu == 1: E_p)
  Every E is multiplied by GAMMA_SLACK = 1.01 (products of errors, all below 1e-3 relative) and gets + ETA.

Rprop has no bound: sign(g prev) of ONE fp32 product, one product by etaminus / etaplus / 1, a clamp, one fma whose product
(+-1 or 0 times step_size) is exact - every operation is a single correctly rounded fp32 operation and nothing can contract,
so `optim_f32` (the step op by op in numpy float32) IS the result, bit for bit.  `optim_f32` evaluates the other kinds the same
way, in torch's order without fma: on the exact data (`exact_case`) those results are determined as well, see there.

Mutations (`mut=`) for tests/test_optim_oracle_cpu.py: each one is a plausible wrong reading of torch's step that the bound must
reject.  Pure numpy / torch on the CPU."""
import zlib

import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -126
GAMMA_SLACK = 1.01
KINDS = ("SGD", "Adadelta", "Adagrad", "Adamax", "ASGD", "RMSprop", "Rprop")
NSTATE = {"SGD": 1, "Adadelta": 2, "Adagrad": 1, "Adamax": 2, "ASGD": 1, "RMSprop": 2, "Rprop": 2}      # at most
STATE_KEYS = {"SGD": ("momentum_buffer",), "Adadelta": ("square_avg", "acc_delta"), "Adagrad": ("sum",),
              "Adamax": ("exp_avg", "exp_inf"), "ASGD": ("ax",), "RMSprop": ("square_avg", "momentum_buffer"),
              "Rprop": ("prev", "step_size")}
MUTATIONS = {
    "SGD": ("wd_dropped", "wd_decoupled", "gs_after_decay", "state_zero"),
    "Adadelta": ("wd_dropped", "wd_decoupled", "gs_after_decay", "state_zero", "eps_outside"),
    "Adagrad": ("wd_dropped", "wd_decoupled", "gs_after_decay", "state_zero"),
    "Adamax": ("wd_dropped", "wd_decoupled", "gs_after_decay", "state_zero", "no_bias_correction", "max_no_decay"),
    "ASGD": ("wd_dropped", "wd_decoupled", "gs_after_decay", "state_zero", "eta_early"),
    "RMSprop": ("wd_dropped", "wd_decoupled", "gs_after_decay", "state_zero", "eps_inside"),
    "Rprop": ("state_zero", "no_zero_on_flip"),
}


def rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


def f32(x):
    return float(np.float32(x))


def ratio(got, ref, bound):
    """max |got - ref| / bound (NaN / inf -> inf; 0 / 0 -> 0): <= 1 passes"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    q = np.where(np.isfinite(got) & ~np.isnan(q), q, np.inf)
    return float(q.max())


def n_state(kind, hp):
    """state streams the kind touches with these hyper-parameters (fplx_optim_step's rule)"""
    if kind == "SGD":
        return 1 if f32(hp[1]) != 0 else 0
    if kind == "RMSprop":
        return 2 if f32(hp[3]) > 0 else 1
    return NSTATE[kind]


def asgd_scalars(lr, lambd, alpha, t0, step):
    """(eta, mu) that ASGD's step number `step` (1-based) uses: torch forms them after step - 1 and keeps them in float32"""
    if step <= 1:
        return f32(lr), 1.0
    s = step - 1
    return f32(lr / ((1 + lambd * lr * s) ** alpha)), f32(1 / max(1, s - t0))


def _sqrt_err(v, e_v):
    sq = np.sqrt(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return sq, np.minimum(np.where(sq > 0, e_v / (2 * sq), np.inf), np.sqrt(e_v)) + U * sq


def _descend(p, lr, x, e_x):
    """p' = p - lr x and its bound (product, sum, either order)"""
    upd = lr * x
    p2 = p - upd
    return p2, lr * e_x + 2 * U * np.abs(upd) + U * np.abs(p) + U * np.abs(p2)


def _fin(e, val):
    return None if e is None else GAMMA_SLACK * e + ETA


def optim_ref(kind, p, g, s0, s1, hp, step, gscale=1.0, mut=None, eta_next=None):
    """one step of `kind` in float64 from fp32 state -> (p', s0', s1', bound p', bound s0', bound s1'); None for a stream the
    kind does not have.  hp: the kind's hyper-parameters in fplx_optim_step's order.  eta_next: for mut = 'eta_early'."""
    hp = [f32(x) for x in hp]
    gscale = f32(gscale)
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    ns = n_state(kind, hp)
    z = np.zeros_like(p)
    a = np.asarray(s0, np.float64) if ns > 0 else None
    b = np.asarray(s1, np.float64) if ns > 1 else None
    if mut == "state_zero":
        a = None if a is None else z
        b = None if b is None else z
    wd = {"SGD": 2, "Adadelta": 3, "Adagrad": 3, "Adamax": 4, "ASGD": 3, "RMSprop": 4}.get(kind)
    wd = hp[wd] if wd is not None else 0.0
    gi = wd * p + g * gscale
    Gi = np.abs(wd * p) + np.abs(g * gscale)
    if mut in ("wd_dropped", "wd_decoupled"):
        gi, Gi = g * gscale, np.abs(g * gscale)
    if mut == "gs_after_decay":
        gi = (wd * p + g) * gscale
    e_gi = 2 * U * Gi
    decoupled = (lambda p2, lr: p2 - lr * wd * p) if mut == "wd_decoupled" else (lambda p2, lr: p2)
    if kind == "SGD":
        lr, mom = hp[0], hp[1]
        if ns:
            b2 = mom * a + gi
            e_b = e_gi + 2 * U * (np.abs(mom * a) + Gi)
            p2, e_p = _descend(p, lr, b2, e_b)
            return decoupled(p2, lr), b2, None, _fin(e_p, p2), _fin(e_b, b2), None
        p2, e_p = _descend(p, lr, gi, e_gi)
        return decoupled(p2, lr), None, None, _fin(e_p, p2), None, None
    if kind == "Adagrad":
        clr = f32(hp[0] / (1.0 + (step - 1) * hp[1]))
        eps = hp[2]
        s2 = a + gi * gi
        e_s = 2 * Gi * e_gi + 2 * U * (np.abs(a) + Gi * Gi) + ETA
        sq, e_sq = _sqrt_err(s2, e_s)
        std = sq + eps
        e_std = e_sq + U * std
        q = gi / std
        e_q = e_gi / std + np.abs(gi) * e_std / (std * std) + U * np.abs(q)
        p2, e_p = _descend(p, clr, q, e_q)
        e_p = e_p + U * np.abs(clr * q)
        return decoupled(p2, clr), s2, None, _fin(e_p, p2), _fin(e_s + U * np.abs(s2), s2), None
    if kind == "RMSprop":
        lr, al, eps, mom = hp[0], hp[1], hp[2], hp[3]
        oma = f32(1.0 - al)
        s2 = al * a + oma * gi * gi
        e_s = oma * 2 * Gi * e_gi + 3 * U * (al * np.abs(a) + oma * Gi * Gi) + ETA
        if mut == "eps_inside":
            avg = np.sqrt(s2 + eps)
            e_avg = np.zeros_like(avg)
        else:
            sq, e_sq = _sqrt_err(s2, e_s)
            avg = sq + eps
            e_avg = e_sq + U * avg
        q = gi / avg
        e_q = e_gi / avg + np.abs(gi) * e_avg / (avg * avg) + U * np.abs(q)
        if ns > 1:
            b2 = mom * b + q
            e_b = e_q + 2 * U * (np.abs(mom * b) + np.abs(q))
            p2, e_p = _descend(p, lr, b2, e_b)
            return decoupled(p2, lr), s2, b2, _fin(e_p, p2), _fin(e_s + U * np.abs(s2), s2), _fin(e_b, b2)
        p2, e_p = _descend(p, lr, q, e_q)
        e_p = e_p + U * np.abs(lr * q)
        return decoupled(p2, lr), s2, None, _fin(e_p, p2), _fin(e_s + U * np.abs(s2), s2), None
    if kind == "Adadelta":
        lr, rho, eps = hp[0], hp[1], hp[2]
        omr = f32(1.0 - rho)
        s2 = rho * a + omr * gi * gi
        e_s = omr * 2 * Gi * e_gi + 3 * U * (rho * np.abs(a) + omr * Gi * Gi) + ETA
        if mut == "eps_outside":
            std, e_std = np.sqrt(s2) + eps, 0.0
            dl, e_dl = np.sqrt(b) + eps, 0.0
        else:
            v = s2 + eps
            std, e_std = _sqrt_err(v, e_s + U * v)
            aa = b + eps
            dl = np.sqrt(aa)
            e_dl = U * aa / (2 * dl) + U * dl
        r = dl / std
        e_r = e_dl / std + dl * e_std / (std * std) + U * r
        delta = r * gi
        e_d = e_r * np.abs(gi) + r * e_gi + U * np.abs(delta)
        acc2 = rho * b + omr * delta * delta
        e_acc = omr * 2 * np.abs(delta) * e_d + 3 * U * (rho * np.abs(b) + omr * delta * delta) + ETA
        p2, e_p = _descend(p, lr, delta, e_d)
        return decoupled(p2, lr), s2, acc2, _fin(e_p, p2), _fin(e_s + U * np.abs(s2), s2), _fin(e_acc + U * np.abs(acc2), acc2)
    if kind == "Adamax":
        lr, b1, bt2, eps = hp[0], hp[1], hp[2], hp[3]
        omb1 = f32(1.0 - b1)
        clr = f32(hp[0] / (1.0 - b1 ** step))
        if mut == "no_bias_correction":
            clr = lr
        m2 = b1 * a + omb1 * gi
        e_m = omb1 * e_gi + 4 * U * (np.abs(b1 * a) + omb1 * Gi)
        dec = b if mut == "max_no_decay" else bt2 * b
        t2 = np.maximum(dec, np.abs(gi) + eps)
        e_t = np.maximum(U * np.abs(bt2 * b), e_gi + U * (np.abs(gi) + eps))
        q = m2 / t2
        e_q = e_m / t2 + np.abs(m2) * e_t / (t2 * t2) + U * np.abs(q)
        p2, e_p = _descend(p, clr, q, e_q)
        e_p = e_p + U * np.abs(clr * q)
        return decoupled(p2, clr), m2, t2, _fin(e_p, p2), _fin(e_m + U * np.abs(m2), m2), _fin(e_t + U * np.abs(t2), t2)
    if kind == "ASGD":
        eta, mu, lambd = hp[0], hp[1], hp[2]
        if mut == "eta_early":
            eta = f32(eta_next)
        d = f32(1.0 - lambd * eta)
        t = p * d
        e_t = U * np.abs(t)
        p2 = t - eta * gi
        e_p = e_t + eta * e_gi + 2 * U * np.abs(eta * gi) + U * (np.abs(t) + np.abs(p2))
        if mu == 1.0:
            ax2, e_ax = p2, e_p
        else:
            ax2 = a + (p2 - a) * mu
            e_ax = mu * e_p + 2 * U * mu * (np.abs(p2) + np.abs(a)) + U * np.abs(ax2)
        return decoupled(p2, eta), ax2, None, _fin(e_p, p2), _fin(e_ax, ax2), None
    raise ValueError("optim_ref: %s has no float64 oracle (Rprop: optim_f32, bitwise)" % kind)


def optim_f32(kind, p, g, s0, s1, hp, step, gscale=1.0, mut=None):
    """the step op by op in numpy float32, torch's order, no fma -> (p', s0', s1') as float32 arrays.  Rprop's oracle on any
    data; the exact oracle of the other kinds on `exact_case` data (where every order gives the same bits)."""
    F = np.float32
    hp = [F(x) for x in hp]
    p, g = np.asarray(p, F), np.asarray(g, F) * F(gscale)
    ns = n_state(kind, hp)
    a = np.asarray(s0, F) if ns > 0 else None
    b = np.asarray(s1, F) if ns > 1 else None
    if mut == "state_zero":
        a, b = np.zeros_like(p), np.zeros_like(p)
        if kind == "Rprop":
            b = np.full_like(p, hp[0])
    if kind == "Rprop":
        lr, etam, etap, smin, smax = hp
        if step == 1:
            a, b = np.zeros_like(p), np.full_like(p, lr)
        s = g * a
        f = np.where(s > 0, etap, np.where(s < 0, etam, F(1))).astype(F)
        b2 = np.minimum(np.maximum(b * f, smin), smax).astype(F)
        gz = g if mut == "no_zero_on_flip" else np.where(s < 0, F(0), g).astype(F)
        p2 = (p - np.sign(gz).astype(F) * b2).astype(F)
        return p2, gz, b2
    wd = {"SGD": 2, "Adadelta": 3, "Adagrad": 3, "Adamax": 4, "ASGD": 3, "RMSprop": 4}[kind]
    gi = (g + hp[wd] * p).astype(F) if hp[wd] != 0 else g
    if kind == "SGD":
        lr, mom = hp[0], hp[1]
        if ns:
            a = (mom * a + gi).astype(F)
            return (p - lr * a).astype(F), a, None
        return (p - lr * gi).astype(F), None, None
    if kind == "Adagrad":
        clr = F(float(hp[0]) / (1.0 + (step - 1) * float(hp[1])))
        a = (a + gi * gi).astype(F)
        std = (np.sqrt(a) + hp[2]).astype(F)
        return (p - clr * (gi / std)).astype(F), a, None
    if kind == "RMSprop":
        lr, al, eps, mom = hp[0], hp[1], hp[2], hp[3]
        oma = F(1.0 - float(al))
        a = (al * a + oma * gi * gi).astype(F)
        avg = (np.sqrt(a) + eps).astype(F)
        if ns > 1:
            b = (mom * b + gi / avg).astype(F)
            return (p - lr * b).astype(F), a, b
        return (p - lr * (gi / avg)).astype(F), a, None
    if kind == "Adadelta":
        lr, rho, eps = hp[0], hp[1], hp[2]
        omr = F(1.0 - float(rho))
        a = (rho * a + omr * gi * gi).astype(F)
        std = np.sqrt(a + eps).astype(F)
        delta = (np.sqrt(b + eps).astype(F) / std * gi).astype(F)
        b = (rho * b + omr * delta * delta).astype(F)
        return (p - lr * delta).astype(F), a, b
    if kind == "Adamax":
        lr, b1, bt2, eps = hp[0], hp[1], hp[2], hp[3]
        omb1 = F(1.0 - float(b1))
        clr = F(float(lr) / (1.0 - float(b1) ** step))
        a = (b1 * a + omb1 * gi).astype(F)
        b = np.maximum(bt2 * b, np.abs(gi) + eps).astype(F)
        return (p - clr * (a / b)).astype(F), a, b
    if kind == "ASGD":
        eta, mu, lambd = hp[0], hp[1], hp[2]
        d = F(1.0 - float(lambd) * float(eta))
        p2 = ((p * d).astype(F) - eta * gi).astype(F)
        a = p2.copy() if mu == 1 else (a + (p2 - a) * mu).astype(F)
        return p2, a, None
    raise ValueError(kind)


# ---------------------------------------------------------------- torch side (CPU, fp32, foreach=False)

def torch_optimizer(kind, p, hp_named, state=None, step=0):
    """torch.optim.<kind>([p]) in fp32 with the named hyper-parameters; `state`: {torch key: numpy array} to start from, with
    `step` steps behind it.  -> (optimizer, parameter)"""
    import torch
    prm = torch.nn.Parameter(torch.from_numpy(np.array(p, np.float32)))
    opt = getattr(torch.optim, kind)([prm], foreach=False, **hp_named)
    if state is not None:
        st = {k: torch.from_numpy(np.array(v, np.float32)) for k, v in state.items()}
        if kind != "SGD":
            st["step"] = torch.tensor(float(step))
        if kind == "ASGD":
            eta, mu = asgd_scalars(hp_named["lr"], hp_named["lambd"], hp_named["alpha"], hp_named["t0"], step + 1)
            st["eta"], st["mu"] = torch.tensor(eta), torch.tensor(mu)
        opt.state[prm] = st
    return opt, prm


def torch_state(kind, opt, prm, ns):
    """the optimiser's state streams as numpy float32, in the kernel's order"""
    st = opt.state[prm] if prm in opt.state else {}
    out = [st[k].detach().numpy().copy() if k in st else None for k in STATE_KEYS[kind][:ns]]
    return out + [None] * (2 - len(out))


def named_hp(kind, lr, wd=0.0, momentum=0.0, **over):
    """torch's keyword arguments for `kind` as get_optimizer would build it (lr, momentum, weight_decay; the rest torch's
    defaults unless overridden), every float rounded to fp32 - the value that crosses the C ABI"""
    d = {"SGD": dict(lr=lr, momentum=momentum, weight_decay=wd),
         "Adadelta": dict(lr=lr, rho=0.9, eps=1e-6, weight_decay=wd),
         "Adagrad": dict(lr=lr, lr_decay=0.0, eps=1e-10, weight_decay=wd),
         "Adamax": dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd),
         "ASGD": dict(lr=lr, lambd=1e-4, alpha=0.75, t0=1e6, weight_decay=wd),
         "RMSprop": dict(lr=lr, alpha=0.99, eps=1e-8, momentum=momentum, weight_decay=wd),
         "Rprop": dict(lr=lr, etas=(0.5, 1.2), step_sizes=(1e-6, 50.0))}[kind]
    d.update(over)
    return {k: (tuple(f32(x) for x in v) if isinstance(v, tuple) else f32(v)) for k, v in d.items()}


def abi_hp(kind, h, step=1):
    """named hyper-parameters -> fplx_optim_step's hp array for step number `step` (ASGD: the eta / mu of that step)"""
    if kind == "SGD":
        return (h["lr"], h["momentum"], h["weight_decay"])
    if kind == "Adadelta":
        return (h["lr"], h["rho"], h["eps"], h["weight_decay"])
    if kind == "Adagrad":
        return (h["lr"], h["lr_decay"], h["eps"], h["weight_decay"])
    if kind == "Adamax":
        return (h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"])
    if kind == "ASGD":
        eta, mu = asgd_scalars(h["lr"], h["lambd"], h["alpha"], h["t0"], step)
        return (eta, mu, h["lambd"], h["weight_decay"])
    if kind == "RMSprop":
        return (h["lr"], h["alpha"], h["eps"], h["momentum"], h["weight_decay"])
    return (h["lr"],) + tuple(h["etas"]) + tuple(h["step_sizes"])


# ---------------------------------------------------------------- data

def variants(kind):
    """(weight decay, momentum) pairs: wd in {0, 1e-5} where the kind has it, momentum in {0, 0.9} where it exists"""
    wds = (0.0,) if kind == "Rprop" else (0.0, 1e-5)
    moms = (0.0, 0.9) if kind in ("SGD", "RMSprop") else (0.0,)
    return [(wd, mom) for wd in wds for mom in moms]


def random_case(kind, n, wd, momentum, late, gscale=1.0):
    """the random data of both test files: p ~ N(0, 1); gradients N(0, 1) 10^k, k drawn per step from -6..0 (as the Adam test's);
    late = False: five steps from zero state; late = True: steps 1000 and 1001 from a state as it is late in training
    (ASGD then with t0 = 500, so that mu != 1).  -> dict(h named hyper-parameters, p, state [s0, s1], steps, grads)"""
    g = rng("optim.%s.%d.%g.%g.%d.%g" % (kind, n, wd, momentum, late, gscale))
    lr = {"Adadelta": 1.0, "Rprop": 1e-2, "Adagrad": 1e-2, "ASGD": 1e-2}.get(kind, 1e-3)
    h = named_hp(kind, lr, wd, momentum, **({"t0": 500.0} if kind == "ASGD" and late else {}))
    p = g.standard_normal(n).astype(np.float32)
    st = [np.zeros(n, np.float32), np.zeros(n, np.float32)]
    if kind == "Rprop":
        st[1] = np.full(n, h["lr"], np.float32)
    if late:
        nrm = lambda s: (g.standard_normal(n) * s).astype(np.float32)
        uni = lambda s: (g.random(n) * s).astype(np.float32)
        st = {"SGD": [nrm(1e-2), None], "Adadelta": [uni(1e-4), uni(1e-6)], "Adagrad": [uni(1e-1), None],
              "Adamax": [nrm(1e-2), uni(1e-2) + np.float32(1e-6)], "ASGD": [p + nrm(1e-3), None],
              "RMSprop": [uni(1e-4), nrm(1e-1)],
              "Rprop": [nrm(1e-3), (np.float32(h["lr"]) * 2.0 ** g.integers(-3, 4, n)).astype(np.float32)]}[kind]
        st = [np.zeros(n, np.float32) if s is None else s for s in st]
    steps = (1000, 1001) if late else (1, 2, 3, 4, 5)
    grads = [(g.standard_normal(n) * 10.0 ** g.integers(-6, 1)).astype(np.float32) for _ in steps]
    return dict(h=h, p=p, state=st, steps=steps, grads=grads, gscale=gscale)


EXACT_STEPS = {("SGD", 0.5): 3, ("SGD", 0.0): 3, ("Rprop", 0.0): 3, ("ASGD", 0.0): 1, ("Adagrad", 0.0): 1, ("RMSprop", 0.5): 1,
               ("RMSprop", 0.0): 1, ("Adamax", 0.0): 1, ("Adadelta", 0.0): 1}


def exact_case(kind, n, momentum=0.0):
    """exact data: p signed multiples of 1/8 in [1/8, 4], g signed multiples of 1/8 in [1/8, 2], every hyper-parameter a power
    of two (or 0.5 / 0.75): lr 2^-3, wd 2^-4, eps 2^-10, momentum 0.5, alpha = rho = 0.75, betas (0.5, 0.75); ASGD lambd 2^-4,
    alpha 1, t0 1; Rprop etas (0.5, 2), step sizes (2^-6, 0.25).  From zero state SGD and Rprop are determined for three steps
    (all operands and results are short dyadic numbers), ASGD for one (its second eta is not dyadic), the others for the first
    step: exact operands up to one or two correctly rounded operations, every later product by a power of two - contraction
    cannot change a bit.  EXACT_STEPS lists the counts."""
    g = rng("optim.exact.%s.%d.%g" % (kind, n, momentum))
    sgn = lambda: np.where(g.random(n) < 0.5, -1.0, 1.0)
    p = (g.integers(1, 33, n) / 8.0 * sgn()).astype(np.float32)
    steps = tuple(range(1, EXACT_STEPS[(kind, momentum)] + 1))
    grads = [(g.integers(1, 17, n) / 8.0 * sgn()).astype(np.float32) for _ in steps]
    over = {"SGD": {}, "Adadelta": dict(rho=0.75, eps=2.0 ** -10), "Adagrad": dict(eps=2.0 ** -10),
            "Adamax": dict(betas=(0.5, 0.75), eps=2.0 ** -10), "ASGD": dict(lambd=2.0 ** -4, alpha=1.0, t0=1.0),
            "RMSprop": dict(alpha=0.75, eps=2.0 ** -10), "Rprop": dict(etas=(0.5, 2.0), step_sizes=(2.0 ** -6, 0.25))}[kind]
    h = named_hp(kind, 2.0 ** -3, 2.0 ** -4, momentum, **over)
    st = [np.zeros(n, np.float32), np.full(n, h["lr"], np.float32) if kind == "Rprop" else np.zeros(n, np.float32)]
    return dict(h=h, p=p, state=st, steps=steps, grads=grads, gscale=1.0)


def torch_sqrt_misrounded(kind, case):
    """elements of an exact case on which the installed torch's CPU float32 sqrt is NOT the correctly rounded one.  Only
    Adadelta takes the square root of an inexact operand on the exact data (v = rho * 0 + (1 - rho) gi^2 + eps, itself exact);
    torch's CPU sqrt goes through a vector math library whose result is within one ulp, not correctly rounded, and picks the
    wrong neighbour where sqrt(v) lies next to a rounding boundary (torch 2.10: 78 of 10007 elements on the library's AVX512
    path of one host, 1566 on another AVX512 host, none on its AVX2 path, 1554 on its SSE4.2 path, each one ulp off; it dispatches on the CPU, so the set is measured
    where the test runs);
    numpy's sqrt and the GPU's sqrtf are correctly rounded (numpy's checked here against float64).  On those elements std, hence
    delta, p and acc_delta, carry torch's own rounding fault, not a property of the step: the exact tests compare torch there
    with nothing, and the kernel with optim_f32 everywhere.  -> boolean mask (all False for the other kinds)"""
    import torch
    n = case["p"].size
    if kind != "Adadelta":
        return np.zeros(n, bool)
    F = np.float32
    h = case["h"]
    gi = (case["grads"][0] + F(h["weight_decay"]) * case["p"]).astype(F)
    v = (F(1.0 - h["rho"]) * gi * gi + F(h["eps"])).astype(F)
    good = np.sqrt(v)
    exact = np.sqrt(v.astype(np.float64))
    assert np.all(np.abs(good.astype(np.float64) - exact) <= np.abs(np.nextafter(good, F(np.inf)).astype(np.float64) - exact))
    assert np.all(np.abs(good.astype(np.float64) - exact) <= np.abs(np.nextafter(good, F(-np.inf)).astype(np.float64) - exact))
    return torch.from_numpy(v).sqrt().numpy() != good


def run_torch(kind, case):
    """torch.optim.<kind> (fp32, CPU, foreach=False) over the case's steps -> [(p, s0, s1) after each step] as numpy float32"""
    import torch
    h, ns = case["h"], n_state(kind, abi_hp(kind, case["h"]))
    late = case["steps"][0] > 1
    state = None
    if late:
        state = {k: s for k, s in zip(STATE_KEYS[kind][:ns], case["state"])}
    opt, prm = torch_optimizer(kind, case["p"], h, state, case["steps"][0] - 1)
    out = []
    for gr in case["grads"]:
        prm.grad = torch.from_numpy((gr * np.float32(case["gscale"])).astype(np.float32))
        opt.step()
        out.append(tuple([prm.detach().numpy().copy()] + torch_state(kind, opt, prm, ns)))
    return out


def check_steps(kind, case, results):
    """results: [(p, s0, s1) after each of the case's steps] of an implementation that started from the case's state ->
    {output: worst ratio}; every step is judged from the implementation's OWN state before it.  Rprop: 0 if bitwise equal to
    optim_f32, else inf."""
    ns = n_state(kind, abi_hp(kind, case["h"]))
    prev = (case["p"], case["state"][0], case["state"][1])
    worst = {}
    for step, gr, got in zip(case["steps"], case["grads"], results):
        hp = abi_hp(kind, case["h"], step)
        if kind == "Rprop":
            ref = optim_f32(kind, prev[0], gr, prev[1], prev[2], hp, step, case["gscale"])
            res = {k: 0.0 if np.array_equal(np.asarray(a, np.float32), b) else np.inf for k, a, b in zip(("p", "s0", "s1"), got, ref)}
        else:
            r = optim_ref(kind, prev[0], gr, prev[1], prev[2], hp, step, case["gscale"])
            res = {k: ratio(got[i], r[i], r[3 + i]) for i, k in enumerate(("p", "s0", "s1")[:1 + ns])}
        for k, x in res.items():
            worst[k] = max(worst.get(k, 0.0), x)
        prev = tuple(got[:1 + ns]) + (None,) * (2 - ns)
    return worst
