"""The two backward schedules (fplx/engine.py Engine, fplx/nets3d.py Schedule3D) against float64 with the DEVICE'S OWN decisions.

fp32 precision, train-mode BatchNorm, dropout 0 (the dropout stream has its own test).  Per case:
  1. engine.forward(..., keep=True) on the device;
  2. a free float64 tape (tests/kinkoracle.py) of the same weights and input on the CPU;
  3. census: every LeakyReLU / PReLU sign and pooling winner of the device that differs from the free float64 run must be a
     near-tie (float64 margin <= 64 x the measured max |device - float64| of the tensor the decision is taken on), at most 16 per
     case may differ or be undecided;
  4. every saved tensor (conv outputs, BatchNorm rows, activations, pooled, up-sampled, logits, running statistics) against the
     float64 tape with the device's decisions forced, reported in forward order;
  5. engine.backward(sv, dlogits, gflat) called directly - no loss kernel - with (a) the float64 reference's loss gradient and
     (b) a dense normal draw of the same RMS, against torch.autograd.grad on that forced tape, reported in backward order;
  6. every device pass twice: identical bits.
Tolerances are measured on the reference, never on the device: per tensor 8 x max(gap, median gap of the case's tensors of the
same kind), gap = the fp32 CPU restatement against float64 under the fp32 run's own decisions (kinkoracle.Reference); a PReLU
slope gradient adds SLOPE_CANCEL_F32 of sum |terms|.  DESIGN.md, "Decision-forced float64 oracle", holds the measured ratios.
"""
import functools

import pytest
import torch

import kinkoracle as K

pytestmark = pytest.mark.gpu

CASES = {}
for _n in ("tiny", "tiny25", "tinybl", "tinybl25", "c4"):
    for _d in (0, 1):
        CASES["%s.d%d" % (_n, _d)] = functools.partial(K.dsbn_case, _n, _d)
CASES["u3d4_ds.ds"] = functools.partial(K.n3d_case, "u3d4_ds", True, None, "ce")
CASES["u3d4_ds.plain"] = functools.partial(K.n3d_case, "u3d4_ds", False, None, "ce")
CASES["u25"] = functools.partial(K.n3d_case, "u25")
# the draw nll1 is the one tests/test_gpu_nll.py and tests/test_gpu_ssl2.py avoid: 1.4e-2 against the free restatement
for _draw in ("nll1", "nll2", "nll4"):
    CASES["u3d4_ds.plain.%s" % _draw] = functools.partial(K.n3d_case, "u3d4_ds", False, _draw, "ce")


def _device_pass(case, douts):
    """a fresh network, one forward with the state kept, one backward per dlogits set -> everything on the CPU"""
    import fplx
    p = dict(case.params, precision="fp32")
    net = (fplx.UNet2D5_dsbn if case.family == "dsbn" else fplx.SegNetDict[p["net_type"]])(p)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in case.weights.items()}, strict=True)
    net.cuda().train()
    net._ensure_flat()
    x = case.x.cuda()
    drop_on = list(net.dropout_active())
    assert not any(drop_on)
    if case.family == "dsbn":
        logits, sv = net.engine.forward(x, case.domain, True, drop_on, net.dropout_seed, 0, keep=True)
        outs = [logits]
    else:
        outs, sv = net.engine.forward(x, True, drop_on, net.dropout_seed, 0, True)
    grads = []
    for d in douts:
        gflat = torch.empty_like(net.flat_params)
        dd = [t.cuda() for t in d]
        net.engine.backward(sv, dd[0] if case.family == "dsbn" else dd, gflat)
        torch.cuda.synchronize()
        grads.append({k: v.detach().cpu().clone() for k, v in net.grad_views(gflat).items()})
    return sv, [o.detach().cpu() for o in outs], {k: v.detach().cpu() for k, v in net.state_dict().items()}, grads


def _bits(dt, outs, sd, grads):
    ts = list(outs) + [sd[k] for k in sorted(sd)] + [g[k] for g in grads for k in sorted(g)]
    for _, dv in dt:
        ts += [dv[k] for k in ("t", "mean", "rstd") if k in dv]
    return ts


@functools.lru_cache(maxsize=None)
def reference(name):
    return K.Reference(CASES[name]())


@pytest.mark.parametrize("name", list(CASES))
def test_backward_schedule_against_float64_with_the_devices_decisions(name):
    ref = reference(name)
    case = ref.case
    sv, outs, sd, dgrads = _device_pass(case, ref.douts)
    dt = K.device_tensors(sv, ref.free.tape)
    # ---- 6. determinism
    sv2, outs2, sd2, dgrads2 = _device_pass(case, ref.douts)
    a, b = _bits(dt, outs, sd, dgrads), _bits(K.device_tensors(sv2, ref.free.tape), outs2, sd2, dgrads2)
    same = [torch.equal(s, t) for s, t in zip(a, b)]
    del sv2
    # ---- 3. census
    dec, undecided, problems = K.device_decisions(dt)
    n_diff, clear, listing = K.census(dt, dec)
    print("%s: %d of %d device decisions differ from the free float64 run, %d undecided (the fp32 CPU restatement: %d differ)" % (
        name, n_diff, ref.n_decisions, undecided, ref.n_differ32))
    for site, idx, margin, err in listing[:K.MAX_DIFFERING]:
        print("    %s %s: float64 margin %.3g, site error %.3g" % (site, idx, margin, err))
    # ---- 4. saved tensors, the device's decisions forced
    forced = K.run(case, torch.float64, forced=dec)
    saved = K.ratios(K.device_saved_report(dt, outs, sd, forced), K.saved_report(forced), ref.saved_tol)
    w = K.worst(saved)
    print("%s: saved tensors, worst %s at %.3g of its tolerance (error %.3g)" % (name, w[0], w[1], w[2]))
    # ---- 5. gradients
    grad_rs = []
    for j, d in enumerate(ref.douts):
        g64, ds = K.grads(forced, d)
        rep64 = K.grad_report(forced, g64)
        got = [(k, kd, dgrads[j][k].double()) for k, kd, _ in rep64]
        rs = K.ratios(got, rep64, ref.grad_tol[j], K.slope_terms(forced, ds))
        w = K.worst(rs)
        print("%s: gradients under the %s dlogits, worst %s at %.3g of its tolerance (error %.3g)" % (
            name, ("loss", "dense")[j], w[0], w[1], w[2]))
        grad_rs.append(rs)
        for k in forced.prm:                               # conv bias in front of train-mode BatchNorm: exactly 0
            if K.is_bn_fed_bias(k):
                assert float(dgrads[j][k].abs().max()) == 0.0, k
            elif g64[k] is None:                            # the other domain's BatchNorm
                assert float(dgrads[j][k].abs().max()) == 0.0, k
    if n_diff:           # what the differing decisions alone cost: the same device gradients against float64 deciding for itself
        gfree, _ = K.grads(ref.free, ref.douts[0])
        repf = K.grad_report(ref.free, gfree)
        gp = K.gaps([(k, kd, dgrads[0][k].double()) for k, kd, _ in repf], repf)
        wk = max(gp, key=gp.get)
        print("%s: gradients under the loss dlogits against the FREE float64 run, worst %s at %.3g of its maximum" % (name, wk, gp[wk]))
    assert all(same), "two passes differ in %d of %d tensors" % (same.count(False), len(same))
    assert not problems, problems
    assert not clear, "decisions that differ with a clear margin (site, index, float64 margin, site error): %s" % clear[:8]
    assert n_diff + undecided <= K.MAX_DIFFERING, (n_diff, undecided)
    bad = K.first_bad(saved)
    assert bad is None, "first saved tensor out of bound in forward order (name, error / tolerance, error, tolerance): %s" % (bad,)
    for j, rs in enumerate(grad_rs):
        bad = K.first_bad(rs)
        assert bad is None, "%s dlogits: first gradient out of bound in backward order (name, error / tolerance, error, " \
            "tolerance): %s" % (("loss", "dense")[j], bad)
