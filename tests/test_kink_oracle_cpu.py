"""The decision tape (tests/kinkoracle.py) without a GPU: a free tape changes nothing, forcing a run's own decisions changes
nothing, the fp32 restatement agrees with a float64 run that takes ITS decisions to round-off, and the tolerance the GPU test
(tests/test_gpu_net_backward_exact.py) derives from that agreement rejects four kinds of wrong backward by a factor of 10."""
import functools

import pytest
import torch

import kinkoracle as K

CASES = {}
for _n in ("tiny", "tiny25", "tinybl25"):
    for _d in (0, 1):
        CASES["%s.d%d" % (_n, _d)] = functools.partial(K.dsbn_case, _n, _d)
for _draw in (None, "nll1", "nll4"):
    CASES["u3d4_ds.plain.%s" % (_draw or "fixture")] = functools.partial(K.n3d_case, "u3d4_ds", False, _draw, "ce")
CASES["u3d4_ds.ds"] = functools.partial(K.n3d_case, "u3d4_ds", True, None, "ce")        # mutant (b) needs the heads
TABLE_CASES = [k for k in CASES if k != "u3d4_ds.ds"]
# a forced gap above this would make the derived tolerance no tighter than the 1e-3 floor of the tests it is to sharpen.  A PReLU
# slope gradient is a cancelling sum over a whole tensor: its gap is taken relative to sum |terms|, the scale of its round-off
FORCED_GAP_MAX = 1e-3 / K.MARGIN


def _forced_gap_ok(ref, j):
    for (n, kind, a), (_, _, b) in zip(ref.g32[j], ref.g64[j]):
        scale = ref.terms[j][n] if kind == "slope" else float(b.abs().max())
        assert float((a - b).abs().max()) <= FORCED_GAP_MAX * scale, (n, float((a - b).abs().max()), scale)


@functools.lru_cache(maxsize=None)
def reference(name):
    return K.Reference(CASES[name]())


def _same(ga, gb):
    return all((ga[k] is None and gb[k] is None) or torch.equal(ga[k], gb[k]) for k in ga)


@pytest.mark.parametrize("name", TABLE_CASES)
def test_a_free_tape_and_a_runs_own_decisions_change_no_bit(name):
    ref = reference(name)
    case, free = ref.case, ref.free
    plain = K.run(case, torch.float64, taped=False)
    own = K.run(case, torch.float64, forced=free.tape.decisions())
    for r in (plain, own):
        assert all(torch.equal(a, b) for a, b in zip(r.outs, free.outs))
        assert all(torch.equal(r.sd[k], free.sd[k]) for k in free.sd)
    for d in ref.douts:
        gf, _ = K.grads(free, d)
        assert _same(K.grads(plain, d)[0], gf) and _same(K.grads(own, d)[0], gf)
    # the fp32 restatement too: its taped run is the untaped one
    p32 = K.run(case, torch.float32, taped=False)
    assert all(torch.equal(a, b) for a, b in zip(p32.outs, ref.r32.outs))
    assert _same(K.grads(p32, ref.douts[0])[0], K.grads(ref.r32, ref.douts[0])[0])


@pytest.mark.parametrize("name", TABLE_CASES)
def test_fp32_restatement_agrees_with_float64_under_its_own_decisions(name):
    """free / forced table: the worst max-normalised parameter-gradient gap of the fp32 restatement against float64 deciding for
    itself, and against float64 taking the fp32 run's decisions.  No flip is asserted: flips depend on the host's summation
    order.  Where no decision differs, free and forced are the same run."""
    ref = reference(name)
    for j, d in enumerate(ref.douts):
        gfree, _ = K.grads(ref.free, d)
        free_rep = K.grad_report(ref.free, gfree)
        free_gap = K.gaps(ref.g32[j], free_rep)
        wf, wg = max(free_gap, key=free_gap.get), max(ref.grad_gap[j], key=ref.grad_gap[j].get)
        print("%-24s %-6s free %.3g (%s)  forced %.3g (%s)  differing decisions %d of %d" % (
            name, ("loss", "dense")[j], free_gap[wf], wf, ref.grad_gap[j][wg], wg, ref.n_differ32, ref.n_decisions))
        rs = K.ratios(ref.g32[j], ref.g64[j], ref.grad_tol[j], ref.terms[j])
        assert K.first_bad(rs) is None, K.first_bad(rs)
        _forced_gap_ok(ref, j)
        if ref.n_differ32 == 0:
            assert all(torch.equal(a[2], b[2]) for a, b in zip(free_rep, ref.g64[j]))
    rs = K.ratios(K.saved_report(ref.r32), K.saved_report(ref.forced32), ref.saved_tol)
    assert K.first_bad(rs) is None, K.first_bad(rs)
    assert max(ref.saved_gap.values()) <= FORCED_GAP_MAX


# ---------------------------------------------------------------------------------------------- mutants
def _mutants(name):
    """(id, kind, argument): (a) skip<k>: the k-th skip connection passes no gradient; (b) head<k>: the k-th deep-supervision
    head gives its level nothing; (c) pool<k>: one window in a thousand of that pooling routes its gradient to the next entry
    of the window; (d) sign<site>: the backward of that activation flips its decision at the 16 voxels with the largest |d out|"""
    ref = reference(name)
    tape = ref.forced32.tape
    out = [("skip%d" % k, "cut", ("skip", k)) for k in range(tape.count["skip"])]
    out += [("head%d" % k, "cut", ("head", k)) for k in range(tape.count.get("head", 0))]
    acts = [i for i, s in enumerate(tape.sites) if s["kind"] == "act"]
    out += [("pool%d" % s["k"], "pool", i) for i, s in enumerate(tape.sites) if s["kind"] == "pool"]
    out += [("sign%02d" % tape.sites[i]["k"], "sign", i) for i in (acts[0], acts[len(acts) // 2 - 1], acts[len(acts) // 2], acts[-1])]
    return out


MUTANT_CASES = ["tiny.d0", "u3d4_ds.ds"]
# ids are fixed by the architecture (4 + 4 + 4 and 3 + 3 + 3 + 4): listed so that collection builds no network
MUTANT_IDS = {"tiny.d0": ["skip0", "skip1", "skip2", "skip3", "pool0", "pool1", "pool2", "pool3", "sign00", "sign08", "sign09", "sign17"],
              "u3d4_ds.ds": ["skip0", "skip1", "skip2", "head0", "head1", "head2", "pool0", "pool1", "pool2", "sign00", "sign06",
                             "sign07", "sign13"]}


@pytest.mark.parametrize("name,mid", [(n, m) for n in MUTANT_CASES for m in MUTANT_IDS[n]])
def test_tolerance_separates_mutant(name, mid):
    """the fp32 restatement stands in for a correct device; the expectation is the forced float64 tape with ONE fault in its
    backward.  Under at least one of the two dlogits some tensor must miss its tolerance by a factor of 10 or more."""
    ref = reference(name)
    muts = {m[0]: m for m in _mutants(name)}
    assert sorted(muts) == sorted(MUTANT_IDS[name])
    _, kind, arg = muts[mid]
    sites = ref.forced32.tape.sites
    best = None
    for j, d in enumerate(ref.douts):
        kw = {}
        if kind == "cut":
            kw["cut"] = {arg}
        elif kind == "pool":
            used = sites[arg]["used"]
            k = sites[arg]["inp"].numel() // used.numel()
            flat = torch.arange(used.numel()).reshape(used.shape)
            kw["bwd"] = {arg: torch.where(flat % 1000 == 0, (used + 1) % k, used)}
        else:
            used, dout = sites[arg]["used"], ref.site_douts[j][arg]
            top = dout.abs().reshape(-1).topk(16).indices
            b = used.clone().reshape(-1)
            b[top] = ~b[top]
            kw["bwd"] = {arg: b.reshape(used.shape)}
        mut = K.run(ref.case, torch.float64, forced=ref.f32dec, **kw)
        assert all(torch.equal(a, b) for a, b in zip(mut.outs, ref.forced32.outs))       # the forward is untouched
        rep = K.grad_report(mut, K.grads(mut, d)[0])
        w = K.worst(K.ratios(ref.g32[j], rep, ref.grad_tol[j], ref.terms[j]))
        if best is None or w[1] > best[1]:
            best = w + (j,)
    print("%s %s: worst tensor %s at %.3g x its tolerance (dlogits %d)" % (name, mid, best[0], best[1], best[4]))
    assert best[1] >= 10.0, best
