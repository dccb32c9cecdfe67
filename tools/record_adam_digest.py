"""Bit-level record of the Adam launches: sha256 digests of fplx_adam_step's and fplx_adam_pack_step's outputs after every step on
fixed inputs, for tests/test_gpu_optim.py::test_adam_bits_equal_the_recorded_parent (`cases` below is shared with it).

    python tools/record_adam_digest.py <tree> <commit> [<output file>]

runs the cases on the GPU against the library built in <tree> (a checkout of <commit> with libfplx.so in place) and writes
tests/golden/adam_parent_digest.json of THIS tree (or the output file).  The fixture is recorded from the commit BEFORE a change to the optimiser
launches and then left alone: the test shows that the change moved no bit.

adam_step:  n = 10007, lr 1e-3, grad_scale 0.125, weight decay 1e-5, steps 1, 2, 3 from zero moments, then step 1000 on moments
            re-seeded as they are late in training (m ~ 1e-2 N(0, 1), v ~ 1e-4 U(0, 1)).  Run twice: all four buffers on a 16-byte
            boundary, and all four one float behind one; the outputs do not depend on the placement.
adam_pack_step:  the layout of test_fused_adam_pack_step_kernel (layers 32x32, 16x64, 64x96, the second without a data-gradient
            pack; gaps 8, 1028, 36, 4097), lr 1e-3, grad_scale 0.5, weight decay 1e-5, steps 1, 2, 3, with stamps.
Every digest covers the named arrays in order (name, then the raw little-endian bytes); `inputs` tells input drift (numpy's
generator, the keys) from output drift."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "adam_parent_digest.json")
N, STEPS, LR, WD = 10007, (1, 2, 3, 1000), 1e-3, 1e-5
PACK_SHAPES, PACK_GAPS = [(32, 32), (16, 64), (64, 96)], [8, 1028, 36, 4097]


def _digest(named):
    h = hashlib.sha256()
    for name, a in named:
        h.update(name.encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _host(t):
    """a device tensor's bytes as numpy (bf16 as its 16-bit patterns)"""
    import torch
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()


def _place(a, behind):
    """a on the device at a 16-byte-aligned base, or `behind` floats behind one"""
    import torch
    buf = torch.zeros(a.size + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[behind:behind + a.size]
    v.copy_(torch.from_numpy(a))
    return v


def step_case(ops, rng, behind, abi=False):
    """-> (inputs digest, [outputs digest after each of STEPS]); abi: through the C entry point fplx_adam_step itself"""
    import torch
    g = rng("adam.bits.step")
    f32 = lambda x: x.astype(np.float32)
    p0 = f32(g.standard_normal(N))
    grads = [f32(g.standard_normal(N) * 10.0 ** g.integers(-6, 1)) for _ in STEPS]
    late = (f32(g.standard_normal(N) * 1e-2), f32(g.random(N) * 1e-4))
    inputs = _digest([("p", p0)] + [("g%d" % s, a) for s, a in zip(STEPS, grads)] + [("m", late[0]), ("v", late[1])])
    zero = np.zeros(N, np.float32)
    p, m, v = _place(p0, behind), _place(zero, behind), _place(zero, behind)
    out = []
    for step, gr in zip(STEPS, grads):
        if step == STEPS[-1]:
            m.copy_(torch.from_numpy(late[0]))
            v.copy_(torch.from_numpy(late[1]))
        gd = _place(gr, behind)
        if abi:
            ops.call("fplx_adam_step", ops.ptr(p), ops.ptr(gd), ops.ptr(m), ops.ptr(v), N, LR, 0.9, 0.999, 1e-8, WD, step, 0.125,
                     ops.stream())
        else:
            ops.adam_step(p, gd, m, v, LR, step, WD, 0.125)
        torch.cuda.synchronize()
        out.append(_digest([("p", _host(p)), ("m", _host(m)), ("v", _host(v))]))
    return inputs, out


def pack_case(ops, rng, abi=False):
    """-> (inputs digest, [outputs digest after steps 1, 2, 3]): p, m, v, every wf / wb and every stamp buffer; abi: through the
    C entry point fplx_adam_pack_step itself"""
    import torch
    offs, pos = [], 0
    for (co, ci), gp in zip(PACK_SHAPES, PACK_GAPS):
        pos += (gp + 3) // 4 * 4
        offs.append(pos)
        pos += co * ci * 27
    n = pos + PACK_GAPS[-1]
    g = rng("adam.bits.pack")
    p0 = (g.standard_normal(n) * 0.1).astype(np.float32)
    grads = [(g.standard_normal(n) * 0.01).astype(np.float32) for _ in range(3)]
    inputs = _digest([("p", p0)] + [("g%d" % (i + 1), a) for i, a in enumerate(grads)])
    p, m, v = torch.from_numpy(p0).cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    bf = dict(dtype=torch.bfloat16, device="cuda")
    layers = [(o, co, ci, torch.zeros((27, co, ci), **bf), None if k == 1 else torch.zeros((27, ci, co), **bf),
               torch.zeros(ops.pack_stamp_floats(co, ci), device="cuda")) for k, (o, (co, ci)) in enumerate(zip(offs, PACK_SHAPES))]
    out = []
    for step, gr in enumerate(grads, 1):
        gd = torch.from_numpy(gr).cuda()
        if abi:
            ops.call("fplx_adam_pack_step", ops.ptr(p), ops.ptr(gd), ops.ptr(m), ops.ptr(v), n, LR, 0.9, 0.999, 1e-8, WD, step, 0.5,
                     *(ops._pack_layer_args(layers) + (ops.stream(),)))
        else:
            ops.adam_pack_step(p, gd, m, v, LR, step, WD, 0.5, (0.9, 0.999), 1e-8, layers)
        torch.cuda.synchronize()
        named = [("p", _host(p)), ("m", _host(m)), ("v", _host(v))]
        for k, l in enumerate(layers):
            named += [("%s%d" % (nm, k), _host(t)) for nm, t in (("wf", l[3]), ("wb", l[4]), ("stamp", l[5])) if t is not None]
        out.append(_digest(named))
    return inputs, out


if __name__ == "__main__":
    tree, commit = os.path.abspath(sys.argv[1]), sys.argv[2]
    sys.path[:0] = [os.path.join(tree, "fpl-plus_amd"), os.path.join(ROOT, "tests")]
    from fplx import _lib, ops
    from optimoracle import rng
    assert os.path.dirname(os.path.dirname(_lib.LIB_PATH)) == os.path.join(tree, "fpl-plus_amd"), _lib.LIB_PATH
    sin, sout = step_case(ops, rng, 0)
    assert step_case(ops, rng, 1) == (sin, sout), "the placement changed the outputs"
    pin, pout = pack_case(ops, rng)
    doc = {"_comment": "sha256 of the inputs and of the outputs after every step of the Adam launches, recorded from a build of "
                       "commit %s (tools/record_adam_digest.py)" % commit,
           "parent": commit, "adam_step": {"inputs": sin, "outputs": sout}, "adam_pack_step": {"inputs": pin, "outputs": pout}}
    dst = sys.argv[3] if len(sys.argv) > 3 else FIXTURE
    with open(dst, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", dst)
