"""Cost of the tracked reverse sweep of the tiled TrackedNeuralODE engine (rnde_node_set_tracking) -> profiles/node_tiled_track.json.  A timing
tool, not a benchmark: bench.py and the headline path are untouched.

The two shapes of profiles/node_tiled.json ([2, 128, 128, 2] TDChain, [64, 192, 64] Chain; tools/time_node_tiled.py's parameters and inputs) at
B = 512, reltol = abstol = 1e-5, the EEst * dt callback on.  One process, one set of inputs; the constant-step sweep (0, 0) and the tracked
sweep at (1, 0) and (1, 1) ALTERNATE, run by run, on handles of their own: 2 warm-up rounds, then the median and range of 5.  Times are the
library's own HIP events (rnde_node_timing): the reverse sweep's launch, and the tile reduction behind it.

The constant sweep reverses the accepted steps, the tracked one every attempt up to the last accepted one, so the figure to hold the tracked
sweep to is (attempts / accepted) x the constant sweep of the same binary, plus one meeting per attempt, plus -- at (1, 1) -- two evaluations,
two VJPs and two meetings per solve for the initial step (a reversed attempt is seven evaluations and seven VJPs: about 2/7 of an attempt).
`ratio_to_expectation` is measured / that product (the meetings and the initial step are in the numerator only).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regneuralde_jl_amd as rn      # noqa: E402
from regneuralde_jl_amd import _lib      # noqa: E402
from time_node_tiled import B, RUNS, TOL, WARM, model_of      # noqa: E402

SETTINGS = ((False, False), (True, False), (True, True))


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def one_run(node, x, p):
    """One taped forward and its backward; (sweep ms, reduction ms, attempts reversed by the tracked sweep, accepted steps)."""
    L = _lib.lib()
    xd, pd = x.clone().requires_grad_(True), p.clone().requires_grad_(True)
    u, nfe, sv = node(xd, pd)
    h = [h for hs in node._handles.values() for h in hs if h.busy][0]
    (u.sum() + sv.saveval.sum()).backward()
    a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
    _lib.check(h.ptr, L.rnde_node_timing(h.ptr, C.byref(a), C.byref(b), C.byref(c)))
    ext = (C.c_float * (6 * node.max_attempts))()
    n = C.c_int32(0)
    _lib.check(h.ptr, L.rnde_node_attempts_ext(h.ptr, ext, node.max_attempts, C.byref(n)))
    acc = np.array(ext[:6 * n.value], dtype=np.float32).reshape(-1, 6)[:, 4]
    last = int(np.nonzero(acc)[0][-1]) + 1      # (attempts behind the last accepted one reach nothing and are not reversed)
    return b.value, c.value, last, int(acc.sum()), (pd.grad.detach().cpu().numpy(), node.last_tspan_bar)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_tiled_track.json"))
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), B=B, reltol=TOL, abstol=TOL, warmup=WARM, runs=RUNS,
               method="rnde_node_timing; (0,0), (1,0), (1,1) alternate in one process on the same inputs", shapes={})
    kw = dict(reltol=TOL, abstol=TOL, max_batch=B, max_attempts=256, track_ctrl=False, track_initdt=False)
    for name, dims, acts, td, factors in (("2-128-128-2 TD", [2, 128, 128, 2], ["tanh", "tanh", "identity"], True, (60.0, 1.0, 0.3)),
                                          ("64-192-64", [64, 192, 64], ["tanh", "identity"], False, (60.0, 0.3))):
        model = model_of(dims, acts, td, 1, factors)
        nodes = {s: rn.TrackedNeuralODE(model, [0.0, 1.0], td, True, engine="tiled", tiled_tracking=s, **kw) for s in SETTINGS}
        x = (torch.rand(B, dims[0], generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
        p = nodes[SETTINGS[0]].p.cuda()
        sweep, red, grads = {s: [] for s in SETTINGS}, {s: [] for s in SETTINGS}, {}
        for it in range(WARM + RUNS):
            for s in SETTINGS:
                b, c, natt, nacc, g = one_run(nodes[s], x, p)
                grads[s] = g
                if it >= WARM:
                    sweep[s].append(b * 1e3)
                    red[s].append(c * 1e3)
        const = statistics.median(sweep[SETTINGS[0]])
        rec = dict(dims=dims, time_dep=td, attempts_reversed=natt, accepted=nacc)
        for s in SETTINGS:
            key = "(%d,%d)" % s
            med = statistics.median(sweep[s])
            rec[key] = dict(sweep_us=stats(sweep[s]), reduction_us=stats(red[s]), us_per_reversed_unit=med / (natt if s[0] else nacc),
                            tspan_bar=[float(v) for v in grads[s][1]],
                            p_bar_rel_to_constant=float(np.abs(grads[s][0] - grads[SETTINGS[0]][0]).max() / np.abs(grads[SETTINGS[0]][0]).max()))
            if s[0]:
                expect = const * natt / nacc
                rec[key]["expectation_us"] = expect
                rec[key]["ratio_to_expectation"] = med / expect
                rec[key]["ratio_to_constant"] = med / const
        out["shapes"][name] = rec
        print(name, json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
