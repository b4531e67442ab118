"""Cost of saved points on the tiled TrackedNeuralODE engine (rnde_node_tiled_reserve_saveat) -> profiles/node_tiled_saveat.json.  A timing
tool, not a benchmark: bench.py and the headline path are untouched.

The two shapes of profiles/node_tiled.json ([2, 128, 128, 2] TDChain, [64, 192, 64] Chain; tools/time_node_tiled.py's parameters and inputs) at
B = 512, reltol = abstol = 1e-5, the EEst * dt callback on.  One process, one handle with a capacity of 49 and one set of inputs per shape and
tracking setting; the END-STATE call (rnde_node_forward: the kernels and the bits of a handle that never reserved -- the code path of the
commit before saved points existed, which is what the saving call is compared with) and the SAVING call (rnde_node_forward_saveat, 49 equally
spaced times from t0 to t1) ALTERNATE, run by run, each followed by its backward: 2 warm-up rounds, then the median and range of 5.  Times are
the library's own HIP events (rnde_node_timing): the solve's launch, the reverse sweep's launch.  Both calls take the same attempts (asserted),
so `ratio` = saving / end-state is the cost of the saved points alone: per point and tile a read of the stage values and one write in the
solve, and in the sweep a read of the cotangent and an update of the seven stage cotangents.
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
from regneuralde_jl_amd.node import _Handle      # noqa: E402
from time_node_tiled import B, RUNS, TOL, WARM, model_of      # noqa: E402

NSAVE = 49
SETTINGS = ((0, 0), (1, 1))


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def one_run(L, h, x, p, D, P, max_attempts, times):
    """One taped forward (saving at `times`, or the end state when None) and its backward: (solve us, sweep us, attempt log)."""
    Bn = x.shape[0]
    nfe, nsv = C.c_int64(0), C.c_int32(0)
    sv = (C.c_float * (max_attempts + 1))()
    if times is None:
        u = torch.empty((Bn, D), dtype=torch.float32, device="cuda")
        st = L.rnde_node_forward(h, x.data_ptr(), p.data_ptr(), Bn, 0.0, 1.0, u.data_ptr(), C.byref(nfe), sv, C.byref(nsv), 1, None)
    else:
        u = torch.empty((Bn, len(times), D), dtype=torch.float32, device="cuda")
        sa = (C.c_float * len(times))(*times)
        st = L.rnde_node_forward_saveat(h, x.data_ptr(), p.data_ptr(), Bn, 0.0, 1.0, sa, len(times), u.data_ptr(), C.byref(nfe), sv, C.byref(nsv), 1, None)
    _lib.check(h, st)
    ext, n = (C.c_float * (6 * max_attempts))(), C.c_int32(0)
    _lib.check(h, L.rnde_node_attempts_ext(h, ext, max_attempts, C.byref(n)))
    ub, xb, pb = torch.ones_like(u), torch.empty((Bn, D), dtype=torch.float32, device="cuda"), torch.empty(P, dtype=torch.float32, device="cuda")
    svb, tsb = (C.c_float * nsv.value)(*([1.0] * nsv.value)), (C.c_float * 2)()
    torch.cuda.synchronize()
    _lib.check(h, L.rnde_node_backward(h, ub.data_ptr(), svb, xb.data_ptr(), pb.data_ptr(), tsb, None))
    a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
    _lib.check(h, L.rnde_node_timing(h, C.byref(a), C.byref(b), C.byref(c)))
    _lib.check(h, L.rnde_node_release_tape(h))
    return a.value * 1e3, b.value * 1e3, bytes(ext)[: 24 * n.value]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_tiled_saveat.json"))
    args = ap.parse_args()
    L = _lib.lib()
    times = [float(v) for v in np.linspace(0.0, 1.0, NSAVE, dtype=np.float32)]
    out = dict(device=torch.cuda.get_device_name(0), B=B, reltol=TOL, abstol=TOL, warmup=WARM, runs=RUNS, n_saveat=NSAVE,
               method="rnde_node_timing; the end-state call and the saving call alternate in one process on the same handle and inputs",
               comparison="end_state is rnde_node_forward / rnde_node_backward on the same handle: the kernels and the bits of a handle that never "
                          "reserved a capacity, i.e. the code path of the commit before saved points; ratio = saving / end_state",
               shapes={})
    kw = dict(reltol=TOL, abstol=TOL, max_batch=B, max_attempts=256, track_ctrl=False, track_initdt=False)
    for name, dims, acts, td, factors in (("2-128-128-2 TD", [2, 128, 128, 2], ["tanh", "tanh", "identity"], True, (60.0, 1.0, 0.3)),
                                          ("64-192-64", [64, 192, 64], ["tanh", "identity"], False, (60.0, 0.3))):
        model = model_of(dims, acts, td, 1, factors)
        layer = rn.TrackedNeuralODE(model, [0.0, 1.0], td, True, engine="tiled", **kw)
        x = (torch.rand(B, dims[0], generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
        p = layer.p.cuda()
        rec = dict(dims=dims, time_dep=td)
        for s in SETTINGS:
            hd = _Handle(layer._config(0, "error_est"), "tiled")
            h = hd.ptr
            _lib.check(h, L.rnde_node_tiled_reserve_saveat(h, NSAVE))
            _lib.check(h, L.rnde_node_set_tracking(h, *s))
            t = {k: dict(solve=[], sweep=[]) for k in ("end_state", "saving")}
            logs = {}
            for it in range(WARM + RUNS):
                for k, tm in (("end_state", None), ("saving", times)):
                    a, b, logs[k] = one_run(L, h, x, p, dims[0], layer.P, layer.max_attempts, tm)
                    if it >= WARM:
                        t[k]["solve"].append(a)
                        t[k]["sweep"].append(b)
            assert logs["end_state"] == logs["saving"], "the saving solve did not take the end-state solve's attempts"
            n_att = len(logs["saving"]) // 24
            r = dict(attempts=n_att)
            for k in t:
                r[k] = dict(solve_us=stats(t[k]["solve"]), sweep_us=stats(t[k]["sweep"]))
            r["ratio_solve"] = r["saving"]["solve_us"]["median"] / r["end_state"]["solve_us"]["median"]
            r["ratio_sweep"] = r["saving"]["sweep_us"]["median"] / r["end_state"]["sweep_us"]["median"]
            rec["(%d,%d)" % s] = r
            del hd
        out["shapes"][name] = rec
        print(name, json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
