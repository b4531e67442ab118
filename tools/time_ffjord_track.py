"""Cost of the tracked-controller reverse sweep of the tiled TrackedFFJORD engine (rnde_ffjord_set_track_ctrl) against the constant-step sweep,
on the same inputs: two handles of one geometry (setting 1 and setting 0) tape the same forward, then their backward calls alternate in one
process -- 2 warm-ups, then the median of 5 per side, each read from rnde_ffjord_timing (HIP events around the sweep and its reduction).

Geometries: the tabular experiment's MLPDynamics(43, 100) and the gaussian experiment's MLPDynamics(2, 16), B = 1024, tol 1.4e-8, the
experiments' initial weights, cotangents of the training loss -mean(logpx) + lambda mean(saveval).  The tracked sweep walks every attempt where
the constant-step sweep walks the accepted ones, so the figure to compare is the time per ATTEMPT of the one against the time per ACCEPTED step
of the other, with the attempts / accepted ratio beside it.  Writes profiles/ffjord_track_ctrl.json.

    python tools/time_ffjord_track.py
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Handle:
    def __init__(self, rn, D, H, B, tol, track):
        self.rn, self.L, self.h = rn, rn._lib.lib(), C.c_void_p()
        cfg = rn._lib.FfjordConfig()
        cfg.in_dims, cfg.hidden, cfg.dynamics, cfg.time_dep, cfg.regularize, cfg.kinetic_reg = D, H, 0, 1, 1, 0
        cfg.max_batch, cfg.solver, cfg.reltol, cfg.abstol, cfg.cb_save_start, cfg.max_attempts, cfg.device = B, 0, tol, tol, 1, 4096, 0
        rn._lib.check_ffjord(None, self.L.rnde_ffjord_create_tiled(C.byref(cfg), C.byref(self.h)))
        rn._lib.check_ffjord(self.h, self.L.rnde_ffjord_set_track_ctrl(self.h, int(track)))

    def forward(self, x, p, e):
        self.keep = (x, p, e)
        B = x.shape[0]
        logpx = torch.empty(B, device=x.device)
        nfe, nsv, sv = C.c_int64(), C.c_int32(), (C.c_float * 4097)()
        st = self.L.rnde_ffjord_forward(self.h, x.data_ptr(), p.data_ptr(), e.data_ptr(), B, 0.0, 1.0, 0, logpx.data_ptr(), None, C.byref(nfe), sv,
                                        C.byref(nsv), 1, None)
        self.rn._lib.check_ffjord(self.h, st)
        a, b, n, m = C.c_float(), C.c_float(), C.c_int32(), C.c_int32()
        self.rn._lib.check_ffjord(self.h, self.L.rnde_ffjord_timing(self.h, C.byref(a), C.byref(b), C.byref(n), C.byref(m)))
        self.nsv, self.solve_ms, self.attempts, self.accepted = nsv.value, a.value, n.value, m.value

    def backward(self, g, svb):
        x, p, _ = self.keep
        arr = (C.c_float * self.nsv)(*([svb] * self.nsv))
        pb, xb = torch.empty_like(p), torch.empty_like(x)
        self.rn._lib.check_ffjord(self.h, self.L.rnde_ffjord_backward(self.h, g.data_ptr(), arr, pb.data_ptr(), xb.data_ptr(), None))
        b = C.c_float()
        self.rn._lib.check_ffjord(self.h, self.L.rnde_ffjord_timing(self.h, None, C.byref(b), None, None))
        return b.value, pb

    def close(self):
        self.L.rnde_ffjord_destroy(self.h)


def measure(rn, name, D, H, B, tol, x, seed, lam, warm, reps):
    dev = torch.device("cuda", 0)
    model = rn.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(seed))
    p = model.destructure().to(dev)
    x = x.to(dev).contiguous()
    e = torch.randn(B, D, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    g = torch.full((B,), -1.0 / B, device=dev)
    hs = {"tracked": Handle(rn, D, H, B, tol, 1), "constant": Handle(rn, D, H, B, tol, 0)}
    for h in hs.values():
        h.forward(x, p, e)
    t = hs["tracked"]
    assert (t.attempts, t.accepted) == (hs["constant"].attempts, hs["constant"].accepted)
    ms, grads = {k: [] for k in hs}, {}
    for i in range(warm + reps):
        for k, h in hs.items():                       # alternated: both sides see the same clocks and the same neighbours
            v, grads[k] = h.backward(g, lam / h.nsv)
            if i >= warm:
                ms[k].append(v)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    diff = float((grads["tracked"] - grads["constant"]).norm() / grads["tracked"].norm())
    res = dict(geometry=[D, H], batch=B, tol=tol, attempts=t.attempts, accepted=t.accepted, attempts_per_accepted=t.attempts / t.accepted,
               solve_ms=t.solve_ms, reverse_ms={k: dict(median=med[k], runs=v) for k, v in ms.items()},
               tracked_us_per_attempt=1e3 * med["tracked"] / t.attempts, constant_us_per_accepted_step=1e3 * med["constant"] / t.accepted,
               tracked_over_constant=med["tracked"] / med["constant"],
               tracked_over_expectation=med["tracked"] / (med["constant"] * t.attempts / t.accepted),
               p_bar_tracked_minus_constant_rel_norm=diff)
    for h in hs.values():
        h.close()
    print(name, json.dumps({k: v for k, v in res.items() if k != "reverse_ms"}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--tol", type=float, default=1.4e-8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffjord_track_ctrl.json"))
    a = ap.parse_args()
    import regneuralde_jl_amd as rn
    B = a.batch
    tr, _ = rn.load_gaussian_mixture(B, nsamples=2 * B, ngaussians=6, seed=0)
    xg = torch.from_numpy(tr.X[:B])
    xt = torch.randn(B, 43, generator=torch.Generator().manual_seed(0))
    out = dict(method=f"rnde_ffjord_timing reverse ms, median of {a.reps} after {a.warmup} warm-ups, tracked and constant alternated in one process",
               tabular=measure(rn, "tabular", 43, 100, B, a.tol, xt, 0, 5.0e3, a.warmup, a.reps),
               gaussian=measure(rn, "gaussian", 2, 16, B, a.tol, xg, 0, 2.0e3, a.warmup, a.reps))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
