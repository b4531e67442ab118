"""Solve and reverse times (rnde_ffjord_timing: HIP events) of a kinetic call (TrackedFFJORD{false} with regularize = true) and a plain call on
the same inputs along the same step sequence: MLPDynamics(2, 16) on the one-workgroup engine and MLPDynamics(43, 100) on the tiled engine,
B = 1024.  The sequence is the kinetic adaptive solve's own (tol 1e-5, Glorot weights); both calls then replay it, taped, and run their
reverse sweep.  One warm-up, then the median of --reps runs.  Output: profiles/ffjord_kinetic_timing.json.

    python tools/time_ffjord_kinetic.py
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffjord_kinetic_timing.json"))
    a = ap.parse_args()
    import regneuralde_jl_amd as rn
    dev, B, res = torch.device("cuda", 0), a.batch, []
    for engine, D, H in (("workgroup", 2, 16), ("tiled", 43, 100)):
        m = rn.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(0))
        ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, False, "Tsit5", reltol=1e-5, abstol=1e-5, max_batch=B, engine=engine)
        g = torch.Generator().manual_seed(1)
        x, e = torch.randn(B, D, generator=g).to(dev), torch.randn(B, D, generator=g).to(dev)
        with torch.no_grad():
            ff(x, None, e, regularize=True)
        steps = ff.steps()
        row = dict(engine=engine, D=D, H=H, batch=B, attempts=len(steps) // 2, accepted=int(sum(steps[1::2])))
        for kin in (False, True):
            sol, rev = [], []
            for i in range(a.reps + 1):
                p = ff.p.clone().requires_grad_(True)
                lp, l1, l2, _, _ = ff(x, p, e, regularize=kin, steps=steps)
                (-lp.mean() + 0.01 * l1.mean() + 0.01 * l2.mean()).backward()
                torch.cuda.synchronize()
                s, r, _, _ = ff.timing()
                if i:
                    sol.append(s); rev.append(r)
            row["kinetic" if kin else "plain"] = dict(solve_ms=float(np.median(sol)), reverse_ms=float(np.median(rev)))
        row["solve_ratio"] = row["kinetic"]["solve_ms"] / row["plain"]["solve_ms"]
        row["reverse_ratio"] = row["kinetic"]["reverse_ms"] / row["plain"]["reverse_ms"]
        print(json.dumps(row), flush=True)
        res.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
