"""Timings of TrackedFFJORD's exact-trace mode against the Hutchinson mode in one session -> profiles/ffjord_exact.json.

For each case -- ConcatSquash (2, 16) at B = 512, ConcatSquash (43, 100) at B = 1000 (engine 1) and the TD chain [5, 40, 24, 5] (tanh, tanh,
tanh) at B = 512 (engine 2) -- one layer, one set of weights, one batch:

  * an adaptive Hutchinson forward fixes the step sequence (its accepted steps);
  * the Hutchinson and the exact forward + backward (-mean(logpx) + lambda mean(saveval)) are then replayed along that sequence, so both do
    the same number of stages; solve ms and reverse ms are the library's HIP-event times (rnde_ffjord_timing), 2 warm-ups, median of --reps;
  * the exact adaptive solve's own attempt count is recorded beside them.

    python tools/time_ffjord_exact.py
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAM = 100.0


def measure(ff, x, e, reps):
    with torch.no_grad():
        ff(x, None, e)
    acc = [float(d) for d, f in np.array(ff.steps()).reshape(-1, 2) if f]
    steps = sum(([d, 1.0] for d in acc), [])
    with torch.no_grad():
        ff(x, exact=True)
    exact_attempts = ff.timing()[2]

    def run(exact):
        sol, rev = [], []
        for i in range(reps + 2):
            p = ff.p.clone().requires_grad_(True)
            lp, _, _, _, sv = ff(x, p, steps=steps, exact=True) if exact else ff(x, p, e, steps=steps)
            (-lp.mean() + LAM * sv.saveval.mean()).backward()
            torch.cuda.synchronize()
            s, r, _, _ = ff.timing()
            if i >= 2:
                sol.append(s); rev.append(r)
        return float(np.median(sol)), float(np.median(rev))

    hs, hr = run(False)
    es, er = run(True)
    return dict(batch=x.shape[0], D=x.shape[1], replayed_steps=len(acc), exact_adaptive_attempts=exact_attempts,
                hutchinson=dict(solve_ms=hs, reverse_ms=hr), exact=dict(solve_ms=es, reverse_ms=er),
                solve_ratio=es / hs, reverse_ratio=er / hr, reverse_ratio_expected_baseline=x.shape[1] + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffjord_exact.json"))
    a = ap.parse_args()
    import regneuralde_jl_amd as rn
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    rng = np.random.default_rng(1234)
    res = dict(device=torch.cuda.get_device_name(0), tol=a.tol, lam=LAM, reps=a.reps)

    def data(B, D):
        A = rng.standard_normal((D, D)) / np.sqrt(D)
        x = torch.from_numpy((rng.standard_normal((B, D)) @ A).astype(np.float32)).to(dev)
        return x, torch.randn(x.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def layer(model, B):
        return rn.TrackedFFJORD(model, [0.0, 1.0], True, True, "Tsit5", reltol=a.tol, abstol=a.tol, max_batch=B, engine="tiled")

    for key, D, H, B in (("concat_squash_2_16", 2, 16, 512), ("concat_squash_43_100", 43, 100, 1000)):
        x, e = data(B, D)
        res[key] = measure(layer(rn.ffjord.MLPDynamics(D, H, generator=gen), B), x, e, a.reps)
        res[key].update(H=H, engine="tiled")
        print(key, json.dumps(res[key]), flush=True)
    dims, acts, B = [5, 40, 24, 5], ["tanh", "tanh", "tanh"], 512
    x, e = data(B, dims[0])
    model = rn.TDChain(*[rn.Dense(dims[l] + 1, dims[l + 1], acts[l], gen) for l in range(len(acts))])
    res["td_5_40_24_5"] = measure(layer(model, B), x, e, a.reps)
    res["td_5_40_24_5"].update(dims=dims, acts=acts, time_dep=True, engine="chain")
    print("td_5_40_24_5", json.dumps(res["td_5_40_24_5"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
