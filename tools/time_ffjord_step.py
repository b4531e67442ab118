"""Host time of one whole FFJORD training step, composed against one-call -> profiles/ffjord_one_call.json.

    python tools/time_ffjord_step.py            # gaussian MLPDynamics(2, 16) on both engines, tabular MLPDynamics(43, 100) tiled

Two legs, alternated inside every round of one process:
    composed   the layer call, the torch loss, backward() and FluxADAM(weight_decay=1e-5) as they stand (forward and backward as two library
               calls, the saved values and their cotangents through the host, the weight decay as two torch kernels)
    one_call   fused_ffjord_loss_and_grad (rnde_ffjord_nll_grad) and FluxADAM(one_launch=True) (rnde_adam_wd_step)
A step ends in a device synchronise.  B = 1024, reltol = abstol = 1.4e-8, regularize = 1, lambda_r = 1e3.  The weights are restored and the
probe is the same in every step, so both legs run the same solve: the tool asserts that their NFE agree.  Median (min - max) of 7 rounds
after 2 warm-up rounds."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAM = 1.0e3


def _stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def shape(rn, name, D, H, engine, B, rounds, warmup, seed):
    dev = torch.device("cuda", 0)
    model = rn.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(seed))
    ff = rn.TrackedFFJORD(model, [0.0, 1.0], True, True, "Tsit5", reltol=1.4e-8, abstol=1.4e-8, max_batch=B, engine=engine)
    rng = np.random.default_rng(seed)
    if D == 2:
        x = torch.from_numpy(rn.load_gaussian_mixture(B, nsamples=2 * B, ngaussians=6, seed=seed)[0].X[:B]).to(dev)
    else:
        x = torch.from_numpy((rng.standard_normal((B, D)) * 0.5).astype(np.float32)).to(dev)
    e = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(dev)
    p0 = ff.p.clone()
    p = ff.p.clone().requires_grad_(True)
    nfes = {}

    def restore(opt):
        with torch.no_grad():
            p.copy_(p0)
        for m, v in zip(opt.m, opt.v):
            m.zero_(); v.zero_()
        opt.t = 0
        p.grad = None

    composed_opt = rn.FluxADAM([p], eta=1e-2, weight_decay=1e-5)
    one_opt = rn.FluxADAM([p], eta=1e-2, weight_decay=1e-5, one_launch=True)

    def composed():
        logpx, _, _, nfe, sv = ff(x, p, e)
        (-logpx.mean() + LAM * sv.saveval.mean()).backward()
        composed_opt.step()
        return nfe

    def one_call():
        nfe = rn.fused_ffjord_loss_and_grad(ff, x, p, e, lam_r=LAM)[4]
        one_opt.step()
        return nfe

    legs = dict(composed=(composed, composed_opt), one_call=(one_call, one_opt))
    ms = {k: [] for k in legs}
    for r in range(warmup + rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            fn, opt = legs[k]
            restore(opt)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nfe = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            nfes.setdefault(k, nfe)
            assert nfe == nfes[k], (name, k, nfe, nfes[k])
            if r >= warmup:
                ms[k].append(dt)
    assert nfes["composed"] == nfes["one_call"], (name, nfes)
    a, b = _stats(ms["composed"]), _stats(ms["one_call"])
    res = dict(in_dims=D, hidden=H, engine=engine, batch=B, nfe=int(nfes["composed"]), composed=a, one_call=b,
               ranges_overlap=bool(a["min_ms"] <= b["max_ms"] and b["min_ms"] <= a["max_ms"]))
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffjord_one_call.json"))
    a = ap.parse_args()
    import regneuralde_jl_amd as rn
    res = dict(method="host clock around one whole training step, ending in a device synchronise; the two legs alternated inside every round of "
                      "one process; median (min - max) of %d rounds after %d warm-up rounds; weights restored and the probe fixed every step, NFE "
                      "asserted equal between the legs; composed: layer call, torch loss, backward(), FluxADAM default; one_call: "
                      "fused_ffjord_loss_and_grad + FluxADAM(one_launch=True)" % (a.rounds, a.warmup),
               tol=1.4e-8, regularize=1, lambda_r=LAM)
    for name, D, H, engine in (("gaussian_workgroup", 2, 16, "workgroup"), ("gaussian_tiled", 2, 16, "tiled"), ("tabular_tiled", 43, 100, "tiled")):
        res[name] = shape(rn, name, D, H, engine, a.batch, a.rounds, a.warmup, a.seed)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
