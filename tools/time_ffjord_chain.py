"""Timings of TrackedFFJORD's default dynamics on Dense chains (rnde_ffjord_create_chain) in one session -> profiles/ffjord_chain.json:

  * HIP-event time per forward attempt and per reversed step (rnde_ffjord_timing) at B = 1024, reltol = abstol = 1.4e-8, for
    TD [2, 16, 16, 2] (softplus, softplus, identity) and TD [48, 64, 64, 48] (tanh, softplus, tanh);
  * the same figures for the ConcatSquash tiled engine at MLPDynamics(2, 16) on the same batch;
  * for each, one training step (-mean(logpx) + lambda mean(saveval), forward + backward) at equal work against an eager-torch fp32
    restatement on the GPU: same batch, probe, weights and step sequence (the device's own accepted steps), 2 warm-ups, median and range of
    --reps runs (the protocol of profiles/ffjord_tabular.json).

The eager restatements: the chain's f with eJ from torch.autograd.grad(f, z, e, create_graph=True) (Tracker.forward + back) stated here
for tensors on the device; tests/ffjord_ref.py (imported from the repository tree) for ConcatSquash, Tsit5 and the replay.

    python tools/time_ffjord_chain.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACT = {"identity": lambda z: z, "tanh": torch.tanh, "softplus": torch.nn.functional.softplus, "sigmoid": torch.sigmoid,
       "relu": torch.relu, "elu": torch.nn.functional.elu}
LAM = 100.0


def chain_rhs(dims, acts, td, p, u, t, e):
    """[f(z, t); -e . eJ] of u = [z; l], eager torch in the precision and on the device of its inputs."""
    D = dims[0]
    with torch.enable_grad():
        z = u[:, :D]
        z = z if z.requires_grad else z.detach().requires_grad_(True)
        x, o = z, 0
        for l, a in enumerate(acts):
            n_in, n_out = dims[l] + (1 if td else 0), dims[l + 1]
            W = p[o:o + n_in * n_out].view(n_in, n_out)
            o += n_in * n_out
            b = p[o:o + n_out]
            o += n_out
            if td:
                x = torch.cat([x, torch.full((x.shape[0], 1), float(t), dtype=x.dtype, device=x.device)], 1)
            x = ACT[a](x @ W + b)
        eJ = torch.autograd.grad(x, z, e, create_graph=True)[0]
    return torch.cat([x, -(e * eJ).sum(1, keepdim=True)], 1)


def timed(fn, reps):
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), max_ms=float(max(out)), runs=reps)


def measure(ff, F_of, x, e, reps, tol):
    """Event times per attempt / reversed step of `ff` on (x, e), then the training step against the eager restatement F_of(p) at equal work."""
    from tests import ffjord_ref as R
    D, B = x.shape[1], x.shape[0]
    fa, rs, att, accd = [], [], 0, 0
    for i in range(reps + 1):
        p = ff.p.clone().requires_grad_(True)
        lp, _, _, _, sv = ff(x, p, e)
        (-lp.mean() + LAM * sv.saveval.mean()).backward()
        torch.cuda.synchronize()
        s, r, att, accd = ff.timing()
        if i:
            fa.append(s / att * 1e3)
            rs.append(r / accd * 1e3)
    acc = [float(d) for d, f in np.array(ff.steps()).reshape(-1, 2) if f]
    p = ff.p.clone().requires_grad_(True)

    def device_step():
        lp, _, _, _, sv = ff(x, p, e, steps=sum(([d, 1.0] for d in acc), []))
        (-lp.mean() + LAM * sv.saveval.mean()).backward()
        p.grad = None

    pt = ff.p.detach().clone().requires_grad_(True)
    F = F_of(pt)

    def eager_step():
        u, eests = R.replay(F, torch.cat([x, torch.zeros(B, 1, device=x.device)], 1), 0.0, acc, tol, tol)
        loss = -R.logpx_of(u, D).mean() + LAM * torch.stack([ee * d for ee, d in zip(eests, acc)]).sum() / (len(acc) + 1)
        loss.backward()
        pt.grad = None

    dev_t, eager_t = timed(device_step, reps), timed(eager_step, reps)
    return dict(batch=B, attempts=att, accepted=accd, us_per_forward_attempt=float(np.median(fa)), us_per_reversed_step=float(np.median(rs)),
                equal_work_step=dict(accepted_steps=len(acc), device=dev_t, eager_torch_fp32=eager_t,
                                     speedup_median=eager_t["median_ms"] / dev_t["median_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1.4e-8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffjord_chain.json"))
    a = ap.parse_args()
    import regneuralde_jl_amd as rn
    from tests import ffjord_ref as R
    dev = torch.device("cuda", 0)
    B = a.batch
    tr, _ = rn.load_gaussian_mixture(B, nsamples=2048, seed=0)
    x2 = torch.from_numpy(next(iter(tr))).to(dev)[:B]
    gen = torch.Generator().manual_seed(0)
    res = dict(tol=a.tol, lam=LAM)

    def chain_case(dims, acts, x):
        layers = [rn.Dense(dims[l] + 1, dims[l + 1], acts[l], gen) for l in range(len(acts))]
        ff = rn.TrackedFFJORD(rn.TDChain(*layers), [0.0, 1.0], True, True, "Tsit5", reltol=a.tol, abstol=a.tol, max_batch=x.shape[0], engine="tiled")
        e = torch.randn(x.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        out = measure(ff, lambda pt: (lambda u, t: chain_rhs(dims, acts, True, pt, u, t, e)), x, e, a.reps, a.tol)
        out.update(dims=dims, acts=acts, time_dep=True, engine="chain")
        return out

    res["td_2_16_16_2"] = chain_case([2, 16, 16, 2], ["softplus", "softplus", "identity"], x2)
    print(json.dumps(res["td_2_16_16_2"]), flush=True)
    m = rn.ffjord.MLPDynamics(2, 16, generator=gen)
    ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, True, "Tsit5", reltol=a.tol, abstol=a.tol, max_batch=x2.shape[0], engine="tiled")
    e2 = torch.randn(x2.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    res["concat_squash_2_16_tiled"] = measure(ff, lambda pt: (lambda u, t: R.rhs(pt, 2, 16, u, t, e2)), x2, e2, a.reps, a.tol)
    res["concat_squash_2_16_tiled"].update(D=2, H=16, engine="tiled")
    print(json.dumps(res["concat_squash_2_16_tiled"]), flush=True)
    rng = np.random.default_rng(1234)
    A48 = rng.standard_normal((48, 48)) / np.sqrt(48)
    x48 = torch.from_numpy((rng.standard_normal((x2.shape[0], 48)) @ A48).astype(np.float32)).to(dev)
    res["td_48_64_64_48"] = chain_case([48, 64, 64, 48], ["tanh", "softplus", "tanh"], x48)
    print(json.dumps(res["td_48_64_64_48"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
