"""Timing of the tiled engine of TrackedNeuralODE (engine="tiled"; include/rnde.h: rnde_node_create_tiled) -> profiles/node_tiled.json.  A timing
tool, not a benchmark: bench.py and the headline path are untouched.

What is measured, at B = 512, reltol = abstol = 1e-5, the EEst * dt callback on, parameters of the fast, modest right-hand side the tests use
(first layer x 60, last layer x 0.3: an error-limited solve of some tens of attempts):
  * [2, 128, 128, 2] (TDChain, tanh / tanh / identity) and [64, 192, 64] (Chain, tanh / identity) on the tiled engine: microseconds per forward
    attempt (the one-launch solve over its attempts, start-up included) and per reversed step (the reverse sweep over the accepted steps), from
    the HIP events of rnde_node_timing;
  * each against an eager-torch fp32 restatement on the same GPU at EQUAL WORK: the same Tsit5 stages along the device's own attempt sequence
    (rejected attempts evaluated too, as the solve does), the reverse by autograd through the accepted steps; the method of
    tools/train_ffjord_tabular.py: 2 warm-up runs, then median and range of 5;
  * the latent widths [20, 50, ..., 20] (8 tanh layers) on the tiled engine and on the chain engine (col_tile 0), both with the track flags at 0,
    timed at the level of the layer call (torch events around the call and around backward(): the chain engine's reverse records no events of
    its own, so this is the one measure both offer alike; host work and launches are in it).
The expectation the tiled FFJORD engine was held to is >= 3x eager torch at equal work; it is a figure to report against, whichever way it falls.
--bench: one plain `bench.py --gpus 1` run in a child process, its JSON line stored under "headline_bench" (the headline must not have moved).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import regneuralde_jl_amd as rn      # noqa: E402
from regneuralde_jl_amd import _lib      # noqa: E402

B, TOL, WARM, RUNS = 512, 1e-5, 2, 5
A = [[], [0.161], [-0.008480655492356989, 0.335480655492357], [2.8971530571054935, -6.359448489975075, 4.3622954328695815],
     [5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525],
     [5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383],
     [0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774]]
CS = [0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0]
BT = [-0.001780011052225777, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629, 0.5823571654525552, -0.45808210592918697,
      0.015151515151515152]


def model_of(dims, acts, td, seed, factors):
    g = torch.Generator().manual_seed(seed)
    layers = [rn.Dense(dims[l] + (1 if td else 0), dims[l + 1], acts[l], g) for l in range(len(acts))]
    for l, f in zip(layers, factors):
        l.b = 0.3 * torch.randn(l.n_out, generator=g)
        l.W, l.b = l.W * f, l.b * f
    return (rn.TDChain if td else rn.Chain)(*layers)


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def time_engine(node, x, p):
    """us per forward attempt and per reversed step from the library's own events; returns the figures and the attempt log."""
    L = _lib.lib()
    fa, rs = [], []
    log = None
    for it in range(WARM + RUNS):
        xd, pd = x.clone().requires_grad_(True), p.clone().requires_grad_(True)
        u, nfe, sv = node(xd, pd)
        h = [h for hs in node._handles.values() for h in hs if h.busy][0]
        (u.sum() + sv.saveval.sum()).backward()
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        _lib.check(h.ptr, L.rnde_node_timing(h.ptr, C.byref(a), C.byref(b), C.byref(c)))
        steps = (C.c_float * (4 * node.max_attempts))()
        n = C.c_int32(0)
        L.rnde_node_steps(h.ptr, steps, node.max_attempts, C.byref(n))
        log = np.array(steps[:4 * n.value], dtype=np.float32).reshape(-1, 4)
        natt, nacc = len(log), int(log[:, 3].sum())
        if it >= WARM:
            fa.append(a.value * 1e3 / natt)
            rs.append((b.value + c.value) * 1e3 / nacc)
    return dict(us_per_forward_attempt=stats(fa), us_per_reversed_step=stats(rs), attempts=len(log), accepted=int(log[:, 3].sum())), log


def time_calls(node, x, p):
    """us per forward attempt and per reversed step at the level of the layer call: torch events around node(x, p) and around backward(), host
    work and launches included -- the one measure both engines offer alike (the chain engine's reverse records no events of its own)."""
    fa, rs = [], []
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for it in range(WARM + RUNS):
        xd, pd = x.clone().requires_grad_(True), p.clone().requires_grad_(True)
        torch.cuda.synchronize()
        e[0].record()
        u, nfe, sv = node(xd, pd)
        e[1].record()
        (u.sum() + sv.saveval.sum()).backward()
        e[2].record()
        torch.cuda.synchronize()
        natt, nacc = (nfe - 3) // 6, sv.saveval.numel() - 1
        if it >= WARM:
            fa.append(e[0].elapsed_time(e[1]) * 1e3 / natt)
            rs.append(e[1].elapsed_time(e[2]) * 1e3 / nacc)
    return dict(us_per_forward_attempt=stats(fa), us_per_reversed_step=stats(rs), attempts=natt, accepted=nacc)


def eager(model, td, x, log):
    """The same attempts in eager torch fp32 on the GPU; the reverse by autograd through the accepted steps."""
    Ws = [l.W.cuda().requires_grad_(True) for l in model.layers]
    bs = [l.b.cuda().requires_grad_(True) for l in model.layers]
    acts = [{"tanh": torch.tanh, "identity": lambda z: z}[l.act] for l in model.layers]

    def f(u, t):
        for W, b, a in zip(Ws, bs, acts):
            if td:
                u = torch.cat([u, torch.full((u.shape[0], 1), t, device=u.device)], 1)
            u = a(u @ W + b)
        return u

    fa, rs = [], []
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    natt, nacc = len(log), int(log[:, 3].sum())
    for it in range(WARM + RUNS):
        xd = x.clone().requires_grad_(True)
        e[0].record()
        u, k1, sv = xd, f(xd, 0.0), []
        for t, dt, eest, acc in log.tolist():
            k = [k1]
            for s in range(1, 7):
                k.append(f(u + dt * sum(A[s][j] * k[j] for j in range(s)), t + CS[s] * dt))
            un = u + dt * sum(A[6][j] * k[j] for j in range(6))
            err = dt * sum(BT[j] * k[j] for j in range(7)) / (TOL + torch.maximum(u.abs(), un.abs()) * TOL)
            ee = err.pow(2).mean().sqrt()
            if acc:
                sv.append(ee * dt)
                u, k1 = un, k[6]
        loss = u.sum() + torch.stack(sv).sum()
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        if it >= WARM:
            fa.append(e[0].elapsed_time(e[1]) * 1e3 / natt)
            rs.append(e[1].elapsed_time(e[2]) * 1e3 / nacc)
    return dict(us_per_forward_attempt=stats(fa), us_per_reversed_step=stats(rs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_tiled.json"))
    ap.add_argument("--bench", action="store_true", help="also run bench.py --gpus 1 once (child process) and store its JSON line")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), B=B, reltol=TOL, abstol=TOL, warmup=WARM, runs=RUNS, target="tiled >= 3x eager torch at equal work",
               shapes={})
    kw = dict(reltol=TOL, abstol=TOL, max_batch=B, max_attempts=256, track_ctrl=False, track_initdt=False)
    for name, dims, acts, td, factors in (("2-128-128-2 TD", [2, 128, 128, 2], ["tanh", "tanh", "identity"], True, (60.0, 1.0, 0.3)),
                                          ("64-192-64", [64, 192, 64], ["tanh", "identity"], False, (60.0, 0.3))):
        model = model_of(dims, acts, td, 1, factors)
        node = rn.TrackedNeuralODE(model, [0.0, 1.0], td, True, engine="tiled", **kw)
        x = (torch.rand(B, dims[0], generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
        tiled, log = time_engine(node, x, node.p.cuda())
        eg = eager(model, td, x, log)
        rec = dict(dims=dims, time_dep=td, lds_bytes=rn.node.tiled_lds_bytes(dims), tiled=tiled, eager_torch_fp32=eg,
                   speedup_forward=eg["us_per_forward_attempt"]["median"] / tiled["us_per_forward_attempt"]["median"],
                   speedup_reverse=eg["us_per_reversed_step"]["median"] / tiled["us_per_reversed_step"]["median"])
        out["shapes"][name] = rec
        print(name, json.dumps(rec))
    dims = [20, 50, 20, 50, 20, 50, 20, 50, 20]
    model = model_of(dims, ["tanh"] * 8, False, 1, (4.0,) + (1.0,) * 7)
    x = (torch.rand(B, 20, generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    lat = {}
    for eng in ("tiled", None):
        node = rn.TrackedNeuralODE(model, [0.0, 1.0], False, True, engine=eng, **kw)
        lat["tiled" if eng else "chain"] = time_calls(node, x, node.p.cuda())
    lat["tiled_over_chain_forward"] = lat["tiled"]["us_per_forward_attempt"]["median"] / lat["chain"]["us_per_forward_attempt"]["median"]
    lat["tiled_over_chain_reverse"] = lat["tiled"]["us_per_reversed_step"]["median"] / lat["chain"]["us_per_reversed_step"]["median"]
    lat["method"] = "torch events around the layer call and around backward(): host work and launches included, the same for both engines"
    out["latent_widths"] = lat
    print("latent", json.dumps(lat))
    if args.bench:      # a child process of its own (this one holds the GPU open; the child opens it afresh)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup",
                            str(args.bench_warmup)], capture_output=True, text=True, cwd=ROOT)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        out["headline_bench"] = json.loads(lines[-1]) if lines else dict(error=r.stderr[-2000:])
        print("bench", lines[-1] if lines else r.stderr[-500:])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
