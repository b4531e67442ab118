"""Time of ClassifierNSDE's evaluation call and of its several-trajectory training step, old path against the one-call path, at the size of
reference experiments/mnist_nsde.jl:154-155 (512 inputs x 10 trajectories = 5,120 columns; Dense(784, 32) -> SDE 32 -> Dense(32, 10), tolerance 0.14).

  evaluation   model(x, trajectories=10)            the host-language repeat, the pre-layer on 5,120 rows, the solve, torch post-layer and mean
               model.predict(x, trajectories=10)    the pre-layer on 512 rows, then ONE rnde_nsde_classifier_predict
               (both on the same explicit noise pool: the same sample paths, the same number of attempts)
  training     fused_nsde_loss_and_grad(T = 10) under RNDE_ONE_CALL=0 (the chain of torch products around rnde_nsde_forward / _backward_async)
               and under RNDE_ONE_CALL=1 (ONE rnde_nsde_classifier_grad_traj), two models with the same seed advancing in step

Every sample is a pair of HIP events around `--inner` consecutive calls, divided by their number; the variants of a pair alternate inside every
round of one process, after `--warmup` untimed rounds.  Writes min / median / max per variant to profiles/nsde_eval_traj.json.

    python tools/time_nsde_eval.py [--rounds 7] [--inner 5] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(rn, B, T, seed, dev):
    g = torch.Generator().manual_seed(seed)
    nsde = rn.TrackedNeuralDSDE(rn.Chain(rn.Dense(32, 64, "tanh", g), rn.Dense(64, 32, "identity", g)), rn.Dense(32, 32, "identity", g), [0.0, 1.0], True,
                                "SOSRI", save_everystep=False, reltol=1.4e-1, abstol=1.4e-1, save_start=False, max_batch=B * T, max_attempts=256, seed=seed)
    return rn.ClassifierNSDE(rn.Dense(784, 32, "identity", g), nsde, rn.Dense(32, 10, "identity", g), device=dev)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(variants, warmup, rounds, inner):
    ms = {k: [] for k in variants}
    for r in range(warmup + rounds):
        for k, fn in variants.items():                # alternated: both sides see the same clocks and the same neighbours
            v = timed(fn, inner)
            if r >= warmup:
                ms[k].append(v)
    return {k: dict(min=float(np.min(v)), median=float(np.median(v)), max=float(np.max(v)), samples_ms=v) for k, v in ms.items()}


def overlap(a, b):
    return not (a["max"] < b["min"] or b["max"] < a["min"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--trajectories", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pool", type=int, default=96)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nsde_eval_traj.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert a.rounds >= 5
    import regneuralde_jl_amd as rn
    dev = torch.device("cuda", 0)
    B, T = a.batch, a.trajectories
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 784, generator=g).to(dev)
    y = torch.eye(10)[torch.randint(0, 10, (B,), generator=g)].to(dev)
    noise = torch.randn(a.pool, 2, B * T, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(2))

    model = make(rn, B, T, 7, dev)
    nfe = {}

    def layer_call():
        with torch.no_grad():
            nfe["layer_call"] = model(x, trajectories=T, func="error_est", noise=noise)[1:3]

    def predict():
        nfe["predict"] = model.predict(x, trajectories=T, noise=noise)[1:3]
    ev = alternate({"layer_call": layer_call, "predict": predict}, a.warmup, a.rounds, a.inner)
    assert nfe["layer_call"] == nfe["predict"], nfe
    with torch.no_grad():
        dz = float((model(x, trajectories=T, func="error_est", noise=noise)[0] - model.predict(x, trajectories=T, noise=noise)[0]).abs().max())

    m0, m1 = make(rn, B, T, 11, dev), make(rn, B, T, 11, dev)
    last = {}

    def chain():
        os.environ["RNDE_ONE_CALL"] = "0"
        last["chain"] = rn.fused_nsde_loss_and_grad(m0, x, y, trajectories=T, lam=10.0)

    def one_call():
        os.environ["RNDE_ONE_CALL"] = "1"
        last["one_call"] = rn.fused_nsde_loss_and_grad(m1, x, y, trajectories=T, lam=10.0)
    tr = alternate({"chain_RNDE_ONE_CALL_0": chain, "one_call_RNDE_ONE_CALL_1": one_call}, a.warmup, a.rounds, a.inner)
    os.environ.pop("RNDE_ONE_CALL", None)
    torch.cuda.synchronize()
    assert last["chain"][3:] == last["one_call"][3:], (last["chain"][3:], last["one_call"][3:])
    gdiff = max(float((p.grad - q.grad).abs().max() / p.grad.abs().max()) for p, q in zip(m0.trainable(), m1.trainable()))

    out = dict(method=f"HIP events around {a.inner} consecutive calls, per call; {a.rounds} rounds after {a.warmup} warm-up rounds, the two variants of a "
                      "pair alternated inside every round of one process",
               batch=B, trajectories=T, columns=B * T,
               evaluation=dict(ms_per_call=ev, nfe=list(nfe["predict"]), logits_max_abs_difference=dz,
                               ranges_overlap=overlap(ev["layer_call"], ev["predict"]),
                               median_ratio_layer_call_over_predict=ev["layer_call"]["median"] / ev["predict"]["median"]),
               training=dict(ms_per_call=tr, nfe=list(last["one_call"][3:]), gradients_max_rel_difference=gdiff,
                             ranges_overlap=overlap(tr["chain_RNDE_ONE_CALL_0"], tr["one_call_RNDE_ONE_CALL_1"]),
                             median_ratio_chain_over_one_call=tr["chain_RNDE_ONE_CALL_0"]["median"] / tr["one_call_RNDE_ONE_CALL_1"]["median"]))
    print(json.dumps({k: ({kk: vv for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in out.items()}, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
