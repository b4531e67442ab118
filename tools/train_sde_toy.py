"""The reference's neural-SDE toy problem (experiments/sde_toy_problem.jl) end to end on the device, seed 5, REGULARIZE = false and true:

    drift     Chain(x -> x .^ 3, Dense(2, 50, tanh), Dense(50, 2)),  diffusion Dense(2, 2)
    layer     TrackedNeuralDSDE(drift, diffusion, [0, 1 + eps(Float32)], REGULARIZE, SOSRI(); saveat = range(0, 1, length = 30), reltol = abstol = 0.3)
    data      data/sde_demo.bson (tests/golden/sde_demo, tools/bson_fixture.py)
    loss      l2_means + l2_vars (+ 0.2 sum(sv.saveval) when regularised), u0 = (2, 0) repeated 100 times
    training  250 iterations of AdaBelief(0.01), one fused call per iteration (rnde_nsde_moment_grad) + one optimiser launch

Prints the reference's @show fields every 50 iterations (i, loss, l2_means, l2_vars, reg, nfe1, nfe2) and at the end the loss and NFE at the
last parameters (loss_function(u0, ps_best, -1)), the training time per iteration and the prediction time of one layer call; writes
profiles/sde_toy.json.  ms_per_iter is what the reference's total_time covers (sde_toy_problem.jl:69-73): the forward and the gradient, synchronised,
WITHOUT the optimiser update; ms_per_iter_with_update adds the AdaBelief launch.  Weights come from torch's generator seeded with the seed
(Julia's Random.seed! stream is not reproduced).

    python tools/train_sde_toy.py [--iters 250] [--seed 5] [--out profiles/sde_toy.json]
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

import regneuralde_jl_amd as rn  # noqa: E402


def load_fixture(name):
    """(T, D) float32 tensor of a D x T fixture of tests/golden/sde_demo (exact bit patterns)."""
    bits, size = [], None
    for line in open(os.path.join(ROOT, "tests", "golden", "sde_demo", name + ".txt")):
        if line.startswith("# size"):
            size = [int(v) for v in line.split()[2:]]
        elif not line.startswith("#"):
            bits.append(int(line.split()[0], 16))
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).reshape(size[1], size[0]).copy())


def run(regularize, seed, iters, dev):
    g = torch.Generator().manual_seed(seed)
    drift = rn.Chain(lambda x: x ** 3, rn.Dense(2, 50, "tanh", g), rn.Dense(50, 2, "identity", g))
    nsde = rn.TrackedNeuralDSDE(drift, rn.Dense(2, 2, "identity", g), [0.0, 1.0 + float(np.finfo(np.float32).eps)], regularize, "SOSRI",
                                saveat=torch.linspace(0, 1, 30), reltol=0.3, abstol=0.3, max_batch=100, seed=seed)
    dm, dv = load_fixture("sde_data").to(dev), load_fixture("sde_data_vars").to(dev)
    u0 = torch.tensor([[2.0, 0.0]], device=dev).repeat(100, 1)
    p = nsde.p.to(dev)
    opt = rn.FluxAdaBelief([p], eta=0.01)
    rn.fused_moment_loss_and_grad(nsde, u0, dm, dv, c=0.2, p=p)      # the reference's warm-up gradient (not counted)
    p.grad = None
    torch.cuda.synchronize()
    total, total_step = 0.0, 0.0
    for it in range(1, iters + 1):
        t = time.perf_counter()
        loss, l2m, l2v, reg, n1, n2 = rn.fused_moment_loss_and_grad(nsde, u0, dm, dv, c=0.2, p=p)
        torch.cuda.synchronize()
        t_grad = time.perf_counter()
        opt.step()
        torch.cuda.synchronize()
        total += t_grad - t                          # the reference's total_time: forward + gradient, not update_parameters!
        total_step += time.perf_counter() - t
        if it % 50 == 0:
            print(f"(i, loss, l2_means, l2_vars, reg, nfe1, nfe2) = ({it}, {float(l2m + l2v):.6g}, {float(l2m):.6g}, {float(l2v):.6g}, {reg:.6g}, {n1}, {n2})",
                  flush=True)
    with torch.no_grad():
        sol, nfe1, nfe2, sv = nsde(u0, p)
        l2 = rn.moment_loss(sol, dm, dv)
        final = float(l2[0] + l2[1])
        for _ in range(3):
            nsde(u0, p)
        torch.cuda.synchronize()
        reps, t = 20, time.perf_counter()
        for _ in range(reps):
            nsde(u0, p)
        torch.cuda.synchronize()
        ptime = (time.perf_counter() - t) / reps
    res = dict(regularize=regularize, seed=seed, iters=iters, final_loss=final, nfe=int(nfe1), ms_per_iter=1e3 * total / iters,
               ms_per_iter_covers="forward + gradient (rnde_nsde_moment_grad), synchronised; not the optimiser update",
               ms_per_iter_with_update=1e3 * total_step / iters,
               train_s=total, predict_ms=1e3 * ptime, finite=bool(np.isfinite(final)))
    print(f"(train time, loss, nfe, prediction time) = ({total:.3f} s, {final:.6g}, {nfe1}, {1e3 * ptime:.3f} ms)   "
          f"{res['ms_per_iter']:.3f} ms per iteration (forward + gradient), {res['ms_per_iter_with_update']:.3f} with the update", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=250)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sde_toy.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_sde_toy.py needs the MI355X")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "runs": [run(reg, a.seed, a.iters, dev) for reg in (False, True)]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
