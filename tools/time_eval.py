"""Time of the evaluation passes of the two ODE experiments, the torch path against the path behind the C ABI, at the experiments' sizes.

  mnist    ClassifierNODE(MLPDynamics(784, 100), Tsit5 at 1.4e-8, Dense(784, 10)), 20 batches of 512 (experiments/mnist_node.jl:185-186)
           accuracy(model, batches)        the layer call, then u @ W + b, argmax, ==, .sum().item() in torch: a read-back per batch
           node_accuracy(model, batches)   ONE rnde_node_classifier_predict per batch into one device counter, one read-back per pass
  latent   the reference's latent-ODE model, batches of 512 x 49 save times (experiments/latent_ode.jl:271-292)
           torch composition               LatentTimeSeriesModel.__call__ (GRU, encoder, decoder as eager torch ops around the layer call),
                                           then sum(sum((pred .* m - d .* m) .^ 2) ./ sum(m)) and a read-back per batch
           latent_total_loss               rnde_latent_encode, rnde_node_forward_saveat (untaped), rnde_latent_decode_mse; one read-back per pass
           (both on the same reparameterisation samples)

A sample is the host time of one whole pass between two device synchronisations (both passes end in a read-back); the two variants of a pair
alternate inside every round of one process, after `--warmup` untimed rounds.  The NFE of every batch is asserted equal between the two paths.
Writes min / median / max per variant to profiles/eval_device.json.

    python tools/time_eval.py [--rounds 7] [--warmup 2] [--batches 20] [--latent-batches 4]
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(variants, warmup, rounds):
    ms = {k: [] for k in variants}
    for r in range(warmup + rounds):
        for k, fn in variants.items():                # alternated: both sides see the same clocks and the same neighbours
            v = timed(fn)
            if r >= warmup:
                ms[k].append(v)
    return {k: dict(min=float(np.min(v)), median=float(np.median(v)), max=float(np.max(v)), samples_ms=v) for k, v in ms.items()}


def overlap(a, b):
    return not (a["max"] < b["min"] or b["max"] < a["min"])


def pair(res, old, new):
    return dict(ms_per_pass=res, ranges_overlap=overlap(res[old], res[new]), median_ratio_old_over_new=res[old]["median"] / res[new]["median"])


def mnist_leg(rn, dev, B, n_batches, warmup, rounds):
    g = torch.Generator().manual_seed(7)
    node = rn.TrackedNeuralODE(rn.MLPDynamics(784, 100, generator=g), [0.0, 1.0], True, True, "Tsit5", save_everystep=False, reltol=1.4e-8, abstol=1.4e-8,
                               save_start=False, max_batch=B, max_attempts=160)
    model = rn.ClassifierNODE(node, rn.Dense(784, 10, generator=g), device=dev)
    batches = [(torch.rand(B, 784, generator=g).to(dev), torch.eye(10)[torch.randint(0, 10, (B,), generator=g)].to(dev)) for _ in range(n_batches)]
    got = {}

    def torch_path():
        got["accuracy"] = rn.accuracy(model, batches)

    def device_path():
        got["node_accuracy"] = rn.node_accuracy(model, batches)
    res = alternate({"accuracy": torch_path, "node_accuracy": device_path}, warmup, rounds)
    assert got["accuracy"] == got["node_accuracy"], got
    with torch.no_grad():
        nfe_t = [int(model(x)[1]) for x, _ in batches]
    nfe_d = [int(model.predict(x)[1]) for x, _ in batches]
    assert nfe_t == nfe_d, (nfe_t, nfe_d)
    out = pair(res, "accuracy", "node_accuracy")
    out.update(batch=B, batches=n_batches, nfe_per_batch=nfe_d, accuracy=got["accuracy"])
    return out


def latent_leg(rn, dev, B, T, n_batches, warmup, rounds):
    g = torch.Generator().manual_seed(5)
    grid = torch.linspace(0, 1, T)
    model = rn.build_latent_ode(saveat=grid.tolist(), regularize=True, generator=g, device=dev, max_batch=B, max_attempts=256)
    batches, eps = [], []
    for _ in range(n_batches):
        data = torch.randn(B, T, 37, generator=g).to(dev)
        mask = (torch.rand(B, T, 37, generator=g) < 0.3).float().to(dev)
        mask[:, 0, 0] = 1.0
        t_row = torch.full((B, T, 1), 1.0 / (T - 1), device=dev); t_row[:, -1] = 0.0
        batches.append((data, mask, t_row))
        eps.append(torch.randn(B, 20, generator=g).to(dev))
    got, nfe = {}, {}
    real_randn = torch.randn

    def torch_path():                                   # total_loss_on_dataset as the reference writes it, on LatentTimeSeriesModel.__call__
        loss, count, n = 0.0, 0, []
        with torch.no_grad():
            for (d, m, t), e in zip(batches, eps):
                try:
                    torch.randn = lambda *a, **k: e      # the same sample as the device path (time_series.jl:58 draws it)
                    result, _, _, k, _ = model(torch.cat([d, m, t], dim=2))
                finally:
                    torch.randn = real_randn
                dp = result * m - d * m
                loss += float(((dp ** 2).sum(dim=(1, 2)) / m.sum(dim=(1, 2))).sum().item())
                count += d.shape[0]
                n.append(int(k))
        got["torch"], nfe["torch"] = loss / count, n

    def device_path():
        got["device"] = rn.latent_total_loss(model, batches, eps=eps)
        nfe["device"] = list(model.last_eval_nfe)
    res = alternate({"torch_composition": torch_path, "latent_total_loss": device_path}, warmup, rounds)
    assert nfe["torch"] == nfe["device"], nfe
    out = pair(res, "torch_composition", "latent_total_loss")
    out.update(batch=B, save_times=T, batches=n_batches, nfe_per_batch=nfe["device"], loss_torch=got["torch"], loss_device=got["device"],
               loss_rel_difference=abs(got["torch"] - got["device"]) / abs(got["torch"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--latent-batches", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_device.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert a.rounds >= 5
    import regneuralde_jl_amd as rn
    dev = torch.device("cuda", 0)
    out = dict(method=f"host clock around one whole pass between two device synchronisations; {a.rounds} rounds after {a.warmup} warm-up rounds, the two variants "
                      "of a pair alternated inside every round of one process; NFE of every batch asserted equal between the two paths",
               mnist=mnist_leg(rn, dev, a.batch, a.batches, a.warmup, a.rounds),
               latent=latent_leg(rn, dev, a.batch, 49, a.latent_batches, a.warmup, a.rounds))
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
