"""The reference's gaussian-mixture FFJORD experiment (experiments/ffjord_gaussian.jl) on the device: MLPDynamics(2, 16), TrackedFFJORD
with Tsit5 at reltol = abstol = 1.4e-8, Optimiser(WeightDecay(1e-5), ADAM(4e-2)), 20 epochs of batches of 1024, lambda 2000 -> 1000
(lambda_func), --regularize 0|1.

Per epoch: NFE of an inference call on the first batch, train / test log-likelihood (src/metrics.jl:20-33), train time, inference time;
then the sampling time of 1024 points (minimum of 10 runs).  In the same run: the training step of an eager-torch fp32 restatement on the
GPU along the device's own step sequence (equal work) against the device's step, both warmed up, median and range of --reps runs each.
The restatement is tests/ffjord_ref.py (the fp64 reference of the test suite, run here in fp32): the tool imports it from the repository
tree, which it puts on sys.path itself.  Solve and reverse times per step come from the library's HIP events.  Output: one entry per
--regularize setting in profiles/ffjord_gaussian.json.

--kinetic LK LJ (opt-in; with --regularize 0) trains with the RNODE regulariser instead: the {false} method called with regularize = true,
loss = -mean(logpx) + LK mean(lambda1) + LJ mean(lambda2) (kinetic energy, Jacobian norm); the entry "kinetic" goes to
profiles/ffjord_gaussian_kinetic.json.

--exact-eval reports the train / test log-likelihood with the exact trace (no probe, no variance) and --exact-train also trains through it
(ffjord(x, p, exact=True): the reverse sweep costs about D + 1 = 3 Hutchinson ones at D = 2); both run the layer on engine="tiled", and their
entries go to profiles/ffjord_gaussian_exact.json.  The equal-work comparison stays the Hutchinson step's.

    python tools/train_ffjord_gaussian.py --regularize 1
    python tools/train_ffjord_gaussian.py --regularize 1 --exact-eval --exact-train
    python tools/train_ffjord_gaussian.py --regularize 0 --kinetic 0.01 0.01
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


def _sync():
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regularize", type=int, default=1, choices=[0, 1])
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7, help="timed runs of each side of the equal-work comparison (after 2 warm-up runs)")
    ap.add_argument("--kinetic", type=float, nargs=2, default=None, metavar=("LK", "LJ"),
                    help="train with LK mean(lambda1) + LJ mean(lambda2) (kinetic energy, Jacobian norm); needs --regularize 0")
    ap.add_argument("--exact-eval", action="store_true", help="train / test log-likelihood with the exact trace (engine=\"tiled\")")
    ap.add_argument("--exact-train", action="store_true", help="train through the exact trace too (engine=\"tiled\"; not with --kinetic)")
    ap.add_argument("--track-ctrl", action="store_true",
                    help="differentiate the step controller in the reverse pass (engine=\"tiled\", needs --regularize 1; the equal-work comparison's "
                         "eager restatement keeps its constant steps)")
    ap.add_argument("--eval-groups", type=int, default=1, metavar="K",
                    help="train / test log-likelihood with K consecutive batches per launch (engine=\"tiled\"; 1: one solve per batch)")
    ap.add_argument("--one-call", action="store_true",
                    help="the training step through rnde_ffjord_nll_grad and rnde_adam_wd_step (fused_ffjord_loss_and_grad, "
                         "FluxADAM(one_launch=True)) instead of the layer call, the torch loss, backward() and the composed optimiser")
    ap.add_argument("--out", default=None, help="default: profiles/ffjord_gaussian.json (profiles/ffjord_gaussian_kinetic.json with --kinetic, "
                                                "profiles/ffjord_gaussian_exact.json with --exact-eval / --exact-train, "
                                                "profiles/ffjord_gaussian_track.json with --track-ctrl)")
    a = ap.parse_args()
    if a.kinetic and a.regularize:
        ap.error("--kinetic needs --regularize 0 (the {true} method never passes regularize on)")
    if a.kinetic and a.exact_train:
        ap.error("--exact-train does not go with --kinetic (the Jacobian norm row is defined on the probe)")
    if a.track_ctrl and not a.regularize:
        ap.error("--track-ctrl needs --regularize 1 (without a saved value the tracked and the constant-step sweep agree to O(tol))")
    if a.eval_groups < 1:
        ap.error("--eval-groups K needs K >= 1")
    exact_any = a.exact_eval or a.exact_train
    a.out = a.out or os.path.join(ROOT, "profiles", "ffjord_gaussian_kinetic.json" if a.kinetic else
                                  ("ffjord_gaussian_track.json" if a.track_ctrl else
                                   ("ffjord_gaussian_exact.json" if exact_any else "ffjord_gaussian.json")))
    kin = bool(a.kinetic)
    lk, lj = a.kinetic or (0.0, 0.0)
    import regneuralde_jl_amd as rn
    from tests import ffjord_kinetic_ref as K
    from tests import ffjord_ref as R

    dev = torch.device("cuda", 0)
    tr, te = rn.load_gaussian_mixture(a.batch, nsamples=2048, ngaussians=6, seed=a.seed)
    model = rn.ffjord.MLPDynamics(2, 16, generator=torch.Generator().manual_seed(a.seed))
    ff = rn.TrackedFFJORD(model, [0.0, 1.0], True, bool(a.regularize), "Tsit5", reltol=1.4e-8, abstol=1.4e-8, max_batch=a.batch,
                          **(dict(engine="tiled") if exact_any or a.track_ctrl or a.eval_groups > 1 else {}), track_ctrl=a.track_ctrl)
    p = ff.p.clone().requires_grad_(True)
    ll = lambda data: rn.loglikelihood(ff, data, p.detach(), exact=a.exact_eval, groups=a.eval_groups)
    opt = rn.FluxADAM([p], eta=4e-2, weight_decay=1e-5, one_launch=a.one_call)
    lam0, lam1 = 2.0e3, 1.0e3
    k = np.log(lam0 / lam1) / a.epochs
    dummy = torch.from_numpy(tr.X[:a.batch]).to(dev)

    def infer():
        _sync()
        t0 = time.perf_counter()
        with torch.no_grad():
            _, _, _, nfe, _ = ff(dummy, p.detach())
        _sync()
        return nfe, time.perf_counter() - t0

    rows = []
    nfe, ti = infer()
    rows.append(dict(epoch=0, nfe=nfe, train_ll=ll(tr), test_ll=ll(te),
                     train_s=0.0, infer_s=ti))
    print(rows[-1], flush=True)
    step_ms, solve_ms, rev_ms, att, accd = [], [], [], [], []
    for epoch in range(1, a.epochs + 1):
        lam = lam0 * np.exp(-k * (epoch - 1))
        timing = 0.0
        for xb in tr:
            x = torch.from_numpy(xb).to(dev)
            _sync()
            t0 = time.perf_counter()
            if a.one_call:        # (the loss stays a device scalar; it is read once per epoch, below)
                nll, reg, m1, m2, nfe = rn.fused_ffjord_loss_and_grad(ff, x, p, lam_r=float(lam) if a.regularize else 0.0,
                                                                      kinetic=(lk, lj) if kin else None, exact=a.exact_train)
                loss = nll + reg + lk * m1 + lj * m2
            else:
                logpx, l1, l2, nfe, sv = ff(x, p, exact=True) if a.exact_train else ff(x, p, regularize=kin)
                loss = -logpx.mean() + (lam * sv.saveval.mean() if a.regularize else 0.0)
                if kin:
                    loss = loss + lk * l1.mean() + lj * l2.mean()
                loss.backward()
            opt.step()
            _sync()
            dt = time.perf_counter() - t0
            timing += dt
            if x.shape[0] == a.batch:
                step_ms.append(dt * 1e3)
                s, r, n, m = ff.timing()
                solve_ms.append(s); rev_ms.append(r); att.append(n); accd.append(m)
        nfe, ti = infer()
        rows.append(dict(epoch=epoch, nfe=nfe, train_ll=ll(tr), test_ll=ll(te),
                         train_s=timing, infer_s=ti, loss_last=float(loss.detach())))
        print(rows[-1], flush=True)
    samp = []
    for _ in range(10):
        _sync()
        t0 = time.perf_counter()
        rn.sample(ff, 2, p.detach(), nsamples=a.batch)
        _sync()
        samp.append(time.perf_counter() - t0)

    # the eager-torch fp32 restatement: the training step along the device's own step sequence of the same batch, probe and weights
    x = dummy
    e = torch.randn(a.batch, 2, device=dev)
    lam_end = lam0 * np.exp(-k * (a.epochs - 1))

    def device_step():
        logpx, l1, l2, _, sv = ff(x, p, e, regularize=kin)
        loss = -logpx.mean() + (lam_end * sv.saveval.mean() if a.regularize else 0.0)
        if kin:
            loss = loss + lk * l1.mean() + lj * l2.mean()
        loss.backward()
        p.grad = None

    device_step()
    acc = [float(d) for d, f in np.array(ff.steps()).reshape(-1, 2) if f]
    pt = p.detach().clone().requires_grad_(True)
    F = (lambda u, t: K.rhs_kinetic(pt, 2, 16, u, t, e)) if kin else (lambda u, t: R.rhs(pt, 2, 16, u, t, e))

    def eager_step():
        u, eests = R.replay(F, torch.cat([x, torch.zeros(a.batch, 3 if kin else 1, device=dev)], 1), 0.0, acc, 1.4e-8, 1.4e-8)
        l2 = -R.logpx_of(u, 2).mean()
        if kin:
            l2 = l2 + lk * u[:, 3].mean() + lj * u[:, 4].mean()
        if a.regularize:
            l2 = l2 + lam_end * torch.stack([ee * d for ee, d in zip(eests, acc)]).sum() / (len(acc) + 1)
        l2.backward()
        pt.grad = None

    def timed(fn):
        for _ in range(2):
            fn()
        out = []
        for _ in range(a.reps):
            _sync()
            t0 = time.perf_counter()
            fn()
            _sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), max_ms=float(max(out)), runs=a.reps)

    dev_t = timed(device_step)
    eager_t = timed(eager_step)
    res = dict(regularize=a.regularize, track_ctrl=a.track_ctrl, exact_eval=a.exact_eval, exact_train=a.exact_train, engine=ff.engine, kinetic=list(a.kinetic) if kin else None, epochs=rows, sampling_time_s=min(samp), batch=a.batch,
               train_step_ms_median=float(np.median(step_ms)), solve_launch_ms_median=float(np.median(solve_ms)),
               reverse_ms_median=float(np.median(rev_ms)), attempts_median=float(np.median(att)), accepted_median=float(np.median(accd)),
               us_per_forward_attempt=float(np.median(np.array(solve_ms) / np.array(att)) * 1e3),
               us_per_reversed_step=float(np.median(np.array(rev_ms) / np.array(accd)) * 1e3),
               equal_work_step=dict(accepted_steps=len(acc), device=dev_t, eager_torch_fp32=eager_t,
                                    speedup_median=dev_t and eager_t["median_ms"] / dev_t["median_ms"]))
    print(json.dumps({k: v for k, v in res.items() if k != "epochs"}), flush=True)
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["kinetic" if kin else "regularize_%d" % a.regularize] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
