"""The reference's tabular FFJORD experiment (experiments/ffjord_tabular.jl) on the device with the tiled engine: MLPDynamics(43, 100),
TrackedFFJORD with Tsit5 at reltol = abstol = 1.4e-8, Optimiser(WeightDecay(1e-5), ADAM(1e-2)), batches of 1024, lambda 5000 -> 1000
(lambda_func), --regularize 0|1.  Data: MiniBooNE (load_miniboone, src/dataset.jl:33-56) when --data points at miniboone.npy, otherwise a
fixed synthetic 43-dimensional dataset (correlated gaussians, 4096 samples, the same 80 / 20 split).

Per epoch: NFE of an inference call on the first batch, train / test log-likelihood (src/metrics.jl:20-33), train time, inference time;
then the sampling time of 1024 points (minimum of 10 runs).  In the same run: the training step of an eager-torch fp32 restatement on the
GPU along the device's own step sequence (equal work) against the device's step, both warmed up, median and range of --reps runs each.
The restatement is tests/ffjord_ref.py (the fp64 reference of the test suite, run here in fp32): the tool imports it from the repository
tree, which it puts on sys.path itself.  Solve and reverse times per step come from the library's HIP events.  Output: one entry per
--regularize setting in profiles/ffjord_tabular.json, plus (--gaussian-geometry) the tiled engine's forward and reverse times at the
gaussian experiment's MLPDynamics(2, 16), B = 1024, for the comparison with the one-workgroup engine.

--kinetic LK LJ (opt-in; with --regularize 0) trains with the RNODE regulariser instead: the {false} method called with regularize = true,
loss = -mean(logpx) + LK mean(lambda1) + LJ mean(lambda2) (kinetic energy, Jacobian norm); the entry "kinetic" goes to
profiles/ffjord_tabular_kinetic.json.

--exact-eval reports the train / test log-likelihood with the exact trace (ffjord(x, p, exact=True): no probe, no variance) on
engine="tiled"; training stays on the Hutchinson estimate (an exact reverse sweep costs about D + 1 = 44 of them here).  The entry goes to
profiles/ffjord_tabular_exact.json.

    python tools/train_ffjord_tabular.py --regularize 1 --epochs 3
    python tools/train_ffjord_tabular.py --regularize 1 --epochs 3 --exact-eval
    python tools/train_ffjord_tabular.py --regularize 0 --kinetic 0.01 0.01 --epochs 3
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


def synthetic(batch, D, seed, n=4096, split=0.8):
    """A fixed 43-dimensional dataset: correlated gaussians with a few heavy columns, shuffled, split as load_miniboone splits."""
    import regneuralde_jl_amd as rn
    rng = np.random.default_rng(1234)
    A = rng.standard_normal((D, D)) / np.sqrt(D)
    X = rng.standard_normal((n, D)) @ A
    X[:, :5] = np.sinh(X[:, :5])
    X = ((X - X.mean(0)) / X.std(0, ddof=1)).astype(np.float32)
    X = X[np.random.default_rng(seed).permutation(n)]
    ntr = int(split * n)
    return rn.ffjord._Loader(X[:ntr].copy(), batch, True, seed + 1), rn.ffjord._Loader(X[ntr:].copy(), batch, False, seed + 2)


def gaussian_geometry(rn, engine, dev, B=1024, reps=5):
    """Forward us per attempt and reverse us per reversed step of `engine` at MLPDynamics(2, 16), B = 1024, tol 1.4e-8 (median of reps)."""
    tr, _ = rn.load_gaussian_mixture(B, nsamples=2048, seed=0)
    m = rn.ffjord.MLPDynamics(2, 16, generator=torch.Generator().manual_seed(0))
    ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, True, "Tsit5", reltol=1.4e-8, abstol=1.4e-8, max_batch=B, engine=engine)
    x = torch.from_numpy(next(iter(tr))).to(dev)
    fa, rs = [], []
    for i in range(reps + 1):
        p = ff.p.clone().requires_grad_(True)
        lp, _, _, _, sv = ff(x, p)
        (-lp.mean() + 1e3 * sv.saveval.mean()).backward()
        torch.cuda.synchronize()
        s, r, n, acc = ff.timing()
        if i:
            fa.append(s / n * 1e3); rs.append(r / acc * 1e3)
    return dict(engine=engine, D=2, H=16, batch=B, us_per_forward_attempt=float(np.median(fa)), us_per_reversed_step=float(np.median(rs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regularize", type=int, default=1, choices=[0, 1])
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--data", default=None, help="miniboone.npy (default: the synthetic dataset)")
    ap.add_argument("--engine", default="tiled", choices=["tiled", "workgroup"])
    ap.add_argument("--gaussian-geometry", type=int, default=1, help="also time the engine at MLPDynamics(2, 16), B = 1024")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7, help="timed runs of each side of the equal-work comparison (after 2 warm-up runs)")
    ap.add_argument("--kinetic", type=float, nargs=2, default=None, metavar=("LK", "LJ"),
                    help="train with LK mean(lambda1) + LJ mean(lambda2) (kinetic energy, Jacobian norm); needs --regularize 0")
    ap.add_argument("--exact-eval", action="store_true", help="train / test log-likelihood with the exact trace (needs --engine tiled)")
    ap.add_argument("--track-ctrl", action="store_true",
                    help="differentiate the step controller in the reverse pass (needs --engine tiled and --regularize 1)")
    ap.add_argument("--eval-groups", type=int, default=1, metavar="K",
                    help="train / test log-likelihood with K consecutive batches per launch (needs --engine tiled; 1: one solve per batch)")
    ap.add_argument("--one-call", action="store_true",
                    help="the training step through rnde_ffjord_nll_grad and rnde_adam_wd_step (fused_ffjord_loss_and_grad, "
                         "FluxADAM(one_launch=True)) instead of the layer call, the torch loss, backward() and the composed optimiser")
    ap.add_argument("--out", default=None, help="default: profiles/ffjord_tabular.json (profiles/ffjord_tabular_kinetic.json with --kinetic, "
                                                "profiles/ffjord_tabular_exact.json with --exact-eval, profiles/ffjord_tabular_track.json with "
                                                "--track-ctrl)")
    a = ap.parse_args()
    if a.kinetic and a.regularize:
        ap.error("--kinetic needs --regularize 0 (the {true} method never passes regularize on)")
    if a.exact_eval and a.engine != "tiled":
        ap.error("--exact-eval needs --engine tiled (the exact trace is served by the tiled engine only)")
    if a.track_ctrl and (a.engine != "tiled" or not a.regularize):
        ap.error("--track-ctrl needs --engine tiled and --regularize 1 (without a saved value the tracked and the constant-step sweep agree to O(tol))")
    if a.eval_groups < 1 or (a.eval_groups > 1 and a.engine != "tiled"):
        ap.error("--eval-groups K needs K >= 1, and --engine tiled for K > 1 (the one-workgroup engine has no tiles to share a launch between)")
    a.out = a.out or os.path.join(ROOT, "profiles", "ffjord_tabular_kinetic.json" if a.kinetic else
                                  ("ffjord_tabular_track.json" if a.track_ctrl else
                                   ("ffjord_tabular_exact.json" if a.exact_eval else "ffjord_tabular.json")))
    kin = bool(a.kinetic)
    lk, lj = a.kinetic or (0.0, 0.0)
    import regneuralde_jl_amd as rn
    from tests import ffjord_kinetic_ref as K
    from tests import ffjord_ref as R

    dev = torch.device("cuda", 0)
    D, H = 43, 100
    if a.data:
        tr, te = rn.load_miniboone(a.batch, a.data, 0.8, seed=a.seed)
    else:
        tr, te = synthetic(a.batch, D, a.seed)
    model = rn.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(a.seed))
    ff = rn.TrackedFFJORD(model, [0.0, 1.0], True, bool(a.regularize), "Tsit5", reltol=1.4e-8, abstol=1.4e-8, max_batch=a.batch, engine=a.engine,
                          track_ctrl=a.track_ctrl)
    p = ff.p.clone().requires_grad_(True)
    ll = lambda data: rn.loglikelihood(ff, data, p.detach(), exact=a.exact_eval, groups=a.eval_groups)
    opt = rn.FluxADAM([p], eta=1e-2, weight_decay=1e-5, one_launch=a.one_call)
    lam0, lam1 = 5.0e3, 1.0e3
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
                                                                      kinetic=(lk, lj) if kin else None)
                loss = nll + reg + lk * m1 + lj * m2
            else:
                logpx, l1, l2, nfe, sv = ff(x, p, regularize=kin)
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
        rn.sample(ff, D, p.detach(), nsamples=a.batch)
        _sync()
        samp.append(time.perf_counter() - t0)

    # the eager-torch fp32 restatement: the training step along the device's own step sequence of the same batch, probe and weights
    x = dummy
    e = torch.randn(a.batch, D, device=dev)
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
    F = (lambda u, t: K.rhs_kinetic(pt, D, H, u, t, e)) if kin else (lambda u, t: R.rhs(pt, D, H, u, t, e))

    def eager_step():
        u, eests = R.replay(F, torch.cat([x, torch.zeros(a.batch, 3 if kin else 1, device=dev)], 1), 0.0, acc, 1.4e-8, 1.4e-8)
        l2 = -R.logpx_of(u, D).mean()
        if kin:
            l2 = l2 + lk * u[:, D + 1].mean() + lj * u[:, D + 2].mean()
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
    res = dict(regularize=a.regularize, track_ctrl=a.track_ctrl, exact_eval=a.exact_eval, kinetic=list(a.kinetic) if kin else None, engine=a.engine, data=("miniboone" if a.data else "synthetic"), epochs=rows, sampling_time_s=min(samp), batch=a.batch,
               train_step_ms_median=float(np.median(step_ms)), solve_launch_ms_median=float(np.median(solve_ms)),
               reverse_ms_median=float(np.median(rev_ms)), attempts_median=float(np.median(att)), accepted_median=float(np.median(accd)),
               us_per_forward_attempt=float(np.median(np.array(solve_ms) / np.array(att)) * 1e3),
               us_per_reversed_step=float(np.median(np.array(rev_ms) / np.array(accd)) * 1e3),
               equal_work_step=dict(accepted_steps=len(acc), device=dev_t, eager_torch_fp32=eager_t,
                                    speedup_median=dev_t and eager_t["median_ms"] / dev_t["median_ms"]))
    if a.gaussian_geometry and not kin:
        res["gaussian_geometry"] = gaussian_geometry(rn, a.engine, dev)
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
