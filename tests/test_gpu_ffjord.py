"""TrackedFFJORD on the device (rnde_ffjord_*) against the fp64 torch restatements of tests/ffjord_ref.py (themselves checked against the CPU
oracle, torch.autograd.functional.jacobian and double-backward in tests/test_ffjord_host.py): one evaluation of the augmented right-hand side,
the solve and its reverse along a fixed step sequence, the adaptive controller in the truncation regime, sample(), and a training step."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ffjord_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _layer(D, H, B, seed, regularize=True, tol=1e-5, scale=1.0, **kw):
    import regneuralde_jl_amd as rn
    m = rn.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(seed))
    ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, regularize, "Tsit5", reltol=tol, abstol=tol, max_batch=B, **kw)
    rng = np.random.default_rng(seed)
    ff.p = torch.from_numpy(R.glorot_params(D, H, rng, scale=scale)).to(DEV)
    return ff, rng


def _aug(x):
    return torch.cat([x, torch.zeros(x.shape[0], 1, dtype=x.dtype)], 1)


@pytest.mark.parametrize("D,H", [(2, 16), (16, 64)])
@pytest.mark.parametrize("B", [1, 1000, 1024])
def test_rhs_matches_fp64(D, H, B):
    """f and the trace row, Hutchinson and exact, against fp64 at the experiment's shape and at (16, 64); B = 1, a partial tile, a full batch."""
    ff, rng = _layer(D, H, B, 1)
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
    e = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
    P = ff.p.cpu().double()
    for t in (0.0, 0.71):
        got = ff.feval(x.to(DEV), t, e.to(DEV)).cpu()
        ref = R.rhs(P, D, H, _aug(x.double()), t, e.double())
        assert _rel(got[:, :D], ref[:, :D]) <= 2e-6 and _rel(got[:, D], ref[:, D]) <= 2e-5
        got = ff.feval(x.to(DEV), t).cpu()
        ref = R.rhs(P, D, H, _aug(x.double()), t)
        assert _rel(got[:, D], ref[:, D]) <= 2e-5


@pytest.mark.parametrize("D,H", [(2, 16), (16, 64)])
def test_replay_forward_and_reverse(D, H):
    """Along a fixed all-accepted sequence: logpx and the saved values EEst * dt against the fp64 replay; p-bar and x-bar against autograd
    through it, with and without the EEst * dt cotangent.  Weights and steps are large enough that EEst is truncation error (0.2 .. 3 here), not
    fp32 rounding (~1e-4 at this tolerance): with EEst at its rounding floor no fp32 implementation can match fp64."""
    B = 37
    ff, rng = _layer(D, H, B, 2, scale=3.0)
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
    e = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
    dts = [0.5, 0.5]
    steps = sum(([dt, 1.0] for dt in dts), [])
    Pg = ff.p.cpu().double().requires_grad_(True)
    Xg = x.double().requires_grad_(True)
    F = lambda u, t: R.rhs(Pg, D, H, u, t, e.double())
    u, eests = R.replay(F, _aug(Xg), 0.0, dts, 1e-5, 1e-5)
    lp_ref = R.logpx_of(u, D)
    sv_ref = torch.stack([torch.zeros((), dtype=torch.float64)] + [ee * dt for ee, dt in zip(eests, dts)])
    g = torch.from_numpy(rng.standard_normal(B))
    for with_sv in (False, True):
        xd = x.to(DEV).requires_grad_(True)
        p = ff.p.clone().requires_grad_(True)
        logpx, _, _, nfe, sv = ff(xd, p, e.to(DEV), steps=steps)
        assert nfe == 3 + 6 * len(dts) and sv.saveval.numel() == len(dts) + 1
        assert _rel(logpx, lp_ref) <= 1e-5
        assert _rel(sv.saveval, sv_ref) <= 5e-3
        w = torch.linspace(0.5, 1.5, len(dts) + 1, dtype=torch.float64) * 100.0 if with_sv else torch.zeros(len(dts) + 1, dtype=torch.float64)
        loss = (logpx * g.float().to(DEV)).sum() + (sv.saveval * w.float().to(DEV)).sum()
        loss.backward()
        ref = (lp_ref * g).sum() + (sv_ref * w).sum()
        gx, gp = torch.autograd.grad(ref, (Xg, Pg), retain_graph=True)
        tol = 5e-3 if with_sv else 1e-3
        assert _rel(xd.grad, gx) <= tol, _rel(xd.grad, gx)
        assert _rel(p.grad, gp) <= tol, _rel(p.grad, gp)
        if with_sv:        # the cotangent reached p-bar through EEst
            g0 = torch.autograd.grad((lp_ref * g).sum(), Pg, retain_graph=True)[0]
            assert _rel(gp, g0) > 1e-3


def test_adaptive_solve_truncation_regime_and_reference_tolerance():
    """tol 1e-5: attempted and accepted steps equal those of the fp64 controller.  tol 1.4e-8: the solution along the device's own steps, and one
    saved value per accepted step (plus the one at init); no NFE is asserted there.  (The case is stiff enough that every attempt's EEst is
    >= 0.02 in fp64, two orders above the fp32 rounding floor.)"""
    D, H, B = 2, 16, 256
    ff, rng = _layer(D, H, B, 5, scale=8.0)
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32) * 3)
    e = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
    P = ff.p.cpu().double()
    F = lambda u, t: R.rhs(P, D, H, u, t, e.double())
    with torch.no_grad():
        logpx, _, _, nfe, sv = ff(x.to(DEV), None, e.to(DEV))
    st = np.array(ff.steps()).reshape(-1, 2)
    _, log = R.solve(F, _aug(x.double()), 0.0, 1.0, 1e-5, 1e-5)
    assert min(l[2] for l in log) >= 0.02 and sum(not l[3] for l in log) > 0
    assert len(st) == len(log) and [bool(a) for a in st[:, 1]] == [a for *_, a in log]
    # dt follows to fp32 EEst (1 % of 0.02 at worst) except the last, clamped step t1 - t, which inherits the sum of the differences
    assert np.abs(st[:-1, 0] / np.array([l[1] for l in log[:-1]]) - 1).max() <= 2e-2
    assert nfe == 3 + 6 * len(st) and sv.saveval.numel() == int(st[:, 1].sum()) + 1
    # the reference tolerance, on a model at the Glorot scale the experiment starts from (the stiff one above needs > 4096 attempts there)
    ff2, rng = _layer(D, H, B, 3, tol=1.4e-8)
    P = ff2.p.cpu().double()
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
    with torch.no_grad():
        logpx, _, _, nfe, sv = ff2(x.to(DEV), None, e.to(DEV))
    st = np.array(ff2.steps()).reshape(-1, 2)
    acc = [float(d) for d, a in st if a]
    assert sv.saveval.numel() == len(acc) + 1 and torch.isfinite(sv.saveval).all()
    with torch.no_grad():
        u, _ = R.replay(F, _aug(x.double()), 0.0, acc, 1.4e-8, 1.4e-8)
    assert _rel(logpx, R.logpx_of(u, D)) <= 1e-5


def test_sample_matches_reverse_time_replay_and_round_trips():
    """sample() against the fp64 solve of -F(u, t1 - tau) with the exact trace along the device's steps; a forward solve of the samples returns z."""
    import regneuralde_jl_amd as rn
    D, H, B = 2, 16, 300
    ff, rng = _layer(D, H, B, 4, tol=1e-6)
    z = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
    xs = rn.sample(ff, D, nsamples=B, z=z.to(DEV))
    st = np.array(ff.steps()).reshape(-1, 2)
    acc = [float(d) for d, a in st if a]
    P = ff.p.cpu().double()
    with torch.no_grad():
        u, _ = R.replay(lambda u, tau: -R.rhs(P, D, H, u, 1.0 - tau), _aug(z.double()), 0.0, acc, 1e-6, 1e-6)
    assert _rel(xs, u[:, :D]) <= 1e-4
    # round trip: forward from the samples returns the drawn z (Hutchinson probe: the data rows do not depend on it)
    L, h = rn._lib.lib(), ff._handle().h
    e = torch.randn(B, D, device=DEV)
    lp, zo, nfe = torch.empty(B, device=DEV), torch.empty(B, D, device=DEV), C.c_int64()
    rn._lib.check_ffjord(h, L.rnde_ffjord_forward(h, xs.data_ptr(), ff.p.data_ptr(), e.data_ptr(), B, 0.0, 1.0, 0, lp.data_ptr(), zo.data_ptr(),
                                                  C.byref(nfe), None, None, 0, None))
    torch.cuda.synchronize()
    assert (zo.cpu() - z).abs().max() <= 1e-3
    # the library's own normals when no z is given
    xs2 = rn.sample(ff, D, nsamples=B)
    assert xs2.shape == (B, D) and torch.isfinite(xs2).all()


def test_training_step_and_reference_loop():
    """-mean(logpx) + lambda mean(saveval) -> backward -> FluxADAM(weight_decay = 1e-5): the gradient against autograd through the fp64 replay along
    the device's steps, the update against Optimiser(WeightDecay, ADAM) restated; then 40 steps of the reference loop (20 epochs x 2 batches)."""
    import regneuralde_jl_amd as rn
    D, H = 2, 16
    tr, _ = rn.load_gaussian_mixture(1024, nsamples=2048, seed=0)
    m = rn.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(0))
    tol = 1e-5          # (the gradient check: at 1.4e-8 the fp32 error estimate, and so the saved values, are rounding noise -- DESIGN 2.1)
    ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, True, "Tsit5", reltol=tol, abstol=tol, max_batch=1024)
    ff.p = torch.from_numpy(R.glorot_params(D, H, np.random.default_rng(5), scale=3.0)).to(DEV)   # (EEst above the fp32 floor)
    p = ff.p.clone().requires_grad_(True)
    opt = rn.FluxADAM([p], eta=4e-2, weight_decay=1e-5)
    x = torch.from_numpy(next(iter(tr))).to(DEV)
    e = torch.randn(x.shape[0], D, device=DEV)
    lam = 2000.0
    logpx, _, _, nfe, sv = ff(x, p, e)
    loss = -logpx.mean() + lam * sv.saveval.mean()
    loss.backward()
    st = np.array(ff.steps()).reshape(-1, 2)
    acc = [float(d) for d, a in st if a]
    Pg = p.detach().cpu().double().requires_grad_(True)
    F = lambda u, t: R.rhs(Pg, D, H, u, t, e.cpu().double())
    u, eests = R.replay(F, _aug(x.cpu().double()), 0.0, acc, tol, tol)
    svr = torch.stack([ee * dt for ee, dt in zip(eests, acc)])
    ref = -R.logpx_of(u, D).mean() + lam * svr.sum() / (len(acc) + 1)
    gp = torch.autograd.grad(ref, Pg)[0]
    assert _rel(p.grad, gp) <= 5e-3, _rel(p.grad, gp)
    g32, p0 = p.grad.detach().cpu().double(), p.detach().cpu().double()
    opt.step()
    want, _, _ = R.flux_adam_wd(p0, g32, torch.zeros_like(p0), torch.zeros_like(p0), 1, 4e-2, wd=1e-5)
    assert _rel(p.detach().cpu() - p0.float(), want - p0) <= 1e-4
    # the reference loop at the reference tolerance: lambda 2000 -> 1000 (lambda_func), 20 epochs x 2 batches
    ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, True, "Tsit5", reltol=1.4e-8, abstol=1.4e-8, max_batch=1024)
    p = ff.p.clone().requires_grad_(True)      # (the Glorot initialisation of MLPDynamics(2, 16), as the experiment starts)
    opt = rn.FluxADAM([p], eta=4e-2, weight_decay=1e-5)
    k = np.log(2.0) / 20
    losses = []
    for epoch in range(1, 21):
        lam = 2000.0 * np.exp(-k * (epoch - 1))
        for xb in tr:
            logpx, _, _, nfe, sv = ff(torch.from_numpy(xb).to(DEV), p)
            loss = -logpx.mean() + lam * sv.saveval.mean()
            loss.backward()
            opt.step()
            losses.append(float(loss))
    assert len(losses) == 40 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_tapes_survive_other_calls_and_are_checked():
    """Each taped forward keeps its own tape until its backward: an inference call, a sample and a second taped forward in between do not change
    the first one's gradient; a second backward through a released tape raises; the probe and z must have the (B, D) orientation."""
    import regneuralde_jl_amd as rn
    D, H, B = 2, 16, 64
    ff, rng = _layer(D, H, B, 6, tol=1e-5)
    xa = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(DEV)
    xb = torch.from_numpy(rng.standard_normal((B - 10, D)).astype(np.float32)).to(DEV)
    ea, eb = torch.randn(B, D, device=DEV), torch.randn(B - 10, D, device=DEV)

    def grad_alone(x, e):
        p = ff.p.clone().requires_grad_(True)
        lp, _, _, _, sv = ff(x, p, e)
        (-lp.mean() + 10.0 * sv.saveval.mean()).backward()
        return p.grad.clone()

    ga, gb = grad_alone(xa, ea), grad_alone(xb, eb)
    pa, pb = ff.p.clone().requires_grad_(True), ff.p.clone().requires_grad_(True)
    lpa, _, _, _, sva = ff(xa, pa, ea)
    with torch.no_grad():
        ff(xb, ff.p, eb)                                   # an inference probe (untaped)
    rn.sample(ff, D, nsamples=B)                           # and a sample
    lpb, _, _, _, svb = ff(xb, pb, eb)                     # a second taped forward before the first backward
    loss_a = -lpa.mean() + 10.0 * sva.saveval.mean()
    loss_a.backward(retain_graph=True)
    (-lpb.mean() + 10.0 * svb.saveval.mean()).backward()
    assert torch.equal(pa.grad, ga) and torch.equal(pb.grad, gb)       # deterministic reverse: the same bits as alone
    with pytest.raises(RuntimeError, match="released"):
        loss_a.backward()
    with torch.no_grad():
        _, _, _, _, _ = ff(xa, ff.p, ea)
    with pytest.raises(ValueError, match="shape"):
        ff(xa, ff.p, ea.t().contiguous())                  # the Julia D x B orientation
    with pytest.raises(ValueError, match="shape"):
        rn.sample(ff, D, nsamples=B, z=torch.randn(D, B, device=DEV))
