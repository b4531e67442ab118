"""The tiled TrackedFFJORD engine (engine="tiled", rnde_ffjord_create_tiled) on the device, against the fp64 restatements of tests/ffjord_ref.py
(width-generic, checked independently in tests/test_ffjord_host.py; the closed-form exact trace in tests/test_ffjord_tiled_host.py).
Batches of 1, 17, 1000 and 1024 columns cover one tile, a partial last tile, the meeting on one XCD (<= 32 tiles) and the agent-scope meeting
(63 and 64 tiles).

Bounds: the one-workgroup engine's (tests/test_gpu_ffjord.py) scaled for the tabular width.  A layer product there is a chain of <= 64 fp32
fmas, here it is up to K = 112 MFMA-accumulated products: the relative rounding of a dot product grows like sqrt(K) (sqrt(112 / 16) ~ 2.6), and
the trace row sums three such chains, so the bounds below are 5x those of the (2, 16) / (16, 64) tests."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ffjord_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(43, 100), (16, 64), (2, 16)]


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _layer(D, H, B, seed, regularize=True, tol=1e-5, scale=1.0, engine="tiled", **kw):
    import regneuralde_jl_amd as rn
    m = rn.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(seed))
    ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, regularize, "Tsit5", reltol=tol, abstol=tol, max_batch=B, engine=engine, **kw)
    rng = np.random.default_rng(seed)
    ff.p = torch.from_numpy(R.glorot_params(D, H, rng, scale=scale)).to(DEV)
    return ff, rng


def _aug(x):
    return torch.cat([x, torch.zeros(x.shape[0], 1, dtype=x.dtype)], 1)


def _randn(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


@pytest.mark.parametrize("D,H", SHAPES)
@pytest.mark.parametrize("B", [1, 17, 1000, 1024])
def test_rhs_matches_fp64(D, H, B):
    """f and the trace row through feval, Hutchinson and the closed-form exact trace, against fp64 (exact: D unit-probe VJPs)."""
    ff, rng = _layer(D, H, B, 1)
    assert ff._handle() and ff.engine == "tiled"
    import regneuralde_jl_amd as rn
    assert rn._lib.lib().rnde_ffjord_engine(ff._handle().h) == 1
    x, e = _randn(rng, B, D), _randn(rng, B, D)
    P = ff.p.cpu().double()
    for t in (0.0, 0.71):
        got = ff.feval(x.to(DEV), t, e.to(DEV)).cpu()
        ref = R.rhs(P, D, H, _aug(x.double()), t, e.double())
        assert _rel(got[:, :D], ref[:, :D]) <= 1e-5 and _rel(got[:, D], ref[:, D]) <= 1e-4
        got = ff.feval(x.to(DEV), t).cpu()
        ref = R.rhs(P, D, H, _aug(x.double()), t)
        assert _rel(got[:, :D], ref[:, :D]) <= 1e-5 and _rel(got[:, D], ref[:, D]) <= 1e-4


@pytest.mark.parametrize("D,H", SHAPES)
def test_replay_forward_and_reverse(D, H):
    """Along a fixed all-accepted sequence (B = 37: three tiles, the last partial): logpx and EEst * dt against the fp64 replay, p-bar and
    x-bar against autograd through it, with and without the EEst * dt cotangent (EEst is truncation error here, as in the one-workgroup test)."""
    B = 37
    ff, rng = _layer(D, H, B, 2, scale=3.0 if D < 40 else 1.5)
    x, e = _randn(rng, B, D), _randn(rng, B, D)
    dts = [0.5, 0.5]
    steps = sum(([dt, 1.0] for dt in dts), [])
    Pg = ff.p.cpu().double().requires_grad_(True)
    Xg = x.double().requires_grad_(True)
    F = lambda u, t: R.rhs(Pg, D, H, u, t, e.double())
    u, eests = R.replay(F, _aug(Xg), 0.0, dts, 1e-5, 1e-5)
    assert min(float(v) for v in eests) >= 0.02
    lp_ref = R.logpx_of(u, D)
    sv_ref = torch.stack([torch.zeros((), dtype=torch.float64)] + [ee * dt for ee, dt in zip(eests, dts)])
    g = torch.from_numpy(rng.standard_normal(B))
    for with_sv in (False, True):
        xd = x.to(DEV).requires_grad_(True)
        p = ff.p.clone().requires_grad_(True)
        logpx, _, _, nfe, sv = ff(xd, p, e.to(DEV), steps=steps)
        assert nfe == 3 + 6 * len(dts) and sv.saveval.numel() == len(dts) + 1
        assert _rel(logpx, lp_ref) <= 5e-5
        assert _rel(sv.saveval, sv_ref) <= 2e-2
        w = torch.linspace(0.5, 1.5, len(dts) + 1, dtype=torch.float64) * 100.0 if with_sv else torch.zeros(len(dts) + 1, dtype=torch.float64)
        loss = (logpx * g.float().to(DEV)).sum() + (sv.saveval * w.float().to(DEV)).sum()
        loss.backward()
        ref = (lp_ref * g).sum() + (sv_ref * w).sum()
        gx, gp = torch.autograd.grad(ref, (Xg, Pg), retain_graph=True)
        tol = 2e-2 if with_sv else 5e-3
        assert _rel(xd.grad, gx) <= tol, _rel(xd.grad, gx)
        assert _rel(p.grad, gp) <= tol, _rel(p.grad, gp)
        if with_sv:
            g0 = torch.autograd.grad((lp_ref * g).sum(), Pg, retain_graph=True)[0]
            assert _rel(gp, g0) > 1e-3


def test_adaptive_solve_truncation_regime_and_reference_tolerance():
    """tol 1e-5 on the stiff (2, 16) case of the one-workgroup test: attempts and acceptances as the fp64 controller's, over 256 columns
    (16 tiles: one-XCD meeting) and 1000 (agent scope).  tol 1.4e-8 at (43, 100), B = 1024: the solution along the device's own steps."""
    D, H = 2, 16
    for B in (256, 1000):
        ff, rng = _layer(D, H, B, 5, scale=8.0)
        x = _randn(rng, B, D) * 3
        e = _randn(rng, B, D)
        P = ff.p.cpu().double()
        F = lambda u, t: R.rhs(P, D, H, u, t, e.double())
        with torch.no_grad():
            logpx, _, _, nfe, sv = ff(x.to(DEV), None, e.to(DEV))
        st = np.array(ff.steps()).reshape(-1, 2)
        _, log = R.solve(F, _aug(x.double()), 0.0, 1.0, 1e-5, 1e-5)
        assert min(l[2] for l in log) >= 0.01 and sum(not l[3] for l in log) > 0 and min(abs(l[2] - 1) for l in log) >= 0.1
        # every decision of the fp64 controller is taken alike (no EEst within 10 % of 1); the step sizes follow to fp32 EEst, so the last
        # step t1 - t may come out as one clamped step or as a step and a remainder of a few 1e-5
        n = len(log) - 1
        assert [bool(a) for a in st[:n, 1]] == [a for *_, a in log[:n]] and len(log) <= len(st) <= len(log) + 1 and st[n:, 1].all()
        assert np.abs(st[:n, 0] / np.array([l[1] for l in log[:n]]) - 1).max() <= 2e-2
        assert abs(float(st[:, 0][st[:, 1] > 0].sum()) - 1.0) <= 1e-5
        assert nfe == 3 + 6 * len(st) and sv.saveval.numel() == int(st[:, 1].sum()) + 1
    D, H, B = 43, 100, 1024
    ff, rng = _layer(D, H, B, 3, tol=1.4e-8)
    P = ff.p.cpu().double()
    x, e = _randn(rng, B, D), _randn(rng, B, D)
    with torch.no_grad():
        logpx, _, _, nfe, sv = ff(x.to(DEV), None, e.to(DEV))
    st = np.array(ff.steps()).reshape(-1, 2)
    acc = [float(d) for d, a in st if a]
    assert sv.saveval.numel() == len(acc) + 1 and torch.isfinite(sv.saveval).all()
    with torch.no_grad():
        u, _ = R.replay(lambda u, t: R.rhs(P, D, H, u, t, e.double()), _aug(x.double()), 0.0, acc, 1.4e-8, 1.4e-8)
    assert _rel(logpx, R.logpx_of(u, D)) <= 5e-5


@pytest.mark.parametrize("D,H,B", [(43, 100, 17), (2, 16, 300)])
def test_sample_matches_reverse_time_replay_and_round_trips(D, H, B):
    """sample() against the fp64 solve of -F(u, t1 - tau) with the exact trace along the device's steps; a forward solve returns z."""
    import regneuralde_jl_amd as rn
    ff, rng = _layer(D, H, B, 4, tol=1e-6)
    z = _randn(rng, B, D)
    xs = rn.sample(ff, D, nsamples=B, z=z.to(DEV))
    st = np.array(ff.steps()).reshape(-1, 2)
    acc = [float(d) for d, a in st if a]
    P = ff.p.cpu().double()
    with torch.no_grad():
        u, _ = R.replay(lambda u, tau: -R.rhs(P, D, H, u, 1.0 - tau), _aug(z.double()), 0.0, acc, 1e-6, 1e-6)
    assert _rel(xs, u[:, :D]) <= 1e-4
    L, h = rn._lib.lib(), ff._handle().h
    e = torch.randn(B, D, device=DEV)
    lp, zo, nfe = torch.empty(B, device=DEV), torch.empty(B, D, device=DEV), C.c_int64()
    rn._lib.check_ffjord(h, L.rnde_ffjord_forward(h, xs.data_ptr(), ff.p.data_ptr(), e.data_ptr(), B, 0.0, 1.0, 0, lp.data_ptr(), zo.data_ptr(),
                                                  C.byref(nfe), None, None, 0, None))
    torch.cuda.synchronize()
    assert (zo.cpu() - z).abs().max() <= 1e-3
    xs2 = rn.sample(ff, D, nsamples=B)
    assert xs2.shape == (B, D) and torch.isfinite(xs2).all()


def test_determinism_forward_backward_bitwise():
    """Two identical forward + backward calls at (43, 100) over 1000 columns (63 tiles, agent-scope meeting): the same bits, p-bar included."""
    D, H, B = 43, 100, 1000
    ff, rng = _layer(D, H, B, 8)
    x, e = _randn(rng, B, D).to(DEV), _randn(rng, B, D).to(DEV)
    outs = []
    for _ in range(2):
        p = ff.p.clone().requires_grad_(True)
        xd = x.clone().requires_grad_(True)
        lp, _, _, nfe, sv = ff(xd, p, e)
        (-lp.mean() + 100.0 * sv.saveval.mean()).backward()
        outs.append((lp.detach().clone(), sv.saveval.detach().clone(), p.grad.clone(), xd.grad.clone(), ff.steps()))
    a, b = outs
    assert all(torch.equal(u, v) for u, v in zip(a[:4], b[:4])) and a[4] == b[4]


def test_cross_engine_agreement():
    """At (2, 16) the tiled and the one-workgroup engines agree to the fp64 bounds: feval, logpx and the gradients along one step sequence."""
    D, H, B = 2, 16, 100
    ft, rng = _layer(D, H, B, 9, scale=3.0)
    fw, _ = _layer(D, H, B, 9, scale=3.0, engine="workgroup")
    assert torch.equal(ft.p, fw.p)
    x, e = _randn(rng, B, D).to(DEV), _randn(rng, B, D).to(DEV)
    for t in (0.0, 0.5):
        assert _rel(ft.feval(x, t, e), fw.feval(x, t, e)) <= 2e-5
        assert _rel(ft.feval(x, t), fw.feval(x, t)) <= 2e-5
    steps = [0.5, 1.0, 0.5, 1.0]      # (EEst is truncation error along these steps, well above the fp32 floor)
    gs = []
    for ff in (ft, fw):
        p = ff.p.clone().requires_grad_(True)
        lp, _, _, _, sv = ff(x, p, e, steps=steps)
        (-lp.mean() + 10.0 * sv.saveval.mean()).backward()
        gs.append((lp.detach(), sv.saveval.detach(), p.grad))
    assert _rel(gs[0][0], gs[1][0]) <= 1e-5 and _rel(gs[0][1], gs[1][1]) <= 5e-3 and _rel(gs[0][2], gs[1][2]) <= 5e-3, \
        (_rel(gs[0][0], gs[1][0]), _rel(gs[0][1], gs[1][1]), _rel(gs[0][2], gs[1][2]))


def test_tapes_on_tiled_handles():
    """Pooled taped handles, untaped calls in between, a released tape raising: as on the one-workgroup engine."""
    import regneuralde_jl_amd as rn
    D, H, B = 16, 64, 40
    ff, rng = _layer(D, H, B, 6)
    xa, xb = _randn(rng, B, D).to(DEV), _randn(rng, B - 10, D).to(DEV)
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
        ff(xb, ff.p, eb)
    rn.sample(ff, D, nsamples=B)
    lpb, _, _, _, svb = ff(xb, pb, eb)
    loss_a = -lpa.mean() + 10.0 * sva.saveval.mean()
    loss_a.backward(retain_graph=True)
    (-lpb.mean() + 10.0 * svb.saveval.mean()).backward()
    assert torch.equal(pa.grad, ga) and torch.equal(pb.grad, gb)
    assert all(rn._lib.lib().rnde_ffjord_engine(hd.h) == 1 for hd in ff._pool)
    with pytest.raises(RuntimeError, match="released"):
        loss_a.backward()


def test_training_steps_lower_the_nll():
    """A few steps of the tabular loop at (43, 100), B = 1024, on a fixed synthetic 43-dimensional dataset: the NLL goes down."""
    import regneuralde_jl_amd as rn
    D, H, B = 43, 100, 1024
    rng = np.random.default_rng(0)
    A = rng.standard_normal((D, D)) / np.sqrt(D)
    X = torch.from_numpy((rng.standard_normal((B, D)) @ A * 0.5 + 0.3).astype(np.float32)).to(DEV)
    m = rn.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(0))
    ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, False, "Tsit5", reltol=1e-5, abstol=1e-5, max_batch=B, engine="tiled")
    p = ff.p.clone().requires_grad_(True)
    opt = rn.FluxADAM([p], eta=1e-2, weight_decay=1e-5)
    nll = []
    for _ in range(6):
        logpx, _, _, nfe, _ = ff(X, p)
        loss = -logpx.mean()
        loss.backward()
        opt.step()
        nll.append(float(loss))
    assert all(np.isfinite(nll)) and nll[-1] < nll[0] - 1.0, nll
