"""TrackedFFJORD's exact-trace mode (ffjord(x, exact=True); rnde_ffjord_forward_exact / _replay and the exact variant of the tile driver's
reverse sweep) on the device, engines 1 (ConcatSquash) and 2 (Dense chains), against the fp64 restatements' exact right-hand side
(tests/ffjord_ref.rhs and tests/ffjord_chain_ref.rhs with e = None: D unit probes; checked against torch.autograd.functional.jacobian in
tests/test_ffjord_exact_host.py) and autograd through R.replay.

Tolerances are the project's own for this arithmetic (header of tests/test_gpu_ffjord_chain.py): logpx 5e-5, saved values 2e-2, x-bar / p-bar
5e-3 (2e-2 with the saved-value cotangent).  The fp32 restatement alone sits at <= 4e-6 of fp64 for logpx, x-bar and p-bar in all six cases
without the saved-value cotangent.  Only smooth activations: no kink vetting."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import ffjord_chain_ref as CR
from tests import ffjord_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = [0.5, 0.5]
STEPS = sum(([dt, 1.0] for dt in DTS), [])
SEED, SCALE = 21, 2.0
# name: (engine, shape, time_dep, activations, B) -- what each reaches:
CASES = {
    "td2": ("chain", [2, 10, 2], True, ["tanh", "identity"], 20),                       # two tiles, partial last tile, the meeting
    "td5": ("chain", [5, 12, 9, 5], True, ["softplus", "sigmoid", "tanh"], 20),         # three layers, second derivatives of two activations
    "td18": ("chain", [18, 24, 18], True, ["tanh", "identity"], 20),                    # unit probes past the first 16-row tile
    "plain18": ("chain", [18, 24, 18], False, ["softplus", "tanh"], 5),                 # one partial tile, no time row
    "cs2": ("tiled", (2, 16), None, None, 20),                                          # the gaussian experiment's shape
    "cs18": ("tiled", (18, 20), None, None, 20),                                        # D > 16 with the closed-form forward
}
NAMES = list(CASES)


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@functools.lru_cache(maxsize=None)
def _draw(name):
    """p, x, e (float32) and g (float64, the cotangent of logpx) of a case; the ConcatSquash probe is drawn after g."""
    eng, shape, td, acts, B = CASES[name]
    if eng == "chain":
        p, x, e, rng = CR.draw(shape, td, B, seed=SEED, scale=SCALE)
        g = torch.from_numpy(rng.standard_normal(B))
    else:
        D, H = shape
        rng = np.random.default_rng(SEED)
        p = torch.from_numpy(R.glorot_params(D, H, rng, SCALE))
        x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
        g = torch.from_numpy(rng.standard_normal(B))
        e = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
    return p, x, e, g


def _dim(name):
    eng, shape = CASES[name][:2]
    return shape[0]


def _rhs(name, P):
    """The exact right-hand side of a case in P's precision: F(u, t)."""
    eng, shape, td, acts, B = CASES[name]
    if eng == "chain":
        return lambda u, t: CR.rhs(shape, acts, td, P, u, t)
    return lambda u, t: R.rhs(P, shape[0], shape[1], u, t)


def _layer(name, regularize=True, tol=1e-5, engine="tiled"):
    import regneuralde_jl_amd as rn
    eng, shape, td, acts, B = CASES[name]
    p = _draw(name)[0]
    if eng == "chain":
        layers = [rn.Dense(shape[l] + (1 if td else 0), shape[l + 1], acts[l]) for l in range(len(acts))]
        model = rn.TDChain(*layers) if td else rn.Chain(*layers)
    else:
        td, model = True, rn.ffjord.MLPDynamics(*shape)
    ff = rn.TrackedFFJORD(model, [0.0, 1.0], td, regularize, "Tsit5", reltol=tol, abstol=tol, max_batch=B, engine=engine)
    assert ff.p.numel() == p.numel()
    ff.p = p.to(DEV)
    return ff


def replay_reference(name, dtype=torch.float64):
    """The exact replay along DTS at tol 1e-5 in `dtype` (fp64: the reference; fp32: the rounding yardstick, for measuring by hand)."""
    p, x, e, g = _draw(name)
    D = _dim(name)
    g = g.to(dtype)
    Pg, Xg = p.to(dtype).clone().requires_grad_(True), x.to(dtype).clone().requires_grad_(True)      # (clones: _draw's tensors are shared)
    u, eests = R.replay(_rhs(name, Pg), CR.aug(Xg), 0.0, DTS, 1e-5, 1e-5)
    lp = R.logpx_of(u, D)
    sv = torch.stack([torch.zeros((), dtype=dtype)] + [ee * dt for ee, dt in zip(eests, DTS)])
    w = (torch.linspace(0.5, 1.5, len(DTS) + 1, dtype=torch.float64) * 100.0).to(dtype)
    out = {"w": w, "lp": lp.detach(), "sv": sv.detach(), "eests": [float(v.detach()) for v in eests]}
    out["gx0"], out["gp0"] = torch.autograd.grad((lp * g).sum(), (Xg, Pg), retain_graph=True)
    out["gx1"], out["gp1"] = torch.autograd.grad((lp * g).sum() + (sv * w).sum(), (Xg, Pg))
    return out


@functools.lru_cache(maxsize=None)
def _replay_ref(name):
    return replay_reference(name)


def _exact_call(ff, name, with_sv=True, steps=STEPS):
    """One taped exact forward + backward on ff: (logpx, saved values, x-bar, p-bar), detached."""
    p, x, e, g = _draw(name)
    xd = x.to(DEV).requires_grad_(True)
    pd = ff.p.clone().requires_grad_(True)
    logpx, z1, z2, nfe, sv = ff(xd, pd, steps=steps, exact=True)
    loss = (logpx * g.float().to(DEV)).sum()
    if with_sv and sv is not None:
        w = _replay_ref(name)["w"][:sv.saveval.numel()]
        loss = loss + (sv.saveval * w.float().to(DEV)).sum()
    loss.backward()
    return logpx.detach().clone(), (sv.saveval.detach().clone() if sv is not None else None), xd.grad.clone(), pd.grad.clone(), nfe


def _hutch_call(ff, name, e, steps=STEPS):
    p, x, _, g = _draw(name)
    xd = x.to(DEV).requires_grad_(True)
    pd = ff.p.clone().requires_grad_(True)
    logpx, _, _, nfe, sv = ff(xd, pd, e.to(DEV), steps=steps)
    (logpx * g.float().to(DEV)).sum().backward()
    return logpx.detach().clone(), xd.grad.clone(), pd.grad.clone()


# ---- 1. replay, forward and reverse ----
@pytest.mark.parametrize("name", NAMES)
def test_exact_replay_forward_and_reverse(name):
    """Along a fixed all-accepted sequence, {true} layers: logpx and EEst * dt against the fp64 exact replay, p-bar and x-bar against autograd
    through it, with and without the EEst * dt cotangent (EEst is truncation error here: asserted on the fp64 side)."""
    ref = _replay_ref(name)
    assert min(ref["eests"]) >= 0.02, ref["eests"]
    ff = _layer(name)
    import regneuralde_jl_amd as rn
    for with_sv in (False, True):
        logpx, sv, gx, gp, nfe = _exact_call(ff, name, with_sv)
        assert nfe == 3 + 6 * len(DTS) and sv.numel() == len(DTS) + 1
        k = "1" if with_sv else "0"
        devs = (_rel(logpx, ref["lp"]), _rel(sv, ref["sv"]), _rel(gx, ref["gx" + k]), _rel(gp, ref["gp" + k]))
        print(name, "with_sv" if with_sv else "plain", "logpx / saveval / x-bar / p-bar:", devs, "EEst", ref["eests"])
        tol = 2e-2 if with_sv else 5e-3
        assert devs[0] <= 5e-5 and devs[1] <= 2e-2 and devs[2] <= tol and devs[3] <= tol, devs
        if with_sv:
            assert _rel(ref["gp1"], ref["gp0"]) > 1e-3                  # (the cotangent reaches p-bar through EEst)
    assert rn._lib.lib().rnde_ffjord_engine(ff._pool[0].h) == (2 if CASES[name][0] == "chain" else 1)


# ---- 2. it really is the exact trace ----
@pytest.mark.parametrize("name", ["td5", "cs2"])
def test_exact_is_not_the_estimate_and_leaves_the_handle_as_it_was(name):
    """The exact logpx is not the Hutchinson one; exact calls are bit-identical to each other, whatever probes the handle served in between;
    a Hutchinson call keeps its bits across an exact call on the same handle."""
    p, x, e, g = _draw(name)
    ff = _layer(name)
    e2 = torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(e.shape)).astype(np.float32))
    h0 = _hutch_call(ff, name, e)
    a = _exact_call(ff, name)
    b = _exact_call(ff, name)
    _hutch_call(ff, name, e2)
    h1 = _hutch_call(ff, name, e)
    c = _exact_call(ff, name)
    assert len(ff._pool) == 1                                           # (one taped handle served every sweep)
    diff = _rel(a[0], h0[0])
    print(name, "exact against Hutchinson, logpx:", diff, "p-bar:", _rel(a[3], h0[2]))
    assert diff > 1e-2
    for other in (b, c):
        assert all(torch.equal(u, v) for u, v in zip(a[:4], other[:4]))
    assert all(torch.equal(u, v) for u, v in zip(h0, h1))
    assert torch.isfinite(a[3]).all() and a[3].abs().max() > 0


# ---- 3. the adaptive solve ----
def _adaptive(name, tol):
    p, x, e, g = _draw(name)
    D = _dim(name)
    ff = _layer(name, tol=tol)
    with torch.no_grad():
        logpx, _, _, nfe, sv = ff(x.to(DEV), exact=True)
    log = ff.step_log()
    assert nfe == 3 + 6 * len(log) and len(ff.steps()) == 2 * len(log)
    acc = [float(dt) for _, dt, _, a in log if a]
    assert abs(sum(acc) - 1.0) <= 1e-5 and sv.saveval.numel() == len(acc) + 1
    t = ff.timing()
    assert t[0] > 0 and t[2] == len(log) and t[3] == len(acc)
    with torch.no_grad():
        u, _ = R.replay(_rhs(name, p.double()), CR.aug(x.double()), 0.0, acc, tol, tol)
    dev = _rel(logpx, R.logpx_of(u, D))
    print(name, "tol", tol, "attempts", len(log), "accepted", len(acc), "logpx", dev)
    return dev


@pytest.mark.parametrize("name", ["td5", "cs2"])
def test_exact_adaptive_solve(name):
    """tol 1e-5, B = 20: NFE is 3 + 6 per attempt, the accepted steps cover [0, 1], logpx against the fp64 replay of the accepted steps."""
    assert _adaptive(name, 1e-5) <= 5e-5


def test_exact_reference_tolerance_along_the_device_steps():
    """tol 1.4e-8 (the reference's) on ConcatSquash (2, 16): logpx against the fp64 replay along the device's own accepted steps."""
    assert _adaptive("cs2", 1.4e-8) <= 5e-5


# ---- 4. one training step ----
def test_exact_training_step_gradient_and_descent():
    """cs2, B = 20, a {false} layer: -mean(logpx) through exact=True; the gradient against fp64 autograd along the device's accepted steps,
    and one plain gradient-descent update lowers the exact loss."""
    name, tol, lr = "cs2", 1e-5, 1e-3
    p, x, e, g = _draw(name)
    ff = _layer(name, regularize=False, tol=tol)
    xd = x.to(DEV)
    pd = ff.p.clone().requires_grad_(True)
    logpx, _, _, nfe, sv = ff(xd, pd, exact=True)
    assert sv is None
    loss = -logpx.mean()
    loss.backward()
    acc = [float(dt) for _, dt, _, a in ff.step_log() if a]
    Pg = p.double().requires_grad_(True)
    u, _ = R.replay(_rhs(name, Pg), CR.aug(x.double()), 0.0, acc, tol, tol)
    ref = -R.logpx_of(u, 2).mean()
    gp = torch.autograd.grad(ref, Pg)[0]
    with torch.no_grad():
        after = -ff(xd, pd.detach() - lr * pd.grad, exact=True)[0].mean()
    loss, ref = loss.detach(), ref.detach()
    print("accepted", len(acc), "loss", float(loss), float(ref), "after one step", float(after), "p-bar", _rel(pd.grad, gp))
    assert abs(float(loss) - float(ref)) <= 5e-5 * abs(float(ref))
    assert _rel(pd.grad, gp) <= 5e-3
    assert float(after) < float(loss)


# ---- 5. refusals on the device, loglikelihood ----
def test_exact_refusals_on_the_device():
    """Engine 0 refuses the exact forward by name (the message points at the tiled engine); rnde_ffjord_backward_kinetic refuses an exact tape,
    and the tape is still good for rnde_ffjord_backward afterwards."""
    import regneuralde_jl_amd as rn
    L, BAD = rn._lib.lib(), rn._lib.BAD_ARG
    p, x, e, g = _draw("cs2")
    B = x.shape[0]
    wg = _layer("cs2", regularize=False, engine="workgroup")
    h = wg._handle().h
    assert L.rnde_ffjord_engine(h) == 0
    xd, lp, nfe = x.to(DEV), torch.empty(B, device=DEV), C.c_int64()
    assert L.rnde_ffjord_forward_exact(h, xd.data_ptr(), wg.p.data_ptr(), B, 0.0, 1.0, lp.data_ptr(), None, C.byref(nfe), None, None, 0, None) == BAD
    assert b"tiled" in L.rnde_ffjord_last_error(h) and b"exact" in L.rnde_ffjord_last_error(h)
    arr = (C.c_float * 4)(*STEPS)
    assert L.rnde_ffjord_forward_exact_replay(h, xd.data_ptr(), wg.p.data_ptr(), B, 0.0, 1.0, arr, 2, lp.data_ptr(), None, C.byref(nfe), None, None, 0,
                                              None) == BAD
    with pytest.raises(ValueError, match='engine="tiled" only'):
        wg(xd, exact=True)

    ff = _layer("cs2", regularize=False)
    pd = ff.p.clone().requires_grad_(True)
    logpx = ff(xd, pd, steps=STEPS, exact=True)[0]
    hd = ff._pool[0]
    gl, pb = torch.ones(B, device=DEV), torch.empty_like(ff.p)
    assert L.rnde_ffjord_backward_kinetic(hd.h, gl.data_ptr(), None, pb.data_ptr(), None, None) == BAD
    assert b"exact" in L.rnde_ffjord_last_error(hd.h)
    logpx.sum().backward()
    assert torch.isfinite(pd.grad).all() and pd.grad.abs().max() > 0


def test_loglikelihood_with_the_exact_trace():
    """loglikelihood(..., exact=True) is the mean of the exact logpx over the batches (two batches of unequal size)."""
    import regneuralde_jl_amd as rn
    p, x, e, g = _draw("cs2")
    ff = _layer("cs2", regularize=False)
    batches = [x[:12].numpy(), x[12:].numpy()]
    got = rn.ffjord.loglikelihood(ff, batches, exact=True)
    with torch.no_grad():
        lps = [ff(torch.from_numpy(b).to(DEV), exact=True)[0] for b in batches]
    want = float(sum(float(l.sum()) for l in lps) / x.shape[0])
    assert abs(got - want) <= 1e-6 * abs(want)
    est = rn.ffjord.loglikelihood(ff, batches)                          # (the default keeps the Hutchinson estimate)
    assert np.isfinite(est) and est != got
