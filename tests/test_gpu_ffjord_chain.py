"""TrackedFFJORD's default dynamics (Tracker.forward, then back) for Dense chains on the device (rnde_ffjord_create_chain, engine 2) against
the fp64 restatements of tests/ffjord_chain_ref.py (checked independently in tests/test_ffjord_chain_host.py).  Batches of 1, 17 and 37
columns cover a one-column tile, a partial last tile and three tiles (the meeting runs); 256 and 300 columns cover 16 and 19 tiles.

Tolerances are the tiled ConcatSquash engine's for the same arithmetic (tests/test_gpu_ffjord_tiled.py): f rows 1e-5, trace and kinetic rows
1e-4, logpx 5e-5, saved values 2e-2, x-bar / p-bar 5e-3 (2e-2 with the saved-value cotangent).  Every case meets them as they stand."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import ffjord_chain_ref as CR
from tests import ffjord_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINK = 1e-4                                  # tests/test_gpu_activations.py's guard
T5 = [5, 40, 24, 5]


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _layer(dims, acts, td, B, p, regularize=True, tol=1e-5, **kw):
    import regneuralde_jl_amd as rn
    layers = [rn.Dense(dims[l] + (1 if td else 0), dims[l + 1], acts[l]) for l in range(len(acts))]
    model = rn.TDChain(*layers) if td else rn.Chain(*layers)
    ff = rn.TrackedFFJORD(model, [0.0, 1.0], td, regularize, "Tsit5", reltol=tol, abstol=tol, max_batch=B, engine="tiled", **kw)
    assert ff.p.numel() == p.numel()
    ff.p = p.to(DEV)
    return ff


# ---- 1. one evaluation ----
# (seed 34: the relu / elu pre-activations of all six evaluations stay 3.8e-4 / 5.5e-4 away from the kink in the restatement)
FEVAL = [("td2", [2, 10, 2], True, ["tanh", "identity"], 1)] + \
        [("td5-" + a, T5, True, [a, a, "tanh"], s) for a, s in (("identity", 1), ("tanh", 1), ("relu", 34), ("sigmoid", 1), ("softplus", 1), ("elu", 34))] + \
        [("plain5", T5, False, ["tanh", "tanh", "identity"], 1), ("td48", [48, 64, 64, 48], True, ["tanh", "softplus", "tanh"], 1),
         ("latent", CR.LATENT, False, ["tanh"] * 8, 1)]


@pytest.mark.parametrize("name,dims,td,acts,seed", FEVAL, ids=[c[0] for c in FEVAL])
def test_rhs_matches_fp64(name, dims, td, acts, seed):
    """f, the trace row (Hutchinson and exact) and the kinetic rows through feval against fp64, B in {1, 17, 37}, t in {0, 0.71}."""
    import regneuralde_jl_amd as rn
    D = dims[0]
    for B in (1, 17, 37):
        p, x, e, _ = CR.draw(dims, td, B, seed, 1.0)
        ff = _layer(dims, acts, td, B, p, regularize=False)
        assert rn._lib.lib().rnde_ffjord_engine(ff._handle().h) == 2
        P, X, E = p.double(), x.double(), e.double()
        for t in (0.0, 0.71):
            pre = []
            ref = CR.rhs_kinetic(dims, acts, td, P, CR.aug(X, 3), t, E, pre).detach()
            assert CR.kink_margin(acts, pre) > KINK, f"a pre-activation within {KINK} of the kink: pick another seed"
            got = ff.feval(x.to(DEV), t, e.to(DEV), regularize=True).cpu()
            assert got.shape == (B, D + 3)
            devs = [_rel(got[:, :D], ref[:, :D])] + [_rel(got[:, D + i], ref[:, D + i]) for i in range(3)]
            hut = ff.feval(x.to(DEV), t, e.to(DEV)).cpu()
            assert torch.equal(hut, got[:, :D + 1])                     # the plain rows are the plain call's
            ex = ff.feval(x.to(DEV), t).cpu()
            rex = CR.rhs(dims, acts, td, P, CR.aug(X), t).detach()
            devs += [_rel(ex[:, :D], rex[:, :D]), _rel(ex[:, D], rex[:, D])]
            print(name, B, t, "f / trace / ke / jn / f (exact) / exact trace:", devs)
            assert devs[0] <= 1e-5 and devs[4] <= 1e-5 and max(devs[1], devs[2], devs[3], devs[5]) <= 1e-4, devs


# ---- 2. replay, forward and reverse ----
REPLAY = [("td2", [2, 10, 2], True, ["tanh", "identity"], 37, 21, 2.0)] + \
         [("td5-" + a, T5, True, [a, a, "tanh"], 37, 21, 2.0) for a in ("identity", "tanh", "sigmoid", "softplus")] + \
         [("td48", [48, 64, 64, 48], True, ["tanh", "softplus", "tanh"], 37, 21, 1.5), ("latent", CR.LATENT, False, ["tanh"] * 8, 37, 21, 1.5),
          ("td5s-relu", [5, 12, 9, 5], True, ["relu", "relu", "tanh"], 8, 18, 2.0), ("td5s-elu", [5, 12, 9, 5], True, ["elu", "elu", "tanh"], 8, 16, 2.0)]
DTS = [0.5, 0.5]


def replay_reference(dims, td, acts, B, seed, scale, dtype=torch.float64):
    """The replay along DTS at tol 1e-5 in `dtype` (fp64: the reference; fp32: the rounding yardstick, for measuring by hand): logpx, saved values, the gradients of sum g logpx (+ sum w sv), the kink margin."""
    D = dims[0]
    p, x, e, rng = CR.draw(dims, td, B, seed, scale)
    g = torch.from_numpy(rng.standard_normal(B)).to(dtype)
    Pg, Xg = p.to(dtype).requires_grad_(True), x.to(dtype).requires_grad_(True)
    pre = []
    u, eests = R.replay(lambda u, t: CR.rhs(dims, acts, td, Pg, u, t, e.to(dtype), pre), CR.aug(Xg), 0.0, DTS, 1e-5, 1e-5)
    lp = R.logpx_of(u, D)
    sv = torch.stack([torch.zeros((), dtype=dtype)] + [ee * dt for ee, dt in zip(eests, DTS)])
    w = (torch.linspace(0.5, 1.5, len(DTS) + 1, dtype=torch.float64) * 100.0).to(dtype)
    out = {"p": p, "x": x, "e": e, "g": g, "w": w, "lp": lp.detach(), "sv": sv.detach(), "eests": [float(v.detach()) for v in eests],
           "kink": CR.kink_margin(acts, pre)}
    out["gx0"], out["gp0"] = torch.autograd.grad((lp * g).sum(), (Xg, Pg), retain_graph=True)
    out["gx1"], out["gp1"] = torch.autograd.grad((lp * g).sum() + (sv * w).sum(), (Xg, Pg))
    return out


@functools.lru_cache(maxsize=None)
def _replay_ref(name):
    c = next(c for c in REPLAY if c[0] == name)
    return replay_reference(*c[1:])


@pytest.mark.parametrize("name,dims,td,acts,B,seed,scale", REPLAY, ids=[c[0] for c in REPLAY])
def test_replay_forward_and_reverse(name, dims, td, acts, B, seed, scale):
    """Along a fixed all-accepted sequence: logpx and EEst * dt against the fp64 replay, p-bar and x-bar against autograd through it, with and
    without the EEst * dt cotangent (EEst is truncation error here: asserted on the fp64 side); the cotangent reaches p-bar through EEst."""
    ref = _replay_ref(name)
    assert min(ref["eests"]) >= 0.02, ref["eests"]
    assert ref["kink"] > KINK, f"a pre-activation within {KINK} of the kink ({ref['kink']:.2e}): pick another seed"
    ff = _layer(dims, acts, td, B, ref["p"])
    steps = sum(([dt, 1.0] for dt in DTS), [])
    x, e, g = ref["x"], ref["e"], ref["g"]
    for with_sv in (False, True):
        xd = x.to(DEV).requires_grad_(True)
        p = ff.p.clone().requires_grad_(True)
        logpx, _, _, nfe, sv = ff(xd, p, e.to(DEV), steps=steps)
        assert nfe == 3 + 6 * len(DTS) and sv.saveval.numel() == len(DTS) + 1
        w = ref["w"] if with_sv else torch.zeros(len(DTS) + 1, dtype=torch.float64)
        loss = (logpx * g.float().to(DEV)).sum() + (sv.saveval * w.float().to(DEV)).sum()
        loss.backward()
        k = "1" if with_sv else "0"
        gx, gp = ref["gx" + k], ref["gp" + k]
        devs = (_rel(logpx, ref["lp"]), _rel(sv.saveval, ref["sv"]), _rel(xd.grad, gx), _rel(p.grad, gp))
        print(name, "with_sv" if with_sv else "plain", "logpx / saveval / x-bar / p-bar:", devs, "EEst", ref["eests"], "kink", ref["kink"])
        tol = 2e-2 if with_sv else 5e-3
        assert devs[0] <= 5e-5 and devs[1] <= 2e-2 and devs[2] <= tol and devs[3] <= tol, devs
        if with_sv:
            assert _rel(gp, ref["gp0"]) > 1e-3


# ---- 3. kinetic replay ----
@pytest.mark.parametrize("dims,acts", [([2, 10, 2], ["tanh", "identity"]), (T5, ["softplus", "tanh", "tanh"])], ids=["td2", "td5"])
def test_kinetic_replay_and_joint_gradient(dims, acts):
    """logpx, lambda1, lambda2 along a fixed sequence and their joint gradient (cotangents on all three) against autograd through the
    D + 3-row fp64 replay; the plain sweep on the same handle afterwards keeps its bits."""
    td, B, D, tol = True, 37, dims[0], 1e-5
    p, x, e, rng = CR.draw(dims, td, B, 21, 2.0)
    g, g1, g2 = (torch.from_numpy(rng.standard_normal(B)) for _ in range(3))
    steps = sum(([dt, 1.0] for dt in DTS), [])
    Pg, Xg = p.double().requires_grad_(True), x.double().requires_grad_(True)
    u, _ = R.replay(lambda u, t: CR.rhs_kinetic(dims, acts, td, Pg, u, t, e.double()), CR.aug(Xg, 3), 0.0, DTS, tol, tol)
    lp_ref, l1_ref, l2_ref = R.logpx_of(u, D), u[:, D + 1], u[:, D + 2]
    terms = [(lp_ref * g).sum(), (l1_ref * g1).sum(), (l2_ref * g2).sum()]
    (gx0, gp0), (gx1, gp1), (gx2, gp2) = (torch.autograd.grad(v, (Xg, Pg), retain_graph=True) for v in terms)
    gx, gp = gx0 + gx1 + gx2, gp0 + gp1 + gp2
    moved = (_rel(gp0 + gp1, gp0), _rel(gp0 + gp2, gp0))
    assert min(moved) > 1e-2, moved                                    # (each lambda cotangent moves the gradient: it cannot be dropped unseen)

    ff = _layer(dims, acts, td, B, p, regularize=False)
    xdev, edev = x.to(DEV), e.to(DEV)

    def plain():
        xd, pd = xdev.clone().requires_grad_(True), ff.p.clone().requires_grad_(True)
        lp = ff(xd, pd, edev, steps=steps)[0]
        (lp * g.float().to(DEV)).sum().backward()
        return lp.detach().clone(), xd.grad.clone(), pd.grad.clone()

    before = plain()
    xd, pd = xdev.clone().requires_grad_(True), ff.p.clone().requires_grad_(True)
    logpx, l1, l2, nfe, sv = ff(xd, pd, edev, regularize=True, steps=steps)
    assert nfe == 3 + 6 * len(DTS) and sv is None and l1.shape == l2.shape == (B,)
    fw = (_rel(logpx, lp_ref), _rel(l1, l1_ref), _rel(l2, l2_ref))
    (logpx * g.float().to(DEV)).sum().add((l1 * g1.float().to(DEV)).sum()).add((l2 * g2.float().to(DEV)).sum()).backward()
    bw = (_rel(xd.grad, gx), _rel(pd.grad, gp))
    print(dims, "forward", fw, "reverse", bw, "moved", moved)
    assert fw[0] <= 5e-5 and max(fw[1:]) <= 1e-4, fw
    assert max(bw) <= 5e-3, bw
    after = plain()
    assert len(ff._pool) == 1                                           # (the same taped handle served all three sweeps)
    assert all(torch.equal(a, b) for a, b in zip(before, after))


# ---- 4. the adaptive controller ----
CTRL = dict(dims=[2, 10, 2], acts=["tanh", "tanh"], td=True, seed=8, scale=10.0, xscale=3.0, B=40, tol=1.4e-3)


def controller_reference(dtype):
    c = CTRL
    p, x, e, _ = CR.draw(c["dims"], c["td"], c["B"], c["seed"], c["scale"], c["xscale"])
    F = lambda u, t: CR.rhs(c["dims"], c["acts"], c["td"], p.to(dtype), u, t, e.to(dtype)).detach()
    _, log = R.solve(F, CR.aug(x.to(dtype)), 0.0, 1.0, c["tol"], c["tol"])
    return p, x, e, log


def test_adaptive_controller_takes_the_fp64_decisions():
    """tol 1.4e-3 (test/test_ffjord.jl's): attempts, accept pattern and step sizes as the fp64 controller's.  The recipe's own properties are
    asserted first, so a change of recipe cannot void the comparison: 13 attempts with one rejection, no EEst within 0.7 of the accept
    threshold (0.728 measured), and the fp32 restatement on the CPU takes the same decisions with every dt but the last (the clamped
    remainder t1 - t) within 3e-3 of fp64 (2.82e-3 measured) -- seven times inside the device's bound of 2e-2."""
    c = CTRL
    p, x, e, log = controller_reference(torch.float64)
    _, _, _, log32 = controller_reference(torch.float32)
    acc = [l[3] for l in log]
    assert len(log) == 13 and acc.count(False) == 1 and min(abs(l[2] - 1.0) for l in log) >= 0.7
    assert [l[3] for l in log32] == acc and max(abs(a[1] / b[1] - 1) for a, b in zip(log32[:-1], log[:-1])) <= 3e-3
    ff = _layer(c["dims"], c["acts"], c["td"], c["B"], p, tol=c["tol"])
    with torch.no_grad():
        logpx, _, _, nfe, sv = ff(x.to(DEV), None, e.to(DEV))
    st = np.array(ff.steps()).reshape(-1, 2)
    print("device steps", st.tolist(), "fp64", [(l[1], l[3]) for l in log])
    assert len(st) == len(log) and [bool(a) for a in st[:, 1]] == acc
    assert np.abs(st[:-1, 0] / np.array([l[1] for l in log[:-1]]) - 1).max() <= 2e-2
    assert nfe == 3 + 6 * len(st) and sv.saveval.numel() == int(st[:, 1].sum()) + 1


@pytest.mark.parametrize("B", [256, 513])
def test_reference_tolerance_along_the_device_steps(B):
    """tol 1.4e-8 over 256 columns (16 tiles, meeting on one XCD) and over 513 (33 tiles, the last one partial: the smallest batch that meets
    at agent scope): logpx against the fp64 replay along the device's own accepted steps."""
    c = CTRL
    tol = 1.4e-8
    p, x, e, _ = CR.draw(c["dims"], c["td"], B, c["seed"], c["scale"], c["xscale"])
    ff = _layer(c["dims"], c["acts"], c["td"], B, p, tol=tol)
    with torch.no_grad():
        logpx, _, _, nfe, sv = ff(x.to(DEV), None, e.to(DEV))
    st = np.array(ff.steps()).reshape(-1, 2)
    accd = [float(d) for d, a in st if a]
    assert sv.saveval.numel() == len(accd) + 1 and torch.isfinite(sv.saveval).all()
    with torch.no_grad():
        u, _ = R.replay(lambda u, t: CR.rhs(c["dims"], c["acts"], c["td"], p.double(), u, t, e.double()).detach(), CR.aug(x.double()), 0.0, accd, tol, tol)
    print("attempts", len(st), "accepted", len(accd), "logpx", _rel(logpx, R.logpx_of(u, 2)))
    assert _rel(logpx, R.logpx_of(u, 2)) <= 5e-5


# ---- 5. sample ----
def test_sample_matches_reverse_time_replay_and_round_trips():
    """sample() against the fp64 solve of -F(u, t1 - tau) with the exact trace along the device's steps; a forward solve returns z."""
    import regneuralde_jl_amd as rn
    dims, acts, td, B, tol = T5, ["softplus", "tanh", "identity"], True, 20, 1e-6
    D = dims[0]
    p, z, _, _ = CR.draw(dims, td, B, 4, 1.0)
    ff = _layer(dims, acts, td, B, p, tol=tol)
    xs = rn.sample(ff, D, nsamples=B, z=z.to(DEV))
    st = np.array(ff.steps()).reshape(-1, 2)
    acc = [float(d) for d, a in st if a]
    with torch.no_grad():
        u, _ = R.replay(lambda u, tau: -CR.rhs(dims, acts, td, p.double(), u, 1.0 - tau).detach(), CR.aug(z.double()), 0.0, acc, tol, tol)
    print("sample: accepted", len(acc), "x", _rel(xs, u[:, :D]))
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


# ---- 6. determinism and tapes ----
def test_determinism_forward_backward_bitwise():
    """Two identical forward + backward calls over 300 columns (19 tiles): the same bits, p-bar included."""
    dims, acts, td, B = T5, ["softplus", "tanh", "tanh"], True, 300
    p, x, e, _ = CR.draw(dims, td, B, 9, 1.5)
    ff = _layer(dims, acts, td, B, p)
    x, e = x.to(DEV), e.to(DEV)
    outs = []
    for _ in range(2):
        pp = ff.p.clone().requires_grad_(True)
        xd = x.clone().requires_grad_(True)
        lp, _, _, nfe, sv = ff(xd, pp, e)
        (-lp.mean() + 100.0 * sv.saveval.mean()).backward()
        outs.append((lp.detach().clone(), sv.saveval.detach().clone(), pp.grad.clone(), xd.grad.clone(), ff.steps()))
    a, b = outs
    assert all(torch.equal(u, v) for u, v in zip(a[:4], b[:4])) and a[4] == b[4]
    assert torch.isfinite(a[2]).all() and a[2].abs().max() > 0


def test_tapes_on_chain_handles():
    """Pooled taped handles, untaped calls in between, a released tape raising: as on the tiled ConcatSquash engine."""
    import regneuralde_jl_amd as rn
    dims, acts, td, B = [5, 12, 9, 5], ["tanh", "sigmoid", "identity"], False, 40
    D = dims[0]
    p, xa, ea, rng = CR.draw(dims, td, B, 6, 1.0)
    ff = _layer(dims, acts, td, B, p)
    xa, ea = xa.to(DEV), ea.to(DEV)
    xb = torch.from_numpy(rng.standard_normal((B - 10, D)).astype(np.float32)).to(DEV)
    eb = torch.from_numpy(rng.standard_normal((B - 10, D)).astype(np.float32)).to(DEV)

    def grad_alone(x, e):
        pp = ff.p.clone().requires_grad_(True)
        lp, _, _, _, sv = ff(x, pp, e)
        (-lp.mean() + 10.0 * sv.saveval.mean()).backward()
        return pp.grad.clone()

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
    assert all(rn._lib.lib().rnde_ffjord_engine(hd.h) == 2 for hd in ff._pool)
    with pytest.raises(RuntimeError, match="released"):
        loss_a.backward()
    t = ff.timing()
    assert t[0] > 0 and t[1] > 0 and t[2] >= t[3] > 0
    assert ff.step_log().shape == (t[2], 4)


# ---- 7. one training step ----
def test_training_step_gradient_and_descent():
    """-mean(logpx) + lambda mean(saveval) on TD [2, 16, 16, 2]: the gradient against autograd through the fp64 replay along the device's
    steps; ten FluxADAM steps lower the loss."""
    import regneuralde_jl_amd as rn
    dims, acts, td, B, tol, lam = [2, 16, 16, 2], ["softplus", "softplus", "identity"], True, 64, 1e-5, 100.0
    p, x, e, _ = CR.draw(dims, td, B, 3, 2.0)
    x = x * 0.7 + 0.5
    ff = _layer(dims, acts, td, B, p, tol=tol)
    xd, ed = x.to(DEV), e.to(DEV)
    pd = ff.p.clone().requires_grad_(True)
    logpx, _, _, nfe, sv = ff(xd, pd, ed)
    loss = -logpx.mean() + lam * sv.saveval.mean()
    loss.backward()
    acc = [float(dt) for _, dt, _, a in ff.step_log() if a]
    Pg = p.double().requires_grad_(True)
    u, eests = R.replay(lambda u, t: CR.rhs(dims, acts, td, Pg, u, t, e.double()), CR.aug(x.double()), 0.0, acc, tol, tol)
    svr = torch.stack([torch.zeros((), dtype=torch.float64)] + [ee * dt for ee, dt in zip(eests, acc)])
    ref = -R.logpx_of(u, 2).mean() + lam * svr.mean()
    gp = torch.autograd.grad(ref, Pg)[0]
    print("accepted", len(acc), "loss", float(loss), float(ref), "p-bar", _rel(pd.grad, gp), "min EEst", min(float(v) for v in eests))
    assert abs(float(loss) - float(ref)) <= 2e-2 * abs(float(ref))
    assert _rel(pd.grad, gp) <= 2e-2
    pt = ff.p.clone().requires_grad_(True)
    opt = rn.FluxADAM([pt], eta=1e-2)
    losses = []
    for _ in range(10):
        lp, _, _, _, s = ff(xd, pt, ed)
        l = -lp.mean() + lam * s.saveval.mean()
        l.backward()
        opt.step()
        losses.append(float(l))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
