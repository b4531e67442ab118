"""TrackedFFJORD{false} called with regularize = true on the device (rnde_ffjord_*_kinetic, both engines) against the fp64 restatement of
tests/ffjord_kinetic_ref.py (itself checked against torch.autograd.functional.jacobian in tests/test_ffjord_kinetic_host.py): one
evaluation, the solve and its reverse along a fixed step sequence, the controller over D + 3 rows, the layer's five-tuple, and the tapes."""
import numpy as np
import pytest
import torch

from tests import ffjord_kinetic_ref as K
from tests import ffjord_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WG, TL = "workgroup", "tiled"
SHAPES = [(WG, 2, 16), (WG, 16, 64), (WG, 61, 64), (TL, 5, 20), (TL, 43, 100)]


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _layer(engine, D, H, B, p, regularize=False, tol=1e-5):
    import regneuralde_jl_amd as rn
    m = rn.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(0))
    ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, regularize, "Tsit5", reltol=tol, abstol=tol, max_batch=B, engine=engine)
    ff.p = p.to(DEV)
    return ff


@pytest.mark.parametrize("engine,D,H", SHAPES)
def test_kinetic_rhs_matches_fp64(engine, D, H):
    """f, the trace row and the two regulariser rows against fp64; B = 1 and B = 37 (two full tiles and a partial one), t = 0 and 0.71."""
    for B in (1, 37):
        p, x, e, _ = K.draw(D, H, B, 1, 1.0)
        ff = _layer(engine, D, H, B, p)
        for t in (0.0, 0.71):
            got = ff.feval(x.to(DEV), t, e.to(DEV), regularize=True).cpu()
            ref = K.rhs_kinetic(p.double(), D, H, K.aug(x.double(), 3), t, e.double())
            assert got.shape == (B, D + 3)
            devs = [_rel(got[:, :D], ref[:, :D])] + [_rel(got[:, D + i], ref[:, D + i]) for i in range(3)]
            print(engine, D, H, B, t, devs)
            assert devs[0] <= 2e-6 and max(devs[1:]) <= 2e-5, devs
            assert torch.equal(got[:, :D + 1], ff.feval(x.to(DEV), t, e.to(DEV)).cpu())      # the plain rows are the plain call's


@pytest.mark.parametrize("engine,D,H", SHAPES)
def test_kinetic_replay_forward_and_reverse(engine, D, H):
    """Along a fixed all-accepted sequence: logpx, lambda1, lambda2 against the fp64 replay (1e-5); x-bar and p-bar of
    sum g logpx + sum g1 lambda1 + sum g2 lambda2 against autograd through it (1e-3).  On the reference alone: each lambda cotangent moves the
    gradient by more than 1e-1 of its largest entry (so the test cannot pass with them dropped), and logpx does not depend on the two rows."""
    B, tol, dts = 37, 1e-5, [0.5, 0.5]
    p, x, e, rng = K.draw(D, H, B, 2, 3.0)
    g, g1, g2 = (torch.from_numpy(rng.standard_normal(B)) for _ in range(3))
    steps = sum(([dt, 1.0] for dt in dts), [])
    Pg, Xg = p.double().requires_grad_(True), x.double().requires_grad_(True)
    u, _ = R.replay(lambda u, t: K.rhs_kinetic(Pg, D, H, u, t, e.double()), K.aug(Xg, 3), 0.0, dts, tol, tol)
    lp_ref, l1_ref, l2_ref = R.logpx_of(u, D), u[:, D + 1], u[:, D + 2]
    with torch.no_grad():
        up, _ = R.replay(lambda u, t: R.rhs(Pg, D, H, u, t, e.double()), K.aug(Xg, 1), 0.0, dts, tol, tol)
    assert torch.equal(R.logpx_of(up, D), lp_ref.detach())
    terms = [(lp_ref * g).sum(), (l1_ref * g1).sum(), (l2_ref * g2).sum()]
    (gx0, gp0), (gx1, gp1), (gx2, gp2) = (torch.autograd.grad(v, (Xg, Pg), retain_graph=True) for v in terms)
    gx, gp = gx0 + gx1 + gx2, gp0 + gp1 + gp2
    moved = (_rel(gp0 + gp1, gp0), _rel(gp0 + gp2, gp0), _rel(gx, gx0))
    print(engine, D, H, "reference: the cotangents move the gradients by", moved)
    assert min(moved) > 1e-1, moved

    ff = _layer(engine, D, H, B, p)
    xd, pd = x.to(DEV).requires_grad_(True), ff.p.clone().requires_grad_(True)
    logpx, l1, l2, nfe, sv = ff(xd, pd, e.to(DEV), regularize=True, steps=steps)
    assert nfe == 3 + 6 * len(dts) and sv is None and l1.shape == l2.shape == (B,)
    fw = (_rel(logpx, lp_ref), _rel(l1, l1_ref), _rel(l2, l2_ref))
    (logpx * g.float().to(DEV)).sum().add((l1 * g1.float().to(DEV)).sum()).add((l2 * g2.float().to(DEV)).sum()).backward()
    bw = (_rel(xd.grad, gx), _rel(pd.grad, gp))
    with torch.no_grad():
        plain = ff(x.to(DEV), ff.p, e.to(DEV), steps=steps)[0]
    print(engine, D, H, "forward", fw, "reverse", bw, "logpx against the plain call", _rel(logpx, plain))
    assert max(fw) <= 1e-5, fw
    assert _rel(logpx, plain) <= 1e-5
    assert max(bw) <= 1e-3, bw


@pytest.mark.parametrize("engine,D,H,B,seed", [(WG, 2, 16, 256, 7), (TL, 5, 20, 37, 5)])
def test_kinetic_adaptive_solve_controls_all_rows(engine, D, H, B, seed):
    """tol 1e-5, x = 3 N(0, 1), scale 6: the controller runs over D + 3 rows.  The lambda rows start at zero, so the first steps are tiny and
    their EEst sits below the fp32 floor: the device's step sequence is not the fp64 controller's, and attempt-for-attempt equality is not
    asserted.  Instead each logged EEst is recomputed in fp64 along the device's own (dt, accepted) sequence and compared on the attempts S
    with fp64 EEst >= 0.1, within three times the deviation of an fp32 torch restatement along the same sequence (asserted <= 0.1).  At
    least 10 attempts of S tell the D + 3-row norm from the D + 1-row one by >= 0.25 relative."""
    tol = 1e-5
    p, x, e, _ = K.draw(D, H, B, seed, 6.0, xscale=3.0)
    ff = _layer(engine, D, H, B, p)
    with torch.no_grad():
        logpx, l1, l2, nfe, _ = ff(x.to(DEV), None, e.to(DEV), regularize=True)
    log = ff.step_log()
    assert log.ndim == 2 and log.shape[1] == 4 and nfe == 3 + 6 * len(log)
    assert np.array_equal(log[:, 3] != 0, log[:, 2] <= 1.0)                   # accepted is consistent with the logged EEst
    assert np.array_equal(np.array(ff.steps()).reshape(-1, 2), log[:, [1, 3]])
    seq = [(float(dt), bool(a)) for _, dt, _, a in log]
    P64, P32 = p.double(), p.float()
    F64 = lambda u, t: K.rhs_kinetic(P64, D, H, u, t, e.double())
    F32 = lambda u, t: K.rhs_kinetic(P32, D, H, u, t, e.float())
    u64, e64, e64p = K.eests_along(F64, K.aug(x.double(), 3), 0.0, seq, tol, tol, rows=D + 1)
    _, e32 = K.eests_along(F32, K.aug(x.float(), 3), 0.0, seq, tol, tol)
    e64, e64p, e32 = np.array(e64), np.array(e64p), np.array(e32)
    S = e64 >= 0.1
    disc = S & (np.abs(e64p / e64 - 1) >= 0.25)
    bound = 3 * np.abs(e32[S] / e64[S] - 1).max()
    dev = np.abs(log[S, 2] / e64[S] - 1).max()
    dt_kin = K.initial_dt(F64, K.aug(x.double(), 3), 0.0, 1.0, tol, tol)
    dt_plain = K.initial_dt(lambda u, t: R.rhs(P64, D, H, u, t, e.double()), K.aug(x.double(), 1), 0.0, 1.0, tol, tol)
    print(engine, D, H, "attempts", len(log), "rejected", int((log[:, 3] == 0).sum()), "S", int(S.sum()), "discriminating", int(disc.sum()),
          "bound", bound, "device", dev, "first dt", log[0, 1], "rule over D + 3 rows", dt_kin, "over D + 1 rows", dt_plain)
    assert S.sum() >= 10 and disc.sum() >= 10 and bound <= 0.1                # (conditions on the reference alone)
    assert dt_plain > 10 * dt_kin                                             # (so the first step tells the two rules apart)
    assert dev <= bound, (dev, bound)
    assert abs(log[0, 1] / dt_kin - 1) <= 2e-2
    fw = (_rel(logpx, R.logpx_of(u64, D)), _rel(l1, u64[:, D + 1]), _rel(l2, u64[:, D + 2]))
    print("forward", fw)
    assert max(fw) <= 1e-5, fw


@pytest.mark.parametrize("engine,D,H", [(WG, 2, 16), (TL, 5, 20)])
def test_kinetic_layer_call_and_training_step(engine, D, H):
    """ff(x, p, e, regularize=True) on a {false} layer: the five-tuple with differentiable lambdas; one training step's gradient against autograd
    through the fp64 replay along the device's steps; a {true} layer ignores the keyword; a plain call keeps its bits across a kinetic one."""
    B, tol = 37, 1e-5
    p, x, e, _ = K.draw(D, H, B, 3, 3.0)
    ff = _layer(engine, D, H, B, p)
    xd, ed = x.to(DEV), e.to(DEV)
    with torch.no_grad():
        before = ff(xd, None, ed)[0].clone()
    pa = ff.p.clone().requires_grad_(True)
    lpa = ff(xd, pa, ed)[0]                                                   # a plain tape, held across the handle's first kinetic calls
    pd = ff.p.clone().requires_grad_(True)
    out = ff(xd, pd, ed, regularize=True)
    assert len(out) == 5 and out[4] is None and out[3] == ff.last_nfe
    logpx, l1, l2 = out[:3]
    assert l1.requires_grad and l2.requires_grad and l1.is_cuda and l1.shape == l2.shape == (B,)
    acc = [float(dt) for _, dt, _, a in ff.step_log() if a]
    (-logpx.mean() + 0.01 * l1.mean() + 0.01 * l2.mean()).backward()
    Pg = p.double().requires_grad_(True)
    u, _ = R.replay(lambda u, t: K.rhs_kinetic(Pg, D, H, u, t, e.double()), K.aug(x.double(), 3), 0.0, acc, tol, tol)
    ref = -R.logpx_of(u, D).mean() + 0.01 * u[:, D + 1].mean() + 0.01 * u[:, D + 2].mean()
    gp = torch.autograd.grad(ref, Pg)[0]
    print(engine, D, H, "accepted", len(acc), "p-bar", _rel(pd.grad, gp))
    assert _rel(pd.grad, gp) <= 1e-3
    with torch.no_grad():
        after = ff(xd, None, ed)[0]
        assert torch.equal(ff(xd, None, ed, regularize=True)[1], l1.detach())  # (untaped handle: grown by this call)
        assert torch.equal(ff(xd, None, ed)[0], before)
    assert torch.equal(after, before)
    pb = ff.p.clone().requires_grad_(True)
    (-ff(xd, pb, ed)[0].mean()).backward()
    (-lpa.mean()).backward()
    assert torch.equal(pa.grad, pb.grad)
    # an unused output's None gradient counts as zeros
    pe = ff.p.clone().requires_grad_(True)
    ff(xd, pe, ed, regularize=True)[1].sum().backward()
    assert torch.isfinite(pe.grad).all() and pe.grad.abs().max() > 0
    # {true}: the keyword is ignored (ffjord.jl:119)
    ft = _layer(engine, D, H, B, p, regularize=True)
    with torch.no_grad():
        lp, z1, z2, _, sv = ft(xd, None, ed, regularize=True)
        lp0, _, _, _, sv0 = ft(xd, None, ed)
    assert torch.count_nonzero(z1) == 0 and torch.count_nonzero(z2) == 0 and sv.saveval.numel() > 1
    assert torch.equal(lp, lp0) and torch.equal(sv.saveval, sv0.saveval)


@pytest.mark.parametrize("engine,D,H", [(WG, 2, 16), (TL, 5, 20)])
def test_kinetic_and_plain_tapes_interleave(engine, D, H):
    """A kinetic and a plain taped forward interleaved, an inference call and a sample between them: each gives the gradient of the same call
    run alone, bit for bit; a second backward through a released kinetic tape raises."""
    import regneuralde_jl_amd as rn
    B = 37
    p, x, e, rng = K.draw(D, H, B, 6, 1.0)
    ff = _layer(engine, D, H, B, p)
    xa, ea = x.to(DEV), e.to(DEV)
    xb = torch.from_numpy(rng.standard_normal((B - 10, D)).astype(np.float32)).to(DEV)
    eb = torch.from_numpy(rng.standard_normal((B - 10, D)).astype(np.float32)).to(DEV)

    def kinetic(pp):
        lp, l1, l2, _, _ = ff(xa, pp, ea, regularize=True)
        return -lp.mean() + 0.5 * l1.mean() + 0.25 * l2.mean()

    def plain(pp):
        return -ff(xb, pp, eb)[0].mean()

    def alone(fn):
        pp = ff.p.clone().requires_grad_(True)
        fn(pp).backward()
        return pp.grad.clone()

    ga, gb = alone(kinetic), alone(plain)
    pa, pb = ff.p.clone().requires_grad_(True), ff.p.clone().requires_grad_(True)
    loss_a = kinetic(pa)
    with torch.no_grad():
        ff(xb, ff.p, eb)
    rn.sample(ff, D, nsamples=B)
    loss_b = plain(pb)
    with torch.no_grad():
        ff(xa, ff.p, ea, regularize=True)
    loss_a.backward(retain_graph=True)
    loss_b.backward()
    assert torch.equal(pa.grad, ga) and torch.equal(pb.grad, gb)
    with pytest.raises(RuntimeError, match="released"):
        loss_a.backward()
