"""TrackedFFJORD without a GPU: parameter layout, the refusals, the gaussian-mixture generator, Optimiser(WeightDecay, ADAM), and the fp64
restatements of tests/ffjord_ref.py, each checked against something independent (the CPU oracle's Tsit5 and controller on a plain Dense
chain; e . (J e) with J from torch.autograd.functional.jacobian; autograd double-backward) so that a wrong restatement cannot pass."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import ffjord_ref as R


def _cfg(rn, D, H, **kw):
    cfg = rn._lib.FfjordConfig()
    cfg.in_dims, cfg.hidden, cfg.max_batch, cfg.max_attempts = D, H, 64, 64
    cfg.reltol = cfg.abstol = 1e-5
    cfg.regularize, cfg.cb_save_start, cfg.time_dep = 1, 1, 1
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("D,H,n", [(2, 16, 456), (43, 100, 19572)])
def test_param_count_and_destructure_layout(rnde, D, H, n):
    """456 for the gaussian experiment's MLPDynamics(2, 16), 19,572 for the tabular one's (43, 100): library, package and restatement agree."""
    assert rnde._lib.lib().rnde_ffjord_param_count(C.byref(_cfg(rnde, D, H))) == n
    assert rnde.ffjord.param_count(D, H) == n == R.param_count(D, H)
    m = rnde.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(0))
    p = m.destructure()
    assert p.numel() == n
    # per layer: layer_W column-major, layer_B, bias_W, bias_B, gate_W
    L = R.unpack(p.double(), D, H)
    for (W, b, bw, bb, gw), csl in zip(L, m.layers):
        assert torch.equal(W.float(), csl.W) and torch.equal(b.float(), csl.b) and torch.equal(bw.float(), csl.bw)
        assert torch.equal(bb.float(), csl.bb) and torch.equal(gw.float(), csl.gw)
    assert float(p[D * H]) == 0.0                 # layer_B starts at zero (ffjord_gaussian.jl:56-62)


def test_glorot_init_bounds():
    import regneuralde_jl_amd as rn
    m = rn.ffjord.MLPDynamics(2, 16, generator=torch.Generator().manual_seed(3))
    for csl, (i, o) in zip(m.layers, ((2, 16), (16, 16), (16, 2))):
        assert csl.W.shape == (o, i) and csl.W.abs().max() <= math.sqrt(6 / (i + o))
        assert csl.gw.abs().max() <= math.sqrt(6 / (o + 1)) and torch.count_nonzero(csl.b) == 0


def test_refusals_name_the_limit(rnde):
    """The three out-of-scope cases, in the package and at the C ABI (checked before any device is needed)."""
    ff = rnde.ffjord
    with pytest.raises(ValueError, match="Tracker.forward"):
        ff.TrackedFFJORD(rnde.Chain(rnde.Dense(2, 16), rnde.Dense(16, 2)), [0.0, 1.0], True, False)
    with pytest.raises(ValueError, match="limit of 64"):
        ff.TrackedFFJORD(ff.MLPDynamics(43, 100), [0.0, 1.0], True, False)
    with pytest.raises(ValueError, match="limit of 64"):
        ff.check_served(ff.MLPDynamics(64, 16))
    with pytest.raises(ValueError, match="kinetic energy"):
        ff.check_served(ff.MLPDynamics(2, 16), regularize_kinetic=True)
    L = rnde._lib.lib()
    cases = [(_cfg(rnde, 2, 16, dynamics=1), b"Tracker.forward"), (_cfg(rnde, 43, 100), b"limit of 64"), (_cfg(rnde, 2, 65), b"limit of 64"),
             (_cfg(rnde, 63, 64, kinetic_reg=1), b"kinetic energy")]
    for cfg, msg in cases:
        h = C.c_void_p()
        assert L.rnde_ffjord_create(C.byref(cfg), C.byref(h)) == rnde._lib.BAD_ARG and not h.value
        assert msg in L.rnde_ffjord_last_error(None)


def test_gaussian_mixture_shape_and_statistics(rnde):
    """src/dataset.jl:159-199 with the experiment's arguments: 6 x 341 points, 3 / 4 train, batches of 1024; six clusters on a circle of radius 5
    with per-axis spread sqrt(0.1^2 + 0.3^2)."""
    tr, te = rnde.load_gaussian_mixture(1024, nsamples=2048, ngaussians=6, seed=0)
    assert tr.X.shape == (1534, 2) and te.X.shape == (512, 2) and tr.X.dtype == np.float32
    assert [b.shape[0] for b in tr] == [1024, 510] and [b.shape[0] for b in te] == [512]
    X = np.concatenate([tr.X, te.X])
    ang = np.mod(np.arctan2(X[:, 1], X[:, 0]), 2 * np.pi)
    k = np.mod(np.rint(ang / (np.pi / 3)) - 1, 6).astype(int)            # cluster i sits at angle (i + 1) pi / 3
    assert np.bincount(k, minlength=6).tolist() == [341] * 6
    for i in range(6):
        th = (i + 1) * np.pi / 3
        Y = X[k == i] - 5 * np.array([np.cos(th), np.sin(th)])
        assert np.abs(Y.mean(0)).max() < 0.06
        assert abs(Y.std(0).mean() - math.sqrt(0.01 + 0.09)) < 0.03
    # a seeded generator: the same draws for the same seed, others for another
    tr2, _ = rnde.load_gaussian_mixture(1024, nsamples=2048, seed=0)
    tr3, _ = rnde.load_gaussian_mixture(1024, nsamples=2048, seed=1)
    assert np.array_equal(tr.X, tr2.X) and not np.array_equal(tr.X, tr3.X)


def test_weight_decay_adam_recurrence():
    """Optimiser(WeightDecay(wd), ADAM(eta)) restated: the same recurrence as torch.optim.Adam's L2 weight_decay (g + wd p before the moments)."""
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(50, generator=g, dtype=torch.float64)
    grads = [torch.randn(50, generator=g, dtype=torch.float64) for _ in range(6)]
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=4e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
    p, m, v = p0.clone(), torch.zeros(50, dtype=torch.float64), torch.zeros(50, dtype=torch.float64)
    for t, gr in enumerate(grads, 1):
        q.grad = gr.clone()
        opt.step()
        p, m, v = R.flux_adam_wd(p, gr, m, v, t, 4e-2, wd=1e-5)
    assert torch.allclose(p, q.detach(), rtol=0, atol=1e-12)
    # and the decay term matters
    p2, m2, v2 = p0.clone(), torch.zeros(50, dtype=torch.float64), torch.zeros(50, dtype=torch.float64)
    for t, gr in enumerate(grads, 1):
        p2, m2, v2 = R.flux_adam_wd(p2, gr, m2, v2, t, 4e-2, wd=0.0)
    assert (p - p2).abs().max() > 1e-9


def test_fluxadam_weight_decay_default_changes_nothing():
    import inspect
    from regneuralde_jl_amd import FluxADAM
    assert inspect.signature(FluxADAM.__init__).parameters["weight_decay"].default == 0.0


def _dense64(dims, p, u):
    """Flux Chain(Dense(tanh), Dense) in fp64, the oracle's destructure layout (W as the (in, out) row-major view)."""
    x, o = u, 0
    for l in range(len(dims) - 1):
        W = p[o:o + dims[l] * dims[l + 1]].view(dims[l], dims[l + 1])
        o += dims[l] * dims[l + 1]
        x = x @ W + p[o:o + dims[l + 1]]
        o += dims[l + 1]
        if l < len(dims) - 2:
            x = torch.tanh(x)
    return x


def test_restated_controller_matches_oracle():
    """The restatement's Tsit5 stepper, initial-step rule and PI controller against the CPU oracle (fp64) on a plain Dense chain at tol 1e-5: the
    same attempts, the same accept decisions, dt to 1e-8 and EEst to 1e-7 (fp64 sums in another order), the same end state."""
    from oracle.oracle import Oracle, glorot_params, make_arch
    dims = [3, 8, 3]
    arch = make_arch(dims, ["tanh", "identity"], False)
    rng = np.random.default_rng(1)
    p = glorot_params(arch, rng, np.float64, scale=8.0)
    x = rng.uniform(-2, 2, (5, 3))
    orc = Oracle(arch, np.float64, 1e-5, 1e-5, reg_kind=0, track_ctrl=0, track_initdt=0, max_attempts=500)
    r = orc.forward(x, p)
    assert r["rc"] == 0
    steps = orc.steps_ext()            # t, dt, dtp_in, EEst, accepted, q
    P = torch.from_numpy(p)
    u, log = R.solve(lambda u, t: _dense64(dims, P, u), torch.from_numpy(x), 0.0, 1.0, 1e-5, 1e-5)
    assert len(log) == len(steps) and any(not a for *_, a in log)        # (the case has rejections)
    for (t, dt, e, a), s in zip(log, steps):
        assert bool(a) == bool(s[4])
        assert abs(dt - s[1]) <= 1e-8 * abs(s[1]) and abs(e - s[3]) <= 1e-7 * max(abs(s[3]), 1e-30)
    assert np.abs(u.numpy() - r["u"]).max() <= 1e-10


@pytest.mark.parametrize("D,H", [(2, 16), (5, 7)])
def test_restated_trace_is_hutchinson_of_the_jacobian(D, H):
    """e . eJ of the restated forw_n_back equals e . (J e) with J = d f / d z from torch.autograd.functional.jacobian, and the exact trace is tr J."""
    rng = np.random.default_rng(D)
    p = torch.from_numpy(R.glorot_params(D, H, rng)).double()
    z = torch.from_numpy(rng.standard_normal((4, D)))
    e = torch.from_numpy(rng.standard_normal((4, D)))
    t = 0.37
    f, eJ = R.vjp(p, D, H, z, t, e)
    for b in range(4):
        J = torch.autograd.functional.jacobian(lambda zz: R.mlp(p, D, H, zz[None], t)[0][0], z[b])
        assert torch.allclose(f[b], R.mlp(p, D, H, z[b:b + 1], t)[0][0])
        assert abs(float((e[b] * eJ[b]).sum()) - float(e[b] @ (J @ e[b]))) <= 1e-12 * max(1.0, float(J.abs().max()))
        exact = R.rhs(p, D, H, torch.cat([z, torch.zeros(4, 1, dtype=z.dtype)], 1), t)
        assert abs(float(-exact[b, D]) - float(torch.trace(J))) <= 1e-12


def test_restated_reverse_matches_double_backward():
    """The gradient of the restated trace (an explicit VJP, differentiated by autograd) equals autograd's double-backward of the Hutchinson term
    built with torch.autograd.grad(create_graph=True): sig' and the gate derivatives are right."""
    D, H = 3, 6
    rng = np.random.default_rng(9)
    p = torch.from_numpy(R.glorot_params(D, H, rng)).double().requires_grad_(True)
    z = torch.from_numpy(rng.standard_normal((5, D))).requires_grad_(True)
    e = torch.from_numpy(rng.standard_normal((5, D)))
    w = torch.from_numpy(rng.standard_normal(5))
    t = 0.61
    f, eJ = R.vjp(p, D, H, z, t, e)
    a = ((e * eJ).sum(1) * w).sum() + (f * e).sum()
    ga = torch.autograd.grad(a, (z, p))
    f2 = R.mlp(p, D, H, z, t)[0]
    eJ2 = torch.autograd.grad(f2, z, e, create_graph=True)[0]
    b = ((e * eJ2).sum(1) * w).sum() + (f2 * e).sum()
    gb = torch.autograd.grad(b, (z, p))
    for x, y in zip(ga, gb):
        assert torch.allclose(x, y, rtol=1e-11, atol=1e-13)


def test_restated_replay_is_the_adaptive_solve_along_its_steps():
    """replay() along the accepted steps of solve() reproduces solve()'s end state (the two share tsit5_step; replay adds EEst per step)."""
    D, H = 2, 5
    rng = np.random.default_rng(2)
    p = torch.from_numpy(R.glorot_params(D, H, rng)).double()
    u0 = torch.cat([torch.from_numpy(rng.standard_normal((3, D))), torch.zeros(3, 1, dtype=torch.float64)], 1)
    e = torch.from_numpy(rng.standard_normal((3, D)))
    F = lambda u, t: R.rhs(p, D, H, u, t, e)
    u, log = R.solve(F, u0, 0.0, 1.0, 1e-6, 1e-6)
    acc = [(dt, ee) for (_, dt, ee, a) in log if a]
    u2, eests = R.replay(F, u0, 0.0, [dt for dt, _ in acc], 1e-6, 1e-6)
    assert torch.allclose(u, u2, rtol=0, atol=1e-14)
    assert all(abs(float(x) - y) <= 1e-12 * max(y, 1e-30) for x, (_, y) in zip(eests, acc))
