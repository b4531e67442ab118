"""The leading element-wise map of a Dense chain (include/rnde.h: rnde_pre_act): the cube x -> x .^ 3 of reference
experiments/sde_toy_problem.jl:45 and the tanh of experiments/latent_ode.jl:114, on the ODE chain engine and in the SDE layer.

The CPU oracle knows the tanh only, so the cube is checked against fp64 torch restatements written here (a chain evaluation, a Tsit5 solve
along a given step sequence, an SRI attempt and solve along a given step sequence on a given noise pool), differentiated with autograd.  Each
restatement is first checked against the oracle on a chain without the cube, so that a wrong restatement cannot pass.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRE_CUBE, PRE_TANH = 2, 1


def _pre(sel, u):
    return u ** 3 if sel == PRE_CUBE else (torch.tanh(u) if sel == PRE_TANH else u)


def _chain64(dims, acts, time_dep, pre, p, u, t):
    """Flux re(p)(pre.(u)) in fp64: u (B, D), layer l's W is the (in [+1], out) row-major view of its destructure slice."""
    x, o = _pre(pre, u), 0
    for l in range(len(acts)):
        n_in, n_out = dims[l] + (1 if time_dep else 0), dims[l + 1]
        W = p[o:o + n_in * n_out].view(n_in, n_out)
        o += n_in * n_out
        b = p[o:o + n_out]
        o += n_out
        if time_dep:
            x = torch.cat([x, torch.full((x.shape[0], 1), float(t), dtype=x.dtype)], dim=1)
        x = x @ W + b
        if acts[l] == "tanh":
            x = torch.tanh(x)
    return x


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _params(dims, time_dep, rng, scale=1.0):
    parts = []
    for l in range(len(dims) - 1):
        n_in, n_out = dims[l] + (1 if time_dep else 0), dims[l + 1]
        lim = scale * math.sqrt(6.0 / (n_in + n_out))
        parts += [rng.uniform(-lim, lim, n_in * n_out), 0.1 * rng.standard_normal(n_out)]
    return np.concatenate(parts).astype(np.float32)


SHAPES = {"small_td": ([3, 7, 3], ["tanh", "identity"], True), "deep": ([5, 12, 9, 5], ["tanh", "tanh", "identity"], False)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("col_tile", [64, 0], ids=["one-wave", "four-wave"])
def test_feval_cube_matches_fp64(shape, col_tile):
    """(a) rnde_debug_feval with RNDE_PRE_CUBE against fp64 N(u^3): one time-dependent shape, one deeper time-independent one, both chain kernels."""
    from tests.util import Node, make_cfg
    dims, acts, td = SHAPES[shape]
    rng = np.random.default_rng(1)
    B = 37
    p = _params(dims, td, rng)
    u = rng.uniform(-1.3, 1.3, (B, dims[0])).astype(np.float32)
    node = Node(make_cfg(dims, acts, B, time_dep=td, pre_act=PRE_CUBE, col_tile=col_tile, regularize=0))
    got = node.feval(u, p, 0.3)
    ref = _chain64(dims, acts, td, PRE_CUBE, torch.from_numpy(p).double(), torch.from_numpy(u).double(), 0.3).numpy()
    assert _rel(got, ref) <= 2e-6, _rel(got, ref)
    # and not the tanh it was before the selector
    assert _rel(got, _chain64(dims, acts, td, PRE_TANH, torch.from_numpy(p).double(), torch.from_numpy(u).double(), 0.3).numpy()) > 1e-2
    node.close()


def test_unknown_selector_is_refused():
    import ctypes as C
    from regneuralde_jl_amd import _lib
    from tests.util import make_cfg
    h = C.c_void_p()
    assert _lib.lib().rnde_node_create(C.byref(make_cfg([3, 5, 3], ["tanh", "identity"], 4, time_dep=False, pre_act=3)), C.byref(h)) == _lib.BAD_ARG


def _tsit5_replay64(dims, acts, td, pre, p, x, dts, tab):
    """Tsit5 along the given (all accepted) step sizes, fp64 torch: k1 = f(u), k_s = f(u + dt sum_j a[s][j] k_j, t + c_s dt), u += dt sum a[6][j] k_j."""
    a, c, _ = tab
    u, t = x, 0.0
    k1 = _chain64(dims, acts, td, pre, p, u, t)
    for dt in dts:
        k = [k1]
        for s in range(1, 7):
            g = u + dt * sum(float(a[s][j]) * k[j] for j in range(s) if a[s][j] != 0)
            k.append(_chain64(dims, acts, td, pre, p, g, t + float(c[s]) * dt))
        u = u + dt * sum(float(a[6][j]) * k[j] for j in range(6) if a[6][j] != 0)
        t += dt
        k1 = k[6]
    return u


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_ode_replay_cube_forward_and_reverse(shape):
    """(b) rnde_node_forward_replay + rnde_node_backward along a fixed all-accepted sequence (no controller or initial-step tracking: the
    sequence is a constant of the program) against the fp64 Tsit5 restatement with autograd: u <= 2e-4, x-bar and p-bar <= 1e-3 relative."""
    from oracle.oracle import Oracle, make_arch
    from tests.util import Node, make_cfg
    dims, acts, td = SHAPES[shape]
    rng = np.random.default_rng(2)
    B = 21
    p = _params(dims, td, rng)
    x = rng.uniform(-1.0, 1.0, (B, dims[0])).astype(np.float32)
    dts = [0.125] * 8                                    # sums to t1 = 1 exactly
    orc = Oracle(make_arch(dims, acts, td, pre_act=True), np.float64, 1e-3, 1e-3, reg_kind=0, track_ctrl=0, track_initdt=0, max_attempts=16)
    tab = orc.tableau()
    P, X = torch.from_numpy(p).double(), torch.from_numpy(x).double()
    # the restatement itself, on the oracle's tanh chain
    orc.set_replay(np.array(dts), np.ones(len(dts), np.int32))
    r = orc.forward(x.astype(np.float64), p.astype(np.float64))
    assert r["rc"] == 0 and r["nattempts"] == len(dts)
    assert _rel(_tsit5_replay64(dims, acts, td, PRE_TANH, P, X, dts, tab).numpy(), r["u"]) <= 1e-10
    # the cube on the device
    node = Node(make_cfg(dims, acts, B, time_dep=td, pre_act=PRE_CUBE, regularize=0, track_ctrl=0, track_initdt=0, max_attempts=16))
    got = node.forward_replay(x, p, dts, [1] * len(dts), keep_tape=True)
    assert got["nattempts"] == len(dts) and got["nfe"] > 0
    Pg, Xg = P.clone().requires_grad_(True), X.clone().requires_grad_(True)
    u = _tsit5_replay64(dims, acts, td, PRE_CUBE, Pg, Xg, dts, tab)
    assert _rel(got["u"], u.detach().numpy()) <= 2e-4
    ubar = rng.standard_normal(x.shape).astype(np.float32)
    xb, pb, _ = node.backward(ubar)
    gx, gp = torch.autograd.grad(u, (Xg, Pg), torch.from_numpy(ubar).double())
    assert _rel(xb, gx.numpy()) <= 1e-3 and _rel(pb, gp.numpy()) <= 1e-3
    node.close()


# ---- the SDE layer -------------------------------------------------------------------------------------------------------------------

def _sri_attempt64(tab, drift, diff, u, dt, dW, dZ):
    """One SRI attempt with diagonal noise in fp64 (drift, diff: u -> value); returns (k[4], g[4], unew)."""
    sq = math.sqrt(abs(dt))
    chi2 = (dW + dZ / math.sqrt(3.0)) / 2
    k, g = [], []
    for s in range(4):
        h0 = u + sum(dt * float(tab["A0"][s][j]) * k[j] + chi2 * float(tab["B0"][s][j]) * g[j] for j in range(s)) if s else u
        h1 = u + sum(dt * float(tab["A1"][s][j]) * k[j] + sq * float(tab["B1"][s][j]) * g[j] for j in range(s)) if s else u
        k.append(drift(h0))
        g.append(diff(h1))
    chi1 = (dW * dW - abs(dt)) / (2 * sq)
    chi3 = (dW ** 3 - 3 * dW * dt) / (6 * dt)
    sa = sum(float(tab["alpha"][j]) * k[j] for j in range(4))
    s1, s2, s3, s4 = (sum(float(tab[b][j]) * g[j] for j in range(4)) for b in ("beta1", "beta2", "beta3", "beta4"))
    return k, g, u + dt * sa + chi2 * s3 + chi3 * s4 + dW * s1 + chi1 * s2


TOY = ([2, 50, 2], ["tanh", "identity"], [2, 2], ["identity"])     # experiments/sde_toy_problem.jl:45-46


def _toy_setup(seed, B, n_pool, scale=1.0):
    rng = np.random.default_rng(seed)
    dd, da, gd, ga = TOY
    p = np.concatenate([_params(dd, False, rng, scale), _params(gd, False, rng, 0.5)]).astype(np.float32)
    x = np.tile(np.array([[2.0, 0.0]], np.float32), (B, 1)) + 0.1 * rng.standard_normal((B, 2)).astype(np.float32)
    noise = rng.standard_normal((n_pool, 2, B, 2)).astype(np.float32)
    return p, x, noise


def _nets64(p, pre_f, pre_g, nd):
    dd, da, gd, ga = TOY
    return (lambda v: _chain64(dd, da, False, pre_f, p[:nd], v, 0.0)), (lambda v: _chain64(gd, ga, False, pre_g, p[nd:], v, 0.0))


def _toy_node(B, pre_f, pre_g, **kw):
    import ctypes as C
    from regneuralde_jl_amd import _lib
    from tests.util import NsdeNode, make_nsde_cfg
    dd, da, gd, ga = TOY
    node = NsdeNode(make_nsde_cfg(dd, da, gd, ga, B, **kw))
    _lib.check_nsde(node.h, node.L.rnde_nsde_set_pre_act(node.h, pre_f, pre_g))
    return node


def test_sde_attempt_cube_matches_fp64():
    """(c) rnde_nsde_debug_attempt on the toy's drift (cube, 2 -> 50 -> 2) and diagonal Dense(2, 2) diffusion against the fp64 SRI restatement;
    the restatement checked first against SdeOracle.attempt on the same nets without the cube."""
    from oracle.oracle import make_arch
    from oracle.oracle_sde import SdeOracle, sri_tableau
    dd, da, gd, ga = TOY
    B, dt = 37, 0.07
    p, x, noise = _toy_setup(3, B, 1)
    dW, dZ = math.sqrt(dt) * noise[0, 0], math.sqrt(dt) * noise[0, 1]
    tab = sri_tableau("SOSRI")
    nd = sum((dd[l] * dd[l + 1] + dd[l + 1]) for l in range(len(da)))
    P, X, W, Z = (torch.from_numpy(np.asarray(a, np.float64)) for a in (p, x, dW, dZ))
    o64 = SdeOracle(make_arch(dd, da, False), make_arch(gd, ga, False), np.float64)
    kg_o, un_o, _ = o64.attempt(p, x, dt, dW, dZ)
    k, g, un = _sri_attempt64(tab, *_nets64(P, 0, 0, nd), X, dt, W, Z)
    assert _rel(un.numpy(), un_o) <= 1e-10 and _rel(torch.stack(k + g).numpy(), kg_o) <= 1e-10
    node = _toy_node(B, PRE_CUBE, 0)
    kg, un_d, e = node.attempt(x, p, dt, dW, dZ)
    k, g, un = _sri_attempt64(tab, *_nets64(P, PRE_CUBE, 0, nd), X, dt, W, Z)
    assert _rel(kg, torch.stack(k + g).numpy()) <= 2e-5 and _rel(un_d, un.numpy()) <= 2e-5 and math.isfinite(e)
    node.close()


def test_sde_replay_cube_forward_and_reverse():
    """(c) a full rnde_nsde_forward_replay + rnde_nsde_backward along a fixed all-accepted sequence with an explicit noise pool (step n takes draw n,
    scaled by sqrt(dt)) against the fp64 restatement with autograd, checked first against SdeOracle's replay without the cube."""
    from oracle.oracle import make_arch
    from oracle.oracle_sde import SdeOracle, sri_tableau
    dd, da, gd, ga = TOY
    B = 24
    dts = [0.125] * 8
    p, x, noise = _toy_setup(4, B, 12)
    tab = sri_tableau("SOSRI")
    nd = sum((dd[l] * dd[l + 1] + dd[l + 1]) for l in range(len(da)))

    def solve(Pt, Xt, pre_f):
        drift, diff = _nets64(Pt, pre_f, 0, nd)
        u = Xt
        for n, dt in enumerate(dts):
            W, Z = (math.sqrt(dt) * torch.from_numpy(noise[n, j].astype(np.float64)) for j in (0, 1))
            u = _sri_attempt64(tab, drift, diff, u, dt, W, Z)[2]
        return u

    P, X = torch.from_numpy(p).double(), torch.from_numpy(x).double()
    o64 = SdeOracle(make_arch(dd, da, False), make_arch(gd, ga, False), np.float64, 0.3, 0.3, reg_kind=0, max_attempts=16)
    o64.set_replay(np.array(dts), np.ones(len(dts), np.int32))
    r = o64.forward(x, p, noise)
    assert r["rc"] == 0 and r["nattempts"] == len(dts)
    assert _rel(solve(P, X, 0).numpy(), r["u"]) <= 1e-10
    node = _toy_node(B, PRE_CUBE, 0, reltol=0.3, abstol=0.3, regularize=0, max_attempts=16)
    got = node.forward(x, p, noise, keep_tape=True, replay=np.stack([np.array(dts), np.ones(len(dts))], 1))
    assert got["nattempts"] == len(dts)
    Pg, Xg = P.clone().requires_grad_(True), X.clone().requires_grad_(True)
    u = solve(Pg, Xg, PRE_CUBE)
    assert _rel(got["u"], u.detach().numpy()) <= 2e-4
    ubar = (np.random.default_rng(5).standard_normal(x.shape) / B).astype(np.float32)
    xb, pb = node.backward(ubar)
    gx, gp = torch.autograd.grad(u, (Xg, Pg), torch.from_numpy(ubar).double())
    assert _rel(xb, gx.numpy()) <= 1e-3 and _rel(pb, gp.numpy()) <= 1e-3
    node.close()


@pytest.mark.parametrize("kind", ["nsde", "small"])
def test_sde_leading_tanh_matches_oracle(kind):
    """(d) A leading tanh in the drift is honoured: a full adaptive solve + reverse against SdeOracle built with make_arch(..., pre_act=True) on the
    same noise -- the same attempts, u <= 2e-4, gradients <= 1e-3.  "nsde" is the reference's 32 -> 64 -> 32 shape, whose compile-time-shape
    kernels apply no map: the handle must leave them."""
    from oracle.oracle import make_arch
    from oracle.oracle_sde import SdeOracle, nsde_params
    from tests.util import NsdeNode, make_nsde_cfg
    from regneuralde_jl_amd import _lib
    if kind == "nsde":
        dd, da, gd, ga, B = [32, 64, 32], ["tanh", "identity"], [32, 32], ["identity"], 48
    else:
        dd, da, gd, ga, B = [3, 5, 3], ["tanh", "identity"], [3, 3], ["identity"], 7
    drift, diff = make_arch(dd, da, False, pre_act=True), make_arch(gd, ga, False)
    rng = np.random.default_rng(9)
    p = nsde_params(drift, diff, rng, np.float32, 2.0, 0.5)
    x = rng.standard_normal((B, dd[0])).astype(np.float32)
    noise = rng.standard_normal((300, 2, B, dd[0])).astype(np.float32)
    o32 = SdeOracle(drift, diff, np.float32, max_attempts=299)
    r32 = o32.forward(x, p, noise)
    assert r32["rc"] == 0
    o64 = SdeOracle(drift, diff, np.float64, max_attempts=299)
    o64.set_replay(r32["steps"][:, 1], r32["steps"][:, 3].astype(np.int32))
    r64 = o64.forward(x, p, noise)
    node = NsdeNode(make_nsde_cfg(dd, da, gd, ga, B, max_attempts=299))
    _lib.check_nsde(node.h, node.L.rnde_nsde_set_pre_act(node.h, PRE_TANH, 0))
    got = node.forward(x, p, noise, keep_tape=True)
    assert got["nattempts"] == r32["nattempts"] and np.array_equal(got["steps"][:, 3], r32["steps"][:, 3])
    assert got["nfe1"] == r32["nfe1"] and got["ndraws"] == r32["ndraws"]
    assert _rel(got["u"], r64["u"]) <= 2e-4
    ubar = (rng.standard_normal(x.shape) / B).astype(np.float32)
    svbar = (0.2 * rng.standard_normal(len(got["saveval"]))).astype(np.float32)
    xb, pb = node.backward(ubar, svbar)
    g64 = o64.backward(ubar, svbar)
    assert _rel(xb, g64[0]) <= 1e-3 and _rel(pb, g64[1]) <= 1e-3
    node.close()


def test_layer_call_honours_a_leading_tanh():
    """TrackedNeuralDSDE(Chain(..., pre_act=True), ...) integrates the vector field it was given (the handle gets the selector)."""
    import regneuralde_jl_amd as rn
    from oracle.oracle import make_arch
    from oracle.oracle_sde import SdeOracle
    g = torch.Generator().manual_seed(3)
    B = 9
    nsde = rn.TrackedNeuralDSDE(rn.Chain(rn.Dense(3, 6, "tanh", g), rn.Dense(6, 3, "identity", g), pre_act=True), rn.Dense(3, 3, "identity", g),
                                [0.0, 1.0], False, "SOSRI", reltol=0.14, abstol=0.14, max_batch=B)
    x = torch.randn(B, 3, generator=g)
    noise = torch.randn(200, 2, B, 3, generator=g)
    with torch.no_grad():
        u, nfe1, _, _ = nsde(x.cuda(), nsde.p.cuda(), noise=noise.cuda())
    o = SdeOracle(make_arch([3, 6, 3], ["tanh", "identity"], False, pre_act=True), make_arch([3, 3], ["identity"], False), np.float32, 0.14, 0.14,
                  reg_kind=0, max_attempts=199)
    r = o.forward(x.numpy(), nsde.p.numpy(), noise.numpy())
    assert r["rc"] == 0 and nfe1 == r["nfe1"]
    assert _rel(u.cpu().numpy(), r["u"]) <= 2e-4
