"""The Dense activations relu, sigmoid, softplus and elu (include/rnde.h: rnde_act) on the chain engine and in the SDE layer, against fp64 torch
restatements (tests/act_ref.py) differentiated with autograd.  The CPU oracle knows identity and tanh only, so every restatement is first checked
against it on tanh chains: a wrong restatement cannot pass.

relu and elu have a kink at 0: where a pre-activation sits within rounding of 0 the fp32 device and the fp64 restatement may take different sides,
and a relu derivative differs by 1 there.  The relu / elu cases assert that no pre-activation of the restatement lies within 1e-4 of 0 for the
seeds used, so such a flip cannot make them flaky.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests.act_ref import CODES, NEW, chain64, params, rel, rk_replay64, sri_attempt64

pytestmark = pytest.mark.gpu

KINK = 1e-4
REPLAY_WIDE_SEED = 23      # (vetted for the kink margin of relu)
# (dims, acts with A = the activation under test, time_dep, pre_act)
SHAPES = {
    "small_td": ([3, 7, 3], ["A", "A"], True, 0),                                        # the last layer too: its padding rows must stay 0
    "deep": ([5, 12, 9, 5], ["A", "tanh", "A"], False, 0),
    "latent": ([20, 50, 20, 50, 20, 50, 20, 50, 20], ["A"] * 7 + ["identity"], False, 1),  # latent_ode.jl's widths, a leading tanh: not mw_lat
    "wide": ([38, 45, 38], ["A", "A"], False, 0),            # 33..64 features: the 16-k-step kernels, padding inside the last k-step and tile
}


def _acts(shape, act):
    return [act if a == "A" else a for a in SHAPES[shape][1]]


def _cfg(dims, acts, B, **kw):
    from tests.util import make_cfg
    cfg = make_cfg(dims, ["identity"] * len(acts), B, **kw)
    for i, a in enumerate(acts):
        cfg.act[i] = CODES[a]
    return cfg


def _kink_free(act, preacts):
    if act in ("relu", "elu"):
        m = min(float(z.abs().min()) for z in preacts)
        assert m > KINK, f"a pre-activation within {KINK} of the kink ({m:.2e}): pick another seed"


SEEDS = {"small_td": 11, "deep": 11, "latent": 12, "wide": 11}      # (vetted for the kink margin of relu / elu)


def _feval_case(shape, act, seed=None, B=8):
    dims, _, td, pre = SHAPES[shape]
    seed = SEEDS[shape] if seed is None else seed
    acts = _acts(shape, act)
    rng = np.random.default_rng(seed)
    p = params(dims, td, rng, bias=0.3)
    u = rng.uniform(-1.3, 1.3, (B, dims[0])).astype(np.float32)
    pa = []
    ref = chain64(dims, acts, td, pre, torch.from_numpy(p).double(), torch.from_numpy(u).double(), 0.3, pa).numpy()
    return dims, acts, td, pre, p, u, ref, pa


# ---- the restatements, on tanh chains, against the CPU oracle ------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_chain_restatement_matches_oracle_on_tanh(shape):
    from oracle.oracle import Oracle, make_arch
    dims, acts, td, pre, p, u, ref, _ = _feval_case(shape, "tanh")
    orc = Oracle(make_arch(dims, acts, td, pre_act=bool(pre)), np.float64)
    assert rel(ref, orc.f_eval(p.astype(np.float64), u.astype(np.float64), 0.3)) <= 1e-12


@pytest.mark.parametrize("solver", ["Tsit5", "DP5"])
def test_rk_replay_restatement_matches_oracle_on_tanh(solver):
    """A sequence with a rejected attempt in it (FSAL: k1 is kept across the rejection)."""
    from oracle.oracle import Oracle, make_arch
    dims, acts, td = [3, 7, 3], ["tanh", "tanh"], True
    rng = np.random.default_rng(2)
    p, x = params(dims, td, rng, bias=0.3), rng.uniform(-1, 1, (6, 3))
    dtp, acc = [0.25, 0.5, 0.25, 0.25, 0.25], [1, 0, 1, 1, 1]
    orc = Oracle(make_arch(dims, acts, td), np.float64, 1e-3, 1e-3, reg_kind=0, track_ctrl=0, track_initdt=0, max_attempts=16, solver=solver)
    orc.set_replay(np.array(dtp), np.array(acc, np.int32))
    r = orc.forward(x, p.astype(np.float64))
    assert r["rc"] == 0 and r["nattempts"] == len(dtp)
    att = [(float(s[0]), float(s[1]), int(s[3])) for s in r["steps"]]
    f = lambda v, t: chain64(dims, acts, td, 0, torch.from_numpy(p).double(), v, t)
    assert rel(rk_replay64(f, torch.from_numpy(x), att, orc.tableau()).numpy(), r["u"]) <= 1e-10


def test_sri_restatement_matches_oracle_on_tanh():
    from oracle.oracle import make_arch
    from oracle.oracle_sde import SdeOracle, sri_tableau
    dd, da, gd, ga = [32, 64, 32], ["tanh", "identity"], [32, 32], ["tanh"]
    rng = np.random.default_rng(3)
    B, dt = 5, 0.05
    p = np.concatenate([params(dd, False, rng), params(gd, False, rng, 0.5)])
    x = rng.standard_normal((B, 32))
    dW, dZ = math.sqrt(dt) * rng.standard_normal((B, 32)), math.sqrt(dt) * rng.standard_normal((B, 32))
    nd = 32 * 64 + 64 + 64 * 32 + 32
    P = torch.from_numpy(p).double()
    drift = lambda v: chain64(dd, da, False, 0, P[:nd], v, 0.0)
    diff = lambda v: chain64(gd, ga, False, 0, P[nd:], v, 0.0)
    k, g, un = sri_attempt64(sri_tableau("SOSRI"), drift, diff, torch.from_numpy(x), dt, torch.from_numpy(dW), torch.from_numpy(dZ))
    o64 = SdeOracle(make_arch(dd, da, False), make_arch(gd, ga, False), np.float64)
    kg_o, un_o, _ = o64.attempt(p, x, dt, dW, dZ)
    assert rel(un.numpy(), un_o) <= 1e-10 and rel(torch.stack(k + g).numpy(), kg_o) <= 1e-10


# ---- one evaluation ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act", NEW)
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("col_tile", [64, 0], ids=["one-wave", "four-wave"])
def test_feval_matches_fp64(act, shape, col_tile):
    """rnde_debug_feval against the fp64 chain, both chain kernels; and not what tanh in those layers would give (codes 2-5 once ran tanh)."""
    from tests.util import Node
    dims, acts, td, pre, p, u, ref, pa = _feval_case(shape, act)
    _kink_free(act, pa)
    node = Node(_cfg(dims, acts, u.shape[0], time_dep=td, pre_act=pre, col_tile=col_tile, regularize=0))
    got = node.feval(u, p, 0.3)
    assert rel(got, ref) <= 2e-6, rel(got, ref)
    tanh_ref = chain64(dims, [("tanh" if a == act else a) for a in acts], td, pre, torch.from_numpy(p).double(), torch.from_numpy(u).double(), 0.3)
    assert rel(got, tanh_ref.numpy()) > 1e-2
    node.close()


# ---- Tsit5 / DP5 along a given sequence, forward and reverse -------------------------------------------------------------------------

REPLAY = [("relu", "Tsit5", 1, "small"), ("sigmoid", "Tsit5", 1, "small"), ("softplus", "Tsit5", 1, "small"), ("elu", "Tsit5", 1, "small"),
          ("softplus", "AutoTsit5", 2, "small"), ("elu", "DP5", 1, "small"), ("relu", "Tsit5", 1, "wide"), ("softplus", "Tsit5", 1, "wide")]
# (dims, time_dep, seed): "wide" has 33..64 features, the 16-k-step kernels
REPLAY_SHAPES = {"small": ([3, 9, 3], True, 4), "wide": ([36, 40, 36], False, REPLAY_WIDE_SEED)}


REPLAY_CASES = [(a, s, r, sh, ct) for a, s, r, sh in REPLAY for ct in (64, 0) if not (s == "DP5" and ct == 64)]


@pytest.mark.parametrize("act,solver,reg,shape,col_tile", REPLAY_CASES,
                         ids=[f"{a}-{s}-{sh}-{'one-wave' if ct == 64 else 'four-wave'}" for a, s, _, sh, ct in REPLAY_CASES])
def test_replay_forward_and_reverse(act, solver, reg, shape, col_tile):
    """rnde_node_forward_replay + rnde_node_backward along a fixed all-accepted sequence (step sizes are constants of the program: a rejected attempt
    would carry the controller's dependence on its error estimate into the reverse pass, which the restatement does not model) against the fp64
    restatement with autograd: u <= 2e-4, x-bar and p-bar <= 1e-3 relative.  reg 1: RNDE_REG_ERR; AutoTsit5 with reg 2: the stiffness
    callback.  (DP5 runs on the four-wave kernels only: rnde_node_create refuses it with col_tile 64.)"""
    from oracle.oracle import Oracle, make_arch
    from tests.util import Node
    dims, td, seed = REPLAY_SHAPES[shape]
    acts = [act, act]
    rng = np.random.default_rng(seed)
    B = 6
    p, x = params(dims, td, rng, bias=0.3), rng.uniform(-1.0, 1.0, (B, dims[0])).astype(np.float32)
    dtp, acc = [0.25] * 4, [1] * 4
    tab = Oracle(make_arch(dims, ["tanh", "tanh"], td), np.float64, solver="DP5" if solver == "DP5" else "Tsit5").tableau()
    node = Node(_cfg(dims, acts, B, time_dep=td, regularize=reg, track_ctrl=0, track_initdt=0, max_attempts=16, col_tile=col_tile, solver=solver))
    got = node.forward_replay(x, p, dtp, acc, keep_tape=True)
    assert got["nattempts"] == len(dtp)
    att = [(float(s[0]), float(s[1]), int(s[3])) for s in got["steps"]]
    assert [a[2] for a in att] == acc
    P, X = torch.from_numpy(p).double().requires_grad_(True), torch.from_numpy(x).double().requires_grad_(True)
    pa = []
    u = rk_replay64(lambda v, t: chain64(dims, acts, td, 0, P, v, t, pa), X, att, tab)
    _kink_free(act, pa)
    assert rel(got["u"], u.detach().numpy()) <= 2e-4
    ubar = rng.standard_normal(x.shape).astype(np.float32)
    xb, pb, _ = node.backward(ubar)
    gx, gp = torch.autograd.grad(u, (X, P), torch.from_numpy(ubar).double())
    assert rel(xb, gx.numpy()) <= 1e-3 and rel(pb, gp.numpy()) <= 1e-3
    node.close()


@pytest.mark.parametrize("act", ["sigmoid", "softplus"])
@pytest.mark.parametrize("col_tile", [64, 0], ids=["one-wave", "four-wave"])
def test_adaptive_solve_matches_fp64_replay_of_its_steps(act, col_tile):
    """A full adaptive solve (controller, initial step, EEst*dt callback) against the fp64 replay of the device's own attempts: u <= 2e-4, and the
    controller did its work (rejections allowed, every attempt logged).  (Smooth activations: the step sequence is not known in advance, so no
    seed can be vetted for the kink.)"""
    from oracle.oracle import Oracle, make_arch
    from tests.util import Node
    dims, acts, td = [4, 16, 4], [act, "identity"], True
    rng = np.random.default_rng(5)
    B = 24
    p, x = params(dims, td, rng, scale=2.0, bias=0.3), rng.uniform(-1.0, 1.0, (B, 4)).astype(np.float32)
    node = Node(_cfg(dims, acts, B, time_dep=td, reltol=1e-5, abstol=1e-5, regularize=1, max_attempts=128, col_tile=col_tile))
    got = node.forward(x, p)
    assert got["nattempts"] >= 3 and len(got["saveval"]) >= 2
    att = [(float(s[0]), float(s[1]), int(s[3])) for s in got["steps"]]
    assert abs(sum(a[1] for a in att if a[2]) - 1.0) <= 1e-5
    tab = Oracle(make_arch(dims, ["tanh", "identity"], td), np.float64).tableau()
    u = rk_replay64(lambda v, t: chain64(dims, acts, td, 0, torch.from_numpy(p).double(), v, t), torch.from_numpy(x).double(), att, tab)
    assert rel(got["u"], u.numpy()) <= 2e-4
    assert np.isfinite(got["saveval"]).all() and (got["saveval"] >= 0).all()
    node.close()


# ---- the SDE layer at the MNIST-NSDE shape ---------------------------------------------------------------------------------------------

NSDE = ([32, 64, 32], ["softplus", "identity"], [32, 32], ["sigmoid"])


def _nsde_setup(seed, B, n_pool):
    rng = np.random.default_rng(seed)
    dd, da, gd, ga = NSDE
    p = np.concatenate([params(dd, False, rng, 1.0, 0.3), params(gd, False, rng, 0.5, 0.3)]).astype(np.float32)
    x = rng.standard_normal((B, 32)).astype(np.float32)
    noise = rng.standard_normal((n_pool, 2, B, 32)).astype(np.float32)
    return p, x, noise


def _nets64(P):
    dd, da, gd, ga = NSDE
    nd = 32 * 64 + 64 + 64 * 32 + 32
    return (lambda v: chain64(dd, da, False, 0, P[:nd], v, 0.0)), (lambda v: chain64(gd, ga, False, 0, P[nd:], v, 0.0))


def _nsde_node(B, **kw):
    from tests.util import NsdeNode, make_nsde_cfg
    dd, da, gd, ga = NSDE
    cfg = make_nsde_cfg(dd, ["identity"] * 2, gd, ["identity"], B, **kw)
    for i, a in enumerate(da):
        cfg.drift_act[i] = CODES[a]
    cfg.diff_act[0] = CODES[ga[0]]
    return NsdeNode(cfg)


def test_sde_attempt_matches_fp64():
    from oracle.oracle_sde import sri_tableau
    B, dt = 20, 0.07
    p, x, noise = _nsde_setup(6, B, 1)
    dW, dZ = math.sqrt(dt) * noise[0, 0], math.sqrt(dt) * noise[0, 1]
    node = _nsde_node(B)
    kg, un_d, e = node.attempt(x, p, dt, dW, dZ)
    P = torch.from_numpy(p).double()
    k, g, un = sri_attempt64(sri_tableau("SOSRI"), *_nets64(P), torch.from_numpy(x).double(), dt, *(torch.from_numpy(a).double() for a in (dW, dZ)))
    assert rel(kg, torch.stack(k + g).numpy()) <= 2e-5 and rel(un_d, un.numpy()) <= 2e-5 and math.isfinite(e)
    # and not the tanh the codes once ran
    dd, _, gd, _ = NSDE
    nd = 32 * 64 + 64 + 64 * 32 + 32
    g_tanh = chain64(gd, ["tanh"], False, 0, P[nd:], torch.from_numpy(x).double(), 0.0)
    assert rel(kg[4], g_tanh.numpy()) > 1e-2
    node.close()


def test_sde_replay_forward_and_reverse():
    from oracle.oracle_sde import sri_tableau
    B = 16
    dts = [0.125] * 8
    p, x, noise = _nsde_setup(7, B, 12)
    tab = sri_tableau("SOSRI")

    def solve(Pt, Xt):
        drift, diff = _nets64(Pt)
        u = Xt
        for n, dt in enumerate(dts):
            W, Z = (math.sqrt(dt) * torch.from_numpy(noise[n, j].astype(np.float64)) for j in (0, 1))
            u = sri_attempt64(tab, drift, diff, u, dt, W, Z)[2]
        return u

    node = _nsde_node(B, reltol=0.3, abstol=0.3, regularize=0, max_attempts=16)
    got = node.forward(x, p, noise, keep_tape=True, replay=np.stack([np.array(dts), np.ones(len(dts))], 1))
    assert got["nattempts"] == len(dts)
    P, X = torch.from_numpy(p).double().requires_grad_(True), torch.from_numpy(x).double().requires_grad_(True)
    u = solve(P, X)
    assert rel(got["u"], u.detach().numpy()) <= 2e-4
    ubar = (np.random.default_rng(8).standard_normal(x.shape) / B).astype(np.float32)
    xb, pb = node.backward(ubar)
    gx, gp = torch.autograd.grad(u, (X, P), torch.from_numpy(ubar).double())
    assert rel(xb, gx.numpy()) <= 1e-3 and rel(pb, gp.numpy()) <= 1e-3
    node.close()


# ---- the Python layers -----------------------------------------------------------------------------------------------------------

def test_ode_layer_call_with_relu():
    """TrackedNeuralODE(Chain(Dense(2, 16, "relu"), Dense(16, 2))): called and differentiated through torch; the solve matches the fp64 replay of
    its attempts (the value is continuous across the kink, so no seed vetting is needed for it), the gradients are the C-ABI reverse pass's."""
    import regneuralde_jl_amd as rn
    from oracle.oracle import Oracle, make_arch
    from tests.util import Node
    g = torch.Generator().manual_seed(21)
    B = 10
    chain = rn.Chain(rn.Dense(2, 16, "relu", g), rn.Dense(16, 2, "identity", g))
    for l in chain.layers:
        l.b = 0.3 * torch.randn(l.n_out, generator=g)
    node = rn.TrackedNeuralODE(chain, [0.0, 1.0], False, False, "Tsit5", reltol=1e-5, abstol=1e-5, max_batch=B)
    x = torch.randn(B, 2, generator=g)
    xd, pd = x.cuda().requires_grad_(True), node.p.cuda().requires_grad_(True)
    u, nfe, _ = node(xd, pd)
    w = torch.randn(B, 2, generator=g)
    (u * w.cuda()).sum().backward()
    assert nfe > 0 and torch.isfinite(xd.grad).all() and torch.isfinite(pd.grad).all()
    ref = Node(node._config(0, None))
    r = ref.forward(x.numpy(), node.p.numpy(), keep_tape=True)
    assert np.array_equal(r["u"], u.detach().cpu().numpy()) and r["nfe"] == nfe
    xb, pb, _ = ref.backward(w.numpy())
    assert rel(xd.grad.cpu().numpy(), xb) <= 1e-6 and rel(pd.grad.cpu().numpy(), pb) <= 1e-6
    att = [(float(s[0]), float(s[1]), int(s[3])) for s in r["steps"]]
    tab = Oracle(make_arch([2, 16, 2], ["tanh", "identity"], False), np.float64).tableau()
    u64 = rk_replay64(lambda v, t: chain64([2, 16, 2], ["relu", "identity"], False, 0, node.p.double(), v, t), x.double(), att, tab)
    assert rel(u.detach().cpu().numpy(), u64.numpy()) <= 2e-4
    ref.close()


def test_sde_layer_call_with_softplus():
    """TrackedNeuralDSDE with a softplus drift layer: called and differentiated through torch; the same numbers as the C-ABI handle on the same
    noise, and a solve of the right kind (finite, the drift evaluation count the handle reports)."""
    import regneuralde_jl_amd as rn
    from tests.util import NsdeNode
    g = torch.Generator().manual_seed(22)
    B = 12
    sde = rn.TrackedNeuralDSDE(rn.Chain(rn.Dense(3, 8, "softplus", g), rn.Dense(8, 3, "identity", g)), rn.Dense(3, 3, "sigmoid", g), [0.0, 1.0],
                               False, "SOSRI", reltol=0.14, abstol=0.14, max_batch=B)
    x = torch.randn(B, 3, generator=g)
    noise = torch.randn(200, 2, B, 3, generator=g)
    xd, pd = x.cuda().requires_grad_(True), sde.p.cuda().requires_grad_(True)
    u, nfe1, nfe2, _ = sde(xd, pd, noise=noise.cuda())
    w = torch.randn(B, 3, generator=g)
    (u * w.cuda()).sum().backward()
    assert nfe1 > 0 and torch.isfinite(u).all() and torch.isfinite(pd.grad).all()
    ref = NsdeNode(sde._config(0))
    r = ref.forward(x.numpy(), sde.p.numpy(), noise.numpy(), keep_tape=True)
    assert np.array_equal(r["u"], u.detach().cpu().numpy()) and r["nfe1"] == nfe1
    xb, pb = ref.backward(w.numpy())
    assert rel(xd.grad.cpu().numpy(), xb) <= 1e-6 and rel(pd.grad.cpu().numpy(), pb) <= 1e-6
    ref.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_unknown_code_is_refused_by_both_create_calls():
    from regneuralde_jl_amd import _lib
    from tests.util import make_nsde_cfg
    L = _lib.lib()
    h = C.c_void_p()
    cfg = _cfg([3, 5, 3], ["tanh", "identity"], 4, time_dep=False)
    cfg.act[1] = 6
    assert L.rnde_node_create(C.byref(cfg), C.byref(h)) == _lib.BAD_ARG
    msg = L.rnde_last_error(None).decode()
    assert "act[1] = 6" in msg and "relu" in msg and "elu" in msg
    scfg = make_nsde_cfg([3, 5, 3], ["tanh", "identity"], [3, 3], ["identity"], 4)
    scfg.diff_act[0] = 6
    assert L.rnde_nsde_create(C.byref(scfg), C.byref(h)) == _lib.BAD_ARG
    assert "diff_act[0] = 6" in L.rnde_nsde_last_error(None).decode()
    scfg.diff_act[0], scfg.drift_act[0] = 0, -1
    assert L.rnde_nsde_create(C.byref(scfg), C.byref(h)) == _lib.BAD_ARG
    assert "drift_act[0] = -1" in L.rnde_nsde_last_error(None).decode()


@pytest.mark.parametrize("act", NEW)
def test_stage_engine_form_refuses_other_second_layer_activations(act):
    """The two-layer TDChain form with act[0] = tanh (784 / 100: only the stage engine serves those widths) takes identity or tanh in act[1]; the
    rest is refused by name, not run as tanh."""
    from regneuralde_jl_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    cfg = _cfg([784, 100, 784], ["tanh", act], 16, time_dep=True)
    assert L.rnde_node_create(C.byref(cfg), C.byref(h)) == _lib.BAD_ARG
    msg = L.rnde_last_error(None).decode()
    assert f"act[1] = {act}" in msg and "stage engine" in msg
