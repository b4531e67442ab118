"""The tiled engine of TrackedNeuralODE (rnde_node_create_tiled, engine="tiled"): Dense chains wider than 64 on the tile layout, against the fp64
restatements of tests/act_ref.py and the CPU oracle (identity / tanh; track_ctrl = track_initdt = 0, set_replay).

Shapes: the smallest at which these kernels can go wrong -- padding in every dimension and a partial last tile (pad_td), a wave whose output-tile
loop runs twice and widths above 64 (two_pass), more than 64 state rows (wide_state), 8 layers with every activation (deep), the largest LDS
footprint of the README's example (limit).

Bounds.  feval: 2e-6 where every width is <= 64 (test_gpu_activations.py::test_feval_matches_fp64); for wider shapes four times the error of a
float32 CPU evaluation of the same chain against fp64 on the same inputs (another summation order, the 1.65-ulp tanh), never below 2e-6; the test
prints both figures.  Measured on an MI355X (the formed bound came out at its floor of 2e-6 on all three wide shapes): pad_td 7.1e-8 (B = 5) and
1.0e-7 (B = 37), deep 1.3e-7, two_pass 2.3e-7, wide_state 3.1e-7, limit 2.3e-7.
Replay (a rejection in the sequence: the attempt after it starts from the kept k1): u <= 2e-4; measured 1.6e-7 .. 4.1e-7.
Adaptive solve at reltol = abstol = 1e-5, against the fp64 oracle solving on its own: the same accept / reject sequence, step sizes <= 2e-2
(measured 1.9e-4, 8.5e-3, 2.7e-3), nfe, the accepted steps summing to 1, u <= 2e-4 of the fp64 replay of the device's own attempts (3e-7);
asserted condition: every EEst of the fp64 oracle lies outside [0.9, 1.1].  The seeds are vetted on the CPU: the fp32 and the fp64 oracle take
the same sequence.  pad_td_rej contains a natural rejection; pad_td and wide_state accept every attempt (test 2 carries a rejection for all three
shapes).
Saved values <= 1e-3 of the fp64 oracle's: the oracle is run along the device's own attempts for this comparison, as for u (measured 2.3e-4,
2.6e-4, 1.5e-4).  Against the oracle solving on its own the saved values EEst dt carry the sixth power of the step-size differences above and
come out at 5.3e-4, 1.8e-2 and 4.5e-3; the CPU's own fp32 oracle is 2.3e-4, 1.4e-3 and 1.7e-3 from its fp64 one there, so that figure measures
fp32 against fp64 step-size control and not this engine.  Both figures are printed.
Reverse: x-bar, p-bar <= 1e-3 along the device's own step sequence (measured: 1.7e-4 / 1.1e-4 pad_td, 8.2e-5 / 4.5e-5 wide_state, 7.5e-5 / 4.6e-5
limit with the saved values' cotangent; 1.9e-7 / 4.6e-7 two_pass, 1.4e-7 / 3.1e-7 deep without).  `deep` (relu and elu: a kink at 0) runs its
reverse along a given two-step sequence, so that its seed could be vetted on the CPU for the 1e-4 kink margin; the margin is asserted.
Tiled against chain engine on the latent widths: the same decisions from the same first step, u 3.9e-7; the step sizes of that 7-attempt solve
(EEst of order 1e-2, still in the controller's growth phase) differ by up to 4.3e-2 between the two summation orders, printed and not asserted.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.act_ref import CODES, chain64, params, rel, rk_replay64

pytestmark = pytest.mark.gpu

KINK = 1e-4
# name: (dims, acts, time_dep, B, seed)
SHAPES = {
    "pad_td": ([3, 7, 3], ["tanh", "identity"], True, 37, 3),
    "two_pass": ([6, 80, 72, 6], ["softplus", "tanh", "identity"], False, 20, 5),
    "wide_state": ([70, 96, 70], ["tanh", "tanh"], True, 17, 7),
    "deep": ([5, 20, 9, 20, 9, 20, 9, 20, 5], ["relu", "sigmoid", "elu", "softplus", "tanh", "sigmoid", "softplus", "identity"], False, 8, 1),
    "limit": ([2, 128, 128, 2], ["tanh", "tanh", "identity"], True, 16, 9),
}
LIMIT_SHAPES = {"served_3": [2, 128, 128, 2], "served_2": [64, 192, 64]}
# The adaptive cases: (shape, seed, per-layer factors on the parameters).  A fast right-hand side of modest size (first layer x 60 or more, last
# layer x 0.3 or less) keeps the solve error-limited over most of [0, 1] (15 - 30 attempts, EEst of a few tenths): the fp32 rounding of
# EEst = ||dt sum_j bt_j k_j / sk|| is about 6e-3 dt |k| in absolute terms, so only small dt |k| against an EEst of that size gives a controller
# path, and saved values, that two fp32 implementations share to a few 1e-4.  Vetted on the CPU (fp32 against fp64 oracle): the same sequence.
ADAPTIVE = {
    "pad_td": ("pad_td", 3, (60.0, 0.3)),
    "pad_td_rej": ("pad_td", 2, (240.0, 0.1)),      # a natural rejection (attempt 22 of 28 on the CPU oracles, EEst 1.68)
    "wide_state": ("wide_state", 3, (120.0, 0.1)),
    "limit": ("limit", 1, (60.0, 1.0, 0.3)),
}
REPLAY_DTP, REPLAY_ACC = [0.25, 0.5, 0.25, 0.25, 0.25], [1, 0, 1, 1, 1]


def case(name, B=None):
    dims, acts, td, B0, seed = SHAPES[name]
    B = B0 if B is None else B
    rng = np.random.default_rng(seed)
    p = params(dims, td, rng, bias=0.3)
    x = rng.uniform(-1.0, 1.0, (B, dims[0])).astype(np.float32)
    return dims, acts, td, p, x


def adaptive_case(key):
    name, seed, factors = ADAPTIVE[key]
    dims, acts, td, B, _ = SHAPES[name]
    rng = np.random.default_rng(seed)
    p = params(dims, td, rng, bias=0.3)
    o = 0
    for l, f in enumerate(factors):
        n = (dims[l] + (1 if td else 0)) * dims[l + 1] + dims[l + 1]
        p[o:o + n] *= f
        o += n
    x = rng.uniform(-1.0, 1.0, (B, dims[0])).astype(np.float32)
    return dims, acts, td, p, x


def make_cfg(dims, acts, td, B, **kw):
    from tests.util import make_cfg as mk
    kw.setdefault("track_ctrl", 0)
    kw.setdefault("track_initdt", 0)
    kw.setdefault("regularize", 0)
    cfg = mk(dims, ["identity"] * len(acts), B, time_dep=int(td), **kw)
    for i, a in enumerate(acts):
        cfg.act[i] = CODES[a]
    return cfg


def tiled(cfg):
    from regneuralde_jl_amd import _lib
    from tests.util import Node

    class TiledNode(Node):
        def __init__(self, cfg):
            self.L = _lib.lib()
            self.h = C.c_void_p()
            _lib.check(None, self.L.rnde_node_create_tiled(C.byref(cfg), C.byref(self.h)))
            self.cfg, self.D, self.stream, self._tstream = cfg, cfg.dims[0], None, None

    return TiledNode(cfg)


def attempts(steps):
    return [(float(s[0]), float(s[1]), int(s[3])) for s in steps]


def tableau():
    from oracle.oracle import Oracle, make_arch
    return Oracle(make_arch([3, 7, 3], ["tanh", "tanh"], True), np.float64).tableau()


def kink_margin(acts, preacts):
    n = len(acts)
    return min((float(z.abs().min()) for i, z in enumerate(preacts) if acts[i % n] in ("relu", "elu")), default=1.0)


# ---- 1. one evaluation ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B", [("pad_td", 5), ("pad_td", 37), ("two_pass", None), ("wide_state", None), ("deep", None), ("limit", None)])
def test_feval_matches_fp64(name, B):
    dims, acts, td, p, x = case(name, B)
    u = (1.3 * x).astype(np.float32)
    P64, U64 = torch.from_numpy(p).double(), torch.from_numpy(u).double()
    pa = []
    ref = chain64(dims, acts, td, 0, P64, U64, 0.3, pa).numpy()
    assert kink_margin(acts, pa) > KINK
    bound = 2e-6
    if max(dims) > 64:
        e32 = rel(chain64(dims, acts, td, 0, torch.from_numpy(p), torch.from_numpy(u), 0.3).numpy(), ref)
        bound = max(2e-6, 4 * e32)
    node = tiled(make_cfg(dims, acts, td, u.shape[0]))
    got = node.feval(u, p, 0.3)
    node.close()
    print(f"feval {name} B={u.shape[0]}: rel {rel(got, ref):.3e} bound {bound:.3e}")
    assert rel(got, ref) <= bound, (rel(got, ref), bound)


# ---- 2. a given sequence with a rejection in it ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pad_td", "two_pass", "wide_state"])
def test_replay_matches_fp64(name):
    dims, acts, td, p, x = case(name)
    node = tiled(make_cfg(dims, acts, td, x.shape[0], max_attempts=16))
    got = node.forward_replay(x, p, REPLAY_DTP, REPLAY_ACC)
    node.close()
    assert got["nattempts"] == len(REPLAY_DTP) and got["nfe"] == 3 + 6 * len(REPLAY_DTP)
    att = attempts(got["steps"])
    assert [a[2] for a in att] == REPLAY_ACC and [a[1] for a in att] == REPLAY_DTP
    P = torch.from_numpy(p).double()
    u = rk_replay64(lambda v, t: chain64(dims, acts, td, 0, P, v, t), torch.from_numpy(x).double(), att, tableau())
    print(f"replay {name}: rel {rel(got['u'], u.numpy()):.3e}")
    assert rel(got["u"], u.numpy()) <= 2e-4


# ---- 3. the adaptive solve ---------------------------------------------------------------------------------------------------------------

def _oracle(dims, acts, td, dtype, **kw):
    from oracle.oracle import Oracle, make_arch
    return Oracle(make_arch(dims, acts, td), dtype, 1e-5, 1e-5, reg_kind=1, track_ctrl=0, track_initdt=0, max_attempts=128, **kw)


def _adaptive(name):
    dims, acts, td, p, x = adaptive_case(name)
    node = tiled(make_cfg(dims, acts, td, x.shape[0], reltol=1e-5, abstol=1e-5, regularize=1, max_attempts=128))
    got = node.forward(x, p, keep_tape=True)
    return dims, acts, td, p, x, node, got


@pytest.mark.parametrize("name", ["pad_td", "pad_td_rej", "wide_state"])
def test_adaptive_solve_matches_oracle(name):
    dims, acts, td, p, x, node, got = _adaptive(name)
    node.close()
    o64 = _oracle(dims, acts, td, np.float64)
    r = o64.forward(x.astype(np.float64), p.astype(np.float64))
    assert r["rc"] == 0
    assert all(not 0.9 <= float(s[2]) <= 1.1 for s in r["steps"]), "an EEst of the fp64 oracle within rounding of the accept threshold: pick another seed"
    att = attempts(got["steps"])
    print(f"adaptive {name}: {len(att)} attempts, {sum(1 - a[2] for a in att)} rejected")
    assert [a[2] for a in att] == [int(s[3]) for s in r["steps"]]
    assert rel(got["steps"][:, 1], r["steps"][:, 1]) <= 2e-2
    assert got["nfe"] == 3 + 6 * len(att)
    assert abs(sum(a[1] for a in att if a[2]) - 1.0) <= 1e-5
    P = torch.from_numpy(p).double()
    u = rk_replay64(lambda v, t: chain64(dims, acts, td, 0, P, v, t), torch.from_numpy(x).double(), att, tableau())
    assert rel(got["u"], u.numpy()) <= 2e-4
    assert len(got["saveval"]) == len(r["saveval"]) == 1 + sum(a[2] for a in att) and got["saveval"][0] == 0.0
    # the saved values against the fp64 oracle along the device's own attempts, as u above (the free-running figure is printed: see the docstring)
    o64.set_replay(got["steps"][:, 1].astype(np.float64), got["steps"][:, 3].astype(np.int32))
    rr = o64.forward(x.astype(np.float64), p.astype(np.float64))
    print(f"adaptive {name}: step sizes {rel(got['steps'][:, 1], r['steps'][:, 1]):.3e}, u {rel(got['u'], u.numpy()):.3e}, saved values "
          f"{rel(got['saveval'], rr['saveval']):.3e} (own attempts) {rel(got['saveval'], r['saveval']):.3e} (free-running oracle)")
    assert rel(got["saveval"], rr["saveval"]) <= 1e-3
    if name == "pad_td_rej":
        assert 0 in [a[2] for a in att]      # the natural rejection this seed was chosen for


def test_cb_save_start_off_drops_the_leading_zero():
    dims, acts, td, p, x = adaptive_case("pad_td")
    a = tiled(make_cfg(dims, acts, td, 37, reltol=1e-5, abstol=1e-5, regularize=1, cb_save_start=0))
    b = tiled(make_cfg(dims, acts, td, 37, reltol=1e-5, abstol=1e-5, regularize=1, cb_save_start=1))
    ga, gb = a.forward(x, p), b.forward(x, p)
    a.close(), b.close()
    assert np.array_equal(ga["saveval"], gb["saveval"][1:]) and np.array_equal(ga["u"], gb["u"])


# ---- 4. determinism and layout -------------------------------------------------------------------------------------------------------------

def test_bit_identical_run_to_run_and_under_a_larger_max_batch():
    dims, acts, td, p, x = adaptive_case("pad_td")
    runs = []
    for mb in (37, 37, 64):
        node = tiled(make_cfg(dims, acts, td, mb, reltol=1e-5, abstol=1e-5, regularize=1))
        g = node.forward(x, p, keep_tape=True)
        xb, pb, _ = node.backward(np.ones_like(x), np.ones(len(g["saveval"])))
        g2 = node.forward(x, p)
        assert all(np.array_equal(g[k], g2[k]) for k in ("u", "saveval", "steps"))
        runs.append((g, xb, pb))
        node.close()
    for g, xb, pb in runs[1:]:
        assert all(np.array_equal(g[k], runs[0][0][k]) for k in ("u", "saveval", "steps"))
        assert np.array_equal(xb, runs[0][1]) and np.array_equal(pb, runs[0][2])


# ---- 5. the reverse sweep ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pad_td", "wide_state", "limit"])
def test_reverse_matches_oracle(name):
    dims, acts, td, p, x, node, got = _adaptive(name)
    rng = np.random.default_rng(100)
    ubar = rng.standard_normal(x.shape).astype(np.float32)
    # of order 1: the saved values' share of the gradient is then a few per cent or more (asserted below, ten times the bound), and the fp32
    # rounding of that share (some 5e-3 of it: EEst is a small difference of large terms) stays well inside the bound
    svbar = rng.uniform(0.5, 1.5, len(got["saveval"])).astype(np.float32)
    xb, pb, tsb = node.backward(ubar, svbar)
    node.close()
    o64 = _oracle(dims, acts, td, np.float64)
    o64.set_replay(got["steps"][:, 1].astype(np.float64), got["steps"][:, 3].astype(np.int32))
    r = o64.forward(x.astype(np.float64), p.astype(np.float64))
    assert r["rc"] == 0 and r["nattempts"] == got["nattempts"] and len(r["saveval"]) == len(got["saveval"])
    gx, gp, _ = o64.backward(ubar.astype(np.float64), svbar.astype(np.float64))
    print(f"reverse {name}: x-bar {rel(xb, gx):.3e} p-bar {rel(pb, gp):.3e} ({got['nattempts']} attempts)")
    assert rel(xb, gx) <= 1e-3 and rel(pb, gp) <= 1e-3
    assert tuple(tsb) == (0.0, 0.0)
    # and the saved values' cotangent is in it: without it the gradient is another one
    o64.forward(x.astype(np.float64), p.astype(np.float64))
    _, gp0, _ = o64.backward(ubar.astype(np.float64), None)
    assert rel(gp0, gp) > 1e-2


@pytest.mark.parametrize("name", ["two_pass", "deep"])
def test_reverse_matches_autograd(name):
    dims, acts, td, p, x = case(name)
    node = tiled(make_cfg(dims, acts, td, x.shape[0], reltol=1e-4, abstol=1e-4, regularize=0, max_attempts=128))
    if name == "deep":      # a given sequence: the seed is vetted for the kink margin along it
        got = node.forward_replay(x, p, [0.5, 0.5], [1, 1], keep_tape=True)
    else:
        got = node.forward(x, p, keep_tape=True)
    ubar = np.random.default_rng(101).standard_normal(x.shape).astype(np.float32)
    xb, pb, tsb = node.backward(ubar)
    node.close()
    att = attempts(got["steps"])
    P, X = torch.from_numpy(p).double().requires_grad_(True), torch.from_numpy(x).double().requires_grad_(True)
    pa = []
    u = rk_replay64(lambda v, t: chain64(dims, acts, td, 0, P, v, t, pa), X, att, tableau())
    assert kink_margin(acts, pa) > KINK, f"a relu / elu pre-activation within {KINK} of the kink: pick another seed"
    assert rel(got["u"], u.detach().numpy()) <= 2e-4
    gx, gp = torch.autograd.grad(u, (X, P), torch.from_numpy(ubar).double())
    print(f"reverse {name}: x-bar {rel(xb, gx.numpy()):.3e} p-bar {rel(pb, gp.numpy()):.3e} ({len(att)} attempts)")
    assert rel(xb, gx.numpy()) <= 1e-3 and rel(pb, gp.numpy()) <= 1e-3
    assert tuple(tsb) == (0.0, 0.0)


def test_backward_without_a_tape_and_after_release():
    from regneuralde_jl_amd import _lib
    dims, acts, td, p, x = case("pad_td", 5)
    node = tiled(make_cfg(dims, acts, td, 5))
    node.forward(x, p)
    with pytest.raises(_lib.RndeError) as e:
        node.backward(np.ones_like(x))
    assert e.value.status == _lib.NO_TAPE
    node.forward(x, p, keep_tape=True)
    ref = node.backward(np.ones_like(x))
    node.forward(x, p, keep_tape=True)
    node.forward(2 * x, p)                        # an untaped probe in between leaves the tape alone
    again = node.backward(np.ones_like(x))
    assert np.array_equal(ref[0], again[0]) and np.array_equal(ref[1], again[1])
    node.L.rnde_node_release_tape(node.h)
    with pytest.raises(_lib.RndeError):
        node.backward(np.ones_like(x))
    node.close()


# ---- 6. the chain engine on the widths both serve --------------------------------------------------------------------------------------------

def test_latent_widths_agree_with_the_chain_engine():
    from tests.util import Node
    dims, acts = [20, 50, 20, 50, 20, 50, 20, 50, 20], ["tanh"] * 8
    rng = np.random.default_rng(12)
    p, x = params(dims, False, rng, bias=0.3), rng.uniform(-1, 1, (24, 20)).astype(np.float32)
    kw = dict(reltol=1e-5, abstol=1e-5, regularize=1, max_attempts=128)
    a, b = tiled(make_cfg(dims, acts, False, 24, **kw)), Node(make_cfg(dims, acts, False, 24, col_tile=0, **kw))
    ga, gb = a.forward(x, p), b.forward(x, p)
    a.close(), b.close()
    # the same attempts: as many, with the same decisions, from the same first step (the initial-step rule); the later step sizes drift apart by
    # a few per cent, printed below: at 7 attempts over [0, 1] the controller is still growing the step, EEst is of order 1e-2 and its fp32
    # rounding, which differs with the summation order of the two engines, is a sizeable part of it
    assert [s[3] for s in ga["steps"]] == [s[3] for s in gb["steps"]] and ga["nfe"] == gb["nfe"]
    assert abs(ga["steps"][0, 1] / gb["steps"][0, 1] - 1) <= 1e-5
    print(f"latent widths, tiled against chain engine: step sizes {rel(ga['steps'][:, 1], gb['steps'][:, 1]):.3e}, u {rel(ga['u'], gb['u']):.3e}")
    assert rel(ga["u"], gb["u"]) <= 2e-4


# ---- 7. the Python layer -----------------------------------------------------------------------------------------------------------------

def test_python_layer():
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(31)
    B = 16
    model = rn.TDChain(rn.Dense(3, 128, "tanh", g), rn.Dense(129, 128, "tanh", g), rn.Dense(129, 2, "identity", g))
    node = rn.TrackedNeuralODE(model, [0, 1], True, True, engine="tiled", track_ctrl=False, track_initdt=False, reltol=1e-5, abstol=1e-5, max_batch=B)
    x = torch.randn(B, 2, generator=g)
    xd, pd = x.cuda().requires_grad_(True), node.p.cuda().requires_grad_(True)
    with torch.no_grad():
        for _ in range(6):      # more probes than a layer may hold tapes: none of them pins one
            u0, nfe0, _ = node(xd, pd)
    assert not any(h.busy for hs in node._handles.values() for h in hs)
    u, nfe, sv = node(xd, pd)
    assert torch.equal(u, u0) and nfe == nfe0
    (u.sum() + sv.saveval.sum()).backward()
    assert not any(h.busy for hs in node._handles.values() for h in hs)
    ref = tiled(node._config(0, None))
    r = ref.forward(x.numpy(), node.p.numpy(), keep_tape=True)
    assert r["nfe"] == nfe == 3 + 6 * r["nattempts"] and np.array_equal(r["u"], u.detach().cpu().numpy())
    assert np.array_equal(r["saveval"], sv.saveval.detach().cpu().numpy())
    xb, pb, _ = ref.backward(np.ones((B, 2), np.float32), np.ones(len(r["saveval"]), np.float32))
    ref.close()
    assert rel(xd.grad.cpu().numpy(), xb) <= 1e-6 and rel(pd.grad.cpu().numpy(), pb) <= 1e-6
    assert node.last_tspan_bar == (0.0, 0.0)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------

def _refused(cfg, *words):
    from regneuralde_jl_amd import _lib
    L, h = _lib.lib(), C.c_void_p()
    assert L.rnde_node_create_tiled(C.byref(cfg), C.byref(h)) == _lib.BAD_ARG
    msg = L.rnde_last_error(None).decode()
    assert all(w in msg for w in words), msg


def test_create_refusals():
    d, a = [3, 7, 3], ["tanh", "identity"]
    _refused(make_cfg(d, a, True, 8, solver="DP5"), "Tsit5")
    _refused(make_cfg(d, a, True, 8, solver="DOP853"), "Tsit5")
    for reg in (2, 3, 4):
        _refused(make_cfg(d, a, True, 8, regularize=reg), "stiffness", "RNDE_REG_ERR")
    _refused(make_cfg(d, a, True, 8, pre_act=1), "pre_act")
    _refused(make_cfg(d, a, True, 8, col_tile=65), "col_tile")
    _refused(make_cfg(d, a, True, 8, track_ctrl=1), "track_ctrl", "track_initdt")
    _refused(make_cfg(d, a, True, 8, track_initdt=1), "track_ctrl", "track_initdt")
    _refused(make_cfg(d, a, True, 4097), "4096")
    _refused(make_cfg(d, a, True, 8, max_attempts=8001), "8000")
    _refused(make_cfg([64, 256, 64], a, False, 8), "192768 bytes", "163840")
    _refused(make_cfg([3, 7, 4], a, True, 8), "dims[0]")


def test_lds_bytes_match_the_python_mirror():
    from regneuralde_jl_amd import _lib
    from regneuralde_jl_amd.node import tiled_lds_bytes
    L = _lib.lib()
    for dims in [s[0] for s in SHAPES.values()] + list(LIMIT_SHAPES.values()) + [[64, 256, 64]]:
        cfg = make_cfg(dims, ["tanh"] * (len(dims) - 1), False, 8)
        assert L.rnde_node_tiled_lds_bytes(C.byref(cfg)) == tiled_lds_bytes(dims), dims
    assert tiled_lds_bytes([2, 128, 128, 2]) == 120512 and tiled_lds_bytes([64, 192, 64]) == 146944


def test_limit_shapes_are_created():
    for dims in LIMIT_SHAPES.values():
        tiled(make_cfg(dims, ["tanh"] * (len(dims) - 1), False, 16)).close()


def test_call_refusals():
    from regneuralde_jl_amd import _lib
    dims, acts, td, p, x = case("pad_td", 5)
    node = tiled(make_cfg(dims, acts, td, 5))
    L, h = node.L, node.h
    xd, pd = node.dev(x), node.dev(p)
    out = torch.empty(6, 5, 3, device="cuda")
    nfe, n32, f32 = C.c_int64(0), C.c_int32(0), C.c_float(0)
    sv, th = (C.c_float * 200)(), (C.c_float * 200)()
    sa = (C.c_float * 2)(0.5, 1.0)

    def refused(status, *words):
        assert status == _lib.BAD_ARG
        msg = L.rnde_last_error(h).decode()
        assert "tiled engine" in msg and all(w in msg for w in words), msg

    refused(L.rnde_node_forward_saveat(h, xd.data_ptr(), pd.data_ptr(), 5, 0.0, 1.0, sa, 2, out.data_ptr(), C.byref(nfe), sv, C.byref(n32), 0, None),
            "rnde_node_forward_saveat")
    refused(L.rnde_node_forward_everystep(h, xd.data_ptr(), pd.data_ptr(), 5, 0.0, 1.0, 1, out.data_ptr(), 2, th, C.byref(n32), C.byref(nfe), sv,
                                          C.byref(n32), 0, None), "rnde_node_forward_everystep")
    refused(L.rnde_debug_attempt(h, xd.data_ptr(), xd.data_ptr(), pd.data_ptr(), 5, 0.0, 0.1, out.data_ptr(), out.data_ptr(), C.byref(f32), None),
            "rnde_debug_attempt")
    refused(L.rnde_bench_attempt(h, xd.data_ptr(), pd.data_ptr(), 5, 1, C.byref(f32), None), "rnde_bench_attempt")
    refused(L.rnde_bench_attempt_taped(h, xd.data_ptr(), pd.data_ptr(), 5, 1, C.byref(f32), None), "rnde_bench_attempt")
    refused(L.rnde_bench_attempt_cold_tape(h, xd.data_ptr(), pd.data_ptr(), 5, 1, 2, C.byref(f32), None), "rnde_bench_attempt")
    refused(L.rnde_node_set_coupling(h, C.c_void_p(1), 8), "rnde_node_set_coupling")
    refused(L.rnde_node_set_matrix_mode(h, 1), "rnde_node_set_matrix_mode")
    assert L.rnde_node_set_matrix_mode(h, 0) == _lib.OK and L.rnde_node_matrix_mode(h) == 0
    refused(L.rnde_node_classifier_grad(h, xd.data_ptr(), pd.data_ptr(), pd.data_ptr(), xd.data_ptr(), 5, 10, 0.0, 1.0, 0.0, out.data_ptr(),
                                        out.data_ptr(), None, out.data_ptr(), None, None, None, None), "rnde_node_classifier_grad")
    node.forward(x, p, keep_tape=True)
    refused(L.rnde_node_backward_async(h, xd.data_ptr(), None, out.data_ptr(), out.data_ptr(), None, None), "rnde_node_backward_async")
    node.close()
    # a tape pool holds rnde_node_create instances: a shape only the tiled engine serves is refused there, and the message says where it runs
    L.rnde_tapes_create.argtypes = [C.POINTER(_lib.NodeConfig), C.c_int32, C.POINTER(C.c_void_p)]
    L.rnde_tapes_last_error.restype = C.c_char_p
    L.rnde_tapes_last_error.argtypes = [C.c_void_p]
    t = C.c_void_p()
    wide = make_cfg([2, 128, 128, 2], ["tanh", "tanh", "identity"], True, 8)
    assert L.rnde_tapes_create(C.byref(wide), 2, C.byref(t)) == _lib.BAD_ARG
    assert "rnde_node_create_tiled" in L.rnde_tapes_last_error(None).decode()
    # the create call that refuses the shape points at the tiled engine
    assert L.rnde_node_create(C.byref(wide), C.byref(t)) == _lib.BAD_ARG and "rnde_node_create_tiled" in L.rnde_last_error(None).decode()


def test_timing_reports_the_three_phases():
    dims, acts, td, p, x = case("pad_td", 5)
    node = tiled(make_cfg(dims, acts, td, 5))
    node.forward(x, p, keep_tape=True)
    node.backward(np.ones_like(x))
    a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
    assert node.L.rnde_node_timing(node.h, C.byref(a), C.byref(b), C.byref(c)) == 0
    assert a.value > 0 and b.value > 0 and c.value > 0
    node.close()
