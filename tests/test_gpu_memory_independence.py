"""Every engine's results are independent of what device memory held before: uninitialised (fresh allocations filled with NaN bytes by
RNDE_POISON=1, csrc/rnde_alloc.h) and stale (a handle that has just served a larger, different call).  docs/memory_audit.md is the audit by
reading that goes with this file: who writes each buffer before who reads it.

One pattern per engine.  A case is a call sequence S -- a taped forward and the backward it serves, on a ragged batch -- run three ways:
  (a) on a fresh handle;
  (b) on a fresh handle created and run under RNDE_POISON=1; the library's counters (rnde_debug_poison_allocs / _bytes) must grow by at least
      the handle's allocation count and the bytes of its tape (chain engine: of its reverse slabs, which another translation unit
      allocates in the first backward) while it is created and serves S, so that a translation unit that allocates past the wrapper cannot
      pass here unnoticed;
  (c) on a dirty handle of the same max_batch that first served S's call shapes at the full max_batch with other inputs (x times 3, cycled up
      to max_batch rows) and other parameters (another seed), through the same variant (tracking, saving, kinetic, exact).
Every output of (a), (b) and (c) -- u, logpx, the regulariser rows, saved states, saved values, the step log, x-bar, p-bar, tspan-bar -- must be
finite and bit-equal: no tolerance, every engine is deterministic.  The stage engine runs (a) and (c) only (its (b) is
tests/test_gpu_edge.py::test_results_do_not_depend_on_uninitialised_memory).

Non-finite input: one NaN, and separately one +Inf, in the last valid column of the partial tile gives RNDE_ERR_NONFINITE with the engine's
message on a max_attempts = 16 handle, and the free-running S (taped forward, tracked backward where there is one) run on that handle
afterwards equals the same S on a fresh handle bit for bit, step log included: a NaN left in the controller's state (the proposed dt, the
previous EEst, the initial-step record) would change it.  These handles solve at a looser tolerance (1e-2; 0.3 and smaller parameter factors
on the SDE engine), at which S fits in 16 attempts; each test prints the count and asserts at least three.  The stage and chain engines have this test in
tests/test_gpu_edge.py; the latent caller has no solve and no such status.

The coupled controller (rnde_node_set_coupling): four ranks of an in-process group, each a chain-engine handle on a non-blocking stream and
a host thread of its own, the time-dependent chain3 chain, a cotangent on the saved values.  This is the case that showed that the
poison fill itself must be complete before an allocation is handed out (csrc/rnde_alloc.h).

That the pattern can fail (scratch builds, one zeroing of float payload dropped each).  Tile driver: without the clear of pacc in
rnde_tile_reverse_kernel all 24 cases of the three tile-driver engines are red.  One-workgroup FFJORD engine: without the clear of pacc in
rnde_ffjord_reverse_kernel its four cases are red.  For the other families every clear of device memory on their paths was dropped in turn and
each proved redundant, which is the reason no suitable zeroing exists there:
  chain and stage engines -- the clear of the padded columns of the tape's copy of x (rnde_node_forward): every kernel loads x through a
    col < B, row < D mask into registers and writes each array it later reads (arena records, slab rows, f0 / u1 / f1, the partials) in full,
    padded rows and columns included, from those masked values; cotangents are loaded under the same mask, so padded columns carry exact
    zeros times finite numbers.  Their other clears are control or protocol words (initrec, mailbox, abort and slab tags) and the f0 clear
    of rnde_debug_attempt, an entry no S calls;
  SDE engine -- the clear of the fragment tables at creation (the pack kernel rewrites every fragment that is read) and the clear of the
    evaluation-time table ev_t (its chains have no time row: the weight-gradient kernel is handed the table and never multiplies by it);
  latent caller -- the clear of the three padding columns of the decoder's delta rows (gD: they only form output rows past M = 37, which the
    scatter drops); its other zeroings are of LDS and registers.
So for these families the three legs prove the absence of a dependence that a clear would have to remove; they have not been seen red.

Shapes: the smallest of the engines' own test files at which padding exists in every dimension (rows, columns of the last tile, a tile of
max_batch that is not launched, tape records past n_acc)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NONFINITE = 4
NONFINITE_TOL = 1e-2      # reltol = abstol of the max_attempts = 16 handles: the free-running S of every case fits in 16 attempts there


# ---- the pattern ---------------------------------------------------------------------------------------------------------------------------------

def _counters():
    from regneuralde_jl_amd import _lib
    L = _lib.lib()
    return int(L.rnde_debug_poison_allocs()), int(L.rnde_debug_poison_bytes())


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _same(ref, got, what):
    assert ref.keys() == got.keys(), what
    for k in ref:
        a, b = _np(ref[k]), _np(got[k])
        assert np.isfinite(a).all() and np.isfinite(b).all(), (what, k)
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) if a.shape == b.shape else (a.shape, b.shape))


def _cycle(x, n, factor=3.0):
    """x times factor, its rows cycled up to n rows"""
    x = _np(x)
    return np.ascontiguousarray(np.resize(factor * x, (n,) + x.shape[1:]), dtype=np.float32)


def three_ways(monkeypatch, make, S, dirty, min_allocs, min_bytes, poison=True):
    """make() -> handle (with .close()); S(handle) -> dict of outputs; dirty(handle): the predecessor call of leg (c)."""
    monkeypatch.delenv("RNDE_POISON", raising=False)
    h = make(); a = S(h); h.close()
    assert len(a) > 0
    if poison:
        c0 = _counters()
        monkeypatch.setenv("RNDE_POISON", "1")
        h = make()
        b = S(h)
        c1 = _counters()      # (behind S: several engines allocate their reverse buffers in the first backward, in another translation unit)
        assert c1[0] - c0[0] >= min_allocs and c1[1] - c0[1] >= min_bytes, (c0, c1, min_allocs, min_bytes)
        h.close()
        monkeypatch.delenv("RNDE_POISON")
        c2 = _counters()
        _same(a, b, "poisoned handle")
    h = make()
    if poison:
        assert _counters() == c2      # off again: nothing is filled
    dirty(h)
    c = S(h); h.close()
    _same(a, c, "dirty handle")
    return a


def _expect_nonfinite(call, message):
    from regneuralde_jl_amd._lib import RndeError
    with pytest.raises(RndeError) as e:
        call()
    assert e.value.status == NONFINITE and message in str(e.value), (e.value.status, str(e.value))


def _with(x, value):
    """x with `value` in the last valid column (the partial tile's), last row"""
    y = _np(x).copy()
    y[-1, -1] = value
    return y


# ---- the tiled TrackedNeuralODE engine (rnde_node_create_tiled) -------------------------------------------------------------------------------

NODE_CASES = {"pad_td": ("pad_td_rej", 64), "wide_state": ("wide_state", 32)}      # the vetted ADAPTIVE inputs, max_batch
NODE_LEGS = ["const", "tracked", "saveat-const", "saveat-tracked", "everystep"]


def _node_inputs(case):
    from tests.act_ref import params
    from tests.test_gpu_node_tiled import ADAPTIVE, adaptive_case
    key, mb = NODE_CASES[case]
    dims, acts, td, p, x = adaptive_case(key)
    factors = ADAPTIVE[key][2]
    p2 = params(dims, td, np.random.default_rng(991), bias=0.3)      # the same recipe from another seed
    o = 0
    for l, f in enumerate(factors):
        n = (dims[l] + (1 if td else 0)) * dims[l + 1] + dims[l + 1]
        p2[o:o + n] *= f
        o += n
    return dims, acts, td, p, x, p2, _cycle(x, mb), mb


def _node_make(dims, acts, td, mb, max_attempts=128, tol=None):
    """tol: None = that of tests/test_gpu_node_tiled_saveat.py (1e-5)"""
    from regneuralde_jl_amd import _lib
    from tests.test_gpu_node_tiled import make_cfg, tiled
    from tests.test_gpu_node_tiled_saveat import TOL

    def make():
        node = tiled(make_cfg(dims, acts, td, mb, reltol=tol or TOL, abstol=tol or TOL, regularize=1, max_attempts=max_attempts))
        _lib.check(node.h, node.L.rnde_node_tiled_reserve_saveat(node.h, min(129, max_attempts + 1)))
        return node
    return make


def _node_run(leg, node, x, p):
    from regneuralde_jl_amd import _lib
    from tests.test_gpu_node_tiled_saveat import SAVE_ADAPT, _everystep
    from tests.test_gpu_node_tiled_track import set_tracking
    set_tracking(node, *((1, 1) if "tracked" in leg else (0, 0)))
    rng = np.random.default_rng(5)
    B, D = x.shape
    out = {}
    if leg == "everystep":
        st, n, times, u = _everystep(node, x, p, 1, 129, keep_tape=True)
        _lib.check(node.h, st)
        out.update(u=u, times=times)
        ubar, svbar = rng.uniform(0.5, 1.5, u.shape).astype(np.float32), None
    else:
        f = node.forward_saveat(x, p, SAVE_ADAPT, keep_tape=True) if leg.startswith("saveat") else node.forward(x, p, keep_tape=True)
        out.update(u=f["u"], saveval=f["saveval"], steps=f["steps"], nfe=np.array([f["nfe"]]))
        ubar = rng.uniform(0.5, 1.5, f["u"].shape).astype(np.float32)
        svbar = rng.uniform(0.5, 1.5, len(f["saveval"])).astype(np.float32)
    out["x_bar"], out["p_bar"], out["tspan_bar"] = node.backward(ubar, svbar)
    return out


@pytest.mark.parametrize("leg", NODE_LEGS)
@pytest.mark.parametrize("case", list(NODE_CASES))
def test_tiled_node(case, leg, monkeypatch):
    dims, acts, td, p, x, p2, x2, mb = _node_inputs(case)
    tape_bytes = 129 * dims[0] * mb * 4
    a = three_ways(monkeypatch, _node_make(dims, acts, td, mb), lambda n: _node_run(leg, n, x, p), lambda n: _node_run(leg, n, x2, p2), 13, tape_bytes)
    if case == "pad_td" and leg != "everystep":
        assert 0 in [int(s[3]) for s in a["steps"]]      # the natural rejection this input was vetted for


@pytest.mark.parametrize("case", list(NODE_CASES))
def test_tiled_node_nonfinite_input(case):
    dims, acts, td, p, x, _, _, mb = _node_inputs(case)
    make = _node_make(dims, acts, td, mb, max_attempts=16, tol=NONFINITE_TOL)
    fresh = make(); ref = _node_run("tracked", fresh, x, p); fresh.close()
    print(f"nonfinite {case}: the free-running S takes {len(ref['steps'])} attempts at tol {NONFINITE_TOL}")
    assert len(ref["steps"]) >= 3      # (a controller with a history: dt proposals and the previous EEst matter)
    node = make()
    for bad in (np.nan, np.inf):
        _expect_nonfinite(lambda: node.forward(_with(x, bad), p, keep_tape=True), "non-finite error estimate or dt")
    _same(ref, _node_run("tracked", node, x, p), "after a non-finite input")
    node.close()


# ---- TrackedFFJORD: the tiled engines (ConcatSquash, Dense chains) and the one-workgroup engine ----------------------------------------------

CS2, CS43, CS16 = ("cs", 2, 16), ("cs", 43, 100), ("cs", 16, 64)
TD2 = ("chain", [2, 10, 2], ["tanh", "identity"], True)                       # tests/test_gpu_ffjord_chain.py: its smallest TDChain
CH5 = ("chain", [5, 12, 9, 5], ["tanh", "sigmoid", "identity"], False)        # ... and its smallest Chain
# name: (dynamics, B, max_batch, engine0, (recipe of the inputs))
FF_CASES = {
    "tiled-cs43": (CS43, 17, 48, False, (1.0, 1.0)), "tiled-cs2": (CS2, 37, 64, False, (5.0, 2.0)),
    "chain-td2": (TD2, 37, 64, False, (2.0,)), "chain-ch5": (CH5, 37, 64, False, (1.5,)),
    "onewg-cs2": (CS2, 37, 64, True, (5.0, 2.0)), "onewg-cs16": (CS16, 37, 64, True, (1.5, 1.0)),
}
FF_LEGS = {"tiled-cs43": ["hutch", "kinetic", "exact", "track", "sample"], "tiled-cs2": ["hutch", "kinetic", "exact", "track", "sample"],
           "chain-td2": ["hutch", "kinetic", "exact"], "chain-ch5": ["hutch", "kinetic", "exact"],
           "onewg-cs2": ["hutch", "kinetic"], "onewg-cs16": ["hutch", "kinetic"]}


def _ff_inputs(dyn, recipe, B, seed):
    from tests import ffjord_chain_ref as CR
    from tests import ffjord_ref as R
    if dyn[0] == "chain":
        p, x, e, rng = CR.draw(dyn[1], dyn[3], B, seed, recipe[0])
    else:
        rng = np.random.default_rng(seed)
        p = torch.from_numpy(R.glorot_params(dyn[1], dyn[2], rng, recipe[0]))
        x = torch.from_numpy((rng.standard_normal((B, dyn[1])) * recipe[1]).astype(np.float32))
        e = torch.from_numpy(rng.standard_normal((B, dyn[1])).astype(np.float32))
    g = torch.from_numpy((rng.standard_normal(B) * 0.02 / B).astype(np.float32))
    return p, x, e, g


def _ff_make(dyn, mb, engine0, leg, max_attempts=512, tol=None):
    """tol: None = that of tests/test_gpu_ffjord_track.py (1e-5), whose Handle reads the module's TOL when it is created"""
    from tests import test_gpu_ffjord_track as T

    def make():
        keep = T.TOL
        try:
            T.TOL = tol or keep
            return T.Handle(dyn, mb, regularize=0 if leg == "kinetic" else 1, track=1 if leg == "track" else None, engine0=engine0, max_attempts=max_attempts)
        finally:
            T.TOL = keep
    return make


def _ff_run(leg, hd, p, x, e, g):
    from tests.test_gpu_ffjord_track import DEV
    chk = lambda st: hd.rn._lib.check_ffjord(hd.h, st)
    B, D = x.shape
    if leg in ("hutch", "track", "exact"):
        logpx, sv, log = hd.forward(x, p, None if leg == "exact" else e)
        pb, xb = hd.backward(g, 0.7)
        return dict(logpx=logpx, saveval=sv, steps=np.array(log, dtype=np.float32), p_bar=pb, x_bar=xb)
    xd, pd, ed, gd = (v.to(DEV).contiguous() for v in (x, p, e, g))
    if leg == "sample":
        xs = torch.empty_like(xd)
        chk(hd.L.rnde_ffjord_sample(hd.h, pd.data_ptr(), xd.data_ptr(), B, 0.0, 1.0, 0, xs.data_ptr(), None))
        torch.cuda.synchronize()
        return dict(sample=xs)
    assert leg == "kinetic"
    logpx, reg, nfe = torch.empty(B, device=DEV), torch.empty(2 * B, device=DEV), C.c_int64()
    chk(hd.L.rnde_ffjord_forward_kinetic(hd.h, xd.data_ptr(), pd.data_ptr(), ed.data_ptr(), B, 0.0, 1.0, 0, logpx.data_ptr(), reg.data_ptr(), None,
                                         C.byref(nfe), 1, None))
    rb = torch.full((2 * B,), 0.01 / B, device=DEV)
    pb, xb = torch.empty_like(pd), torch.empty_like(xd)
    chk(hd.L.rnde_ffjord_backward_kinetic(hd.h, gd.data_ptr(), rb.data_ptr(), pb.data_ptr(), xb.data_ptr(), None))
    torch.cuda.synchronize()
    return dict(logpx=logpx, reg=reg, nfe=np.array([nfe.value]), p_bar=pb, x_bar=xb)


def _ff_cases():
    return [(c, leg) for c in FF_CASES for leg in FF_LEGS[c]]


@pytest.mark.parametrize("case,leg", _ff_cases(), ids=[f"{c}-{l}" for c, l in _ff_cases()])
def test_ffjord(case, leg, monkeypatch):
    dyn, B, mb, engine0, recipe = FF_CASES[case]
    p, x, e, g = _ff_inputs(dyn, recipe, B, 31)
    p2, _, e2, g2 = _ff_inputs(dyn, recipe, mb, 977)
    x2 = torch.from_numpy(_cycle(x, mb))
    D = x.shape[1]
    Bp = (mb + 63) // 64 * 64 if engine0 else (mb + 15) // 16 * 16
    three_ways(monkeypatch, _ff_make(dyn, mb, engine0, leg), lambda h: _ff_run(leg, h, p, x, e, g), lambda h: _ff_run(leg, h, p2, x2, e2, g2),
               12, 513 * (D + 1) * Bp * 4)


@pytest.mark.parametrize("case", list(FF_CASES))
def test_ffjord_nonfinite_input(case):
    dyn, B, mb, engine0, recipe = FF_CASES[case]
    p, x, e, g = _ff_inputs(dyn, recipe, B, 31)
    make = _ff_make(dyn, mb, engine0, "hutch", max_attempts=16, tol=NONFINITE_TOL)
    fresh = make(); ref = _ff_run("hutch", fresh, p, x, e, g); fresh.close()
    print(f"nonfinite {case}: the free-running S takes {len(ref['steps'])} attempts at tol {NONFINITE_TOL}")
    assert len(ref["steps"]) >= 3
    hd = make()
    for bad in (np.nan, np.inf):
        _expect_nonfinite(lambda: hd.forward(torch.from_numpy(_with(x, bad)), p, e), "non-finite error estimate or dt")
    _same(ref, _ff_run("hutch", hd, p, x, e, g), "after a non-finite input")
    hd.close()


# ---- the chain engine (rnde_node_create, widths <= 64) -------------------------------------------------------------------------------------------

CHAIN_CASES = {"latent": (37, 48, 1.5, np.linspace(0.0, 1.0, 7).astype(np.float32)), "chain3": (19, 32, 2.0, None)}      # B, max_batch, scale, saveat


def _chain_run(node, x, p, saveat):
    f = node.forward(x, p, keep_tape=True) if saveat is None else node.forward_saveat(x, p, saveat, keep_tape=True)
    rng = np.random.default_rng(5)
    ubar = rng.standard_normal(f["u"].shape).astype(np.float32)
    svbar = rng.uniform(0.5, 1.5, len(f["saveval"])).astype(np.float32)
    xb, pb, tb = node.backward(ubar, svbar)      # (track_ctrl = track_initdt = 1: the tracked reverse)
    return dict(u=f["u"], saveval=f["saveval"], steps=f["steps"], nfe=np.array([f["nfe"]]), x_bar=xb, p_bar=pb, tspan_bar=tb)


@pytest.mark.parametrize("col_tile,solver", [(64, "Tsit5"), (0, "Tsit5"), (0, "DP5")], ids=["one-wave", "four-wave", "four-wave-dp5"])
@pytest.mark.parametrize("kind", list(CHAIN_CASES))
def test_chain_engine(kind, col_tile, solver, monkeypatch):
    from tests.test_gpu_chain import _setup
    from tests.test_gpu_forward import _cfg
    from tests.util import Node
    B, mb, scale, saveat = CHAIN_CASES[kind]
    arch, p, x = _setup(kind, B, 3, scale)
    _, p2, _ = _setup(kind, B, 971, scale)
    x2 = _cycle(x, mb)
    make = lambda: Node(_cfg(arch, mb, reltol=1e-3, abstol=1e-3, col_tile=col_tile, solver=solver, track_ctrl=1, track_initdt=1))
    # (create: rnde.hip; the reverse buffers and the two weight-gradient slabs, 96 P and 16 P floats: rnde_reverse.hip, in the first backward)
    three_ways(monkeypatch, make, lambda n: _chain_run(n, x, p, saveat), lambda n: _chain_run(n, x2, p2, saveat), 20, arch.dims[0] * mb * 4 + 112 * len(p) * 4)


# ---- the stage engine: the dirty handle (its poisoned leg is tests/test_gpu_edge.py's) ---------------------------------------------------------

@pytest.mark.parametrize("saving", [False, True], ids=["end-state", "saveat"])
@pytest.mark.parametrize("x3", ["1", "0"], ids=["bf16x3", "f32"])
@pytest.mark.parametrize("kind,B,mb", [("mnist", 19, 32), ("small", 33, 48)])
def test_stage_engine_dirty_handle(kind, B, mb, x3, saving, monkeypatch):
    from tests.test_gpu_forward import _cfg, _setup
    from tests.util import Node
    monkeypatch.setenv("RNDE_X3", x3)
    arch, p, x = _setup(kind, B, 3, 3.0)
    _, p2, _ = _setup(kind, B, 971, 3.0)
    x2 = np.clip(_cycle(x, mb), 0.0, 3.0)
    saveat = np.array([0.0, 0.25, 1.0], dtype=np.float32) if saving else None
    make = lambda: Node(_cfg(arch, mb, reltol=1e-3, abstol=1e-3, col_tile=16, track_ctrl=1, track_initdt=1))
    three_ways(monkeypatch, make, lambda n: _chain_run(n, x, p, saveat), lambda n: _chain_run(n, x2, p2, saveat), 0, 0, poison=False)


# ---- the SDE engine ------------------------------------------------------------------------------------------------------------------------------

SDE_NONFINITE_TOL = 0.3      # with parameter factors (0.5, 0.1) and the fast controller of tests/test_gpu_nsde.py S fits in 16 attempts


def _sde_run(node, x, p, noise, saveat):
    f = node.forward(x, p, noise, keep_tape=True, saveat=saveat)
    rng = np.random.default_rng(5)
    ubar = (rng.standard_normal(f["u"].shape) / x.shape[0]).astype(np.float32)
    svbar = rng.uniform(0.5, 1.5, len(f["saveval"])).astype(np.float32)
    xb, pb = node.backward(ubar, svbar)
    return dict(u=f["u"], saveval=f["saveval"], steps=f["steps"], nfe=np.array([f["nfe1"], f["nfe2"], f["ndraws"]]), x_bar=xb, p_bar=pb)


@pytest.mark.parametrize("saving", [False, True], ids=["end-state", "saveat"])
@pytest.mark.parametrize("solver,reg", [("SOSRI", 1), ("SOSRI2", 2)], ids=["sosri", "stiff_est"])
def test_sde_engine(solver, reg, saving, monkeypatch):
    """`small` of tests/test_gpu_nsde.py (D = 3: padded rows; the generic one-wave kernels) at B = 7 under max_batch 20, an explicit noise pool.
    The dirty predecessor solves at max_batch over [0, 2] with a tighter controller, so it takes more steps: the tape, the reverse slabs and
    the evaluation-time table have grown for it and are reused, partly, by S."""
    from tests.test_gpu_nsde import AGGR, _cfg, _setup
    from tests.util import NsdeNode
    B, mb = 7, 20
    drift, diff, p, x, noise = _setup("small", B, 13, 400, 2.0, 0.5)
    _, _, p2, _, noise2 = _setup("small", mb, 977, 400, 2.0, 0.5)
    x2 = _cycle(x, mb)
    saveat = np.array([0.13, 0.5, 0.77], dtype=np.float32) if saving else None
    make = lambda: NsdeNode(_cfg(drift, diff, mb, reltol=0.05, abstol=0.05, solver=solver, regularize=reg, max_attempts=399, **AGGR))

    def dirty(node):
        f = node.forward(x2, p2, noise2, t1=2.0, keep_tape=True, saveat=None if saveat is None else 2.0 * saveat)
        node.backward(np.ones_like(f["u"]), np.ones(len(f["saveval"]), np.float32))

    A = ((mb + 15) // 16) * 4 * 64
    three_ways(monkeypatch, make, lambda n: _sde_run(n, x, p, noise, saveat), dirty, 8, (2 * 399 + 8) * 2 * A * 4)


@pytest.mark.parametrize("solver,reg", [("SOSRI", 1), ("SOSRI2", 2)], ids=["sosri", "stiff_est"])
def test_sde_engine_nonfinite_input(solver, reg):
    from tests.test_gpu_nsde import AGGR, _cfg, _setup
    from tests.util import NsdeNode
    B, mb = 7, 20
    drift, diff, p, x, noise = _setup("small", B, 13, 64, 0.5, 0.1)      # (smaller parameter factors: 7 attempts on the CPU oracle, 23 / 34 at 2.0, 0.5)
    make = lambda: NsdeNode(_cfg(drift, diff, mb, reltol=SDE_NONFINITE_TOL, abstol=SDE_NONFINITE_TOL, solver=solver, regularize=reg, max_attempts=16, **AGGR))
    fresh = make(); ref = _sde_run(fresh, x, p, noise, None); fresh.close()
    print(f"nonfinite sde {solver}: the free-running S takes {len(ref['steps'])} attempts at tol {SDE_NONFINITE_TOL}")
    assert len(ref["steps"]) >= 3
    node = make()
    for bad in (np.nan, np.inf):
        _expect_nonfinite(lambda: node.forward(_with(x, bad), p, noise, keep_tape=True), "non-finite error estimate or dt")
    _same(ref, _sde_run(node, x, p, noise, None), "after a non-finite input")
    node.close()


# ---- the latent-ODE caller -----------------------------------------------------------------------------------------------------------------------

class _Latent:
    def __init__(self, max_batch, max_T):
        from regneuralde_jl_amd import _lib
        self.lib, self.L, self.h = _lib, _lib.lib(), C.c_void_p()
        cfg = _lib.LatentConfig(max_batch=max_batch, max_T=max_T, device=0)
        _lib.check_latent(None, self.L.rnde_latent_create(C.byref(cfg), C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.rnde_latent_destroy(self.h)
            self.h = None

    def run(self, B, T, seed):
        """encode, decode_loss, encode_backward on the inputs of tests/test_gpu_latent.py::_case"""
        from tests.test_gpu_latent import _case
        _, x, p1, p2, p4, eps, res, z0b = _case(B, T, seed)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        L, h, chk = self.L, self.h, self.lib.check_latent
        xd, p1d, p2d, p4d, epsd, resd, z0bd = dev(x), dev(p1), dev(p2), dev(p4), dev(eps), dev(res), dev(z0b)
        z0d, mu0d, lvd = (torch.empty(B, 20, device="cuda") for _ in range(3))
        loss2, resbd, p4bd = torch.empty(2, device="cuda"), torch.empty(B, T, 20, device="cuda"), torch.empty(777, device="cuda")
        p1bd, p2bd = torch.empty(29320, device="cuda"), torch.empty(7090, device="cuda")
        torch.cuda.synchronize()
        chk(h, L.rnde_latent_encode(h, xd.data_ptr(), p1d.data_ptr(), p2d.data_ptr(), epsd.data_ptr(), B, T, z0d.data_ptr(), mu0d.data_ptr(), lvd.data_ptr(), None))
        chk(h, L.rnde_latent_decode_loss(h, resd.data_ptr(), p4d.data_ptr(), xd.data_ptr(), B, T, loss2.data_ptr(), resbd.data_ptr(), p4bd.data_ptr(), None))
        chk(h, L.rnde_latent_encode_backward(h, z0bd.data_ptr(), 0.7, p1d.data_ptr(), p2d.data_ptr(), xd.data_ptr(), p1bd.data_ptr(), p2bd.data_ptr(), None))
        torch.cuda.synchronize()
        return dict(z0=z0d, mu0=mu0d, logvar=lvd, loss2=loss2, res_bar=resbd, p4_bar=p4bd, p1_bar=p1bd, p2_bar=p2bd)


def test_latent_caller(monkeypatch):
    """One handle of max_batch 37, max_T 49: S at B = 16, T = 7; the dirty predecessor is the same sequence at B = 37, T = 49 (other inputs, other
    parameters: another seed).  16 create-time allocations; the activation tape alone is 37 x 49 records."""
    three_ways(monkeypatch, lambda: _Latent(37, 49), lambda h: h.run(16, 7, 3), lambda h: h.run(37, 49, 2), 16, 37 * 49 * 40 * 4)


# ---- the coupled controller on the chain engine's multi-wave kernels ----------------------------------------------------------------------

class _CoupledGroup:
    """world ranks in one process (tests/test_gpu_coupled.py): one handle, one non-blocking stream and one host thread per rank"""

    def __init__(self, arch, per, world, tol):
        from regneuralde_jl_amd import _lib
        from tests.test_gpu_forward import _cfg
        from tests.util import Node
        self.L, self.world, self.per = _lib.lib(), world, per
        self.comms = (C.c_void_p * world)()
        assert self.L.rnde_comm_create_local_group(world, 0, self.comms) == 0, self.L.rnde_comm_last_error(None)
        self.nodes = [Node(_cfg(arch, per, reltol=tol, abstol=tol, col_tile=65)).own_stream() for _ in range(world)]
        for n, c in zip(self.nodes, self.comms):
            _lib.check(n.h, self.L.rnde_node_set_coupling(n.h, C.c_void_p(c), per * world))

    def close(self):
        for n in self.nodes:
            n.close()
        for c in self.comms:
            self.L.rnde_comm_destroy(C.c_void_p(c))
        self.nodes, self.comms = [], []

    def run(self, x, p, ubar, svb):
        out, per = [None] * self.world, self.per

        def work(r):
            g = self.nodes[r].forward(x[r * per:(r + 1) * per], p, keep_tape=True)
            out[r] = (g,) + self.nodes[r].backward(ubar[r * per:(r + 1) * per] * float(self.world), np.full(len(g["saveval"]), svb, dtype=np.float32))

        th = [threading.Thread(target=work, args=(r,)) for r in range(self.world)]
        [t.start() for t in th]
        [t.join(120) for t in th]
        assert all(o is not None for o in out), "a rank did not finish"
        res = {}
        for r, (g, gx, gp, gt) in enumerate(out):
            res.update({f"r{r}/u": g["u"], f"r{r}/saveval": g["saveval"], f"r{r}/steps": g["steps"], f"r{r}/x_bar": gx, f"r{r}/p_bar": gp, f"r{r}/tspan_bar": gt})
        return res


def test_coupled_chain_engine(monkeypatch):
    """chain3 of tests/test_gpu_coupled.py (128 columns over four ranks, tol 1e-4, a cotangent of 3 on every saved value).  The handles'
    reverse buffers, the evaluation-time table among them, are allocated by the first backward and used at once on the rank's own stream."""
    from tests.test_gpu_chain import _setup
    B, world, tol, scale = 128, 4, 1e-4, 2.0
    arch, p, x = _setup("chain3", B, 21, scale)
    _, p2, _ = _setup("chain3", B, 971, scale)
    ubar = np.random.default_rng(22).standard_normal(x.shape).astype(np.float32) / B
    a = three_ways(monkeypatch, lambda: _CoupledGroup(arch, B // world, world, tol), lambda g: g.run(x, p, ubar, 3.0),
                   lambda g: g.run(_cycle(x, B), p2, ubar, 1.0), world * 20, world * 112 * len(p) * 4)
    assert all(np.array_equal(a[f"r{r}/steps"], a["r0/steps"]) for r in range(world))      # every rank holds the same controller history
