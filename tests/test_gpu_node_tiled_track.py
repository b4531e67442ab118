"""The tracked reverse sweep of the tiled TrackedNeuralODE engine (rnde_node_set_tracking; rnde_tile_reverse_kernel<NtDyn, false, true>): the step-size
controller, the clamps to t1 and the initial-step rule differentiated, against the fp64 CPU oracle with the same flags.

Cases: the adaptive inputs of tests/test_gpu_node_tiled.py (imported) -- pad_td ([3,7,3] TD, B = 37: three tiles, a partial last one, padding
in every dimension), pad_td_rej (a natural rejection), wide_state ([70,96,70], B = 17: more than 64 state rows), limit ([2,128,128,2], B = 16:
the largest LDS footprint) -- at reltol = abstol = 1e-5; [3,7,3] at B = 528 (33 tiles: the agent-scope meeting); the forced-rejection sequence
REPLAY_DTP / REPLAY_ACC of that file on its plain pad_td and wide_state inputs.

Reference and bound.  The fp64 oracle runs along the device's own attempts (set_replay with dtp_in and accepted from rnde_node_attempts_ext, so
that it clamps to t1 where the device did).  Per quantity (x-bar, p-bar, tspan-bar; max|a - b| / max|b|) the bound is
max(1e-3, 4 x the distance of the fp32 oracle, replayed along the same attempts, from the fp64 one): the tracked gradient carries EEst-bar
through every attempt, and EEst is a small difference of large terms, so fp32 arithmetic itself is that far from fp64.  On the CPU (fp32
oracle's own sequence) that distance is, x-bar / p-bar / tspan-bar with the saved values' cotangent alone: pad_td 1.7e-3 / 2.2e-3 / 2.3e-3,
pad_td_rej 8.0e-4 / 9.5e-4 / 4.4e-3, wide_state 5.6e-3 / 2.2e-3 / 1.5e-2, limit 6.6e-2 / 1.4e-2 / 5.9e-2 (a short solve whose gradient is
dominated by two attempts); with the end state's cotangent too it is 4e-3 or less.  All three figures are printed per case.
Asserted so that the comparison means something: no fp64 EEst in [0.9, 1.1]; the device's q of an attempt sits at a clamp (1 / qmax, 1 / qmin)
only where the oracle's does; the device's first proposed step is within 1e-3 of the free-running fp64 oracle's (the same branch of the
initial-step rule).
Measured on an MI355X, device against fp64 [fp32 oracle against fp64], (1, 1), x-bar / p-bar / tspan-bar.  With u-bar: pad_td 1.7e-3 / 8.4e-4 /
2.7e-3 [1.5e-3 / 5.1e-4 / 2.6e-3], pad_td_rej 1.7e-3 / 2.0e-3 / 5.7e-2 [6.0e-4 / 5.3e-4 / 6.5e-2] (p-bar 1.98e-3 against a bound of 2.12e-3: the
closest call), wide_state 8.2e-4 / 8.5e-5 / 2.6e-4 [7.4e-4 / 1.1e-4 / 3.8e-6], limit 1.7e-3 / 4.3e-4 / 1.5e-3 [2.9e-3 / 5.7e-4 / 7.4e-3].  Saved
values only: pad_td 2.6e-3 / 2.5e-3 / 1.6e-3 [2.5e-3 / 1.5e-3 / 2.5e-3], pad_td_rej 1.7e-3 / 2.3e-3 / 6.7e-3 [7.1e-4 / 7.3e-4 / 7.3e-3], wide_state
2.3e-3 / 1.1e-3 / 3.2e-3 [2.5e-3 / 1.8e-3 / 8.8e-3], limit 3.1e-2 / 7.5e-3 / 7.8e-3 [5.3e-2 / 1.3e-2 / 1.1e-2].  (1, 0) is the same to two digits.
Forced rejection, p-bar: 2.2e-3 / 9.3e-5 with u-bar, 1.8e-2 / 3.8e-2 without [7.3e-3 / 1.4e-4, 3.9e-2 / 5.0e-2].  33 tiles: 1.3e-5 / 9.2e-6 / 5.9e-5.
Other settings (fp64, saved values only): (0, 0) against (1, 1) 0.85 / 0.93 / 0.37 / 0.59 on p-bar; pad_td (1, 0) 4.7e-2, tspan-bar[0] 3.86 against
-0.35.  The file: 16 cases, 3.3 s.
A cotangent on the end state only.  The expectation was that the controller's share is O(tol) there and that the device's (0, 0) and (1, 1)
sweeps agree to 1e-4.  The fp64 oracle says otherwise on these inputs (first layer x 60 - 240: EEst, and with it every step size, is steep in
the parameters), (1, 1) against (0, 0), x-bar / p-bar, along the device's attempts: pad_td 7.685e-3 / 3.938e-3, pad_td_rej 0.602 / 0.215 (the
oracle's (0, 0) also lets a rejected attempt pass its step's cotangent on), wide_state 1.99e-2 / 3.41e-3, limit 8.63e-5 / 7.16e-5.  On an MI355X
the device's two sweeps differ by 7.674e-3 / 3.941e-3, 0.602 / 0.213, 2.00e-2 / 3.41e-3 and 8.57e-5 / 7.18e-5.  So the 1e-4 agreement is asserted
where the reference itself has it (limit, with the reference's figure asserted too); on every case the tracked gradient of an end-state
cotangent is held to the fp64 oracle's by the bound above, and the device's two sweeps are asserted to be as far apart as the oracle's two
(within the two bounds added); the four figures are printed.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.act_ref import rel
from tests.test_gpu_node_tiled import REPLAY_ACC, REPLAY_DTP, adaptive_case, case, make_cfg, tiled

pytestmark = pytest.mark.gpu

TOL = 1e-5
Q_CLAMPS = (np.float32(1.0 / 10.0), np.float32(1.0 / 0.2))      # 1 / kQmax, 1 / kQmin
END_STATE_ONLY_AGREE = ("limit",)      # where the fp64 oracle's (0, 0) and (1, 1) gradients of an end-state cotangent agree to 1e-4 (module docstring)


def _oracle(dims, acts, td, dtype, ctrl, initdt):
    from oracle.oracle import Oracle, make_arch
    return Oracle(make_arch(dims, acts, td), dtype, TOL, TOL, reg_kind=1, track_ctrl=ctrl, track_initdt=initdt, max_attempts=128)


def _node(dims, acts, td, max_batch, **kw):
    return tiled(make_cfg(dims, acts, td, max_batch, reltol=TOL, abstol=TOL, regularize=1, max_attempts=128, **kw))


def set_tracking(node, ctrl, initdt):
    from regneuralde_jl_amd import _lib
    node.L.rnde_node_release_tape(node.h)
    _lib.check(node.h, node.L.rnde_node_set_tracking(node.h, int(ctrl), int(initdt)))


def attempts_ext(node):
    from regneuralde_jl_amd import _lib
    cap = node.cfg.max_attempts
    out, n = (C.c_float * (6 * cap))(), C.c_int32(0)
    _lib.check(node.h, node.L.rnde_node_attempts_ext(node.h, out, cap, C.byref(n)))
    return np.array(out[:6 * n.value], dtype=np.float32).reshape(-1, 6)


def cotangents(x, nsv, with_u=True):
    """with_u: those of tests/test_gpu_node_tiled.py::test_reverse_matches_oracle (the end state's drawn first).  Without: no cotangent on the end
    state and U(0.5, 1.5) from default_rng(100) on the saved values, the draw the CPU figures of DESIGN 4.10.1 were made with (tspan-bar[0] = 3.85 on
    pad_td, the fp32 oracle 1.4e-2 from the fp64 one on limit)."""
    rng = np.random.default_rng(100)
    if not with_u:
        return np.zeros_like(x), rng.uniform(0.5, 1.5, nsv).astype(np.float32)
    ubar = rng.standard_normal(x.shape).astype(np.float32)
    svbar = rng.uniform(0.5, 1.5, nsv).astype(np.float32)
    return ubar, svbar


def oracle_grad(dims, acts, td, dtype, flags, x, p, ext, ubar, svbar):
    """(x-bar, p-bar, tspan-bar, steps_ext) of the oracle with `flags` along the attempts `ext` (None: solving on its own)."""
    o = _oracle(dims, acts, td, dtype, *flags)
    if ext is not None:
        o.set_replay(ext[:, 2].astype(dtype), ext[:, 4].astype(np.int32))
    r = o.forward(x.astype(dtype), p.astype(dtype))
    assert r["rc"] == 0
    if ext is not None:
        assert r["nattempts"] == len(ext)
    gx, gp, gt = o.backward(ubar.astype(dtype), None if svbar is None else svbar.astype(dtype))
    return gx, gp, gt, o.steps_ext()


def check_against_oracle(label, dims, acts, td, p, x, got, ext, dev, flags, ubar, svbar, free_first=None):
    """The rule of the module docstring: dev = (x-bar, p-bar, tspan-bar) of the device; returns the three bounds."""
    g64 = oracle_grad(dims, acts, td, np.float64, flags, x, p, ext, ubar, svbar)
    g32 = oracle_grad(dims, acts, td, np.float32, flags, x, p, ext, ubar, svbar)
    s64 = g64[3]
    assert all(not 0.9 <= float(e) <= 1.1 for e in s64[:, 3]), "an EEst of the fp64 oracle within rounding of the accept threshold: pick another seed"
    for qd, qo in zip(ext[:, 5], s64[:, 5]):
        if any(abs(qd - c) <= 1e-6 * c for c in Q_CLAMPS):
            assert any(abs(qo - c) <= 1e-6 * c for c in Q_CLAMPS), "the device's q is at a clamp, the fp64 oracle's is not: pick another seed"
    if free_first is not None:
        assert abs(float(ext[0, 2]) / free_first - 1.0) <= 1e-3, "the device and the fp64 oracle chose different branches of the initial-step rule"
    bounds = []
    for name, d, a32, a64 in zip(("x-bar", "p-bar", "tspan-bar"), dev, g32[:3], g64[:3]):
        e32, e = rel(a32, a64), rel(d, a64)
        bound = max(1e-3, 4.0 * e32)
        print(f"tracked {label} {flags} {name}: device {e:.3e}  fp32 oracle {e32:.3e}  bound {bound:.3e}")
        bounds.append((name, e, bound))
    for name, e, bound in bounds:
        assert e <= bound, (label, flags, name, e, bound)
    return [b for _, _, b in bounds], g64


@functools.lru_cache(maxsize=None)
def free_first_step(key):
    """The first proposed step of the fp64 oracle solving `key` on its own."""
    dims, acts, td, p, x = adaptive_case(key)
    o = _oracle(dims, acts, td, np.float64, 1, 1)
    assert o.forward(x.astype(np.float64), p.astype(np.float64))["rc"] == 0
    return float(o.steps_ext()[0, 2])


# ---- 1. the tracked gradient against the fp64 oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["pad_td", "pad_td_rej", "wide_state", "limit"])
def test_tracked_gradient_matches_oracle(key):
    dims, acts, td, p, x = adaptive_case(key)
    node = _node(dims, acts, td, x.shape[0])
    for flags in ((1, 1), (1, 0)):
        set_tracking(node, *flags)
        got = node.forward(x, p, keep_tape=True)
        ext = attempts_ext(node)
        assert np.array_equal(ext[:, [0, 1, 3, 4]], got["steps"])
        for lab, with_u in (("u-bar and saved values", True), ("saved values only", False)):
            ub, svbar = cotangents(x, len(got["saveval"]), with_u)
            dev = node.backward(ub, svbar)
            check_against_oracle(f"{key}, {lab}", dims, acts, td, p, x, got, ext, dev, flags, ub, svbar, free_first_step(key))
            assert np.abs(dev[2]).max() > 0.0
    node.close()


# ---- 2. the other settings are another gradient --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["pad_td", "pad_td_rej", "wide_state", "limit"])
def test_other_settings_are_another_gradient(key):
    dims, acts, td, p, x = adaptive_case(key)
    node = _node(dims, acts, td, x.shape[0])
    set_tracking(node, 1, 1)
    got = node.forward(x, p, keep_tape=True)
    ext = attempts_ext(node)
    zero, svbar = cotangents(x, len(got["saveval"]), False)
    dev11 = node.backward(zero, svbar)
    bounds, g11 = check_against_oracle(f"{key}, saved values only", dims, acts, td, p, x, got, ext, dev11, (1, 1), zero, svbar, free_first_step(key))
    g00 = oracle_grad(dims, acts, td, np.float64, (0, 0), x, p, ext, zero, svbar)
    g10 = oracle_grad(dims, acts, td, np.float64, (1, 0), x, p, ext, zero, svbar)
    d00, d10 = rel(g00[1], g11[1]), rel(g10[1], g11[1])
    print(f"settings {key}: fp64 p-bar (0,0) vs (1,1) {d00:.3e}, (1,0) vs (1,1) {d10:.3e}, bound {bounds[1]:.3e}; tspan-bar[0] (1,1) {g11[2][0]:.4f} (1,0) {g10[2][0]:.4f}")
    assert d00 >= 10.0 * bounds[1]
    if key == "pad_td":
        assert d10 >= 3.0 * bounds[1]
        assert abs(float(g11[2][0]) - float(g10[2][0])) > 1.0
    # a cotangent on the end state only.  The tracked gradient is the reference's there too (the rule of test 1), and where the fp64 oracle's own
    # (0, 0) and (1, 1) gradients agree to 1e-4 the device's two sweeps agree to 1e-4 as well.  That is `limit` alone: see the module docstring.
    ubar, _ = cotangents(x, len(got["saveval"]))
    a = node.backward(ubar, None)
    ub_bounds, h11 = check_against_oracle(f"{key}, u-bar only", dims, acts, td, p, x, got, ext, a, (1, 1), ubar, None, free_first_step(key))
    h00 = oracle_grad(dims, acts, td, np.float64, (0, 0), x, p, ext, ubar, None)
    set_tracking(node, 0, 0)
    got0 = node.forward(x, p, keep_tape=True)
    assert np.array_equal(got0["u"], got["u"]) and np.array_equal(got0["steps"], got["steps"])
    b = node.backward(ubar, None)
    node.close()
    print(f"settings {key}: end-state cotangent only, (1,1) vs (0,0): device x-bar {rel(a[0], b[0]):.3e} p-bar {rel(a[1], b[1]):.3e}; "
          f"fp64 oracle x-bar {rel(h11[0], h00[0]):.3e} p-bar {rel(h11[1], h00[1]):.3e}")
    # the device's two sweeps are as far apart as the reference's two.  a is within its bound B11 of h11 (just asserted) and b within B00 = 1e-3
    # of h00 (the bound tests/test_gpu_node_tiled.py holds the constant sweep to), each relative to its reference's largest entry, and
    # max|h11| <= (1 + o) max|h00| with o the oracle's figure: the two figures differ by at most (B11 + B00) (1 + o)
    for i, name in enumerate(("x-bar", "p-bar")):
        d, o = rel(a[i], b[i]), rel(h11[i], h00[i])
        assert abs(d - o) <= (ub_bounds[i] + 1e-3) * (1.0 + o), (key, name, d, o)
    if key in END_STATE_ONLY_AGREE:
        assert rel(h11[0], h00[0]) <= 1e-4 and rel(h11[1], h00[1]) <= 1e-4      # (the premise, on the reference)
        assert rel(a[0], b[0]) <= 1e-4 and rel(a[1], b[1]) <= 1e-4
    assert tuple(b[2]) == (0.0, 0.0)


# ---- 3. a given sequence with a forced rejection -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pad_td", "wide_state"])
def test_tracked_replay_with_a_forced_rejection(name):
    dims, acts, td, p, x = case(name)
    node = _node(dims, acts, td, x.shape[0])
    set_tracking(node, 1, 1)
    got = node.forward_replay(x, p, REPLAY_DTP, REPLAY_ACC, keep_tape=True)
    ext = attempts_ext(node)
    assert [int(a) for a in ext[:, 4]] == REPLAY_ACC and [float(d) for d in ext[:, 2]] == REPLAY_DTP
    for lab, with_u in (("u-bar and saved values", True), ("saved values only", False)):
        ub, svbar = cotangents(x, len(got["saveval"]), with_u)
        dev = node.backward(ub, svbar)
        check_against_oracle(f"replay {name}, {lab}", dims, acts, td, p, x, got, ext, dev, (1, 1), ub, svbar)
    node.close()


# ---- 4. bits ------------------------------------------------------------------------------------------------------------------------------

def test_tracked_runs_are_bit_identical_and_toggling_leaves_no_trace():
    dims, acts, td, p, x = adaptive_case("pad_td")
    runs = []
    for mb in (37, 37, 64):
        node = _node(dims, acts, td, mb)
        set_tracking(node, 1, 1)
        g = node.forward(x, p, keep_tape=True)
        ubar, svbar = cotangents(x, len(g["saveval"]))
        runs.append((g, node.backward(ubar, svbar)))
        if mb == 64:      # (1, 1), then (0, 0): forward and backward equal a handle that was never switched, bit for bit
            set_tracking(node, 0, 0)
            g0 = node.forward(x, p, keep_tape=True)
            b0 = node.backward(ubar, svbar)
            plain = _node(dims, acts, td, mb)
            g1 = plain.forward(x, p, keep_tape=True)
            b1 = plain.backward(ubar, svbar)
            plain.close()
            assert all(np.array_equal(g0[k], g1[k]) for k in ("u", "saveval", "steps"))
            assert all(np.array_equal(u, v) for u, v in zip(b0, b1)) and tuple(b0[2]) == (0.0, 0.0)
        node.close()
    for g, b in runs[1:]:
        assert all(np.array_equal(g[k], runs[0][0][k]) for k in ("u", "saveval", "steps"))
        assert all(np.array_equal(u, v) for u, v in zip(b, runs[0][1]))


# ---- 5. the agent-scope meeting -----------------------------------------------------------------------------------------------------------

def test_tracked_gradient_over_33_tiles():
    dims, acts, td, p, _ = adaptive_case("pad_td")
    x = np.random.default_rng(528).uniform(-1.0, 1.0, (528, dims[0])).astype(np.float32)      # (vetted on the CPU: EEst <= 0.13, q in [0.38, 1.6])
    node = _node(dims, acts, td, 528)
    set_tracking(node, 1, 1)
    got = node.forward(x, p, keep_tape=True)
    ext = attempts_ext(node)
    ubar, svbar = cotangents(x, len(got["saveval"]))
    dev = node.backward(ubar, svbar)
    node.close()
    o = _oracle(dims, acts, td, np.float64, 1, 1)
    assert o.forward(x.astype(np.float64), p.astype(np.float64))["rc"] == 0
    check_against_oracle("33 tiles", dims, acts, td, p, x, got, ext, dev, (1, 1), ubar, svbar, float(o.steps_ext()[0, 2]))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------

def test_refusals_by_name():
    from regneuralde_jl_amd import _lib
    from tests.util import Node
    dims, acts, td, p, x = case("pad_td", 5)
    node = _node(dims, acts, td, 5)
    L, h = node.L, node.h

    def refused(status, handle, *words):
        assert status == _lib.BAD_ARG
        msg = L.rnde_last_error(handle).decode()
        assert all(w in msg for w in words), msg

    c, i = C.c_int32(-1), C.c_int32(-1)
    assert L.rnde_node_tracking(h, C.byref(c), C.byref(i)) == _lib.OK and (c.value, i.value) == (0, 0)
    refused(L.rnde_node_set_tracking(h, 0, 1), h, "rnde_node_set_tracking", "track_ctrl = 0", "track_initdt = 1")
    refused(L.rnde_node_set_tracking(h, 2, 0), h, "rnde_node_set_tracking", "0 or 1")
    refused(L.rnde_node_set_tracking(h, 1, -1), h, "rnde_node_set_tracking", "0 or 1")
    node.forward(x, p, keep_tape=True)
    refused(L.rnde_node_set_tracking(h, 1, 1), h, "rnde_node_set_tracking", "holds a tape")
    assert L.rnde_node_tracking(h, C.byref(c), C.byref(i)) == _lib.OK and (c.value, i.value) == (0, 0)
    L.rnde_node_release_tape(h)
    for flags in ((1, 0), (1, 1), (0, 0)):
        assert L.rnde_node_set_tracking(h, *flags) == _lib.OK
        assert L.rnde_node_tracking(h, C.byref(c), C.byref(i)) == _lib.OK and (c.value, i.value) == flags
    node.close()
    chain = Node(make_cfg(dims, acts, td, 5, track_ctrl=1, track_initdt=1))      # a handle of rnde_node_create
    refused(L.rnde_node_set_tracking(chain.h, 1, 1), chain.h, "rnde_node_set_tracking", "rnde_node_create_tiled", "cfg.track_ctrl", "cfg.track_initdt")
    assert L.rnde_node_tracking(chain.h, C.byref(c), C.byref(i)) == _lib.OK and (c.value, i.value) == (1, 1)
    chain.close()
    for kw in (dict(track_ctrl=1), dict(track_initdt=1)):      # the create call still refuses either config flag
        hh = C.c_void_p()
        assert L.rnde_node_create_tiled(C.byref(make_cfg(dims, acts, td, 5, **kw)), C.byref(hh)) == _lib.BAD_ARG
        msg = L.rnde_last_error(None).decode()
        assert "track_ctrl" in msg and "track_initdt" in msg


def test_attempts_ext_capacity_and_count():
    from regneuralde_jl_amd import _lib
    dims, acts, td, p, x = case("pad_td", 5)
    node = _node(dims, acts, td, 5)
    got = node.forward(x, p)
    n = C.c_int32(0)
    assert node.L.rnde_node_attempts_ext(node.h, None, 0, C.byref(n)) == _lib.OK and n.value == got["nattempts"]
    small = (C.c_float * 6)()
    assert node.L.rnde_node_attempts_ext(node.h, small, 1, C.byref(n)) == _lib.BAD_ARG
    ext = attempts_ext(node)
    node.close()
    assert ext.shape == (got["nattempts"], 6)
    dt = np.minimum(ext[:, 2], np.float32(1.0) - ext[:, 0])
    assert np.array_equal(ext[:, 1], dt)      # dt = min(dtp_in, t1 - t)


# ---- 7. the Python layer -------------------------------------------------------------------------------------------------------------------

def test_python_layer_tracking():
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(31)
    B = 16
    model = rn.TDChain(rn.Dense(3, 128, "tanh", g), rn.Dense(129, 128, "tanh", g), rn.Dense(129, 2, "identity", g))
    node = rn.TrackedNeuralODE(model, [0, 1], True, True, engine="tiled", track_ctrl=False, track_initdt=False, reltol=TOL, abstol=TOL, max_batch=B)
    x = torch.randn(B, 2, generator=g)
    xd, pd = x.cuda().requires_grad_(True), node.p.cuda().requires_grad_(True)
    L = rn._lib.lib()

    def settings():
        out = []
        for hs in node._handles.values():
            for h in hs:
                c, i = C.c_int32(-1), C.c_int32(-1)
                assert L.rnde_node_tracking(h.ptr, C.byref(c), C.byref(i)) == 0
                out.append((c.value, i.value))
        return out

    with torch.no_grad():
        for _ in range(6):      # more probes than a layer may hold tapes: none of them pins one
            u0, nfe0, _ = node(xd, pd)
    assert not any(h.busy for hs in node._handles.values() for h in hs)
    assert settings() == [(0, 0)]
    node.set_tracking(True, True)
    assert settings() == [(1, 1)]                    # the handle that exists
    u, nfe, sv = node(xd, pd)                        # a taped call: a handle created later
    assert sorted(settings()) == [(1, 1), (1, 1)] and torch.equal(u, u0) and nfe == nfe0
    (u.sum() + sv.saveval.sum()).backward()
    assert not any(h.busy for hs in node._handles.values() for h in hs)
    ref = tiled(node._config(0, None))
    set_tracking(ref, 1, 1)
    r = ref.forward(x.numpy(), node.p.numpy(), keep_tape=True)
    assert np.array_equal(r["u"], u.detach().cpu().numpy()) and np.array_equal(r["saveval"], sv.saveval.detach().cpu().numpy())
    xb, pb, tsb = ref.backward(np.ones((B, 2), np.float32), np.ones(len(r["saveval"]), np.float32))
    ref.close()
    assert rel(xd.grad.cpu().numpy(), xb) <= 1e-6 and rel(pd.grad.cpu().numpy(), pb) <= 1e-6
    assert node.last_tspan_bar == (float(tsb[0]), float(tsb[1])) and node.last_tspan_bar != (0.0, 0.0)
    layer2 = rn.TrackedNeuralODE(model, [0, 1], True, True, engine="tiled", track_ctrl=False, track_initdt=False, reltol=TOL, abstol=TOL, max_batch=B,
                                 tiled_tracking=(True, False))
    assert layer2.tiled_tracking == (True, False)


def test_python_layer_toggles_after_a_backward_and_while_a_forward_is_pending():
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(31)
    B = 16
    model = rn.TDChain(rn.Dense(3, 128, "tanh", g), rn.Dense(129, 128, "tanh", g), rn.Dense(129, 2, "identity", g))
    node = rn.TrackedNeuralODE(model, [0, 1], True, True, engine="tiled", track_ctrl=False, track_initdt=False, reltol=TOL, abstol=TOL, max_batch=B)
    x = torch.randn(B, 2, generator=g).cuda()
    p = node.p.cuda()
    L = rn._lib.lib()

    def settings():
        out = []
        for hs in node._handles.values():
            for h in hs:
                c, i = C.c_int32(-1), C.c_int32(-1)
                assert L.rnde_node_tracking(h.ptr, C.byref(c), C.byref(i)) == 0
                out.append((c.value, i.value))
        return out

    def step():
        xd, pd = x.clone().requires_grad_(True), p.clone().requires_grad_(True)
        u, _, sv = node(xd, pd)
        return xd, pd, u.sum() + sv.saveval.sum()

    def grads(xd, pd, loss):
        loss.backward()
        return xd.grad.clone(), pd.grad.clone(), node.last_tspan_bar

    g00 = grads(*step())
    assert settings() == [(0, 0)] and g00[2] == (0.0, 0.0)
    # after a completed backward the handle is free for the layer but still holds its tape in the library: the switch must reach it
    node.set_tracking(True, True)
    assert settings() == [(1, 1)] and node.tiled_tracking == (True, True)
    g11 = grads(*step())
    assert settings() == [(1, 1)] and g11[2] != (0.0, 0.0) and not torch.equal(g11[1], g00[1])
    # while a taped forward is pending: it keeps the setting it ran under, every other handle takes the new one
    pend = step()
    node.set_tracking(False, False)
    assert settings() == [(1, 1)]
    other = step()                                   # a second handle, created under (0, 0)
    assert settings() == [(1, 1), (0, 0)]
    gb = grads(*other)
    assert gb[2] == (0.0, 0.0) and torch.equal(gb[0], g00[0]) and torch.equal(gb[1], g00[1])
    ga = grads(*pend)                                # the tape remembers (1, 1)
    assert ga[2] == g11[2] and torch.equal(ga[0], g11[0]) and torch.equal(ga[1], g11[1])
    assert not any(h.busy for hs in node._handles.values() for h in hs)
    # the handle that was skipped takes the layer's pair when it is next handed out
    gc = grads(*step())
    assert settings() == [(0, 0), (0, 0)]
    assert gc[2] == (0.0, 0.0) and torch.equal(gc[0], g00[0]) and torch.equal(gc[1], g00[1])
