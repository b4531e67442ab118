"""Saved points on the tiled TrackedNeuralODE engine (rnde_node_tiled_reserve_saveat; rnde_tile_solve_kernel<NtDyn, false, true>,
rnde_tile_reverse_kernel<NtDyn, false, *, true>): rnde_node_forward_saveat / _everystep and the D x n x B backward behind them, against the fp64 CPU
oracle.  Shapes, inputs and helpers are those of tests/test_gpu_node_tiled.py and tests/test_gpu_node_tiled_track.py (imported); reltol =
abstol = 1e-5.  Every case fails without the feature: the reserve symbol does not exist.

A saving solve along a GIVEN sequence.  rnde_node_forward_replay has no saving form on any engine, and none was added.  The solves of every
engine read the handle's replay state whether they save or not (rnde.hip forward_core; node_tiled_forward does the same), but
rnde_node_forward_replay sets that state for its own call and clears it, so no saving call ever met it.  The parity instrument
rnde_debug_arm_replay arms it for the next rnde_node_forward_saveat of the handle; case 1 uses it.

Reference and bounds.  Saved states: <= 2e-4 (the replay bound of tests/test_gpu_node_tiled.py) of the fp64 restatement that file uses for the
shape -- rk_replay64 with the oracle's dense_weights for two_pass (softplus: not an oracle activation), the fp64 oracle under set_replay for
the others, along the device's own attempts.  Gradients: per quantity (x-bar, p-bar, tspan-bar; max|a - b| / max|b|) the bound is
max(1e-3, 4 x the distance of the fp32 oracle, replayed along the same attempts, from the fp64 one), the rule of
tests/test_gpu_node_tiled_track.py.  At (0, 0) x-bar and p-bar only (the device returns tspan_bar = (0, 0) there by contract), and the oracle
runs along the ACCEPTED attempts alone: the constant-step sweep walks accepted steps, a rejected attempt changes no state of the forward, and
the oracle's own (0, 0) would let a rejected attempt pass its step's dt cotangent on into EEst (tests/test_gpu_node_tiled_track.py, module
docstring) -- tests/test_gpu_node_tiled.py::test_reverse_matches_oracle compares on sequences without a rejection for the same reason.
CPU-only figures (fp32 oracle against fp64, this file's cotangents) -- fixed sequence, (1, 1), x-bar / p-bar / tspan-bar: pad_td 1.2e-3 /
1.0e-3 / 4.5e-4, wide_state 6.3e-4 / 4.7e-4 / 5.6e-6; adaptive: at most 1.2e-3 (pad_td_rej x-bar), otherwise below 2e-4.
Asserted on the device's own log so that the adaptive comparison means something: some accepted step holds two save times; no interior save
time lies within 1e-3 of an accepted step's end (where fp32 and fp64 could put it in different steps); no fp64 EEst in [0.9, 1.1]; the
saving solve's attempts are the end-state solve's, bit for bit.

Measured on an MI355X, device against fp64 [fp32 oracle against fp64].  Saved states: fixed pad_td 1.6e-7, two_pass 4.1e-7, wide_state 4.0e-7;
adaptive pad_td 1.7e-7, pad_td_rej 2.6e-7, wide_state 3.0e-7, limit 1.8e-7; 33 tiles 3.2e-7.  Fixed sequence, x-bar / p-bar / tspan-bar: pad_td
(0, 0) 5.7e-6 / 1.5e-6 [4.4e-6 / 3.2e-6], (1, 1) 2.0e-3 / 3.4e-4 / 3.5e-5 [1.2e-3 / 1.0e-3 / 4.5e-4]; wide_state (0, 0) 1.0e-6 / 7.2e-7 [1.4e-6 /
8.4e-7], (1, 1) 6.1e-4 / 3.1e-4 / 2.5e-5 [6.3e-4 / 4.7e-4 / 5.6e-6].  Adaptive, (1, 1), saved states only: pad_td 6.5e-6 / 7.8e-7 / 7.7e-7
[4.5e-6 / 1.4e-6 / 4.0e-6], pad_td_rej 4.2e-4 / 4.0e-5 / 3.5e-4 [3.2e-4 / 1.8e-5 / 3.1e-4], wide_state 1.4e-4 / 8.4e-6 / 1.6e-5 [9.4e-5 / 7.5e-6 /
1.3e-5], limit 2.0e-6 / 3.3e-7 / 5.9e-8 [3.6e-6 / 1.3e-6 / 2.4e-7]; with ones on the saved values too: pad_td 6.4e-4 / 8.1e-5 / 1.2e-4 [5.9e-4 /
5.1e-5 / 1.3e-4], pad_td_rej 2.7e-3 / 4.1e-4 / 8.6e-4 [9.8e-4 / 1.1e-4 / 1.1e-3] (x-bar 2.74e-3 against a bound of 3.91e-3: the closest call),
wide_state 1.6e-4 / 1.6e-5 / 2.3e-5 [2.0e-4 / 2.7e-5 / 1.4e-5], limit 3.3e-4 / 2.6e-5 / 1.9e-5 [5.5e-4 / 3.8e-5 / 5.3e-5].  (1, 0) is the same to
two digits.  33 tiles: 6.2e-6 / 1.5e-7 / 2.3e-7 [1.4e-5 / 7.9e-6 / 1.6e-6].  fp64 (0, 0) against (1, 1), saved states only, x-bar: pad_td 4.1e-3,
pad_td_rej 0.561, wide_state 1.22e-2, limit 4.7e-5.  The file: 13 cases, 6 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.act_ref import chain64, rel
from tests.test_gpu_node_tiled import ADAPTIVE, REPLAY_ACC, REPLAY_DTP, adaptive_case, case, make_cfg, tableau, tiled
from tests.test_gpu_node_tiled_track import attempts_ext, set_tracking

pytestmark = pytest.mark.gpu

TOL = 1e-5
SAVE_FIXED = np.array([0.0, 0.1, 0.2, 0.25, 0.6, 1.0], dtype=np.float32)
SAVE_ADAPT = np.array([0.0, 0.065, 0.35, 0.88, 0.886, 1.0], dtype=np.float32)
PINNED_REFUSAL = "rnde_node_forward_saveat is not served (the end state only; saveat runs on the engines of rnde_node_create)"


def _node(dims, acts, td, max_batch, reserve=8, max_attempts=128):
    from regneuralde_jl_amd import _lib
    node = tiled(make_cfg(dims, acts, td, max_batch, reltol=TOL, abstol=TOL, regularize=1, max_attempts=max_attempts))
    if reserve is not None:
        _lib.check(node.h, node.L.rnde_node_tiled_reserve_saveat(node.h, reserve))
    return node


def arm(node, dtp, acc):
    from regneuralde_jl_amd import _lib
    pairs = (C.c_float * (2 * len(dtp)))()
    for i in range(len(dtp)):
        pairs[2 * i], pairs[2 * i + 1] = float(dtp[i]), float(acc[i] != 0)
    _lib.check(node.h, node.L.rnde_debug_arm_replay(node.h, pairs, len(dtp)))


def _oracle(dims, acts, td, dtype, ctrl, initdt):
    from oracle.oracle import Oracle, make_arch
    return Oracle(make_arch(dims, acts, td), dtype, TOL, TOL, reg_kind=1, track_ctrl=ctrl, track_initdt=initdt, max_attempts=128)


def oracle_saved(dims, acts, td, dtype, flags, x, p, dtp, acc, sa, ubar=None, svbar=None):
    """The oracle with `flags` along the attempts (dtp, acc), saving at `sa`: (forward result, (x-bar, p-bar, tspan-bar) or None, steps_ext)."""
    o = _oracle(dims, acts, td, dtype, *flags)
    o.set_replay(np.asarray(dtp, dtype=dtype), np.asarray(acc, dtype=np.int32))
    r = o.forward(x.astype(dtype), p.astype(dtype), saveat=sa.astype(dtype))
    assert r["rc"] == 0 and r["nattempts"] == len(dtp)
    g = None if ubar is None else o.backward(ubar.astype(dtype), None if svbar is None else svbar.astype(dtype))
    return r, g, o.steps_ext()


def saved_cotangent(shape):
    return np.random.default_rng(100).uniform(0.5, 1.5, shape).astype(np.float32)


def check_gradient(label, dims, acts, td, x, p, dtp, acc, sa, flags, ubar, svbar, dev):
    """The bound rule of the module docstring; dev = (x-bar, p-bar, tspan-bar) of the device.  Returns (bounds, fp64 gradients, fp64 steps_ext)."""
    if flags == (0, 0):      # the accepted attempts alone (module docstring)
        keep = [i for i, a in enumerate(acc) if a]
        dtp, acc = [dtp[i] for i in keep], [acc[i] for i in keep]
    _, g64, s64 = oracle_saved(dims, acts, td, np.float64, flags, x, p, dtp, acc, sa, ubar, svbar)
    _, g32, _ = oracle_saved(dims, acts, td, np.float32, flags, x, p, dtp, acc, sa, ubar, svbar)
    names = ("x-bar", "p-bar") if flags == (0, 0) else ("x-bar", "p-bar", "tspan-bar")
    out = []
    for i, name in enumerate(names):
        e32, e = rel(g32[i], g64[i]), rel(dev[i], g64[i])
        bound = max(1e-3, 4.0 * e32)
        print(f"saveat {label} {flags} {name}: device {e:.3e}  fp32 oracle {e32:.3e}  bound {bound:.3e}")
        out.append((name, e, bound))
    for name, e, bound in out:
        assert e <= bound, (label, flags, name, e, bound)
    return [b for _, _, b in out], g64, s64


# ---- 1. a fixed sequence: step ends at 0.25, 0.5, 0.75, 1 exactly, one rejection ----------------------------------------------------------------
# save times: the start, two points in one step, an interior step end (a copy), a step with no point, t1

@pytest.mark.parametrize("name", ["pad_td", "two_pass", "wide_state"])
def test_fixed_sequence_saved_states_and_gradients(name):
    dims, acts, td, p, x = case(name)
    B, D, T = x.shape[0], dims[0], len(SAVE_FIXED)
    node = _node(dims, acts, td, B, max_attempts=16)
    arm(node, REPLAY_DTP, REPLAY_ACC)
    got = node.forward_saveat(x, p, SAVE_FIXED)
    att = [(float(s[0]), float(s[1]), int(s[3])) for s in got["steps"]]
    assert [a[2] for a in att] == REPLAY_ACC and [a[1] for a in att] == REPLAY_DTP
    assert [a[0] + a[1] for a in att if a[2]] == [0.25, 0.5, 0.75, 1.0]
    assert got["u"].shape == (B, T, D) and np.array_equal(got["u"][:, 0], x)
    if name == "two_pass":      # rk_replay64's stages with the oracle's dense weights
        from oracle.oracle import Oracle, make_arch
        dw = Oracle(make_arch([3, 7, 3], ["tanh", "tanh"], True), np.float64).dense_weights
        a_, c_, _ = tableau()
        P64 = torch.from_numpy(p).double()
        f = lambda v, t: chain64(dims, acts, td, 0, P64, v, t)
        u, ref = torch.from_numpy(x).double(), np.zeros((B, T, D))
        ref[:, 0] = x
        for t, dt, acc in att:
            k = []
            for s in range(7):
                y = u + dt * sum(a_[s, j] * k[j] for j in range(s)) if s else u
                k.append(f(y, t + c_[s] * dt))
            if not acc:
                continue
            un = u + dt * sum(a_[6, j] * k[j] for j in range(6))
            for i, ts in enumerate(SAVE_FIXED.astype(np.float64)):
                if t < ts <= t + dt:
                    b = dw((ts - t) / dt)
                    ref[:, i] = (un if ts == t + dt else u + dt * sum(b[j] * k[j] for j in range(7))).numpy()
            u = un
    else:
        ref = oracle_saved(dims, acts, td, np.float64, (0, 0), x, p, REPLAY_DTP, REPLAY_ACC, SAVE_FIXED)[0]["u"]
    print(f"saveat fixed {name}: saved states {rel(got['u'], ref):.3e}, per time {[float('%.2e' % rel(got['u'][:, i], ref[:, i])) for i in range(T)]}")
    assert rel(got["u"], ref) <= 2e-4
    if name != "two_pass":      # (softplus: the oracle has no such activation; the sweep over wide chains is cases 2 and 7)
        ubar = saved_cotangent((B, T, D))
        for flags in ((0, 0), (1, 1)):
            set_tracking(node, *flags)
            arm(node, REPLAY_DTP, REPLAY_ACC)
            g = node.forward_saveat(x, p, SAVE_FIXED, keep_tape=True)
            assert np.array_equal(g["u"], got["u"]) and np.array_equal(g["steps"], got["steps"])
            svbar = np.ones(len(g["saveval"]), np.float32)
            dev = node.backward(ubar, svbar)
            check_gradient(f"fixed {name}", dims, acts, td, x, p, REPLAY_DTP, REPLAY_ACC, SAVE_FIXED, flags, ubar, svbar, dev)
            if flags == (0, 0):
                assert tuple(dev[2]) == (0.0, 0.0)
            else:
                assert np.abs(dev[2]).max() > 0.0
    node.close()


# ---- 2. the adaptive solve ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", list(ADAPTIVE))
def test_adaptive_saved_states_and_tracked_gradient(key):
    dims, acts, td, p, x = adaptive_case(key)
    B, D, T = x.shape[0], dims[0], len(SAVE_ADAPT)
    node = _node(dims, acts, td, B)
    end = node.forward(x, p)
    ext_end = attempts_ext(node)
    gradients = {}
    for flags in ((1, 1), (1, 0)):
        set_tracking(node, *flags)
        got = node.forward_saveat(x, p, SAVE_ADAPT, keep_tape=True)
        ext = attempts_ext(node)
        assert np.array_equal(ext[:, 4], ext_end[:, 4])                       # the condition: the same accept / reject sequence
        assert ext.tobytes() == ext_end.tobytes()                             # and the assertion: the same attempts, bit for bit
        assert np.array_equal(got["u"][:, -1], end["u"]) and np.array_equal(got["saveval"], end["saveval"])
        dtp, acc = ext[:, 2], ext[:, 4].astype(np.int32)
        ends = [float(a[0] + a[1]) for a in ext if a[4]]
        starts = [float(a[0]) for a in ext if a[4]]
        per_step = [sum(1 for ts in SAVE_ADAPT if lo < ts <= hi) for lo, hi in zip(starts, ends)]
        assert max(per_step) >= 2, "no accepted step holds two save times: pick other times"
        assert all(abs(float(ts) - e) > 1e-3 for ts in SAVE_ADAPT[1:-1] for e in ends), "an interior save time within 1e-3 of a step's end"
        if flags == (1, 1):
            r64, _, s64 = oracle_saved(dims, acts, td, np.float64, flags, x, p, dtp, acc, SAVE_ADAPT)
            assert all(not 0.9 <= float(e) <= 1.1 for e in s64[:, 3]), "an EEst of the fp64 oracle within rounding of the accept threshold"
            print(f"saveat adaptive {key}: {len(ext)} attempts, {int((1 - acc).sum())} rejected, save times per step {per_step}, "
                  f"saved states {rel(got['u'], r64['u']):.3e}")
            assert rel(got["u"], r64["u"]) <= 2e-4
        ubar = saved_cotangent((B, T, D))
        for lab, svbar in (("saved states only", None), ("saved states and values", np.ones(len(got["saveval"]), np.float32))):
            dev = node.backward(ubar, svbar)
            bounds, g64, _ = check_gradient(f"adaptive {key}, {lab}", dims, acts, td, x, p, dtp, acc, SAVE_ADAPT, flags, ubar, svbar, dev)
            gradients[(flags, lab)] = (bounds, g64)
    node.close()
    # the two sweeps are different gradients of the saved points alone, so the test can tell them apart (fp64 oracle, the device's attempts)
    bounds, g11 = gradients[((1, 1), "saved states only")]
    _, g00, _ = oracle_saved(dims, acts, td, np.float64, (0, 0), x, p, dtp, acc, SAVE_ADAPT, saved_cotangent((B, T, D)), None)
    d = rel(g00[0], g11[0])
    print(f"saveat adaptive {key}: fp64 x-bar (0, 0) against (1, 1) {d:.3e}, bound {bounds[0]:.3e}")
    if key in ("pad_td_rej", "wide_state"):
        assert d >= 5.0 * bounds[0]


# ---- 3. bits ------------------------------------------------------------------------------------------------------------------------------------

def test_saving_runs_are_bit_identical_and_leave_no_trace():
    from regneuralde_jl_amd import _lib
    dims, acts, td, p, x = adaptive_case("pad_td")
    B, D, T = x.shape[0], dims[0], len(SAVE_ADAPT)
    ubar, xb1 = saved_cotangent((B, T, D)), np.ones_like(x)
    runs = []
    for mb in (37, 37, 64):
        node = _node(dims, acts, td, mb)
        set_tracking(node, 1, 1)
        g = node.forward_saveat(x, p, SAVE_ADAPT, keep_tape=True)
        runs.append((g, node.backward(ubar, np.ones(len(g["saveval"]), np.float32))))
        node.close()
    for g, b in runs[1:]:
        assert all(np.array_equal(g[k], runs[0][0][k]) for k in ("u", "saveval", "steps"))
        assert all(np.array_equal(u, v) for u, v in zip(b, runs[0][1]))
    fresh = _node(dims, acts, td, 37, reserve=None)
    assert fresh.L.rnde_node_tiled_saveat_capacity(fresh.h) == 0
    f = fresh.forward(x, p, keep_tape=True)
    fb = fresh.backward(xb1, np.ones(len(f["saveval"]), np.float32))
    assert np.array_equal(runs[0][0]["u"][:, -1], f["u"])      # the saving solve's last point (t1) is the end state
    node = _node(dims, acts, td, 37)
    assert node.L.rnde_node_tiled_saveat_capacity(node.h) == 8
    for step in ("reserved", "after a saving call", "released"):
        if step == "after a saving call":
            node.forward_saveat(x, p, SAVE_ADAPT, keep_tape=True)
            node.backward(ubar, None)
        if step == "released":
            node.L.rnde_node_release_tape(node.h)
            _lib.check(node.h, node.L.rnde_node_tiled_reserve_saveat(node.h, 0))
            assert node.L.rnde_node_tiled_saveat_capacity(node.h) == 0
        g = node.forward(x, p, keep_tape=True)
        b = node.backward(xb1, np.ones(len(g["saveval"]), np.float32))
        assert all(np.array_equal(g[k], f[k]) for k in ("u", "saveval", "steps")), step
        assert all(np.array_equal(u, v) for u, v in zip(b, fb)), step
    for n in (node, fresh):      # the pinned refusal is back / never left
        n.L.rnde_node_release_tape(n.h)
        with pytest.raises(_lib.RndeError) as e:
            n.forward_saveat(x, p, SAVE_ADAPT)
        assert e.value.status == _lib.BAD_ARG and PINNED_REFUSAL in str(e.value) and "tiled engine" in str(e.value)
        n.close()


# ---- 4. the agent-scope meeting ------------------------------------------------------------------------------------------------------------------

def test_saving_solve_and_tracked_sweep_over_33_tiles():
    dims, acts, td, p, _ = adaptive_case("pad_td")
    x = np.random.default_rng(528).uniform(-1.0, 1.0, (528, dims[0])).astype(np.float32)      # (the input of the tracked 33-tile test)
    node = _node(dims, acts, td, 528)
    set_tracking(node, 1, 1)
    got = node.forward_saveat(x, p, SAVE_ADAPT, keep_tape=True)
    ext = attempts_ext(node)
    ubar, svbar = saved_cotangent(got["u"].shape), np.ones(len(got["saveval"]), np.float32)
    dev = node.backward(ubar, svbar)
    node.close()
    dtp, acc = ext[:, 2], ext[:, 4].astype(np.int32)
    r64 = oracle_saved(dims, acts, td, np.float64, (1, 1), x, p, dtp, acc, SAVE_ADAPT)[0]
    print(f"saveat 33 tiles: saved states {rel(got['u'], r64['u']):.3e}")
    assert rel(got["u"], r64["u"]) <= 2e-4
    check_gradient("33 tiles", dims, acts, td, x, p, dtp, acc, SAVE_ADAPT, (1, 1), ubar, svbar, dev)


# ---- 5. save_everystep ---------------------------------------------------------------------------------------------------------------------------

def _everystep(node, x, p, save_start, capacity, keep_tape=False):
    B, D = x.shape
    xd, pd = node.dev(x), node.dev(p)
    out = torch.zeros((B * capacity * D,), dtype=torch.float32, device="cuda")
    th, n, nfe, nsv = (C.c_float * capacity)(), C.c_int32(-1), C.c_int64(0), C.c_int32(0)
    sv = (C.c_float * (node.cfg.max_attempts + 1))()
    st = node.L.rnde_node_forward_everystep(node.h, xd.data_ptr(), pd.data_ptr(), B, 0.0, 1.0, int(save_start), out.data_ptr(), capacity, th, C.byref(n),
                                            C.byref(nfe), sv, C.byref(nsv), int(keep_tape), None)
    u = out[: B * max(n.value, 0) * D].reshape(B, max(n.value, 0), D).cpu().numpy() if st == 0 else None
    return st, n.value, np.array(th[: max(n.value, 0)], dtype=np.float32) if st == 0 else None, u


def test_save_everystep():
    from regneuralde_jl_amd import _lib
    dims, acts, td, p, x = adaptive_case("pad_td_rej")
    node = _node(dims, acts, td, x.shape[0], reserve=64)
    end = node.forward(x, p)
    n_acc = int(end["steps"][:, 3].sum())
    assert n_acc < end["nattempts"]      # the natural rejection of this case
    ends = np.array([min(np.float32(s[0]) + np.float32(s[1]), np.float32(1.0)) for s in end["steps"] if s[3]], dtype=np.float32)
    for save_start in (1, 0):
        st, n, times, u = _everystep(node, x, p, save_start, 64, keep_tape=True)
        _lib.check(node.h, st)
        assert n == n_acc + save_start
        assert np.array_equal(times, np.concatenate([[np.float32(0.0)], ends]) if save_start else ends)
        assert np.array_equal(u[:, -1], end["u"])
        xb, pb, _ = node.backward(saved_cotangent(u.shape), None)
        assert np.isfinite(xb).all() and np.isfinite(pb).all() and np.abs(pb).max() > 0.0
        at = node.forward_saveat(x, p, times)
        assert np.array_equal(at["u"], u)      # a step end is a copy of unew in both calls
        st, n_short, _, _ = _everystep(node, x, p, save_start, n - 1)
        assert st == _lib.BAD_ARG and n_short == n
    node.L.rnde_node_release_tape(node.h)
    _lib.check(node.h, node.L.rnde_node_tiled_reserve_saveat(node.h, n_acc))      # the handle's own capacity one short of save_start's count
    st, n_short, _, _ = _everystep(node, x, p, 1, 64)
    assert st == _lib.BAD_ARG and n_short == n_acc + 1
    msg = node.L.rnde_last_error(node.h).decode()
    assert str(n_acc + 1) in msg and f"capacity of {n_acc}" in msg, msg
    node.close()


# ---- 6. refusals by name -------------------------------------------------------------------------------------------------------------------------

def test_refusals_by_name():
    from regneuralde_jl_amd import _lib
    from tests.util import Node
    dims, acts, td, p, x = case("pad_td", 5)
    node = _node(dims, acts, td, 5, reserve=None)
    L, h = node.L, node.h

    def refused(status, handle, *words):
        assert status == _lib.BAD_ARG
        msg = L.rnde_last_error(handle).decode()
        assert all(w in msg for w in words), msg

    assert L.rnde_node_tiled_saveat_capacity(h) == 0 and L.rnde_node_tiled_saveat_capacity(None) == -1
    refused(L.rnde_node_tiled_reserve_saveat(h, -1), h, "rnde_node_tiled_reserve_saveat", "max_saveat = -1", "0..129")
    refused(L.rnde_node_tiled_reserve_saveat(h, 130), h, "rnde_node_tiled_reserve_saveat", "max_saveat = 130", "max_attempts + 1")
    assert L.rnde_node_tiled_reserve_saveat(h, 129) == _lib.OK and L.rnde_node_tiled_saveat_capacity(h) == 129
    assert L.rnde_node_tiled_reserve_saveat(h, 3) == _lib.OK and L.rnde_node_tiled_saveat_capacity(h) == 3
    node.forward(x, p, keep_tape=True)
    refused(L.rnde_node_tiled_reserve_saveat(h, 4), h, "rnde_node_tiled_reserve_saveat", "holds a tape")
    refused(L.rnde_node_tiled_reserve_saveat(h, 0), h, "rnde_node_tiled_reserve_saveat", "holds a tape")
    assert L.rnde_node_tiled_saveat_capacity(h) == 3
    L.rnde_node_release_tape(h)
    with pytest.raises(_lib.RndeError) as e:
        node.forward_saveat(x, p, np.array([0.25, 0.5, 0.75, 1.0], np.float32))
    assert e.value.status == _lib.BAD_ARG and "n_saveat = 4" in str(e.value) and "capacity of 3" in str(e.value)
    for bad in ([0.5, 0.2], [0.5, 1.5], [-0.1, 0.3]):
        with pytest.raises(_lib.RndeError, match="increasing and inside"):
            node.forward_saveat(x, p, np.array(bad, np.float32))
    node.forward_saveat(x, p, np.array([0.25, 0.5, 1.0], np.float32))
    node.close()
    chain = Node(make_cfg(dims, acts, td, 5, track_ctrl=1, track_initdt=1))      # a handle of rnde_node_create
    refused(L.rnde_node_tiled_reserve_saveat(chain.h, 4), chain.h, "rnde_node_tiled_reserve_saveat", "rnde_node_create_tiled")
    assert L.rnde_node_tiled_saveat_capacity(chain.h) == -1
    chain.close()


# ---- 7. the Python layer -------------------------------------------------------------------------------------------------------------------------

def test_python_layer_saveat_and_everystep():
    import regneuralde_jl_amd as rn
    from regneuralde_jl_amd import _lib
    g = torch.Generator().manual_seed(31)
    B, sa = 16, [0.0, 0.3, 0.31, 1.0]
    model = rn.TDChain(rn.Dense(3, 128, "tanh", g), rn.Dense(129, 128, "tanh", g), rn.Dense(129, 2, "identity", g))
    kw = dict(engine="tiled", track_ctrl=False, track_initdt=False, reltol=TOL, abstol=TOL, max_batch=B, tiled_max_saveat=8)
    node = rn.TrackedNeuralODE(model, [0, 1], True, True, saveat=sa, **kw)
    x = torch.randn(B, 2, generator=g)
    ref = tiled(node._config(0, None))
    _lib.check(ref.h, ref.L.rnde_node_tiled_reserve_saveat(ref.h, 8))
    for flags in ((0, 0), (1, 1)):
        node.set_tracking(*flags)
        set_tracking(ref, *flags)
        xd, pd = x.cuda().requires_grad_(True), node.p.cuda().requires_grad_(True)
        u, nfe, sv = node(xd, pd)
        assert u.shape == (B, len(sa), 2)
        r = ref.forward_saveat(x.numpy(), node.p.cpu().numpy(), np.array(sa, np.float32), keep_tape=True)
        assert r["nfe"] == nfe and np.array_equal(r["u"], u.detach().cpu().numpy()) and np.array_equal(r["saveval"], sv.saveval.detach().cpu().numpy())
        w = torch.from_numpy(saved_cotangent(tuple(u.shape))).cuda()
        ((u * w).sum() + sv.saveval.sum()).backward()
        xb, pb, tsb = ref.backward(w.cpu().numpy(), np.ones(len(r["saveval"]), np.float32))
        assert rel(xd.grad.cpu().numpy(), xb) <= 1e-6 and rel(pd.grad.cpu().numpy(), pb) <= 1e-6
        assert node.last_tspan_bar == (float(tsb[0]), float(tsb[1])) and (node.last_tspan_bar != (0.0, 0.0)) == (flags == (1, 1))
    with torch.no_grad():
        u2, _, _ = node(x.cuda(), saveat=[0.5, 1.0])      # the per-call override; the stored times are restored
        assert u2.shape == (B, 2, 2) and node.kwargs["saveat"] == sa
        r2 = ref.forward_saveat(x.numpy(), node.p.cpu().numpy(), np.array([0.5, 1.0], np.float32))
        assert np.array_equal(r2["u"], u2.cpu().numpy())
        with pytest.raises(ValueError, match="9 save times"):
            node(x.cuda(), saveat=np.linspace(0.0, 1.0, 9).tolist())
        every = rn.TrackedNeuralODE(model, [0, 1], True, True, save_everystep=True, **dict(kw, tiled_max_saveat=129))
        ue, _, _ = every(x.cuda(), node.p.cuda())
        n_acc = int(r["steps"][:, 3].sum())
        assert ue.shape == (B, n_acc + 1, 2) and len(every.last_times) == n_acc + 1 and every.last_times[0] == 0.0 and every.last_times[-1] == 1.0
        assert torch.equal(ue[:, 0], x.cuda()) and np.array_equal(ue[:, -1].cpu().numpy(), r["u"][:, -1])
    ref.close()
    assert all(_lib.lib().rnde_node_tiled_saveat_capacity(h.ptr) == 8 for hs in node._handles.values() for h in hs)


def test_latent_time_series_model_over_a_wide_tiled_node():
    """LatentTimeSeriesModel takes the layer as built: a 128-wide latent dynamics, refused by the default engines for its width and by the
    tiled engine without a capacity for saveat, runs and differentiates."""
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(5)
    latent, B, Tn = 20, 4, 7
    grid = np.linspace(0.0, 1.0, Tn).astype(np.float32)
    dyn = rn.Chain(rn.Dense(latent, 128, "tanh", g), rn.Dense(128, latent, "identity", g))
    node = rn.TrackedNeuralODE(dyn, [0.0, 1.0], False, True, engine="tiled", track_ctrl=False, track_initdt=False, reltol=1e-3, abstol=1e-3,
                               max_batch=B, saveat=grid.tolist(), tiled_max_saveat=Tn)
    base = rn.build_latent_ode(saveat=grid.tolist(), generator=g, reltol=1e-3, abstol=1e-3, max_batch=B, max_attempts=64)
    model = rn.LatentTimeSeriesModel(base.rnn, base.enc, node, base.dec.layers[0])
    in_dim = base.dec.layers[0].n_out
    xin = torch.randn(B, Tn, 2 * in_dim + 1, generator=g).cuda()
    result, mu0, logvar, nfe, sv = model(xin, generator=None)
    assert result.shape == (B, Tn, in_dim) and nfe > 0
    (result.sum() + sv.saveval.sum()).backward()
    assert model.p3.grad is not None and torch.isfinite(model.p3.grad).all() and model.p3.grad.abs().max() > 0
