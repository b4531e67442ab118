"""The tracked-controller reverse sweep of the tiled TrackedFFJORD engines (rnde_ffjord_set_track_ctrl; engines 1 and 2) on the device, against
tests/ffjord_track_ref.py along the device's own step log (that restatement is pinned to the fp64 oracle in tests/test_ffjord_track_host.py).

Cases: the chain TD [2, 10, 2] tanh / identity, the plain chain [3, 7, 3] softplus / identity and the ConcatSquash (2, 16), each at B = 5 (one
tile) and B = 20 (two tiles: the meeting carries real sums), tol 1e-5, free-running solves, fixed probes.  Cotangents: 1 on every saved value
and standard normals times 0.02 / B on logpx -- the ratio of the training tools' loss -mean(logpx) + lambda mean(saveval) at lambda = 1e3 and
some 20 saved values, normalised to a saved-value cotangent of 1.

Every case is vetted on the CPU and the test asserts the vetting conditions on the device's own log, replayed in fp64: no EEst in [0.9, 1.1],
no q / gamma within 5 % of a clip bound, and for each dynamics one case with a natural rejection.

Bound of the comparison: max(1e-3, 4 x the fp32 restatement's distance from the fp64 one) per case, formed in the test (the device's matrix
cores associate differently from torch, hence the 4).  The figure is large where the first steps of a solve have an EEst below fp32's floor
for it (some 6e-3 dt |k|): their contribution to the gradient of sum EEst dt is rounding in any fp32 evaluation, the restatement's and the
device's alike.  Measured on an MI355X along the device's own logs, fp32 restatement (p-bar / x-bar) | device against fp64 (p-bar / x-bar):
  td2-B5   34 attempts, 3 rejected   3.7e-2 / 2.9e-2 | 5.1e-2 / 4.9e-2        td2-B20  29 attempts                1.2e-2 / 1.6e-2 | 3.0e-2 / 3.4e-2
  sp3-B5   25 attempts, 2 rejected   1.1e-2 / 7.5e-3 | 1.1e-2 / 6.3e-3        sp3-B20  24 attempts                1.2e-2 / 9.6e-3 | 5.2e-3 / 2.6e-3
  cs-B5    30 attempts, 4 rejected   1.0e-3 / 9.8e-4 | 8.0e-4 / 1.4e-3        cs-B20   20 attempts                4.9e-4 / 5.0e-4 | 4.6e-4 / 1.0e-3
  exact td2x-B5  40 attempts, 5 rejected  7.1e-2 / 7.0e-2 | 5.4e-3 / 1.9e-2   replay sp3-B5  5 attempts, 1 rejected  5.3e-4 / 3.8e-4 | 2.5e-4 / 2.0e-4
  td2-B528 58 attempts                5.0e-3 / 3.2e-3 | 9.4e-3 / 2.7e-3
The constant-step sweep on the same inputs is more than 10 x the bound from the tracked reference in p-bar (measured 2.03, 0.79, 0.74, 2.02, 0.110,
0.106 against 10 x bound 1.48, 0.46, 0.44, 0.48, 0.041, 0.020); with saved-value cotangents 0 the two sweeps lie within the bound of each other
(measured 4e-6 ... 1.9e-3).  The cases were picked on the CPU so that this holds along the fp64 and along the fp32 controller's log: the fp32
figure moves by up to 10 x between two logs that differ in the last digits, so a case with a small margin on one log is not kept.  The layer
equals the ABI path bit for bit at either setting."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import act_ref as A
from tests import ffjord_chain_ref as CR
from tests import ffjord_ref as R
from tests import ffjord_track_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
TD2 = ("chain", [2, 10, 2], ["tanh", "identity"], True)
SP3 = ("chain", [3, 7, 3], ["softplus", "identity"], False)
CS = ("cs", 2, 16)
# name: (dynamics, recipe, seed, B).  Chain recipe: per-layer factors on act_ref.params(bias = 0.3) (a fast right-hand side of modest size keeps the
# solve error-limited: tests/test_gpu_node_tiled.py), x uniform in [-1, 1].  ConcatSquash recipe: (scale of ffjord_ref.glorot_params, scale of x).
CASES = {
    "td2-B5": (TD2, (60.0, 0.3), 5, 5),
    "td2-B20": (TD2, (30.0, 0.3), 9, 20),
    "sp3-B5": (SP3, (40.0, 0.3), 2, 5),
    "sp3-B20": (SP3, (40.0, 0.3), 1, 20),
    "cs-B5": (CS, (5.0, 2.0), 15, 5),
    "cs-B20": (CS, (6.0, 1.0), 1, 20),
    "td2-B528": (TD2, (120.0, 0.1), 3, 528),
    "td2x-B5": (TD2, (120.0, 0.1), 3, 5),            # the exact-trace case (td2-B5's exact solve has an EEst of 0.906)
}
FREE = ["td2-B5", "td2-B20", "sp3-B5", "sp3-B20", "cs-B5", "cs-B20"]
REJECTING = ["td2-B5", "sp3-B5", "cs-B5"]            # (vetted: these contain a natural rejection)
REPLAY_DTP, REPLAY_ACC = [0.25, 0.5, 0.25, 0.25, 0.25], [1, 0, 1, 1, 1]


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    dyn, recipe, seed, B = CASES[name]
    rng = np.random.default_rng(seed)
    if dyn[0] == "chain":
        _, dims, acts, td = dyn
        p = A.params(dims, td, rng, bias=0.3)
        o = 0
        for l, f in enumerate(recipe):
            n = (dims[l] + (1 if td else 0)) * dims[l + 1] + dims[l + 1]
            p[o:o + n] *= f
            o += n
        D = dims[0]
        x = rng.uniform(-1.0, 1.0, (B, D)).astype(np.float32)
    else:
        D = dyn[1]
        p = R.glorot_params(dyn[1], dyn[2], rng, recipe[0])
        x = (rng.standard_normal((B, D)) * recipe[1]).astype(np.float32)
    e = rng.standard_normal((B, D)).astype(np.float32)
    g = (np.random.default_rng(1000 + seed).standard_normal(B) * 0.02 / B).astype(np.float32)
    return tuple(torch.from_numpy(v) for v in (p, x, e, g))


def _rhs(dyn, P, E):
    if dyn[0] == "chain":
        _, dims, acts, td = dyn
        return lambda u, t: T.chain_rhs(dims, acts, td, P, u, t, E)
    return lambda u, t: R.rhs(P, dyn[1], dyn[2], u, t, E)


class Handle:
    """One rnde_ffjord handle of engine 1 or 2 through the C ABI."""

    def __init__(self, dyn, max_batch, regularize=1, track=None, engine0=False, max_attempts=512):
        import regneuralde_jl_amd as rn
        self.rn, self.L, self.h = rn, rn._lib.lib(), C.c_void_p()
        self.max_attempts = max_attempts
        if dyn[0] == "chain":
            cfg = rn._lib.FfjordChainConfig()
            cfg.n_layers = len(dyn[2])
            for i, d in enumerate(dyn[1]):
                cfg.dims[i] = d
            for i, a in enumerate(dyn[2]):
                cfg.act[i] = rn.layers.act_code(a)
            cfg.time_dep = int(dyn[3])
            create = self.L.rnde_ffjord_create_chain
            self.D = dyn[1][0]
        else:
            cfg = rn._lib.FfjordConfig()
            cfg.in_dims, cfg.hidden, cfg.dynamics, cfg.time_dep, cfg.kinetic_reg = dyn[1], dyn[2], 0, 1, 0
            create = self.L.rnde_ffjord_create if engine0 else self.L.rnde_ffjord_create_tiled
            self.D = dyn[1]
        cfg.regularize, cfg.max_batch, cfg.solver, cfg.reltol, cfg.abstol = regularize, max_batch, 0, TOL, TOL
        cfg.cb_save_start, cfg.max_attempts, cfg.device = 1, max_attempts, 0
        rn._lib.check_ffjord(None, create(C.byref(cfg), C.byref(self.h)))
        if track is not None:
            self.set_track(track)

    def close(self):
        if self.h:
            self.L.rnde_ffjord_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_track(self, on):
        """(status, message)"""
        st = self.L.rnde_ffjord_set_track_ctrl(self.h, on)
        return st, self.L.rnde_ffjord_last_error(self.h).decode()

    def forward(self, x, p, e=None, steps=None, keep=1):
        """Hutchinson (e given) or exact-trace (e None) forward, free-running or along steps = [(dt, accepted), ...]; keeps x, p, e alive."""
        self.x, self.p, self.e = x.to(DEV).contiguous(), p.to(DEV).contiguous(), (None if e is None else e.to(DEV).contiguous())
        B = x.shape[0]
        self.B = B
        logpx = torch.empty(B, device=DEV)
        nfe, nsv, sv = C.c_int64(), C.c_int32(), (C.c_float * (self.max_attempts + 1))()
        arr = None if steps is None else (C.c_float * (2 * len(steps)))(*[float(v) for s in steps for v in s])
        L, h = self.L, self.h
        if e is None and steps is None:
            st = L.rnde_ffjord_forward_exact(h, self.x.data_ptr(), self.p.data_ptr(), B, 0.0, 1.0, logpx.data_ptr(), None, C.byref(nfe), sv, C.byref(nsv), keep, None)
        elif e is None:
            st = L.rnde_ffjord_forward_exact_replay(h, self.x.data_ptr(), self.p.data_ptr(), B, 0.0, 1.0, arr, len(steps), logpx.data_ptr(), None,
                                                    C.byref(nfe), sv, C.byref(nsv), keep, None)
        elif steps is None:
            st = L.rnde_ffjord_forward(h, self.x.data_ptr(), self.p.data_ptr(), self.e.data_ptr(), B, 0.0, 1.0, 0, logpx.data_ptr(), None, C.byref(nfe),
                                       sv, C.byref(nsv), keep, None)
        else:
            st = L.rnde_ffjord_forward_replay(h, self.x.data_ptr(), self.p.data_ptr(), self.e.data_ptr(), B, 0.0, 1.0, 0, arr, len(steps),
                                              logpx.data_ptr(), None, C.byref(nfe), sv, C.byref(nsv), keep, None)
        self.rn._lib.check_ffjord(h, st)
        self.nsv = nsv.value
        n = C.c_int32()
        self.rn._lib.check_ffjord(h, L.rnde_ffjord_step_log(h, None, 0, C.byref(n)))
        log = (C.c_float * max(4 * n.value, 1))()
        self.rn._lib.check_ffjord(h, L.rnde_ffjord_step_log(h, log, n.value, C.byref(n)))
        log = np.array(log[:4 * n.value], dtype=np.float32).reshape(-1, 4)
        return logpx, np.array(sv[:nsv.value], dtype=np.float32), [(float(r[0]), float(r[1]), int(r[3])) for r in log]

    def backward(self, g, sv_bar):
        """(p-bar, x-bar) for the logpx cotangent g and the cotangent sv_bar on every saved value."""
        g = g.to(DEV).contiguous()
        svb = (C.c_float * max(self.nsv, 1))(*([float(sv_bar)] * self.nsv))
        pb, xb = torch.empty_like(self.p), torch.empty_like(self.x)
        st = self.L.rnde_ffjord_backward(self.h, g.data_ptr(), svb, pb.data_ptr(), xb.data_ptr(), None)
        self.rn._lib.check_ffjord(self.h, st)
        torch.cuda.synchronize()
        return pb.cpu(), xb.cpu()

    def reverse_ms(self):
        b = C.c_float()
        self.rn._lib.check_ffjord(self.h, self.L.rnde_ffjord_timing(self.h, None, C.byref(b), None, None))
        return b.value


@functools.lru_cache(maxsize=None)
def _device(name, track, exact=False, replay=False, max_batch=None, run=0):
    """One taped forward and two reverse sweeps (saved-value cotangents 1 and 0) on a fresh handle with the given setting (run: a second,
    separately cached run of the same thing)."""
    dyn, _, _, B = CASES[name]
    p, x, e, g = _inputs(name)
    hd = Handle(dyn, max_batch or B, track=track)
    steps = list(zip(REPLAY_DTP, REPLAY_ACC)) if replay else None
    logpx, sv, log = hd.forward(x, p, None if exact else e, steps)
    out = dict(logpx=logpx.cpu(), sv=sv, log=log, g1=hd.backward(g, 1.0), g0=hd.backward(g, 0.0), ms=hd.reverse_ms())
    hd.close()
    return out


def reference_along(name, dtype, log, exact=False, replay=False):
    """The restatement along `log` in `dtype`: p-bar, x-bar for saved-value cotangents 1 and 0, and the vetting figures.  The fp32 run (the
    rounding yardstick) takes the accept decisions from the log."""
    dyn, _, _, B = CASES[name]
    p, x, e, g = _inputs(name)
    P, X = p.clone().to(dtype).requires_grad_(True), x.clone().to(dtype).requires_grad_(True)      # (clones: _inputs is cached)
    F = _rhs(dyn, P, None if exact else e.to(dtype))
    kw = dict(accept_from_log=True, next_dtp=REPLAY_DTP) if replay else dict(accept_from_log=dtype != torch.float64)
    u, eests, dts, info = T.solve_tracked(F, CR.aug(X), 0.0, 1.0, log, TOL, TOL, **kw)
    lp = (R.logpx_of(u, x.shape[1]) * g.to(dtype)).sum()
    sv = sum(T.saved_values(eests, dts, info["accepted"]))
    gx0, gp0 = torch.autograd.grad(lp, (X, P), retain_graph=True)
    gx1, gp1 = torch.autograd.grad(lp + sv, (X, P))
    ee = [float(v.detach()) for v in eests]
    clip = min(min(abs(q / (1.0 / R.QMAX) - 1.0), abs(q / (1.0 / R.QMIN) - 1.0)) for q in info["qg"] if q is not None)
    return dict(g1=(gp1, gx1), g0=(gp0, gx0), eests=ee, clip=clip, accepted=info["accepted"])


@functools.lru_cache(maxsize=None)
def _reference(name, dtype, exact=False, replay=False):
    """reference_along the device's own log."""
    return reference_along(name, dtype, _device(name, 1, exact, replay)["log"], exact, replay)


def _bounds(name, **kw):
    """(bound on p-bar, bound on x-bar, the CPU figures): max(1e-3, 4 x fp32 against fp64 restatement)."""
    r64, r32 = _reference(name, torch.float64, **kw), _reference(name, torch.float32, **kw)
    fig = (_rel(r32["g1"][0], r64["g1"][0]), _rel(r32["g1"][1], r64["g1"][1]))
    return max(1e-3, 4 * fig[0]), max(1e-3, 4 * fig[1]), fig


def _vetted(name, **kw):
    r = _reference(name, torch.float64, **kw)
    assert all(not (0.9 <= v <= 1.1) for v in r["eests"]), ("an EEst within 0.1 of the accept threshold: pick another seed", r["eests"])
    assert r["clip"] >= 0.05, ("q / gamma within 5 % of a clip bound: pick another seed", r["clip"])
    return r


def _check_tracked(name, **kw):
    ref = _vetted(name, **kw)
    bp, bx, fig = _bounds(name, **kw)
    got = _device(name, 1, **kw)
    devs = (_rel(got["g1"][0], ref["g1"][0]), _rel(got["g1"][1], ref["g1"][1]))
    print(f"{name} {kw}: attempts {len(got['log'])} rejected {ref['accepted'].count(False)} fp32 restatement p-bar / x-bar {fig[0]:.3e} / {fig[1]:.3e} "
          f"bounds {bp:.3e} / {bx:.3e} device {devs[0]:.3e} / {devs[1]:.3e} reverse {got['ms']:.3f} ms")
    assert devs[0] <= bp and devs[1] <= bx, (devs, bp, bx)
    return ref, got, bp, bx


# ---- 5. the tracked gradient against the reference ----
@pytest.mark.parametrize("name", FREE)
def test_tracked_gradient_matches_reference(name):
    """p-bar and x-bar for (logpx cotangent random, saved-value cotangents 1) along the device's own step log, under max(1e-3, 4 x the fp32
    restatement's distance from fp64).  Figures: the module docstring."""
    ref, got, _, _ = _check_tracked(name)
    if name in REJECTING:
        assert False in ref["accepted"]              # the natural rejection this case was chosen for
    assert got["sv"][0] == 0.0 and len(got["sv"]) == 1 + ref["accepted"].count(True)


# ---- 6. the comparison tells the two sweeps apart ----
@pytest.mark.parametrize("name", FREE)
def test_constant_step_sweep_is_far_and_agrees_without_saved_value_cotangents(name):
    """On the same inputs the constant-step sweep (setting 0) is more than 10 x the bound from the tracked reference in p-bar; with saved-value
    cotangents 0 the two device sweeps lie within the bound of each other (the log-likelihood gradient does not depend on the setting beyond
    O(tol))."""
    ref = _vetted(name)
    bp, bx, _ = _bounds(name)
    trk, const = _device(name, 1), _device(name, 0)
    assert trk["log"] == const["log"] and torch.equal(trk["logpx"], const["logpx"])
    far = _rel(const["g1"][0], ref["g1"][0])
    near = (_rel(trk["g0"][0], const["g0"][0]), _rel(trk["g0"][1], const["g0"][1]))
    print(f"{name}: constant-step p-bar against the tracked reference {far:.3e} (10 x bound {10 * bp:.3e}); saved-value cotangents 0, tracked "
          f"against constant p-bar / x-bar {near[0]:.3e} / {near[1]:.3e}")
    assert far > 10 * bp, (far, bp)
    assert near[0] <= bp and near[1] <= bx, (near, bp, bx)


# ---- 7. the exact-trace tape ----
def test_exact_trace_tape():
    ref, _, _, _ = _check_tracked("td2x-B5", exact=True)
    assert False in ref["accepted"]


# ---- 8. a replayed sequence with a forced rejection ----
def test_replayed_sequence_with_a_forced_rejection():
    """rnde_ffjord_forward_replay along REPLAY_DTP / REPLAY_ACC: differentiated as if the controller had produced the sequence (the restatement in
    its straight-through form: every proposed step tied to the replayed value, the accept decisions the sequence's)."""
    ref, got, _, _ = _check_tracked("sp3-B5", replay=True)
    assert [a[2] for a in got["log"]] == REPLAY_ACC and [a[1] for a in got["log"]] == REPLAY_DTP


# ---- 9. determinism and the wide meeting ----
def test_runs_are_bit_identical_also_under_a_larger_max_batch():
    a = _device("td2-B20", 1)
    b = _device("td2-B20", 1, run=1)
    c = _device("td2-B20", 1, max_batch=300)
    for other in (b, c):
        assert a["log"] == other["log"]
        assert all(torch.equal(u, v) for k in ("g1", "g0") for u, v in zip(a[k], other[k]))


def test_agent_scope_meeting_at_33_tiles():
    """B = 528: 33 tiles meet at agent scope.  p-bar over the whole batch and x-bar of the first 48 columns against the restatement."""
    name = "td2-B528"
    ref = _vetted(name)
    bp, bx, fig = _bounds(name)
    got = _device(name, 1)
    devs = (_rel(got["g1"][0], ref["g1"][0]), _rel(got["g1"][1][:48], ref["g1"][1][:48]))
    print(f"{name}: attempts {len(got['log'])} fp32 restatement {fig[0]:.3e} / {fig[1]:.3e} device {devs[0]:.3e} / {devs[1]:.3e} reverse {got['ms']:.3f} ms")
    assert devs[0] <= bp and devs[1] <= bx, (devs, bp, bx)


# ---- 10. the C entry points ----
def test_c_refusals_and_default_bits():
    import regneuralde_jl_amd as rn
    BAD = rn._lib.BAD_ARG
    p, x, e, g = _inputs("cs-B5")
    h0 = Handle(CS, 5, engine0=True)
    st, msg = h0.set_track(1)
    assert st == BAD and "one-workgroup engine" in msg and "rnde_ffjord_create_tiled" in msg, msg
    h0.close()
    for dyn in (CS, TD2):
        hr = Handle(dyn, 5, regularize=0)
        st, msg = hr.set_track(1)
        assert st == BAD and "regularize = 0" in msg and "O(tol)" in msg and "2e-10 to 2e-6" in msg, msg
        assert hr.L.rnde_ffjord_track_ctrl(hr.h) == 0
        hr.close()
    hd = Handle(CS, 5)
    assert hd.L.rnde_ffjord_track_ctrl(hd.h) == 0
    assert hd.set_track(2)[0] == BAD
    assert hd.set_track(1)[0] == 0 and hd.L.rnde_ffjord_track_ctrl(hd.h) == 1
    assert hd.set_track(0)[0] == 0 and hd.L.rnde_ffjord_track_ctrl(hd.h) == 0
    # setter never called against set_track_ctrl(h, 0): the same bits, forward and backward
    never = Handle(CS, 5)
    outs = []
    for handle in (never, hd):
        logpx, sv, log = handle.forward(x, p, e)
        outs.append((logpx.cpu(), sv, log) + handle.backward(g, 1.0))
    assert outs[0][2] == outs[1][2] and np.array_equal(outs[0][1], outs[1][1])
    assert all(torch.equal(outs[0][i], outs[1][i]) for i in (0, 3, 4))
    st, msg = hd.set_track(1)                        # a tape is held now
    assert st == BAD and "holds a tape" in msg, msg
    assert hd.L.rnde_ffjord_track_ctrl(hd.h) == 0
    never.close()
    hd.close()


# ---- 11. the Python layer ----
@pytest.mark.parametrize("dyn_name", ["td2-B5", "cs-B5"])
def test_python_layer_passes_the_setting_to_every_handle(dyn_name):
    import regneuralde_jl_amd as rn
    dyn, _, _, B = CASES[dyn_name]
    p, x, e, _ = _inputs(dyn_name)
    lam = 1e3
    if dyn[0] == "chain":
        _, dims, acts, td = dyn
        layers = [rn.Dense(dims[l] + (1 if td else 0), dims[l + 1], acts[l]) for l in range(len(acts))]
        model = rn.TDChain(*layers) if td else rn.Chain(*layers)
    else:
        model = rn.ffjord.MLPDynamics(dyn[1], dyn[2])
    for track in (True, False):
        ff = rn.TrackedFFJORD(model, [0.0, 1.0], True, True, "Tsit5", reltol=TOL, abstol=TOL, max_batch=B, max_attempts=512, engine="tiled",
                              track_ctrl=track)
        assert ff.track_ctrl is track
        grads = []
        for _ in range(2):                           # two taped forwards alive at once: two pooled handles, both with the setting
            xd, pd = x.to(DEV).requires_grad_(True), p.to(DEV).requires_grad_(True)
            logpx, _, _, _, sv = ff(xd, pd, e.to(DEV))
            grads.append((xd, pd, -logpx.mean() + lam * sv.saveval.mean()))
        for xd, pd, loss in grads:
            loss.backward()
        assert len(ff._pool) == 2
        assert all(rn._lib.lib().rnde_ffjord_track_ctrl(hd.h) == int(track) for hd in ff._pool + [ff._handle()])
        assert torch.equal(grads[0][1].grad, grads[1][1].grad) and torch.equal(grads[0][0].grad, grads[1][0].grad)
        # the ABI path with the same cotangents; track False: the setter is never called (today's sweep)
        hd = Handle(dyn, B, track=1 if track else None)
        logpx, sv, _ = hd.forward(x, p, e)
        lb, sb = torch.zeros(B, requires_grad=True), torch.zeros(len(sv), requires_grad=True)
        (-lb.mean() + lam * sb.mean()).backward()     # (the cotangents autograd hands the layer's backward, bit for bit)
        pb, xb = hd.backward(lb.grad, float(sb.grad[0]))
        hd.close()
        devs = (_rel(grads[0][1].grad, pb), _rel(grads[0][0].grad, xb))
        print(dyn_name, "track_ctrl", track, "layer against ABI p-bar / x-bar:", devs)
        if track:
            assert max(devs) <= 1e-6, devs
        else:
            assert torch.equal(grads[0][1].grad.cpu(), pb) and torch.equal(grads[0][0].grad.cpu(), xb)
