"""RNDE_ERR_MAX_ATTEMPTS on the three solve paths of the tile layout -- the single tiled TrackedFFJORD solve, the group call and the tiled
TrackedNeuralODE -- which share one host-side run (csrc/rnde_tile_host.h: tile_run_met, tile_fetch_log; solve_verdict of rnde_fwd_plan.h): the
status, the exact message, the attempt count, and the handle then serving a call that succeeds.

Shapes: the time-dependent chain [2, 10, 2] of tests/test_gpu_ffjord_track.py (td2-B5: its parameters, B = 5 for the single calls; groups of
1 and 17 columns) on engine 2 and on the tiled NeuralODE, and the ConcatSquash dynamics (2, 16) of the same file (cs-B5) on engine 1, which
takes the other branch of the same host path; max_attempts = 2 at reltol = abstol = 1e-8: the free-running solve over [0, 1] needs far
more than two attempts, so every path stops at the limit with two attempts in its log.  The call that succeeds is the same call over the span [0, 1e-6]: the initial-step
rule clamps the first step to the span, and a step of 1e-6 passes the tolerance (its error estimate is rounding noise of order 1e-13 against
a scale of 1e-8), so the solve ends within the two attempts the handle has."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_ffjord_track import CS, DEV, TD2, _inputs

pytestmark = pytest.mark.gpu

TOL, MAX_ATT, SHORT = 1e-8, 2, 1e-6
WORDS = "max_attempts reached"


def _lib():
    from regneuralde_jl_amd import _lib
    return _lib


FF = {"chain": ("td2-B5", TD2), "tiled": ("cs-B5", CS)}      # engine 2, engine 1: (the inputs' case, the dynamics)


def _ff_handle(engine, max_batch):
    lib = _lib()
    import regneuralde_jl_amd as rn
    h = C.c_void_p()
    if engine == "chain":
        _, dims, acts, td = TD2
        cfg, create = lib.FfjordChainConfig(), lib.lib().rnde_ffjord_create_chain
        cfg.n_layers = len(acts)
        for i, d in enumerate(dims):
            cfg.dims[i] = d
        for i, a in enumerate(acts):
            cfg.act[i] = rn.layers.act_code(a)
        cfg.time_dep = int(td)
    else:
        cfg, create = lib.FfjordConfig(), lib.lib().rnde_ffjord_create_tiled
        cfg.in_dims, cfg.hidden, cfg.dynamics, cfg.time_dep, cfg.kinetic_reg = CS[1], CS[2], 0, 1, 0
    cfg.regularize, cfg.max_batch, cfg.solver, cfg.reltol, cfg.abstol = 1, max_batch, 0, TOL, TOL
    cfg.cb_save_start, cfg.max_attempts, cfg.device = 1, MAX_ATT, 0
    lib.check_ffjord(None, create(C.byref(cfg), C.byref(h)))
    return h


def _ff_steps(h, entry, *lead):
    L, n = _lib(), C.c_int32(-1)
    assert entry(h, *lead, None, 0, C.byref(n)) == L.OK
    arr = (C.c_float * max(2 * n.value, 1))()
    assert entry(h, *lead, arr, n.value, C.byref(n)) == L.OK
    return n.value, list(arr[:2 * n.value])


@pytest.mark.parametrize("engine", ["chain", "tiled"])
def test_single_tiled_ffjord_solve_reports_max_attempts_and_serves_the_next_call(engine):
    L = _lib()
    lib = L.lib()
    p, x, e, _ = (v.to(DEV).contiguous() for v in _inputs(FF[engine][0]))
    B = x.shape[0]
    h = _ff_handle(engine, B)
    try:
        logpx = torch.full((B,), float("nan"), device=DEV)
        nfe, nsv, sv = C.c_int64(-1), C.c_int32(-1), (C.c_float * (MAX_ATT + 1))()

        def forward(t1):
            return lib.rnde_ffjord_forward(h, x.data_ptr(), p.data_ptr(), e.data_ptr(), B, 0.0, t1, 0, logpx.data_ptr(), None, C.byref(nfe), sv, C.byref(nsv), 1, None)

        assert forward(1.0) == L.MAX_ATTEMPTS
        assert lib.rnde_ffjord_last_error(h).decode() == WORDS
        n, steps = _ff_steps(h, lib.rnde_ffjord_steps)
        att, acc = C.c_int32(-1), C.c_int32(-1)
        assert lib.rnde_ffjord_timing(h, None, None, C.byref(att), C.byref(acc)) == L.OK
        assert n == MAX_ATT and att.value == MAX_ATT and acc.value == int(sum(steps[1::2]))
        # (the failed forward left no tape)
        pb, g = torch.empty_like(p), torch.zeros(B, device=DEV)
        assert lib.rnde_ffjord_backward(h, g.data_ptr(), None, pb.data_ptr(), None, None) == L.NO_TAPE
        assert forward(SHORT) == L.OK, lib.rnde_ffjord_last_error(h).decode()
        torch.cuda.synchronize()
        n, steps = _ff_steps(h, lib.rnde_ffjord_steps)
        assert 1 <= n <= MAX_ATT and steps[-1] == 1.0 and nfe.value == 3 + 6 * n and bool(torch.isfinite(logpx).all())
        assert lib.rnde_ffjord_backward(h, g.data_ptr(), None, pb.data_ptr(), None, None) == L.OK
        torch.cuda.synchronize()
        assert bool(torch.isfinite(pb).all())
    finally:
        lib.rnde_ffjord_destroy(h)


@pytest.mark.parametrize("engine", ["chain", "tiled"])
def test_group_call_reports_max_attempts_by_group_and_serves_the_next_call(engine):
    L = _lib()
    lib = L.lib()
    sizes = (1, 17)
    cols = sum(sizes)
    p = _inputs(FF[engine][0])[0].to(DEV).contiguous()
    rng = np.random.default_rng(41)
    x = torch.from_numpy(rng.uniform(-1.0, 1.0, (cols, 2)).astype(np.float32)).to(DEV)
    e = torch.from_numpy(rng.standard_normal((cols, 2)).astype(np.float32)).to(DEV)
    h = _ff_handle(engine, max(sizes))
    try:
        assert lib.rnde_ffjord_reserve_groups(h, len(sizes), 16 * 3) == L.OK, lib.rnde_ffjord_last_error(h).decode()
        logpx = torch.full((cols,), float("nan"), device=DEV)
        acc = torch.tensor([1.5, 0.0], dtype=torch.float64, device=DEV)
        before = acc.cpu().view(torch.int64).clone()
        Bs, nfe, gst = (C.c_int32 * 2)(*sizes), (C.c_int64 * 2)(-1, -1), (C.c_int32 * 2)(-1, -1)

        def groups(t1):
            return lib.rnde_ffjord_forward_groups(h, x.data_ptr(), p.data_ptr(), e.data_ptr(), 2, Bs, 0.0, t1, 0, logpx.data_ptr(), nfe, gst, acc.data_ptr(),
                                                  acc.data_ptr() + 8, None)

        assert groups(1.0) == L.MAX_ATTEMPTS
        assert lib.rnde_ffjord_last_error(h).decode() == "TrackedFFJORD groups: group 0: " + WORDS
        assert list(gst) == [L.MAX_ATTEMPTS] * 2 and list(nfe) == [3 + 6 * MAX_ATT] * 2
        for g in range(2):
            assert _ff_steps(h, lib.rnde_ffjord_group_steps, g)[0] == MAX_ATT
        torch.cuda.synchronize()
        assert torch.equal(acc.cpu().view(torch.int64), before)          # a failed call adds nothing
        assert groups(SHORT) == L.OK, lib.rnde_ffjord_last_error(h).decode()
        torch.cuda.synchronize()
        assert list(gst) == [L.OK] * 2 and bool(torch.isfinite(logpx).all())
        for g in range(2):
            n, steps = _ff_steps(h, lib.rnde_ffjord_group_steps, g)
            assert 1 <= n <= MAX_ATT and steps[-1] == 1.0 and nfe[g] == 3 + 6 * n
        assert int(acc.cpu().view(torch.int64)[1]) == cols
    finally:
        lib.rnde_ffjord_destroy(h)


def test_tiled_node_solve_reports_max_attempts_and_serves_the_next_call():
    from tests.test_gpu_node_tiled import make_cfg, tiled
    _, dims, acts, td = TD2
    p, x = (v.numpy() for v in _inputs("td2-B5")[:2])
    node = tiled(make_cfg(dims, acts, td, x.shape[0], reltol=TOL, abstol=TOL, regularize=1, max_attempts=MAX_ATT))
    try:
        _node_checks(node, x, p)
    finally:
        node.close()


def _node_checks(node, x, p):
    from regneuralde_jl_amd._lib import RndeError
    L = _lib()
    with pytest.raises(RndeError) as err:
        node.forward(x, p, keep_tape=True)
    assert err.value.status == L.MAX_ATTEMPTS and str(err.value) == f"rnde status {L.MAX_ATTEMPTS}: {WORDS}"
    assert node.L.rnde_last_error(node.h).decode() == WORDS
    natt = C.c_int32(-1)
    steps = (C.c_float * (4 * MAX_ATT))()
    assert node.L.rnde_node_steps(node.h, steps, MAX_ATT, C.byref(natt)) == L.OK and natt.value == MAX_ATT
    with pytest.raises(RndeError) as err:                                # (the failed forward left no tape)
        node.backward(np.ones_like(x), None)
    assert err.value.status == L.NO_TAPE
    f = node.forward(x, p, 0.0, SHORT, keep_tape=True)
    assert 1 <= f["nattempts"] <= MAX_ATT and f["steps"][-1, 3] == 1.0 and f["nfe"] == 3 + 6 * f["nattempts"] and np.isfinite(f["u"]).all()
    assert len(f["saveval"]) == 1 + int(f["steps"][:, 3].sum())
    xb, pb, _ = node.backward(np.ones_like(x), np.ones(len(f["saveval"]), np.float32))
    assert np.isfinite(xb).all() and np.isfinite(pb).all()
