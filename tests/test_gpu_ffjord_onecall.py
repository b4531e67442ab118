"""The FFJORD training step in one call (rnde_ffjord_nll_grad, rnde_adam_wd_step, include/rnde.h; ffjord.fused_ffjord_loss_and_grad and
FluxADAM(one_launch=True)), through the C ABI and through the package.

The yardstick of the fused call is the pair of calls it replaces: p-bar, x-bar, logpx, NFE and the (dt, accepted) log must EQUAL those of
rnde_ffjord_forward(keep_tape = 1) + rnde_ffjord_backward on a second handle of the same config, with the seeds rebuilt here in numpy fp32
from the formulas of the header comment -- torch.equal / ==, no tolerance: both paths are deterministic and run the same kernels.

Shapes: the smallest that can go wrong.  ConcatSquash MLPDynamics(2, 16) on engine 0 (one workgroup) and engine 1 (tiled), the TD chain
[3, 10, 3] (tanh, identity) on engine 2, reltol = abstol = 1e-4, max_attempts = 300, parameters from glorot_params(2, 16, seed 9, scale 8) /
ffjord_chain_ref.draw (the draws of tests/test_gpu_ffjord_groups.py, where the controller rejects steps), B in {1, 17, 40}: one tile, ragged
tiles, three tiles.  The loss terms run B over {1, 17, 255, 256, 257, 1000}, the edges of the kernel's stride of 256 threads.

Bounds.  The loss terms: a double sum of at most 4096 floats is off by far less than half an fp32 ulp, so against float32(fp64 sum / B) only
a tie can move the rounding: 1 fp32 ulp.  The meaning test carries the bounds of test_replay_forward_and_reverse (tests/test_gpu_ffjord_tiled.py),
5e-3 without and 2e-2 with the saved values' cotangent, along the fused call's own accepted steps.  The optimiser: rtol 1e-5, atol 1e-6, the bound
of test_adam_step_matches_the_torch_recurrence."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import ffjord_chain_ref as CR
from tests import ffjord_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, MAX_ATT = 1e-4, 300
OK, BAD_ARG = 0, 1
CHAIN = ([3, 10, 3], ["tanh", "identity"])
F32 = np.float32


def _rn():
    import regneuralde_jl_amd as rn
    return rn


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _layer(engine, regularize, max_batch=64, track=False, D=2, H=16, tol=TOL, max_attempts=MAX_ATT):
    """engine 0 / 1: MLPDynamics(D, H) on "workgroup" / "tiled", 2: the TD chain [3, 10, 3]; the parameters of the module docstring."""
    rn = _rn()
    if engine == 2:
        dims, acts = CHAIN
        pp = CR.draw(dims, True, 1, 9, 2.0)[0]
        model = rn.TDChain(*[rn.Dense(dims[l] + 1, dims[l + 1], acts[l]) for l in range(len(acts))])
        ff = rn.TrackedFFJORD(model, [0.0, 1.0], True, regularize, "Tsit5", reltol=tol, abstol=tol, max_batch=max_batch, max_attempts=max_attempts,
                              engine="tiled", track_ctrl=track)
        assert ff.p.numel() == pp.numel()
        ff.p = pp.to(DEV)
        return ff
    m = rn.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(9))
    ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, regularize, "Tsit5", reltol=tol, abstol=tol, max_batch=max_batch, max_attempts=max_attempts,
                          engine="tiled" if engine else "workgroup", track_ctrl=track)
    ff.p = torch.from_numpy(R.glorot_params(D, H, np.random.default_rng(9), scale=8.0)).to(DEV)
    return ff


def _handle(ff):
    return _rn().ffjord._Handle(ff.config(), ff.engine, ff.track_ctrl)


def _draw(B, D, seed=11, xscale=2.0):
    rng = np.random.default_rng(seed + B)
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(F32) * F32(xscale)).to(DEV)
    e = torch.from_numpy(rng.standard_normal((B, D)).astype(F32)).to(DEV)
    return x, e


def _steps(h):
    L, n = _rn()._lib, C.c_int32()
    L.check_ffjord(h, L.lib().rnde_ffjord_steps(h, None, 0, C.byref(n)))
    arr = (C.c_float * max(2 * n.value, 1))()
    L.check_ffjord(h, L.lib().rnde_ffjord_steps(h, arr, n.value, C.byref(n)))
    return list(arr[:2 * n.value])


def _step_log(h):
    L, n = _rn()._lib, C.c_int32()
    L.check_ffjord(h, L.lib().rnde_ffjord_step_log(h, None, 0, C.byref(n)))
    arr = (C.c_float * max(4 * n.value, 1))()
    L.check_ffjord(h, L.lib().rnde_ffjord_step_log(h, arr, n.value, C.byref(n)))
    return np.array(arr[:4 * n.value], dtype=F32).reshape(-1, 4)


def _saved_values(ff, log):
    """The saved values the header's host formulas speak of, from the step log: 0 at init (cb_save_start), then fp32 EEst * dt per accepted step."""
    sv = [F32(0)] if ff.cb_save_start else []
    return sv + [F32(r[2]) * F32(r[1]) for r in log if r[3] != 0]


def _fused(ff, hd, x, e, mode=0, lam_r=0.0, lam_k=0.0, lam_j=0.0, seed=0, B=None, t0=0.0, t1=1.0, null=(), p_fill=None):
    """rnde_ffjord_nll_grad on the handle object hd (held by the caller's argument until the call is over) with every output given; `null`
    names arguments passed as NULL."""
    L, h = _rn()._lib, hd.h
    B = x.shape[0] if B is None else B
    pb = torch.full_like(ff.p, float("nan") if p_fill is None else p_fill)
    xb = torch.full_like(x, float("nan"))
    lp = torch.full((x.shape[0],), float("nan"), device=DEV)
    terms = torch.full((3,), float("nan"), device=DEV)
    reg, nfe = C.c_float(float("nan")), C.c_int64(-1)
    arg = lambda name, v: None if name in null else v
    st = L.lib().rnde_ffjord_nll_grad(h, x.data_ptr(), ff.p.data_ptr(), e.data_ptr() if e is not None else None, B, t0, t1, seed, mode, lam_r, lam_k,
                                      lam_j, arg("p_bar", pb.data_ptr()), arg("x_bar", xb.data_ptr()), arg("logpx", lp.data_ptr()),
                                      arg("terms", terms.data_ptr()), arg("reg", C.byref(reg)), arg("nfe", C.byref(nfe)), _stream())
    msg = L.lib().rnde_ffjord_last_error(h).decode()
    torch.cuda.synchronize()
    return dict(st=st, msg=msg, pb=pb.cpu(), xb=xb.cpu(), lp=lp.cpu(), terms=terms.cpu().numpy(), reg=F32(reg.value), nfe=int(nfe.value),
                log=_steps(h) if st == OK else None)


def _two_calls(ff, hd, x, e, mode=0, lam_r=0.0, lam_k=0.0, lam_j=0.0, seed=0):
    """The calls the fused one replaces on the handle object hd, with the seeds built in numpy fp32 from the header's formulas."""
    L, h = _rn()._lib, hd.h
    lib, B = L.lib(), x.shape[0]
    lp = torch.full((B,), float("nan"), device=DEV)
    rows = torch.full((2, B), float("nan"), device=DEV)
    nfe, nsv, sv = C.c_int64(), C.c_int32(), (C.c_float * (ff.max_attempts + 1))()
    ep = e.data_ptr() if e is not None else None
    if mode == 1:
        st = lib.rnde_ffjord_forward_exact(h, x.data_ptr(), ff.p.data_ptr(), B, 0.0, 1.0, lp.data_ptr(), None, C.byref(nfe), sv, C.byref(nsv), 1, _stream())
    elif mode == 2:
        st = lib.rnde_ffjord_forward_kinetic(h, x.data_ptr(), ff.p.data_ptr(), ep, B, 0.0, 1.0, seed, lp.data_ptr(), rows.data_ptr(), None, C.byref(nfe), 1,
                                             _stream())
    else:
        st = lib.rnde_ffjord_forward(h, x.data_ptr(), ff.p.data_ptr(), ep, B, 0.0, 1.0, seed, lp.data_ptr(), None, C.byref(nfe), sv, C.byref(nsv), 1, _stream())
    L.check_ffjord(h, st)
    log = _steps(h)
    lpb = torch.from_numpy(np.full(B, F32(-1.0) / F32(B), F32)).to(DEV)                     # logpx_bar[b] = -1.0f / (float)B
    pb, xb = torch.full_like(ff.p, float("nan")), torch.full_like(x, float("nan"))
    if mode == 2:
        rb = torch.from_numpy(np.stack([np.full(B, F32(lam_k) / F32(B), F32), np.full(B, F32(lam_j) / F32(B), F32)])).to(DEV).contiguous()
        st = lib.rnde_ffjord_backward_kinetic(h, lpb.data_ptr(), rb.data_ptr(), pb.data_ptr(), xb.data_ptr(), _stream())
    else:
        n = nsv.value
        svb = (C.c_float * n)(*([float(F32(lam_r) / F32(n))] * n)) if n else None          # saveval_bar[i] = lambda_r / (float)n
        st = lib.rnde_ffjord_backward(h, lpb.data_ptr(), svb, pb.data_ptr(), xb.data_ptr(), _stream())
    L.check_ffjord(h, st)
    torch.cuda.synchronize()
    return dict(pb=pb.cpu(), xb=xb.cpu(), lp=lp.cpu(), nfe=int(nfe.value), log=log, rows=rows.cpu(), sv=list(sv[:nsv.value]))


def _assert_same(got, ref, what):
    assert got["st"] == OK, (what, got["st"], got["msg"])
    assert torch.isfinite(ref["pb"]).all() and torch.isfinite(ref["xb"]).all() and torch.isfinite(ref["lp"]).all(), what
    assert torch.equal(got["lp"], ref["lp"]), (what, "logpx", float((got["lp"] - ref["lp"]).abs().max()))
    assert torch.equal(got["pb"], ref["pb"]), (what, "p-bar", float((got["pb"] - ref["pb"]).abs().max()))
    assert torch.equal(got["xb"], ref["xb"]), (what, "x-bar", float((got["xb"] - ref["xb"]).abs().max()))
    assert got["nfe"] == ref["nfe"] == 3 + 6 * (len(ref["log"]) // 2), (what, got["nfe"], ref["nfe"])
    assert got["log"] == ref["log"], (what, len(got["log"]) // 2, len(ref["log"]) // 2)


# ---- 1. equality with the two calls ----
@pytest.mark.parametrize("B", [1, 17, 40])
@pytest.mark.parametrize("regularize", [False, True], ids=["false", "true"])
@pytest.mark.parametrize("engine", [0, 1, 2])
def test_fused_call_equals_forward_plus_backward(engine, regularize, B):
    ff = _layer(engine, regularize)
    x, e = _draw(B, ff.in_dims)
    lam_r = 100.0 if regularize else 0.0
    a, b = _handle(ff), _handle(ff)
    assert _rn()._lib.lib().rnde_ffjord_engine(a.h) == engine
    ref = _two_calls(ff, b, x, e, lam_r=lam_r)
    got = _fused(ff, a, x, e, lam_r=lam_r)
    _assert_same(got, ref, (engine, regularize, B))
    assert (len(ref["sv"]) > 1) == regularize
    print("engine", engine, "B", B, "attempts", len(ref["log"]) // 2, "rejected", sum(1 for v in ref["log"][1::2] if v == 0))


@pytest.mark.parametrize("engine", [1, 2])
def test_exact_trace_mode_equals_the_two_calls(engine):
    ff = _layer(engine, True)
    x, _ = _draw(17, ff.in_dims)
    a, b = _handle(ff), _handle(ff)
    _assert_same(_fused(ff, a, x, None, mode=1, lam_r=100.0), _two_calls(ff, b, x, None, mode=1, lam_r=100.0), ("exact", engine))


@pytest.mark.parametrize("engine", [0, 1])
def test_kinetic_mode_equals_the_two_calls(engine):
    ff = _layer(engine, False)
    x, e = _draw(17, ff.in_dims)
    a, b = _handle(ff), _handle(ff)
    ref = _two_calls(ff, b, x, e, mode=2, lam_k=0.01, lam_j=0.05)
    got = _fused(ff, a, x, e, mode=2, lam_k=0.01, lam_j=0.05)
    _assert_same(got, ref, ("kinetic", engine))
    plain = _two_calls(ff, _handle(ff), x, e)                       # (the two weights reached p-bar: they cannot be dropped unseen)
    assert not torch.equal(plain["pb"], got["pb"])


def test_tracked_controller_equals_the_two_calls():
    ff = _layer(1, True, track=True)
    x, e = _draw(17, ff.in_dims)
    a, b = _handle(ff), _handle(ff)
    assert _rn()._lib.lib().rnde_ffjord_track_ctrl(a.h) == 1
    got = _fused(ff, a, x, e, lam_r=100.0)
    _assert_same(got, _two_calls(ff, b, x, e, lam_r=100.0), "track_ctrl")
    off = _layer(1, True)
    assert not torch.equal(_fused(off, _handle(off), x, e, lam_r=100.0)["pb"], got["pb"])        # (the tracked sweep ran)


def test_library_probe_draw_equals_the_forward_with_the_same_seed():
    ff = _layer(1, True)
    x, e = _draw(17, ff.in_dims)
    a, b = _handle(ff), _handle(ff)
    got = _fused(ff, a, x, None, lam_r=100.0, seed=1234)
    _assert_same(got, _two_calls(ff, b, x, None, lam_r=100.0, seed=1234), "e_dev = NULL")
    assert not torch.equal(got["lp"], _fused(ff, a, x, None, lam_r=100.0, seed=1235)["lp"])        # (the seed is read)


# ---- 2. the loss terms ----
@functools.lru_cache(maxsize=None)
def _terms_layers():
    t, f = _layer(1, True, max_batch=1024), _layer(1, False, max_batch=1024)
    return t, _handle(t), f, _handle(f), _handle(f)


def _ulp_apart(got, ref):
    return abs(float(got) - float(ref)) / float(np.spacing(np.abs(F32(ref))))


@pytest.mark.parametrize("B", [1, 17, 255, 256, 257, 1000])
def test_loss_terms(B):
    ft, ht, ff, hf, hk = _terms_layers()
    x, e = _draw(B, 2, xscale=1.0)
    lam = 100.0
    got = _fused(ft, ht, x, e, lam_r=lam)
    assert got["st"] == OK, got["msg"]
    ref = F32(-(got["lp"].double().sum().item()) / B)
    print("B", B, "nll", got["terms"][0], "ref", ref, "ulps", _ulp_apart(got["terms"][0], ref))
    assert np.isfinite(ref) and _ulp_apart(got["terms"][0], ref) <= 1.0
    assert got["terms"][1] == 0.0 and got["terms"][2] == 0.0
    sv = _saved_values(ft, _step_log(ht.h))
    assert len(sv) > 1 and (got["nfe"] - 3) // 6 == len(_step_log(ht.h))
    want = F32(np.float64(F32(lam)) * np.sum(np.asarray(sv, np.float64)) / len(sv))
    assert got["reg"] == want and want > 0, (got["reg"], want)
    # the kinetic means, against the rows rnde_ffjord_forward_kinetic returns
    gk = _fused(ff, hf, x, e, mode=2, lam_k=0.01, lam_j=0.05)
    assert gk["st"] == OK, gk["msg"]
    assert gk["reg"] == 0.0
    rows = _two_calls(ff, hk, x, e, mode=2, lam_k=0.01, lam_j=0.05)["rows"].double()
    assert _ulp_apart(gk["terms"][0], F32(-(gk["lp"].double().sum().item()) / B)) <= 1.0
    for k in (0, 1):
        ref = F32(rows[k].sum().item() / B)
        print("B", B, "lambda", k + 1, gk["terms"][1 + k], "ref", ref)
        assert ref > 0 and _ulp_apart(gk["terms"][1 + k], ref) <= 1.0


# ---- 3. meaning ----
def test_gradient_of_the_loss_matches_fp64_autograd_along_the_accepted_steps():
    """-mean(logpx) + lam * mean(sv) at the setting of test_replay_forward_and_reverse (tests/test_gpu_ffjord_tiled.py: (2, 16), B = 37, seed 2,
    scale 3, tol 1e-5): p-bar and x-bar of the fused call against fp64 autograd through tests/ffjord_ref.replay along the call's own accepted
    steps (read from rnde_ffjord_steps; step sizes are constants of the reverse sweep)."""
    rn = _rn()
    D, H, B, tol = 2, 16, 37, 1e-5
    m = rn.ffjord.MLPDynamics(D, H, generator=torch.Generator().manual_seed(2))
    ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, True, "Tsit5", reltol=tol, abstol=tol, max_batch=B, engine="tiled")
    rng = np.random.default_rng(2)
    ff.p = torch.from_numpy(R.glorot_params(D, H, rng, scale=3.0)).to(DEV)
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(F32))
    e = torch.from_numpy(rng.standard_normal((B, D)).astype(F32))
    for lam, bound in ((0.0, 5e-3), (100.0, 2e-2)):
        xd = x.to(DEV)
        nll, reg, _, _, nfe = rn.fused_ffjord_loss_and_grad(ff, xd, None, e.to(DEV), lam_r=lam, need_x_grad=True)
        st = np.array(ff.steps()).reshape(-1, 2)
        assert nfe == 3 + 6 * len(st)
        dts = [float(F32(dt)) for dt, acc in st if acc != 0]
        assert abs(sum(dts) - 1.0) <= 1e-5
        Pg, Xg = ff.p.cpu().double().requires_grad_(True), x.double().requires_grad_(True)
        u, eests = R.replay(lambda v, t: R.rhs(Pg, D, H, v, t, e.double()), torch.cat([Xg, torch.zeros(B, 1, dtype=torch.float64)], 1), 0.0, dts, tol, tol)
        sv = torch.stack([torch.zeros((), dtype=torch.float64)] + [ee * dt for ee, dt in zip(eests, dts)])
        lp_ref = R.logpx_of(u, D)
        nll_ref = -lp_ref.mean()
        gx, gp = torch.autograd.grad(nll_ref + lam * sv.mean(), (Xg, Pg))
        rel = lambda a, b: float((a.detach().cpu().double() - b).abs().max() / b.abs().max())
        # (a mean of logpx is off by no more than its largest element is: that test's 5e-5 of max |logpx|)
        figs = (abs(float(nll) - float(nll_ref)) / float(lp_ref.abs().max()), rel(xd.grad, gx), rel(ff.p.grad, gp), abs(reg - lam * float(sv.mean())) / max(lam * float(sv.mean()), 1e-30))
        print("lam", lam, "steps", len(dts), "of", len(st), "min EEst", min(float(v) for v in eests), "nll / x-bar / p-bar / reg:", figs)
        assert figs[0] <= 5e-5 and figs[1] <= bound and figs[2] <= bound, figs
        # (figs[3], the regulariser's value, is printed only: the controller's first step is tiny, its EEst of 1e-5 is fp32 rounding and not
        # truncation error, and no fp32 solve matches fp64 there; the value is pinned bit for bit by test_loss_terms)
        if lam:
            g0 = torch.autograd.grad(-R.logpx_of(R.replay(lambda v, t: R.rhs(Pg, D, H, v, t, e.double()),
                                                          torch.cat([Xg, torch.zeros(B, 1, dtype=torch.float64)], 1), 0.0, dts, tol, tol)[0], D).mean(), Pg)[0]
            assert rel(gp, g0) > 1e-3                                  # (the saved values' cotangent reached p-bar)
        ff.p.grad = None


# ---- 4. handle state ----
def test_the_fused_call_consumes_its_tape_and_leaves_the_handle_as_new():
    L = _rn()._lib
    ff = _layer(1, True)
    x, e = _draw(17, ff.in_dims)
    fresh = _two_calls(ff, _handle(ff), x, e, lam_r=100.0)
    a = _handle(ff)
    assert _fused(ff, a, x, e, lam_r=100.0)["st"] == OK
    lpb, pb = torch.zeros(17, device=DEV), torch.zeros_like(ff.p)
    st = L.lib().rnde_ffjord_backward(a.h, lpb.data_ptr(), None, pb.data_ptr(), None, _stream())
    assert st == L.NO_TAPE, (st, L.lib().rnde_ffjord_last_error(a.h).decode())
    again = _two_calls(ff, a, x, e, lam_r=100.0)
    for k in ("pb", "xb", "lp"):
        assert torch.equal(again[k], fresh[k]), k
    assert again["nfe"] == fresh["nfe"] and again["log"] == fresh["log"]


def test_create_fused_call_and_destroy_give_back_every_allocation():
    lib = _rn()._lib.lib()
    ff = _layer(1, False)
    x, e = _draw(17, ff.in_dims)
    torch.cuda.synchronize()
    before = (int(lib.rnde_debug_live_allocs()), int(lib.rnde_debug_live_bytes()))
    a = _handle(ff)
    created = int(lib.rnde_debug_live_allocs())
    assert _fused(ff, a, x, e, mode=2, lam_k=0.01, lam_j=0.05)["st"] == OK
    assert int(lib.rnde_debug_live_allocs()) >= created + 4           # (logpx, logpx_bar, reg, reg_bar: through the owners, counted)
    lib.rnde_ffjord_destroy(a.h)
    a.h = None
    assert (int(lib.rnde_debug_live_allocs()), int(lib.rnde_debug_live_bytes())) == before


# ---- 5. stale memory ----
@pytest.mark.parametrize("mode", [0, 2])
def test_outputs_do_not_depend_on_fresh_allocations(monkeypatch, mode):
    lib = _rn()._lib.lib()
    monkeypatch.delenv("RNDE_POISON", raising=False)
    ff = _layer(1, mode == 0)
    x, e = _draw(40, ff.in_dims)
    kw = dict(mode=2, lam_k=0.01, lam_j=0.05) if mode else dict(lam_r=100.0)
    clean = _fused(ff, _handle(ff), x, e, **kw)
    c0 = int(lib.rnde_debug_poison_allocs())
    monkeypatch.setenv("RNDE_POISON", "1")
    got = _fused(ff, _handle(ff), x, e, **kw)
    monkeypatch.delenv("RNDE_POISON")
    assert int(lib.rnde_debug_poison_allocs()) > c0
    assert clean["st"] == OK and got["st"] == OK
    for k in ("pb", "xb", "lp"):
        assert torch.isfinite(clean[k]).all() and torch.equal(got[k], clean[k]), k
    assert np.array_equal(got["terms"], clean["terms"]) and got["reg"] == clean["reg"] and got["nfe"] == clean["nfe"] and got["log"] == clean["log"]


# ---- 6. refusals ----
REFUSALS = [
    # (id, engine, regularize, keywords of _fused, whether e is given, the reason in the message)
    ("mode", 1, True, dict(mode=3), True, "mode must be 0"),
    ("mode-negative", 1, True, dict(mode=-1), True, "mode must be 0"),
    ("exact-engine0", 0, True, dict(mode=1), False, "rnde_ffjord_create_tiled"),
    ("exact-with-e", 1, True, dict(mode=1), True, "takes no probe"),
    ("kinetic-true-handle", 1, True, dict(mode=2), True, "no kinetic energy rows"),
    ("lambda-k", 1, False, dict(lam_k=0.01), True, "mode 2 only"),
    ("lambda-j", 1, False, dict(mode=1, lam_j=0.05), False, "mode 2 only"),
    ("lambda-r", 1, False, dict(lam_r=1.0), True, "regularize = 0 handle"),
    ("p-bar", 1, True, dict(null=("p_bar",)), True, "are required"),
    ("terms", 1, True, dict(null=("terms",)), True, "are required"),
    ("reg-out", 1, True, dict(null=("reg",)), True, "are required"),
    ("nfe-out", 1, True, dict(null=("nfe",)), True, "are required"),
    ("B-zero", 1, True, dict(B=0), True, "1..max_batch"),
    ("B-above", 1, True, dict(B=65), True, "1..max_batch"),
    ("span", 1, True, dict(t0=1.0, t1=1.0), True, "t1 > t0"),
    ("span-reversed", 2, False, dict(t0=1.0, t1=0.0), True, "t1 > t0"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_name_their_reason_and_touch_nothing(case):
    _, engine, regularize, kw, give_e, why = case
    ff = _layer(engine, regularize)
    x, e = _draw(17, ff.in_dims)
    got = _fused(ff, _handle(ff), x, e if give_e else None, p_fill=-7.5, **kw)
    assert got["st"] == BAD_ARG and why in got["msg"], (got["st"], got["msg"])
    assert bool((got["pb"] == -7.5).all()) and bool(torch.isnan(got["xb"]).all()) and bool(torch.isnan(got["lp"]).all())


def test_kinetic_mode_outside_the_one_workgroup_limit_is_refused():
    ff = _layer(0, False, D=62, H=16)                                  # (63 state rows fit the limit of 64, 65 kinetic rows do not)
    x, e = _draw(17, 62)
    got = _fused(ff, _handle(ff), x, e, mode=2, p_fill=-7.5)
    assert got["st"] == BAD_ARG and "in_dims + 3 <= 64" in got["msg"], (got["st"], got["msg"])
    assert bool((got["pb"] == -7.5).all())


# ---- 7. the optimiser ----
def _adam(entry, p, g, m, v, t, *tail):
    L = _rn()._lib
    L.check(None, getattr(L.lib(), entry)(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), t, 1e-2, 0.9, 0.999, 1e-8, *tail, _stream()))


@pytest.mark.parametrize("n", [1, 255, 5248])
def test_adam_wd_step_matches_the_composed_optimiser(n):
    rn = _rn()
    rng = np.random.default_rng(n)
    p0 = torch.from_numpy(rng.standard_normal(n).astype(F32) * 30).to(DEV)
    gs = [torch.from_numpy(rng.standard_normal(n).astype(F32) * 1e-3).to(DEV) for _ in range(5)]
    pc = p0.clone()
    opt = rn.FluxADAM([pc], eta=1e-2, weight_decay=1e-5)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    pl = p0.clone()
    one = rn.FluxADAM([pl], eta=1e-2, weight_decay=1e-5, one_launch=True)
    for t, g in enumerate(gs, 1):
        pc.grad = g.clone()
        opt.step()
        pl.grad = g.clone()
        one.step()
        _adam("rnde_adam_wd_step", p, g, m, v, t, 1.0, 1e-5)
        assert torch.isfinite(p).all()
        assert torch.allclose(p, pc, rtol=1e-5, atol=1e-6), (t, float((p - pc).abs().max()))
        assert torch.equal(pl, p) and torch.equal(one.m[0], m) and torch.equal(one.v[0], v)
    assert torch.allclose(m, opt.m[0], rtol=1e-5, atol=1e-6) and torch.allclose(v, opt.v[0], rtol=1e-5, atol=1e-6)
    q, mq, vq = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t, g in enumerate(gs, 1):
        _adam("rnde_adam_step", q, g, mq, vq, t, 1.0)
    assert n == 1 or not torch.allclose(q, p, rtol=1e-5, atol=1e-6)    # (wd * p is a third of g here: the decay cannot be dropped unseen)


@pytest.mark.parametrize("n", [1, 255, 5248])
def test_adam_wd_step_without_decay_has_the_bits_of_adam_step(n):
    rng = np.random.default_rng(100 + n)
    p0 = torch.from_numpy(rng.standard_normal(n).astype(F32)).to(DEV)
    a, b = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)], [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    for t in range(1, 6):
        g = torch.from_numpy(rng.standard_normal(n).astype(F32)).to(DEV)
        _adam("rnde_adam_step", a[0], g, a[1], a[2], t, 0.5)
        _adam("rnde_adam_wd_step", b[0], g, b[1], b[2], t, 0.5, 0.0)
        for u, w in zip(a, b):
            assert torch.equal(u, w), t


# ---- 8. the loop ----
def test_six_one_call_steps_lower_the_nll():
    rn = _rn()
    m = rn.ffjord.MLPDynamics(2, 16, generator=torch.Generator().manual_seed(3))
    ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, True, "Tsit5", reltol=TOL, abstol=TOL, max_batch=64, max_attempts=MAX_ATT, engine="tiled")
    rng = np.random.default_rng(3)
    x = torch.from_numpy((rng.standard_normal((64, 2)) * 0.5 + 1.5).astype(F32)).to(DEV)
    e = torch.from_numpy(rng.standard_normal((64, 2)).astype(F32)).to(DEV)
    pool, untaped = list(ff._pool), ff._h
    opt = rn.FluxADAM([ff.p], eta=1e-2, weight_decay=1e-5, one_launch=True)
    nll = []
    for _ in range(6):
        out = rn.fused_ffjord_loss_and_grad(ff, x, None, e, lam_r=0.0)
        assert out[0].dim() == 0 and out[0].is_cuda and out[2].is_cuda and out[3].is_cuda and isinstance(out[1], float) and out[4] > 3
        assert ff.p.grad is not None and torch.isfinite(ff.p.grad).all()
        opt.step()
        nll.append(float(out[0]))
        assert np.isfinite(nll[-1]) and np.isfinite(out[1]) and torch.isfinite(ff.p).all()
    print("nll", nll)
    assert nll[-1] < nll[0], nll
    assert ff._pool == pool and ff._h is untaped                       # (its own handle: the tape pool and the untaped handle were not touched)
