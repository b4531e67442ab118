"""The tiled TrackedFFJORD engine without a GPU: its C entry point and what it refuses before touching a device, the package's engine switch,
the closed-form exact trace it uses for sample() (restated in fp64 and checked against autograd's Jacobian), and load_miniboone."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ffjord_ref as R


def _cfg(rn, D, H, **kw):
    cfg = rn._lib.FfjordConfig()
    cfg.in_dims, cfg.hidden, cfg.max_batch, cfg.max_attempts = D, H, 1024, 4096
    cfg.reltol = cfg.abstol = 1.4e-8
    cfg.regularize, cfg.cb_save_start, cfg.time_dep = 1, 1, 1
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _create_tiled(rn, cfg):
    L, h = rn._lib.lib(), C.c_void_p()
    st = L.rnde_ffjord_create_tiled(C.byref(cfg), C.byref(h))
    msg = L.rnde_ffjord_last_error(h if h.value else None).decode()
    if h.value:
        L.rnde_ffjord_destroy(h)
    return st, msg


def test_create_tiled_validates_before_the_device(rnde):
    """(43, 100) passes every check of the tiled engine (here it then fails only for want of a device); each refusal has its own message."""
    L = rnde._lib.lib()
    assert hasattr(L, "rnde_ffjord_create_tiled") and hasattr(L, "rnde_ffjord_engine")
    assert L.rnde_ffjord_engine(None) == -1
    if not torch.cuda.is_available():
        for D, H in ((43, 100), (16, 64), (2, 16), (64, 112)):
            st, msg = _create_tiled(rnde, _cfg(rnde, D, H))
            assert st == rnde._lib.NO_DEVICE and "no HIP device" in msg, (D, H, msg)
    cases = [(_cfg(rnde, 43, 113), "LDS limit"), (_cfg(rnde, 65, 100), "LDS limit"), (_cfg(rnde, 43, 100, dynamics=1), "Tracker.forward"),
             (_cfg(rnde, 43, 100, kinetic_reg=1), "kinetic energy"), (_cfg(rnde, 43, 100, max_batch=4097), "max_batch above 4096"),
             (_cfg(rnde, 43, 100, solver=1), "only Tsit5"), (_cfg(rnde, 43, 100, max_attempts=9000), "max_attempts above 8000")]
    for cfg, want in cases:
        st, msg = _create_tiled(rnde, cfg)
        assert st == rnde._lib.BAD_ARG and want in msg, (want, msg)
    # the one-workgroup entry point keeps its limit, and now points at the tiled engine
    st = L.rnde_ffjord_create(C.byref(_cfg(rnde, 43, 100)), C.byref(C.c_void_p()))
    assert st == rnde._lib.BAD_ARG and b"limit of 64" in L.rnde_ffjord_last_error(None) and b"tiled" in L.rnde_ffjord_last_error(None)


def test_check_served_engine_switch(rnde):
    ff = rnde.ffjord
    ff.check_served(ff.MLPDynamics(43, 100), engine="tiled")
    ff.check_served(ff.MLPDynamics(64, 112), engine="tiled")
    with pytest.raises(ValueError, match="limit of 64"):
        ff.check_served(ff.MLPDynamics(43, 100))
    with pytest.raises(ValueError, match="LDS limit"):
        ff.check_served(ff.MLPDynamics(43, 113), engine="tiled")
    with pytest.raises(ValueError, match="kinetic energy"):
        ff.check_served(ff.MLPDynamics(43, 100), regularize_kinetic=True, engine="tiled")
    with pytest.raises(ValueError, match="engine"):
        ff.check_served(ff.MLPDynamics(2, 16), engine="auto")
    with pytest.raises(ValueError, match="max_batch above 4096"):
        ff.TrackedFFJORD(ff.MLPDynamics(43, 100), [0.0, 1.0], True, False, engine="tiled", max_batch=5000)


def closed_form_trace(p, D, H, z, t):
    """tr J = a2' (W2 .* M') a1, M = W1 diag(g3) W3, a_l = sig(h_l) .* g_l (the tiled engine's exact trace), per row of z (B, D)."""
    _, (h1, h2, _), (g1, g2, g3), L = R.mlp(p, D, H, z, t)
    W1, W2, W3 = L[0][0], L[1][0], L[2][0]
    M = W1 @ torch.diag(g3) @ W3                       # (H, H)
    Q = W2 * M.t()
    a1, a2 = R.sig(h1) * g1, R.sig(h2) * g2
    return ((a2 @ Q) * a1).sum(1)


@pytest.mark.parametrize("D,H", [(43, 100), (2, 16)])
def test_closed_form_trace_equals_autograd_jacobian(D, H):
    rng = np.random.default_rng(7)
    p = torch.from_numpy(R.glorot_params(D, H, rng, scale=2.0)).double()
    z = torch.from_numpy(rng.standard_normal((5, D)))
    for t in (0.0, 0.37, 1.0):
        got = closed_form_trace(p, D, H, z, t)
        for b in range(z.shape[0]):
            J = torch.autograd.functional.jacobian(lambda v: R.mlp(p, D, H, v[None, :], t)[0][0], z[b])
            assert abs(float(got[b]) - float(torch.trace(J))) <= 1e-12 * max(1.0, abs(float(torch.trace(J))))
        # and the unit-probe restatement the device tests compare sample() against
        ref = -R.rhs(p, D, H, torch.cat([z, torch.zeros(z.shape[0], 1, dtype=z.dtype)], 1), t)[:, D]
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)


def test_load_miniboone_on_a_synthetic_array(rnde, tmp_path):
    rng = np.random.default_rng(0)
    X = (rng.standard_normal((1000, 43)) * rng.uniform(0.5, 4.0, 43) + rng.uniform(-3, 3, 43)).astype(np.float32)
    path = tmp_path / "miniboone.npy"
    np.save(path, X)
    tr, te = rnde.load_miniboone(1024, str(path))
    assert tr.X.shape == (800, 43) and te.X.shape == (200, 43) and tr.X.dtype == np.float32
    A = np.concatenate([tr.X, te.X]).astype(np.float64)
    assert np.abs(A.mean(0)).max() <= 1e-5 and np.abs(A.std(0, ddof=1) - 1).max() <= 1e-5
    # shuffled: the rows are a permutation of the standardised input, not its first 800 in order
    S = (X - X.mean(0)) / X.std(0, ddof=1)
    assert not np.allclose(tr.X[:10], S[:10], atol=1e-5)
    assert np.allclose(np.sort(A[:, 0]), np.sort(S[:, 0]), atol=1e-5)
    assert [b.shape[0] for b in tr] == [800] and [b.shape[0] for b in te] == [200]
