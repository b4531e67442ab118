"""The launches around the one-launch solve folded into it (csrc/rnde_stage_solve.h, switch RNDE_SOLVE_FOLD, read per call).

With the switch on, rnde_stage_solve_kernel runs the initial-step rule itself in front of its attempt loop (what the four launches SM_I1 .. SM_I4 of
rnde_stage_kernel compute: f0, h0, dt0, u1, f1, h1, the three norm sums, InitRec) and stores the final state from registers when it returns (what
rnde_stage_finish_kernel copies).  Both forms call the same functions and form the cross-workgroup sums in the same order, so every output must be
BIT-identical between the two settings: end state, NFE, step log, callback values, and -- through the reverse pass with track_initdt on, which reads
f0 / f1 / h0 / h1 / u1 / initpart / InitRec -- x-bar, p-bar and tspan-bar.  (InitRec and initpart have no getter of their own: the step log's first
proposed step and tspan-bar / p-bar depend on every field of them.)

Headline geometry (D = 784, H = 100: the folded path exists for it alone), small batches: 16 columns = one column tile (7 workgroups), 37 = a ragged
last tile, 100 = 7 tiles.  Tolerance 1e-3 keeps a solve at a handful of attempts; one case runs the headline's 1.4e-8.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_forward import _cfg

pytestmark = pytest.mark.gpu

D, H = 784, 100


def _problem(B, act2, seed, scale, zero_x=False):
    from tests.util import glorot_params, make_arch
    rng = np.random.default_rng(seed)
    arch = make_arch([D, H, D], ["tanh", "tanh" if act2 else "identity"], True)
    p = glorot_params(arch, rng, np.float32, scale)
    p = (p + 0.02 * rng.standard_normal(p.shape)).astype(np.float32)      # (non-zero biases)
    x = np.zeros((B, D), np.float32) if zero_x else rng.uniform(0, 1, (B, D)).astype(np.float32)
    return arch, p, x


def _raw_forward(node, x, p, t0, t1, keep_tape, with_u=True):
    """rnde_node_forward without the wrapper's status check: (status, u or None, nfe, callback values, step log)"""
    xd, pd = node.dev(x), node.dev(p)
    u = torch.full_like(xd, float("nan")) if with_u else None
    nfe, nsv, natt = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    sv = (C.c_float * (node.cfg.max_attempts + 1))()
    torch.cuda.current_stream().synchronize()
    st = node.L.rnde_node_forward(node.h, xd.data_ptr(), pd.data_ptr(), x.shape[0], t0, t1, u.data_ptr() if with_u else None, C.byref(nfe), sv,
                                  C.byref(nsv), int(keep_tape), None)
    steps = (C.c_float * (4 * node.cfg.max_attempts))()
    node.L.rnde_node_steps(node.h, steps, node.cfg.max_attempts, C.byref(natt))
    torch.cuda.synchronize()
    return (st, u.cpu().numpy() if with_u else None, nfe.value, np.array(sv[:nsv.value], dtype=np.float32),
            np.array(steps[:4 * natt.value], dtype=np.float32).reshape(-1, 4))


def _run(monkeypatch, B, tol, act2, reg, x3, seed=5, scale=2.0, zero_x=False, tspan=(0.0, 1.0), max_attempts=96, with_u=True, expect_ok=True):
    """The same taped forward and reverse pass on ONE handle with the switch off, on, and on again (the second folded solve finds the start-up's
    slab buffers and granule rows as the first left them); returns the three result tuples."""
    from tests.util import Node
    monkeypatch.setenv("RNDE_X3", str(x3))
    monkeypatch.setenv("RNDE_WGRAD_SIDE", "0")      # (one partition of the weight-gradient GEMMs: p-bar is then a function of the tape alone, bit for bit)
    arch, p, x = _problem(B, act2, seed, scale, zero_x)
    node = Node(_cfg(arch, B, reltol=tol, abstol=tol, col_tile=16, max_attempts=max_attempts, regularize=reg, track_initdt=1))
    node.L.rnde_node_one_launch_solves.restype = C.c_int32
    outs = []
    for k, fold in enumerate(("0", "1", "1")):
        monkeypatch.setenv("RNDE_SOLVE_FOLD", fold)
        st, u, nfe, sv, steps = _raw_forward(node, x, p, tspan[0], tspan[1], keep_tape=expect_ok, with_u=with_u)
        assert (st == 0) == expect_ok
        grads = None
        if expect_ok:
            assert node.L.rnde_node_one_launch_solves(node.h) == k + 1      # the one-launch solve served it, both settings
            ubar = np.random.default_rng(9).standard_normal((B, D)).astype(np.float32)
            grads = node.backward(ubar, np.full(len(sv), 3.0, dtype=np.float32))
        assert node.L.rnde_node_fallback_count(node.h) == 0
        outs.append((st, u, nfe, sv, steps, grads))
    node.close()
    return outs


def _assert_identical(outs):
    a = outs[0]
    for b in outs[1:]:
        assert a[0] == b[0] and a[2] == b[2]
        if a[1] is not None:
            assert np.array_equal(a[1], b[1], equal_nan=True)
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
        if a[5] is not None:
            for ga, gb in zip(a[5], b[5]):
                assert np.array_equal(ga, gb)


@pytest.mark.parametrize("B,tol,act2,reg,x3", [
    (16, 1e-3, 1, 1, 1), (37, 1e-3, 1, 0, 1), (100, 1e-3, 1, 3, 1), (37, 1e-3, 0, 2, 1), (16, 1.4e-8, 1, 1, 1),
    (16, 1e-3, 0, 1, 0), (37, 1e-3, 1, 3, 0), (100, 1e-3, 0, 0, 0)])
def test_folded_solve_is_bit_identical(B, tol, act2, reg, x3, monkeypatch):
    """both ACT2 values, regularisers none / error_est / the two eigen_est forms (three-value meeting), both matrix modes"""
    outs = _run(monkeypatch, B, tol, act2, reg, x3)
    assert outs[0][2] >= 15 and np.isfinite(outs[0][1]).all()
    _assert_identical(outs)


@pytest.mark.parametrize("x3", [0, 1])
def test_folded_solve_zero_input_takes_the_small_norm_branch(x3, monkeypatch):
    """x = 0: ||u0|| = 0 < 1e-5, the dt0 rule's constant branch (dt0 = 1e-6)"""
    _assert_identical(_run(monkeypatch, 16, 1e-3, 1, 1, x3, zero_x=True))


def test_folded_solve_tspan_not_starting_at_zero(monkeypatch):
    _assert_identical(_run(monkeypatch, 37, 1e-3, 1, 1, 1, tspan=(0.25, 1.5)))


def test_folded_solve_first_attempt_rejected(monkeypatch):
    """stiff dynamics (weights scaled by 30): the initial step is too long and the first two attempts are rejected (EEst 1.7 and 1.1 on the CPU oracle,
    far from the threshold) -- the state handed over at the first accept is still x"""
    outs = _run(monkeypatch, 16, 1e-3, 1, 1, 1, scale=30.0)
    assert outs[0][4][0, 3] == 0.0 and outs[0][4][:, 3].sum() >= 1.0
    _assert_identical(outs)


@pytest.mark.parametrize("x3", [0, 1])
def test_folded_solve_ends_at_max_attempts(x3, monkeypatch):
    """max_attempts = 3 at a tolerance that needs more: the solve ends at the limit and u is the last accepted state (x if there is none) in both forms"""
    outs = _run(monkeypatch, 16, 1e-6, 1, 1, x3, max_attempts=3, expect_ok=False)
    assert np.isfinite(outs[0][1]).all()
    _assert_identical(outs)


def test_folded_solve_without_an_output_buffer(monkeypatch):
    """a null u_out: no store, everything else as before"""
    _assert_identical(_run(monkeypatch, 37, 1e-3, 1, 1, 1, with_u=False))
