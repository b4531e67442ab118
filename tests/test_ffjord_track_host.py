"""The tracked-controller reverse sweep of TrackedFFJORD without a GPU: the torch restatement the device is compared against
(tests/ffjord_track_ref.py) is pinned to the fp64 oracle's track_ctrl = 1, track_initdt = 0 reverse pass, the inputs are shown to tell the
tracked from the constant-step gradient apart, and the package refuses track_ctrl=True where the C entry point would, before a device is needed.

The oracle solves TrackedNeuralODE (no trace row), with the same controller, the same Tsit5 and the same saved value EEst * dt, so the
restatement runs over the plain chain right-hand side here.  Cotangents: 1 on every saved value, standard normals on the end state."""
import functools

import numpy as np
import pytest
import torch

from tests import act_ref as A
from tests import ffjord_chain_ref as CR
from tests import ffjord_track_ref as T

TOL = 1e-5
# (dims, acts, time_dep, seed, per-layer factors on the parameters): tests/test_gpu_node_tiled.py's recipe for error-limited solves (a fast
# right-hand side of modest size), so that the saved values carry weight next to the end state.  td2 and pad_td_rej contain natural rejections.
CASES = {
    "td2": ([2, 10, 2], ["tanh", "identity"], True, 1, (60.0, 0.3)),
    "plain6": ([6, 9, 6], ["tanh", "identity"], False, 1, (60.0, 0.3)),
    "pad_td_rej": ([3, 7, 3], ["tanh", "identity"], True, 2, (240.0, 0.1)),
}
B = 5


def _inputs(name):
    dims, acts, td, seed, factors = CASES[name]
    rng = np.random.default_rng(seed)
    p = A.params(dims, td, rng, bias=0.3)
    o = 0
    for l, f in enumerate(factors):
        n = (dims[l] + (1 if td else 0)) * dims[l + 1] + dims[l + 1]
        p[o:o + n] *= f
        o += n
    x = rng.uniform(-1.0, 1.0, (B, dims[0])).astype(np.float32)
    ub = rng.standard_normal((B, dims[0]))
    return dims, acts, td, p.astype(np.float64), x.astype(np.float64), ub


@functools.lru_cache(maxsize=None)
def _oracle_grads(name, track_ctrl):
    from oracle.oracle import Oracle, make_arch
    dims, acts, td, p, x, ub = _inputs(name)
    orc = Oracle(make_arch(dims, acts, td), np.float64, TOL, TOL, reg_kind=1, cb_save_start=0, track_ctrl=track_ctrl, track_initdt=0, max_attempts=256)
    r = orc.forward(x, p)
    assert r["rc"] == 0
    xb, pb, _ = orc.backward(ub, np.ones(len(r["saveval"])))
    return xb, pb, r


@functools.lru_cache(maxsize=None)
def _reference_grads(name):
    dims, acts, td, p, x, ub = _inputs(name)
    r = _oracle_grads(name, 1)[2]
    log = [(float(s[0]), float(s[1]), int(s[3])) for s in r["steps"]]
    P, X = torch.from_numpy(p).requires_grad_(True), torch.from_numpy(x).requires_grad_(True)
    u, eests, dts, info = T.solve_tracked(lambda v, t: T.chain(dims, acts, td, P, v, t), X, 0.0, 1.0, log, TOL, TOL)
    sv = T.saved_values(eests, dts, info["accepted"])
    gx, gp = torch.autograd.grad((u * torch.from_numpy(ub)).sum() + sum(sv), (X, P))
    return gx.numpy(), gp.numpy(), u.detach().numpy(), np.array([float(s) for s in sv]), info


@pytest.mark.parametrize("name", list(CASES))
def test_reference_equals_the_oracles_tracked_reverse(name):
    """p-bar and x-bar of the restatement along the oracle's own log equal Oracle(..., float64, track_ctrl=1, track_initdt=0).backward to 1e-8
    (both fp64; measured 3e-10 at the most), and so do the end state and the saved values."""
    xb, pb, r = _oracle_grads(name, 1)
    gx, gp, u, sv, info = _reference_grads(name)
    devs = (A.rel(u, r["u"]), A.rel(sv, r["saveval"]), A.rel(gp, pb), A.rel(gx, xb))
    print(name, "attempts", len(info["accepted"]), "rejected", info["accepted"].count(False), "u / saved values / p-bar / x-bar:", devs)
    assert max(devs) <= 1e-8, devs
    if name in ("td2", "pad_td_rej"):
        assert False in info["accepted"]            # the natural rejection these inputs were chosen for


@pytest.mark.parametrize("name", list(CASES))
def test_constant_step_oracle_is_far_from_the_tracked_reference(name):
    """The same comparison with track_ctrl = 0 in the oracle is off by more than 0.2 (measured 0.74, 0.68, 0.90 in p-bar): the inputs tell the two
    sweeps apart."""
    xb, pb, _ = _oracle_grads(name, 0)
    gx, gp = _reference_grads(name)[:2]
    devs = (A.rel(pb, gp), A.rel(xb, gx))
    print(name, "constant-step oracle against the tracked reference, p-bar / x-bar:", devs)
    assert min(devs) > 0.2, devs


def test_chain_restatement_with_t_in_the_graph_keeps_the_values():
    """ffjord_track_ref.chain_rhs is ffjord_chain_ref.rhs with t kept as a tensor: the same values (Hutchinson and exact), and a time derivative
    that agrees with a central difference of the original."""
    dims, acts, td = [2, 10, 2], ["tanh", "identity"], True
    p, x, e, _ = CR.draw(dims, td, 5, 3, 2.0)
    P, U, E = p.double(), CR.aug(x.double()), e.double()
    for probe in (E, None):
        a, b = T.chain_rhs(dims, acts, td, P, U, 0.37, probe), CR.rhs(dims, acts, td, P, U, 0.37, probe)
        assert A.rel(a.detach().numpy(), b.detach().numpy()) <= 1e-14
    t = torch.tensor(0.37, dtype=torch.float64, requires_grad=True)
    w = torch.linspace(0.5, 1.5, U.numel(), dtype=torch.float64).view_as(U)
    g = torch.autograd.grad((T.chain_rhs(dims, acts, td, P, U, t, E) * w).sum(), t)[0]
    h = 1e-6
    fd = ((CR.rhs(dims, acts, td, P, U, 0.37 + h, E) - CR.rhs(dims, acts, td, P, U, 0.37 - h, E)) * w).sum() / (2 * h)
    assert abs(float(g) - float(fd)) <= 1e-7 * max(1.0, abs(float(fd))), (float(g), float(fd))


def test_python_layer_refuses_track_ctrl_before_a_device(rnde):
    ff = rnde.ffjord
    m = ff.MLPDynamics(2, 16)
    with pytest.raises(ValueError, match="one-workgroup engine.*tiled"):
        ff.TrackedFFJORD(m, [0.0, 1.0], True, True, engine="workgroup", track_ctrl=True)
    with pytest.raises(ValueError, match=r"no saved value.*O\(tol\).*2e-10 to 2e-6"):
        ff.TrackedFFJORD(m, [0.0, 1.0], True, False, engine="tiled", track_ctrl=True)
    chain = rnde.TDChain(rnde.Dense(3, 10, "tanh"), rnde.Dense(11, 2))
    with pytest.raises(ValueError, match="no saved value"):
        ff.TrackedFFJORD(chain, [0.0, 1.0], True, False, engine="tiled", track_ctrl=True)
    ff.check_track_ctrl_served("tiled", True)
    # track_ctrl=False builds everywhere as before: nothing new is refused (without a GPU the constructor then stops only for want of a device)
    for engine, reg in (("workgroup", True), ("workgroup", False), ("tiled", True), ("tiled", False)):
        try:
            layer = ff.TrackedFFJORD(m, [0.0, 1.0], True, reg, engine=engine, track_ctrl=False)
            assert layer.track_ctrl is False
        except ValueError:
            raise
        except (RuntimeError, AssertionError):
            assert not torch.cuda.is_available()


def test_c_entries_exist_and_answer_null(rnde):
    L = rnde._lib.lib()
    assert L.rnde_ffjord_track_ctrl(None) == -1
    assert L.rnde_ffjord_set_track_ctrl(None, 1) == rnde._lib.BAD_ARG
