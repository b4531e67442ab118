"""fp64 torch restatement of TrackedFFJORD{false} called with regularize = true (reference src/models/ffjord.jl:53-66 with forw_n_back of
experiments/ffjord_gaussian.jl:98-107): the state [z; l; lambda1; lambda2] with d lambda1 / dt = sum f^2 (kinetic energy) and
d lambda2 / dt = sum eJ^2 (Hutchinson estimate of the Jacobian's Frobenius norm).  The Tsit5 step, replay, solve, eest_of and logpx_of are
those of tests/ffjord_ref.py.  Used by tests/test_ffjord_kinetic_host.py (which checks it against torch.autograd.functional.jacobian) and
tests/test_gpu_ffjord_kinetic.py (which compares the device against it)."""
import math

import numpy as np
import torch

from tests import ffjord_ref as R


def rhs_kinetic(p, D, H, u, t, e):
    """[f(z, t); -e . eJ; sum f^2; sum eJ^2] of u = [z; l; lambda1; lambda2] (B, D + 3)."""
    f, eJ = R.vjp(p, D, H, u[:, :D], t, e)
    return torch.cat([f, -(e * eJ).sum(1, keepdim=True), (f * f).sum(1, keepdim=True), (eJ * eJ).sum(1, keepdim=True)], 1)


def aug(x, rows):
    """[x; 0 ...] with `rows` zero rows appended (1: the plain state, 3: the kinetic one)."""
    return torch.cat([x, torch.zeros(x.shape[0], rows, dtype=x.dtype)], 1)


def draw(D, H, B, seed, scale, xscale=1.0):
    """Inputs as the FFJORD GPU tests draw them: parameters, x, e from one generator in that order, float32.  Returns (p, x, e, rng)."""
    rng = np.random.default_rng(seed)
    p = torch.from_numpy(R.glorot_params(D, H, rng, scale=scale))
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32) * np.float32(xscale))
    e = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32))
    return p, x, e, rng


def initial_dt(F, u0, t0, t1, reltol, abstol):
    """The first attempted step of R.solve (OrdinaryDiffEq's initial-step rule) over all rows of u0."""
    with torch.no_grad():
        N = u0.numel()
        sk = abstol + u0.abs() * reltol
        f0 = F(u0, t0)
        d0, d1 = float(torch.sqrt(((u0 / sk) ** 2).sum() / N)), float(torch.sqrt(((f0 / sk) ** 2).sum() / N))
        dtmax = t1 - t0
        dt0 = min(1e-6 if (d0 < 1e-5 or d1 < 1e-5) else (d0 / d1) / 100.0, dtmax)
        f1 = F(u0 + dt0 * f0, t0 + dt0)
        d2 = float(torch.sqrt((((f1 - f0) / sk) ** 2).sum() / N)) / dt0
        m = max(d1, d2)
        dt1 = max(1e-6, dt0 * 1e-3) if m <= 1e-15 else 10.0 ** (-(2.0 + math.log10(m)) / 5.0)
        return min(100.0 * dt0, dt1, dtmax)


def eests_along(F, u0, t0, seq, reltol, abstol, rows=None):
    """EEst of every attempt along a given (dt, accepted) sequence (a rejected attempt leaves the state where it was).  Returns
    (u_end, [EEst]); with rows, also the list of the norm over the first `rows` rows only."""
    with torch.no_grad():
        u, t, k1, out, part = u0, t0, F(u0, t0), [], []
        for dt, acc in seq:
            unew, k, err = R.tsit5_step(F, u, t, dt, k1)
            out.append(float(R.eest_of(u, unew, err, reltol, abstol)))
            if rows is not None:
                part.append(float(R.eest_of(u[:, :rows], unew[:, :rows], err[:, :rows], reltol, abstol)))
            if acc:
                u, t, k1 = unew, t + dt, k[6]
        return (u, out) if rows is None else (u, out, part)
