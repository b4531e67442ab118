"""torch restatements of TrackedFFJORD's default dynamics (reference src/models/ffjord.jl:21-27: Tracker.forward(z -> m(z, t), z), then
back(e)) for a Dense chain, plain or TDChain.  f is tests/act_ref.chain64; eJ is torch.autograd.grad(f, z, e, create_graph=True), which is
literally Tracker.forward + back; the exact trace is D unit probes (the reference's jacobian_fn).  Tsit5, replay, the controller and logpx are
those of tests/ffjord_ref.py (generic in F); the kinetic rows are appended as in tests/ffjord_kinetic_ref.py.  The restatements run in the
precision of their inputs (fp64 as the reference, fp32 for the rounding yardstick).  Used by tests/test_ffjord_chain_host.py (which checks
them against torch.autograd.functional.jacobian) and tests/test_gpu_ffjord_chain.py (which compares the device against them)."""
import numpy as np
import torch

from tests import act_ref as A

LATENT = [20, 50, 20, 50, 20, 50, 20, 50, 20]


def draw(dims, td, B, seed, scale, xscale=1.0):
    """The input recipe: rng = default_rng(seed); p = act_ref.params(dims, td, rng, scale); x, e = standard normals (B, D), float32."""
    rng = np.random.default_rng(seed)
    p = torch.from_numpy(A.params(dims, td, rng, scale=scale))
    x = torch.from_numpy(rng.standard_normal((B, dims[0])).astype(np.float32) * np.float32(xscale))
    e = torch.from_numpy(rng.standard_normal((B, dims[0])).astype(np.float32))
    return p, x, e, rng


def f_eJ(dims, acts, td, p, z, t, e, preacts=None):
    """(f, eJ): f = m(z, t), eJ = back(e) -- differentiable in p and z (create_graph)."""
    with torch.enable_grad():
        zz = z if z.requires_grad else z.detach().requires_grad_(True)
        f = A.chain64(dims, acts, td, 0, p, zz, t, preacts)
        eJ = torch.autograd.grad(f, zz, e, create_graph=True)[0]
    return f, eJ


def rhs(dims, acts, td, p, u, t, e=None, preacts=None):
    """[f(z, t); -e . eJ] of u = [z; l] (B, D + 1).  e = None: the exact trace by D unit probes."""
    D = dims[0]
    z = u[:, :D]
    if e is not None:
        f, eJ = f_eJ(dims, acts, td, p, z, t, e, preacts)
        tr = (e * eJ).sum(1)
    else:
        tr = 0.0
        for i in range(D):
            ei = torch.zeros_like(z)
            ei[:, i] = 1.0
            f, eJ = f_eJ(dims, acts, td, p, z, t, ei)
            tr = tr + eJ[:, i]
    return torch.cat([f, -tr[:, None]], 1)


def rhs_kinetic(dims, acts, td, p, u, t, e, preacts=None):
    """[f; -e . eJ; sum f^2; sum eJ^2] of u = [z; l; lambda1; lambda2] (B, D + 3) (ffjord.jl:53-66)."""
    f, eJ = f_eJ(dims, acts, td, p, u[:, :dims[0]], t, e, preacts)
    return torch.cat([f, -(e * eJ).sum(1, keepdim=True), (f * f).sum(1, keepdim=True), (eJ * eJ).sum(1, keepdim=True)], 1)


def aug(x, rows=1):
    return torch.cat([x, torch.zeros(x.shape[0], rows, dtype=x.dtype)], 1)


def d2y(name, y):
    """phi'' from the layer's output y: the hand formulas the reverse kernel uses (rnde_device.h::act_d2y)."""
    if name == "tanh":
        return -2 * y * (1 - y * y)
    if name == "sigmoid":
        return y * (1 - y) * (1 - 2 * y)
    if name == "softplus":
        s = -torch.expm1(-y)
        return s * (1 - s)
    if name == "elu":
        return torch.where(y > 0, torch.zeros_like(y), y + 1)
    return torch.zeros_like(y)


def kink_margin(acts, preacts):
    """Smallest |pre-activation| over the relu / elu layers of the evaluations recorded in preacts (a flat list, n layers per evaluation)."""
    n = len(acts)
    m = [float(z.abs().min()) for i, z in enumerate(preacts) if acts[i % n] in ("relu", "elu")]
    return min(m) if m else float("inf")
