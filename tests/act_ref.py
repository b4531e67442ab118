"""fp64 torch restatements of the Dense activations (include/rnde.h: rnde_act) and of what the kernels compute with them: a chain evaluation, a
Tsit5 solve along a given attempt sequence and an SRI attempt with diagonal noise.  Shared by the activation tests; each restatement is checked
against the CPU oracle on tanh chains before it is trusted with anything else (tests/test_gpu_activations.py)."""
import math

import numpy as np
import torch

# the codes of include/rnde.h, by the names the Python layer takes
CODES = {"identity": 0, "tanh": 1, "relu": 2, "sigmoid": 3, "softplus": 4, "elu": 5}
NEW = ("relu", "sigmoid", "softplus", "elu")


def act_fwd(name, z):
    """The forward formulas include/rnde.h documents, in the precision of z (autograd differentiates them)."""
    if name == "identity":
        return z
    if name == "tanh":
        return torch.tanh(z)
    if name == "relu":
        return torch.where(z < 0, torch.zeros_like(z), z)
    t = torch.exp(-z.abs())
    if name == "sigmoid":
        return torch.where(z >= 0, 1 / (1 + t), t / (1 + t))
    if name == "softplus":
        return torch.log1p(t) + torch.clamp(z, min=0)
    if name == "elu":
        return torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0)))
    raise KeyError(name)


def act_dy(name, y):
    """The derivative as the reverse kernels form it: from the layer's output y."""
    if name == "identity":
        return torch.ones_like(y)
    if name == "tanh":
        return 1 - y * y
    if name == "relu":
        return (y > 0).to(y.dtype)
    if name == "sigmoid":
        return y * (1 - y)
    if name == "softplus":
        return -torch.expm1(-y)
    if name == "elu":
        return torch.where(y > 0, torch.ones_like(y), y + 1)
    raise KeyError(name)


def pre_map(pre, u):
    return torch.tanh(u) if pre == 1 else (u ** 3 if pre == 2 else u)


def chain64(dims, acts, time_dep, pre, p, u, t, preacts=None):
    """Flux re(p)(pre.(u)) in fp64: u (B, D); layer l's W is the (in [+1], out) row-major view of its destructure slice.  preacts (a list): every
    layer's pre-activation is appended to it (the kink checks of relu / elu)."""
    x, o = pre_map(pre, u), 0
    for l in range(len(acts)):
        n_in, n_out = dims[l] + (1 if time_dep else 0), dims[l + 1]
        W = p[o:o + n_in * n_out].view(n_in, n_out)
        o += n_in * n_out
        b = p[o:o + n_out]
        o += n_out
        if time_dep:
            x = torch.cat([x, torch.full((x.shape[0], 1), float(t), dtype=x.dtype)], dim=1)
        z = x @ W + b
        if preacts is not None:
            preacts.append(z.detach())
        x = act_fwd(acts[l], z)
    return x


def params(dims, time_dep, rng, scale=1.0, bias=0.1):
    parts = []
    for l in range(len(dims) - 1):
        n_in, n_out = dims[l] + (1 if time_dep else 0), dims[l + 1]
        lim = scale * math.sqrt(6.0 / (n_in + n_out))
        parts += [rng.uniform(-lim, lim, n_in * n_out), bias * rng.standard_normal(n_out)]
    return np.concatenate(parts).astype(np.float32)


def rk_replay64(f, x, attempts, tab):
    """An explicit first-same-as-last pair along given attempts (t, dt, accepted), fp64: k1 = f(u, t0); each attempt forms the stages
    k_s = f(u + dt sum_j a[s][j] k_j, t + c_s dt) and, when accepted, u += dt sum_j a[S-1][j] k_j and k1 = k_S."""
    a, c, _ = tab
    S = len(c)
    u = x
    k1 = f(u, float(attempts[0][0]) if attempts else 0.0)
    for t, dt, acc in attempts:
        k = [k1]
        for s in range(1, S):
            g = u + dt * sum(float(a[s][j]) * k[j] for j in range(s) if a[s][j] != 0)
            k.append(f(g, t + float(c[s]) * dt))
        if acc:
            u = u + dt * sum(float(a[S - 1][j]) * k[j] for j in range(S - 1) if a[S - 1][j] != 0)
            k1 = k[S - 1]
    return u


def sri_attempt64(tab, drift, diff, u, dt, dW, dZ):
    """One SRI attempt with diagonal noise in fp64 (drift, diff: u -> value); returns (k[4], g[4], unew)."""
    sq = math.sqrt(abs(dt))
    chi2 = (dW + dZ / math.sqrt(3.0)) / 2
    k, g = [], []
    for s in range(4):
        h0 = u + sum(dt * float(tab["A0"][s][j]) * k[j] + chi2 * float(tab["B0"][s][j]) * g[j] for j in range(s)) if s else u
        h1 = u + sum(dt * float(tab["A1"][s][j]) * k[j] + sq * float(tab["B1"][s][j]) * g[j] for j in range(s)) if s else u
        k.append(drift(h0))
        g.append(diff(h1))
    chi1 = (dW * dW - abs(dt)) / (2 * sq)
    chi3 = (dW ** 3 - 3 * dW * dt) / (6 * dt)
    sa = sum(float(tab["alpha"][j]) * k[j] for j in range(4))
    s1, s2, s3, s4 = (sum(float(tab[b][j]) * g[j] for j in range(4)) for b in ("beta1", "beta2", "beta3", "beta4"))
    return k, g, u + dt * sa + chi2 * s3 + chi3 * s4 + dW * s1 + chi1 * s2


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
