"""fp64 torch restatements of TrackedFFJORD with the ConcatSquash MLPDynamics (reference experiments/ffjord_gaussian.jl:39-107,
src/models/ffjord.jl): the augmented right-hand side, Tsit5 along a given step sequence, the adaptive controller, and
Optimiser(WeightDecay, ADAM).  Used by tests/test_ffjord_host.py (which checks each restatement against something independent first)
and tests/test_gpu_ffjord.py (which compares the device against them)."""
import math

import numpy as np
import torch

# Tsit5 (Tsitouras 2011): a[s][j], c[s], embedded error weights bt[j]
TS_A = [[0.0],
        [0.161],
        [-0.008480655492356989, 0.335480655492357],
        [2.8971530571054935, -6.359448489975075, 4.3622954328695815],
        [5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525],
        [5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383],
        [0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774]]
TS_C = [0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0]
TS_BT = [-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629, 0.5823571654525552,
         -0.45808210592918697, 0.015151515151515152]
BETA1, BETA2, GAMMA, QMIN, QMAX, QOLDINIT = 7.0 / 50.0, 2.0 / 25.0, 0.9, 0.2, 10.0, 1e-4


def param_count(D, H):
    return (H * D + 4 * H) + (H * H + 4 * H) + (D * H + 4 * D)


def unpack(p, D, H):
    """Flux.destructure order per ConcatSquashLinear: layer_W (out x in, column-major), layer_B, bias_W, bias_B, gate_W."""
    out, o = [], 0
    for n_in, n_out in ((D, H), (H, H), (H, D)):
        W = p[o:o + n_in * n_out].view(n_in, n_out).t()          # column-major (out, in)
        o += n_in * n_out
        b, bw, bb, gw = (p[o + k * n_out:o + (k + 1) * n_out] for k in range(4))
        o += 4 * n_out
        out.append((W, b, bw, bb, gw))
    assert o == p.numel()
    return out


def sig(x):
    """ffjord_gaussian.jl:39-42"""
    t = torch.exp(-x.abs())
    return torch.where(x >= 0, 1.0 / (1.0 + t), t / (1.0 + t))


def softplus(x):
    """ffjord_gaussian.jl:44"""
    return torch.where(x > 0, x + torch.log1p(torch.exp(-x.clamp(min=0))), torch.log1p(torch.exp(x.clamp(max=0))))


def mlp(p, D, H, z, t):
    """MLPDynamics(z, t): z (B, D) -> (B, D), plus the pre-activations h1, h2 and the gates."""
    L = unpack(p, D, H)
    hs, gates, x = [], [], z
    for l, (W, b, bw, bb, gw) in enumerate(L):
        s = sig(gw * t)
        h = (x @ W.t() + b) * s + (bw * t + bb)
        gates.append(s)
        hs.append(h)
        x = softplus(h) if l < 2 else h
    return x, hs, gates, L


def vjp(p, D, H, z, t, e):
    """(f, eJ) as forw_n_back builds them (ffjord_gaussian.jl:98-107): eJ = W1' (s1 sig(h1) W2' (s2 sig(h2) W3' (s3 e)))."""
    f, (h1, h2, _), (s1, s2, s3), L = mlp(p, D, H, z, t)
    W1, W2, W3 = L[0][0], L[1][0], L[2][0]
    v = (e * s3) @ W3
    v = (v * sig(h2) * s2) @ W2
    eJ = (v * sig(h1) * s1) @ W1
    return f, eJ


def rhs(p, D, H, u, t, e=None):
    """Augmented right-hand side [f(z, t); -e . eJ] of u = [z; l] (B, D + 1).  e = None: the exact trace (D unit probes, jacobian_fn)."""
    z = u[:, :D]
    if e is not None:
        f, eJ = vjp(p, D, H, z, t, e)
        tr = (e * eJ).sum(1)
    else:
        tr = 0.0
        for i in range(D):
            ei = torch.zeros_like(z)
            ei[:, i] = 1.0
            f, eJ = vjp(p, D, H, z, t, ei)
            tr = tr + eJ[:, i]
    return torch.cat([f, -tr[:, None]], 1)


def logpx_of(u, D):
    z = u[:, :D]
    return (-(math.log(2 * math.pi) + z * z) / 2).sum(1) - u[:, D]


def tsit5_step(F, u, t, dt, k1):
    """One attempt: stages k1..k7, unew, the embedded error vector dt sum bt k."""
    k = [k1]
    for s in range(1, 7):
        g = u + dt * sum(TS_A[s][j] * k[j] for j in range(s))
        if s == 6:
            unew = g
        k.append(F(g, t + TS_C[s] * dt))
    err = dt * sum(TS_BT[j] * k[j] for j in range(7))
    return unew, k, err


def eest_of(u, unew, err, reltol, abstol):
    sk = abstol + torch.maximum(u.abs(), unew.abs()) * reltol
    return torch.sqrt(((err / sk) ** 2).mean())


def replay(F, u0, t0, dts, reltol, abstol):
    """Tsit5 along a given all-accepted step sequence: (u_end, [EEst of every step]) -- differentiable, step sizes are constants."""
    u, t, k1 = u0, t0, F(u0, t0)
    eests = []
    for dt in dts:
        unew, k, err = tsit5_step(F, u, t, dt, k1)
        eests.append(eest_of(u, unew, err, reltol, abstol))
        u, t, k1 = unew, t + dt, k[6]
    return u, eests


def solve(F, u0, t0, t1, reltol, abstol, max_attempts=100000):
    """The adaptive solve with OrdinaryDiffEq's initial-step rule and PI controller, as the chain engine states them (rnde_fwd.h), in fp64.
    Returns (u_end, [(t, dt, EEst, accepted)])."""
    with torch.no_grad():
        N = u0.numel()
        sk = abstol + u0.abs() * reltol
        f0 = F(u0, t0)
        d0, d1 = float(torch.sqrt(((u0 / sk) ** 2).sum() / N)), float(torch.sqrt(((f0 / sk) ** 2).sum() / N))
        dtmax = t1 - t0
        dt0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else (d0 / d1) / 100.0
        dt0 = min(dt0, dtmax)
        f1 = F(u0 + dt0 * f0, t0 + dt0)
        d2 = float(torch.sqrt((((f1 - f0) / sk) ** 2).sum() / N)) / dt0
        m = max(d1, d2)
        dt1 = max(1e-6, dt0 * 1e-3) if m <= 1e-15 else 10.0 ** (-(2.0 + math.log10(m)) / 5.0)
        dtp = min(100.0 * dt0, dt1, dtmax)
        u, t, k1, qold, log = u0, t0, f0, QOLDINIT, []
        while t < t1:
            if len(log) >= max_attempts:
                raise RuntimeError("max_attempts")
            dt = min(dtp, t1 - t)
            unew, k, err = tsit5_step(F, u, t, dt, k1)
            e = float(eest_of(u, unew, err, reltol, abstol))
            if e == 0.0:
                q = 1.0 / QMAX
            else:
                q11 = e ** BETA1
                q = min(max(q11 / qold ** BETA2 / GAMMA, 1.0 / QMAX), 1.0 / QMIN)
            if e <= 1.0:
                log.append((t, dt, e, True))
                qold = max(e, QOLDINIT)
                t, u, k1 = t + dt, unew, k[6]
                dtp = min(dt / q, dtmax)
            else:
                log.append((t, dt, e, False))
                dtp = min(dt / min(1.0 / QMIN, (e ** BETA1) / GAMMA), dtmax)
        return u, log


def flux_adam_wd(p, g, m, v, t, eta, beta=(0.9, 0.999), eps=1e-8, wd=0.0):
    """Flux.Optimise.Optimiser(WeightDecay(wd), ADAM(eta, beta)): g += wd p, then ADAM with bias correction.  Returns (p, m, v)."""
    g = g + wd * p
    m = beta[0] * m + (1 - beta[0]) * g
    v = beta[1] * v + (1 - beta[1]) * g * g
    step = eta * (m / (1 - beta[0] ** t)) / (torch.sqrt(v / (1 - beta[1] ** t)) + eps)
    return p - step, m, v


def glorot_params(D, H, rng, scale=1.0, bias=0.1):
    """Random parameters in the destructure layout (Glorot weights; small nonzero biases so every term is exercised)."""
    parts = []
    for n_in, n_out in ((D, H), (H, H), (H, D)):
        lim = scale * math.sqrt(6.0 / (n_in + n_out))
        parts += [rng.uniform(-lim, lim, n_in * n_out), bias * rng.standard_normal(n_out), rng.uniform(-1, 1, n_out),
                  bias * rng.standard_normal(n_out), rng.uniform(-1.5, 1.5, n_out)]
    return np.concatenate(parts).astype(np.float32)
