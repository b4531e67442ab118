"""torch restatement of what the tracked-controller reverse sweep of TrackedFFJORD differentiates (rnde_ffjord_set_track_ctrl; track_ctrl = 1,
track_initdt = 0): Tsit5 attempts over a given right-hand side along a per-attempt log (t, dt, accepted), with the PI controller of
rnde_fwd.h::advance_state_t written differentiably.  Branch decisions (clamp to t1, the clips of q, qold' = max(EEst, qoldinit), the dtmax
clamp, accept / reject) are re-derived from the restatement's own values; every dt_n and t_n is tied to the logged value straight-through,
dt_ctrl + (dt_log - dt_ctrl).detach(): values are the log's (the device's), derivatives are the controller's.  The initial step is a
constant, and so are t0 and t1.  Runs in the precision of its inputs (fp64 as the reference, fp32 for the rounding yardstick).

The right-hand sides are those of tests/ffjord_chain_ref.py::rhs and tests/ffjord_ref.py::rhs.  The ConcatSquash one is differentiable in t
as it stands.  act_ref.chain64 appends float(t) to a TDChain layer's input, which cuts t out of the graph, so chain / chain_rhs below restate
it with t kept as a tensor; tests/test_ffjord_track_host.py pins the two to the same values.

Used by tests/test_ffjord_track_host.py (which pins the restatement to the fp64 oracle's track_ctrl = 1 reverse pass) and
tests/test_gpu_ffjord_track.py (which compares the device against it)."""
import torch

from tests import act_ref as A
from tests import ffjord_ref as R


def chain(dims, acts, td, p, u, t):
    """act_ref.chain64 without a leading map, differentiable in t (a tensor or a number)."""
    x, o = u, 0
    tt = torch.as_tensor(t, dtype=u.dtype)
    for l in range(len(acts)):
        n_in, n_out = dims[l] + (1 if td else 0), dims[l + 1]
        W = p[o:o + n_in * n_out].view(n_in, n_out)
        o += n_in * n_out
        b = p[o:o + n_out]
        o += n_out
        if td:
            x = torch.cat([x, tt * torch.ones((x.shape[0], 1), dtype=x.dtype)], dim=1)
        x = A.act_fwd(acts[l], x @ W + b)
    return x


def chain_rhs(dims, acts, td, p, u, t, e=None):
    """ffjord_chain_ref.rhs with t in the graph: [f(z, t); -e . eJ] of u = [z; l] (B, D + 1); e = None: the exact trace by D unit probes."""
    D = dims[0]
    z = u[:, :D]

    def f_eJ(probe):
        with torch.enable_grad():
            zz = z if z.requires_grad else z.detach().requires_grad_(True)
            f = chain(dims, acts, td, p, zz, t)
            return f, torch.autograd.grad(f, zz, probe, create_graph=True)[0]

    if e is not None:
        f, eJ = f_eJ(e)
        tr = (e * eJ).sum(1)
    else:
        tr = 0.0
        for i in range(D):
            ei = torch.zeros_like(z)
            ei[:, i] = 1.0
            f, eJ = f_eJ(ei)
            tr = tr + eJ[:, i]
    return torch.cat([f, -tr[:, None]], 1)


def _tie(v, logged):
    """The logged value, with v's derivative."""
    return v + (logged - v).detach()


def solve_tracked(F, u0, t0, t1, log, reltol, abstol, accept_from_log=False, next_dtp=None, track=True):
    """Tsit5 along log = [(t, dt, accepted), ...] (every attempt, in order) with the controller differentiated.

    Returns (u_end, [EEst_n], [dt_n], info): EEst and dt of EVERY attempt (dt tied to the log), info = dict(accepted=[...], qg=[q / gamma before
    the clips, None where EEst = 0], clamped=[...]).  Accept decisions come from the restatement's own EEst <= 1 and must agree with the log;
    accept_from_log: a replayed sequence, where the log decides (differentiated as if the controller had produced it).  next_dtp (replay): the
    value the proposed step of attempt n is tied to, per attempt -- the replayed sizes (without it only dt is tied, to the log).  track=False:
    step sizes and times are constants (the constant-step sweep's function), everything else unchanged."""
    dt_of = lambda v: torch.as_tensor(v, dtype=u0.dtype)
    t1c, dtmax = dt_of(t1), dt_of(t1 - t0)
    u, k1 = u0, F(u0, dt_of(t0))
    t, dtp, qold = dt_of(t0), dt_of(log[0][1]), dt_of(R.QOLDINIT)
    eests, dts, info = [], [], dict(accepted=[], qg=[], clamped=[])
    for n, (t_log, dt_log, acc_log) in enumerate(log):
        t = _tie(t, dt_of(t_log))
        clamped = bool(t1c - t < dtp)
        dt = _tie(t1c - t if clamped else dtp, dt_of(dt_log))
        if not track:
            t, dt = t.detach(), dt.detach()
        unew, k, err = R.tsit5_step(F, u, t, dt, k1)
        e = R.eest_of(u, unew, err, reltol, abstol)
        ev = float(e.detach())
        accepted = bool(acc_log) if accept_from_log else ev <= 1.0
        assert accepted == bool(acc_log), (n, ev, acc_log)
        eests.append(e); dts.append(dt)
        info["accepted"].append(accepted); info["clamped"].append(clamped)
        q11 = e ** R.BETA1 if ev > 0.0 else None
        if ev == 0.0:
            q, qg = dt_of(1.0 / R.QMAX), None
        else:
            qgt = q11 / qold ** R.BETA2 / R.GAMMA
            qg = float(qgt.detach())
            q = dt_of(1.0 / R.QMAX) if qg < 1.0 / R.QMAX else (dt_of(1.0 / R.QMIN) if qg > 1.0 / R.QMIN else qgt)
        info["qg"].append(qg)
        if accepted:
            qold = e if ev > R.QOLDINIT else dt_of(R.QOLDINIT)
            dtp = dt / q
            t, u, k1 = t + dt, unew, k[6]
        else:
            m = dt_of(1.0 / R.QMIN)
            if q11 is not None and float(q11.detach()) / R.GAMMA < 1.0 / R.QMIN:
                m = q11 / R.GAMMA
            dtp = dt / m
        if float(dtmax) < float(dtp.detach()):
            dtp = dtmax
        if next_dtp is not None and n + 1 < len(log):
            dtp = _tie(dtp, dt_of(next_dtp[n + 1]))
    return u, eests, dts, info


def saved_values(eests, dts, accepted):
    """EEst_n dt_n of the accepted attempts (the SavingCallback's values, without the leading zero of cb_save_start)."""
    return [e * d for e, d, a in zip(eests, dts, accepted) if a]
