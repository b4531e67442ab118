"""Inputs at which the latent-ODE caller (csrc/rnde_latent.h) can go wrong, the fp64 restatement's outputs for them, and the error measure --
shared by tests/test_latent_cases_host.py (what the inputs reach, with the oracle alone) and tests/test_gpu_latent_ragged.py (the device).

`build(B, T, seed, ragged=, gates=, lv_shift=)` returns (S, x, p1, p2, p4, eps, res, z0b) in fp64, in the layout of test_gpu_latent._case, every
value already rounded to fp32 (the device is handed the same numbers the oracle sees).  Three independent switches:

ragged    a keep table per (sample, save time), each entry kept with probability 0.35: irregularly sampled series, another set of empty steps
          per sample (reference experiments/latent_ode.jl:84-87 keeps a sample's state where it observed nothing).  Every sample keeps a step.
          B >= 3: sample 0 keeps only t = T - 1 (the first step the GRU processes), sample 1 only t = 0.
          B >= 5: sample 2 has one observed entry in all (sum(mask) = 1), sample B - 1 every entry.
          B > 16 (T >= 3): the save time T // 2 is empty for all of columns 0..15 and observed in column 16 (an empty tile next to a live one).
          At a dropped (b, t) rows 37..74 are zero; the data rows are multiplied by the mask everywhere.
          B >= 7, T >= 5: the two quirks of the reference's rule `sum(x[38:end, :]) > 0`, which counts the time row -- at one dropped entry of
          samples 3 and 5 dt = 0.02 under an all-zero mask (the GRU takes the step, the likelihood's count does not see it); at one kept
          entry of samples 4 and 6 dt = 0.  `quirks(...)` names those entries.
gates     g1: the first layer of the update and of the reset gate times g1, and [-100, -12, -6, 0, 0, 6, 12, 100, 0, 0] tiled over the 50 rows
          of both gates' output bias (rolled by 3 for the reset gate).  The new-state stack stays at scale 1: the recurrence is not chaotic,
          the gates are saturated (+-100 is past sigmoid_f's clamp at 87; +-12, +-6 put u (1 - u) at 6e-6, 2.5e-3).
lv_shift  a constant added to the last 20 biases of p2, the logvar rows.
"""
import numpy as np

from oracle import latent_oracle as lo

GATE_PATTERN = np.array([-100.0, -12.0, -6.0, 0.0, 0.0, 6.0, 12.0, 100.0, 0.0, 0.0])
KEEP_P = 0.35
LAM_K = 0.7
# outputs compared sample by sample (the error of sample b over the largest entry of sample b); the others over the whole array
PER_SAMPLE = ("mu0", "logvar", "z0", "res-bar")
VALUES = ("mu0", "logvar", "z0", "nll", "kl", "res-bar")
GRU_LAYERS = (("Wu1", 175 * 40 + 40), ("Wu2", 40 * 50 + 50), ("Wr1", 175 * 40 + 40), ("Wr2", 40 * 50 + 50), ("Wn1", 175 * 40 + 40), ("Wn2", 40 * 100 + 100))
GRADIENTS = ("p4-bar", "p2-bar", "p1-bar") + tuple("p1-bar " + n for n, _ in GRU_LAYERS)
TOL_VALUE, TOL_GRAD = 5e-6, 1e-5      # the device's tolerances (tests/test_gpu_latent.py)

# the cases of tests/test_gpu_latent_ragged.py: (B, T, seed, switches)
CASES = [
    (17, 49, 11, dict(ragged=True)),
    (33, 64, 12, dict(ragged=True)),
    (17, 49, 13, dict(ragged=True, gates=4.0)),
    (17, 49, 14, dict(ragged=True, gates=8.0, lv_shift=8.0)),
    (17, 12, 15, dict(ragged=True, gates=4.0, lv_shift=-10.0)),
    (1, 1, 16, dict()),
    (1, 5, 28, dict(ragged=True)),      # (this seed: t = 4 and t = 0 observed, so the reset gate's gradient is not zero)
    (15, 3, 18, dict(ragged=True)),
    (16, 3, 19, dict(ragged=True)),
    (17, 3, 20, dict(ragged=True)),
]


def case_id(c):
    B, T, seed, sw = c
    return f"{B}x{T}" + "".join(f"-{k}{'' if v is True else format(v, 'g')}" for k, v in sw.items())


def round32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _keep_table(rng, B, T):
    keep = rng.uniform(size=(B, T)) < KEEP_P
    if B >= 3:
        keep[0] = False; keep[0, T - 1] = True
        keep[1] = False; keep[1, 0] = True
    if B >= 5:
        keep[2] = False; keep[2, rng.integers(T)] = True
        keep[B - 1] = True
    t_e = T // 2 if (B > 16 and T >= 3) else None
    if t_e is not None:
        keep[:16, t_e] = False
        keep[16, t_e] = True
    for b in range(B):
        if not keep[b].any():
            keep[b, rng.choice([t for t in range(T) if t != t_e or b >= 16])] = True
    return keep, t_e


def quirks(B, T, keep, t_e):
    """((b, t) of the dropped entries that carry dt = 0.02, (b, t) of the kept entries that carry dt = 0): the first such t of each sample."""
    on, off = [], []
    if B >= 7 and T >= 5:
        for b in (3, 5):
            ts = [t for t in range(T) if not keep[b, t] and t != t_e]
            if ts:
                on.append((b, ts[0]))
        for b in (4, 6):
            ts = [t for t in range(T) if keep[b, t]]
            if ts:
                off.append((b, ts[0]))
    return on, off


def build(B, T, seed, ragged=False, gates=None, lv_shift=0.0, with_info=False):
    rng = np.random.default_rng(seed)
    S = lo.GruShape(37, 40, 50)
    x = np.zeros((B, T, 75))
    x[:, :, :37] = rng.standard_normal((B, T, 37))
    mask = (rng.uniform(size=(B, T, 37)) < 0.3).astype(np.float64)
    first = rng.integers(37, size=(B, T))
    np.put_along_axis(mask, first[:, :, None], 1.0, axis=2)                 # an observed step observes something
    dt = 0.002 + np.abs(rng.standard_normal((B, T))) * 0.02
    info = dict(keep=np.ones((B, T), bool), t_empty=None, dt_on=[], dt_off=[])
    if ragged:
        keep, t_e = _keep_table(rng, B, T)
        if B >= 5:
            mask[2] = 0.0; mask[2, np.argmax(keep[2]), first[2, 0]] = 1.0       # sum(mask) = 1
            mask[B - 1] = 1.0                                                # every entry
        mask *= keep[:, :, None]; dt = dt * keep
        on, off = quirks(B, T, keep, t_e)
        for b, t in on:
            dt[b, t] = 0.02
        for b, t in off:
            dt[b, t] = 0.0
        info = dict(keep=keep, t_empty=t_e, dt_on=on, dt_off=off)
    x[:, :, 37:74] = mask
    x[:, :, :37] *= mask if ragged else 1.0
    x[:, :, 74] = dt

    def dense(n_in, n_out, scale=1.0):
        lim = scale * np.sqrt(6.0 / (n_in + n_out))
        return np.concatenate([rng.uniform(-lim, lim, n_in * n_out), scale * rng.uniform(-0.05, 0.05, n_out)])
    g1 = 1.0 if gates is None else float(gates)
    p1 = np.concatenate([dense(175, 40, g1), dense(40, 50), dense(175, 40, g1), dense(40, 50), dense(175, 40), dense(40, 100)])
    if gates is not None:
        pat = np.tile(GATE_PATTERN, 5)
        obu2, obr2 = 175 * 40 + 40 + 40 * 50, 9090 + 175 * 40 + 40 + 40 * 50
        p1[obu2:obu2 + 50] += pat
        p1[obr2:obr2 + 50] += np.roll(pat, 3)
    p2 = np.concatenate([dense(100, 50), dense(50, 40)])
    p2[-20:] += lv_shift
    p4 = dense(20, 37)
    eps = rng.standard_normal((B, 20))
    res = 0.5 * rng.standard_normal((B, T, 20))
    z0b = 0.1 * rng.standard_normal((B, 20))
    out = (S,) + tuple(round32(a) for a in (x, p1, p2, p4, eps, res, z0b))
    return (out, info) if with_info else out


def oracle_outputs(case, dtype=np.float64, lam_k=LAM_K, with_tape=False):
    """Every output the device returns for the three calls, by oracle/latent_oracle.py in `dtype` (every input cast)."""
    S, x, p1, p2, p4, eps, res, z0b = case
    x, p1, p2, p4, eps, res, z0b = (np.asarray(a, dtype=dtype) for a in (x, p1, p2, p4, eps, res, z0b))
    B = x.shape[0]
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):      # exp(100) in fp32 overflows (the intended result); 0 / 0 of an unobserved sample
        y, tape1 = lo.gru_forward(S, p1, x)
        z0, mu0, lv, tape2 = lo.encode_forward(p2, y, eps)
        nll, resb, p4b, ll = lo.decode_loss(p4, res, x[:, :, :37], x[:, :, 37:74])
        kl = lo.kl_per_sample(mu0, lv).mean()
        yb, p2b = lo.encode_backward(p2, tape2, z0b, dtype(lam_k / B))
        p1b = lo.gru_backward(S, p1, tape1, yb)
    out = {"mu0": mu0, "logvar": lv, "z0": z0, "nll": np.array([nll]), "kl": np.array([kl]), "res-bar": resb, "p4-bar": p4b, "p2-bar": p2b, "p1-bar": p1b}
    o = 0
    for name, n in GRU_LAYERS:
        out["p1-bar " + name] = p1b[o:o + n]
        o += n
    out = {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}
    return (out, tape1) if with_tape else out


def rel_errors(got, ref):
    """name -> (error, worst sample or None).  PER_SAMPLE outputs: the largest over b of max|got_b - ref_b| / max|ref_b|; the others: max|got - ref| / max|ref|."""
    errs = {}
    for name, r in ref.items():
        g = np.asarray(got[name], dtype=np.float64).reshape(r.shape)
        if not np.isfinite(g).all():
            errs[name] = (np.inf, None)
        elif name in PER_SAMPLE:
            B = r.shape[0]
            e = np.abs(g - r).reshape(B, -1).max(axis=1) / np.maximum(np.abs(r).reshape(B, -1).max(axis=1), 1e-30)
            errs[name] = (float(e.max()), int(e.argmax()))
        else:
            errs[name] = (float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-30)), None)
    return errs


def tolerance(name):
    return TOL_VALUE if name in VALUES else TOL_GRAD


def check(got, ref, scale=1.0, label=""):
    """Prints every output's error, then asserts each against `scale` times the device's tolerance."""
    errs = rel_errors(got, ref)
    for name, (e, b) in errs.items():
        print(f"{label}{name}: rel err {e:.2e}" + (f" (worst sample {b})" if b is not None else ""))
    bad = {name: (e, b) for name, (e, b) in errs.items() if not e <= scale * tolerance(name)}
    assert not bad, (label, bad)
    return errs
