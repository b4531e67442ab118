"""The latent-ODE caller on the device (csrc/rnde_latent.h, through rnde_latent_encode / _decode_loss / _encode_backward) against the fp64
restatement at the inputs of tests/latent_cases.py: step masks that differ from sample to sample (the per-sample table MK[t * 16 + col] of the
GRU's two kernels), saturated gates driven through the recurrence and its reverse, logvar at +8 and -10, T = 1 and T = 64, B = 1 and the
sizes either side of the 16-column tile, and a handle that serves a small call after a large one.
tests/test_latent_cases_host.py asserts what those inputs reach and that the restatement in float32 is within half of these tolerances.

Tolerances: those of tests/test_gpu_latent.py unchanged (values 5e-6, gradients 1e-5, the six GRU layers one by one); mu0, logvar, z0 and
res-bar sample by sample (one sample's wrong rows do not hide behind the batch), -mean ll and mean KL each on its own (the KL does not hide
behind the likelihood, four orders larger).  The oracle sees the inputs as rounded to fp32.

That these tests see what test_latent_caller_matches_the_fp64_restatement does not (scratch builds, one change each, run once):
  MK[t * 16 + col] -> MK[t * 16] in the forward kernel:  the old test passes (5 cases); here the 8 cases with B >= 15, the handle test and the
                                                          time-row test fail, on values first (mu0 of the worst sample 1.0 .. 2.0 of its largest entry).
  the same change in the reverse kernel:                  the old test passes; here the same 8 cases and the handle test fail on p1-bar and its six
                                                          layers ONLY (0.3 .. 1.2 of the largest entry); every value and p2-bar, p4-bar pass.
  ((1, 1), (1, 5) have one column, the unobserved-sample test blanks no step: they pass both, as they must.)
"""
import ctypes as C

import numpy as np
import pytest

from tests import latent_cases as lc

pytestmark = pytest.mark.gpu


class _Handle:
    def __init__(self, max_batch, max_T):
        from regneuralde_jl_amd import _lib
        self._lib, self.L, self.h = _lib, _lib.lib(), C.c_void_p()
        cfg = _lib.LatentConfig(max_batch=max_batch, max_T=max_T, device=0)
        _lib.check_latent(None, self.L.rnde_latent_create(C.byref(cfg), C.byref(self.h)))

    def close(self):
        self.L.rnde_latent_destroy(self.h)

    def run(self, case, lam_k=lc.LAM_K, backward=True):
        """The three calls of a training step on `case`; every output as a numpy array (fp32 as the device wrote it)."""
        import torch
        _lib, L, h = self._lib, self.L, self.h
        S, x, p1, p2, p4, eps, res, z0b = case
        B, T = x.shape[:2]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        xd, p1d, p2d, p4d, epsd, resd, z0bd = dev(x), dev(p1), dev(p2), dev(p4), dev(eps), dev(res), dev(z0b)
        nan = lambda *s: torch.full(s, float("nan"), device="cuda")              # an output the library does not write stays NaN and fails
        z0d, mu0d, lvd = nan(B, 20), nan(B, 20), nan(B, 20)
        loss2, resbd, p4bd, p1bd, p2bd = nan(2), nan(B, T, 20), nan(777), nan(29320), nan(7090)
        torch.cuda.synchronize()
        _lib.check_latent(h, L.rnde_latent_encode(h, xd.data_ptr(), p1d.data_ptr(), p2d.data_ptr(), epsd.data_ptr(), B, T, z0d.data_ptr(), mu0d.data_ptr(), lvd.data_ptr(), None))
        _lib.check_latent(h, L.rnde_latent_decode_loss(h, resd.data_ptr(), p4d.data_ptr(), xd.data_ptr(), B, T, loss2.data_ptr(), resbd.data_ptr(), p4bd.data_ptr(), None))
        if backward:
            _lib.check_latent(h, L.rnde_latent_encode_backward(h, z0bd.data_ptr(), lam_k, p1d.data_ptr(), p2d.data_ptr(), xd.data_ptr(), p1bd.data_ptr(), p2bd.data_ptr(), None))
        torch.cuda.synchronize()
        host = lambda t: t.detach().cpu().numpy()
        out = {"mu0": host(mu0d), "logvar": host(lvd), "z0": host(z0d), "nll": host(loss2[:1]), "kl": host(loss2[1:]), "res-bar": host(resbd), "p4-bar": host(p4bd)}
        if backward:
            p1b = host(p1bd)
            out.update({"p2-bar": host(p2bd), "p1-bar": p1b})
            o = 0
            for name, n in lc.GRU_LAYERS:
                out["p1-bar " + name] = p1b[o:o + n]
                o += n
        return out


def _run_once(case, max_batch=None, max_T=None, **kw):
    B, T = case[1].shape[:2]
    h = _Handle(max_batch or B, max_T or T)
    try:
        return h.run(case, **kw)
    finally:
        h.close()


@pytest.mark.parametrize("c", lc.CASES, ids=lc.case_id)
def test_latent_caller_matches_fp64_on_ragged_masks_and_saturated_gates(c):
    B, T, seed, sw = c
    case = lc.build(B, T, seed, **sw)
    lc.check(_run_once(case), lc.oracle_outputs(case))


def test_a_handle_serves_a_small_ragged_call_after_a_large_one():
    """max_batch = 40, max_T = 64: the strides come from the call, not the handle, and behind (33, 64) the tapes past (17, 12)'s extent are stale."""
    big, small = lc.build(33, 64, 12, ragged=True), lc.build(17, 12, 21, ragged=True)
    h = _Handle(40, 64)
    try:
        got_big, got_small = h.run(big), h.run(small)
    finally:
        h.close()
    lc.check(got_big, lc.oracle_outputs(big), label="(33, 64) ")
    lc.check(got_small, lc.oracle_outputs(small), label="(17, 12) behind it ")


def test_the_time_row_counts_as_an_observation_on_the_device():
    """The reference's rule sum(x[38:end, :]) > 0 counts the time row (latent_ode.jl:91): a step with dt = 0.02 under an all-zero mask is taken, and
    dt = 0 under a mask that observes something is taken too.  Flipping that one dt to or from 0 changes the device's mu0 in exactly the
    samples in which it changes the oracle's (that sample alone: bit-equal elsewhere), and by the same amount: both sides are within 5e-6 of
    the sample's largest entry before and after, so the two changes agree to twice that."""
    B, T = 17, 12
    case, info = lc.build(B, T, 15, ragged=True, with_info=True)
    assert len(info["dt_on"]) == 2 and len(info["dt_off"]) == 2
    h = _Handle(B, T)
    try:
        base_d, base_o = h.run(case, backward=False)["mu0"], lc.oracle_outputs(case)["mu0"]
        for (b, t), new_dt in [(e, 0.0) for e in info["dt_on"]] + [(e, 0.02) for e in info["dt_off"]]:
            x = case[1].copy()
            x[b, t, 74] = lc.round32(new_dt)
            flipped = (case[0], x) + case[2:]
            got, ref = h.run(flipped, backward=False)["mu0"], lc.oracle_outputs(flipped)["mu0"]
            changed_o, changed_d = (ref != base_o).any(axis=1), (got != base_d).any(axis=1)
            dd, do = got.astype(np.float64) - base_d, ref - base_o
            err = np.abs(dd - do).max() / np.abs(ref[b]).max()
            print(f"dt[{b}, {t}] -> {new_dt}: oracle changes samples {np.flatnonzero(changed_o).tolist()}, device {np.flatnonzero(changed_d).tolist()}; "
                  f"|change| {np.abs(do).max():.2e}, device - oracle {err:.2e} of the sample's largest entry")
            assert changed_o.tolist() == [i == b for i in range(B)] and np.array_equal(changed_d, changed_o)
            assert np.abs(do).max() > 100 * lc.TOL_VALUE * np.abs(ref[b]).max()      # (a change the tolerance can see)
            assert err <= 2 * lc.TOL_VALUE
    finally:
        h.close()


def _classes(a):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN, element by element."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


def test_a_sample_that_observed_nothing_gives_what_the_restatement_gives():
    """B = 5, T = 7, all of rows 37..73 zero for sample 2: the reference divides by sum(mask) = 0 (latent_ode.jl:192-200).  The fp64
    restatement gives ll_2 = (7 * 37 constants > 0) / 0 = +Inf, so -mean ll = -Inf; pred-bar of sample 2 = 0 / 0 = NaN, so its res-bar rows
    and all of p4-bar (a sum over every sample) are NaN.  The device gives the same classes, element by element; the other four samples'
    res-bar rows stay within 5e-6 of the oracle, and the KL term stays finite and right."""
    case = lc.build(5, 7, 22)
    x = case[1].copy()
    x[2, :, 37:74] = 0.0
    case = (case[0], x) + case[2:]
    ref, got = lc.oracle_outputs(case), _run_once(case, backward=False)
    for name in ("nll", "res-bar", "p4-bar"):
        cr, cg = _classes(ref[name]), _classes(got[name])
        print(f"{name}: oracle classes {sorted(set(cr.reshape(-1).tolist()))}, device {sorted(set(cg.reshape(-1).tolist()))} (0 finite, 1 +Inf, 2 -Inf, 3 NaN)")
    assert _classes(ref["nll"]).tolist() == [2] and _classes(got["nll"]).tolist() == [2]
    assert (_classes(ref["res-bar"][2]) == 3).all() and (_classes(got["res-bar"][2]) == 3).all()
    assert (_classes(ref["p4-bar"]) == 3).all() and (_classes(got["p4-bar"]) == 3).all()
    others = [0, 1, 3, 4]
    keep = lambda d: {k: d[k][others] if k in lc.PER_SAMPLE else d[k] for k in ("mu0", "logvar", "z0", "kl", "res-bar")}
    lc.check(keep(got), keep(ref), label="samples 0, 1, 3, 4: ")
