"""What the inputs of tests/test_gpu_latent_ragged.py reach, asserted with the oracle alone (oracle/latent_oracle.py): a device case is only as
good as its inputs.  For every case of tests/latent_cases.py CASES:
  ragged    the share of (sample, step) pairs at which the GRU keeps its state is at least 0.5, and the table has the rows it promises;
  gates     the share of update-gate values outside [1e-3, 1 - 1e-3] is at least 0.3;
  lv_shift  every logvar lies on the shifted side of +-5;
  always    the restatement run in float32 (every input cast) is at most HALF the device's tolerance from the fp64 one, for every output the
            device test compares and in the same measure -- 2.5e-6 for values, 5e-6 for gradients.  An fp32 kernel that evaluates these
            formulas in another order can therefore be held to the full tolerance at these inputs; all-weights scaling (scale = 3 over 49
            steps: chaotic, 2.5e-2) fails this by five orders and is not used.
Measured on the committed seeds: empty share 0.50 .. 0.71 (0.65 and more at T >= 12), saturated share 0.41 .. 0.42, fp32 against fp64 at most
6.0e-7 for values (mu0 at (33, 64)) and 8.8e-7 for gradients (the first reset-gate layer at g1 = 8)."""
import numpy as np
import pytest

from tests import latent_cases as lc


@pytest.fixture(scope="module")
def oracle_runs():
    runs = {}

    def get(c):
        key = lc.case_id(c)
        if key not in runs:
            B, T, seed, sw = c
            case, info = lc.build(B, T, seed, with_info=True, **sw)
            ref, tape = lc.oracle_outputs(case, with_tape=True)
            runs[key] = (case, info, ref, tape)
        return runs[key]
    return get


@pytest.mark.parametrize("c", lc.CASES, ids=lc.case_id)
def test_case_inputs_reach_what_they_are_for(c, oracle_runs):
    B, T, seed, sw = c
    case, info, ref, tape = oracle_runs(c)
    x = case[1]
    m = np.stack([rec[12][:, 0] for rec in tape], axis=1)[:, ::-1]          # the GRU's own step mask, (B, T) in time order
    msum = x[:, :, 37:74].sum(axis=(1, 2))
    assert (msum >= 1).all()                                                  # the likelihood divides by the count
    if sw.get("ragged"):
        keep = info["keep"]
        share = 1.0 - m.mean()
        print(f"empty share {share:.3f}")
        assert share >= 0.5
        observed = m > 0
        for b, t in info["dt_on"]:
            assert not keep[b, t] and observed[b, t] and x[b, t, 37:74].sum() == 0 and x[b, t, 74] == np.float32(0.02)
            keep = keep.copy(); keep[b, t] = True
        for b, t in info["dt_off"]:
            assert keep[b, t] and observed[b, t] and x[b, t, 74] == 0
        assert np.array_equal(observed, keep)
        assert (x[:, :, :37][~observed] == 0).all() and (x[:, :, 37:][~info["keep"]].reshape(-1, 38)[:, :37] == 0).all()
        assert observed.any(axis=1).all()
        if B >= 3:
            assert observed[0].tolist() == [False] * (T - 1) + [True] and observed[1].tolist() == [True] + [False] * (T - 1)
        if B >= 5:
            assert msum[2] == 1 and msum[B - 1] == 37 * T
        if B > 16:
            t_e = info["t_empty"]
            assert not observed[:16, t_e].any() and observed[16, t_e]
        if B >= 7 and T >= 5:
            assert len(info["dt_on"]) == 2 and len(info["dt_off"]) == 2
    if sw.get("gates"):
        u = np.stack([rec[5] for rec in tape])
        sat = float(((u < 1e-3) | (u > 1 - 1e-3)).mean())
        print(f"saturated share {sat:.3f}")
        assert sat >= 0.3
    lv = ref["logvar"]
    print(f"logvar in [{lv.min():.2f}, {lv.max():.2f}]")
    if sw.get("lv_shift", 0.0) > 0:
        assert lv.min() > 5
    if sw.get("lv_shift", 0.0) < 0:
        assert lv.max() < -5


@pytest.mark.parametrize("c", lc.CASES, ids=lc.case_id)
def test_fp32_restatement_is_within_half_the_device_tolerance(c, oracle_runs):
    case, info, ref, tape = oracle_runs(c)
    lc.check(lc.oracle_outputs(case, dtype=np.float32), ref, scale=0.5, label="fp32 restatement ")


def test_builder_is_deterministic_and_fp32_exact():
    a = lc.build(17, 12, 15, ragged=True, gates=4.0, lv_shift=-10.0)
    b = lc.build(17, 12, 15, ragged=True, gates=4.0, lv_shift=-10.0)
    for u, v in zip(a[1:], b[1:]):
        assert u.dtype == np.float64 and np.array_equal(u, v) and np.array_equal(u, lc.round32(u))
