"""The input set of the element-wise sweeps and its yardsticks (tests/elementwise_ref.py), without a GPU: the set has the size it claims, every
window straddles the threshold it is there for, and the yardsticks measure on it what elementwise_ref.RECORDED says (a changed grid, or a numpy
whose float32 exp / log1p / expm1 round differently, is noticed here and not as a shifted bound in the GPU tests)."""
import numpy as np
import pytest

from tests import elementwise_ref as R


def test_the_set_is_deterministic_and_has_its_sizes():
    g = R.grid()
    assert np.array_equal(R.bits(g), R.bits(R.grid()))
    assert 2 * g.size == R.SIZES["grid"] == 2 * 255 * 4096
    e = R.bits(g) >> 23
    assert np.array_equal(np.bincount(e, minlength=256), [4096] * 255 + [0])      # 4096 per biased exponent 0..254; no Inf / NaN in the grid
    m = (R.bits(g) & 0x7FFFFF).reshape(255, 4096)
    assert np.array_equal(m[:, :64], np.tile(np.arange(64), (255, 1))) and np.array_equal(m[:, -64:], np.tile(np.arange(2 ** 23 - 64, 2 ** 23), (255, 1)))
    for k, w in R.windows().items():
        assert w.size == R.SIZES[k], (k, w.size)
        assert (w > 0).all() and (np.diff(w.astype(np.float64)) > 0).all(), k
    x = R.input_set()
    assert x.dtype == np.float32 and x.size == R.SIZES["all"] and not x.flags.writeable
    assert R.specials().size == R.SIZES["specials"]
    # both signs of every finite value: the multiset of bit patterns is closed under flipping the sign bit
    b = R.bits(x[~np.isnan(x)])
    assert np.array_equal(np.sort(b), np.sort(b ^ np.uint32(0x80000000)))


def test_every_window_straddles_its_threshold():
    w = R.windows()
    one = np.float32(1)
    with np.errstate(over="ignore", under="ignore"):
        s = w["seam_0.55"]
        assert s[0] < np.float32(0.55) < s[-1] and np.float32(0.55) in s and np.all(np.diff(R.bits(s)) == 1)      # every float
        c = w["clamp_9.1"]
        assert c[0] < np.float32(9.1) < c[-1] and np.float32(9.1) in c and np.all(np.diff(R.bits(c)) == 1)
        r = w["one_plus_t_rounds_to_one"]
        assert one + np.exp(-r[0]) > one and one + np.exp(-r[-1]) == one
        u = w["exp_goes_subnormal"]
        assert np.exp(-u[0]) >= np.float32(R.TINY) and 0 < np.exp(-u[-1]) < np.float32(R.TINY)
        assert np.isfinite(np.exp(u[0])) and np.isinf(np.exp(u[-1]))                                                  # ... and exp(+z) overflows inside it
        z = w["exp_goes_to_zero"]
        assert np.exp(-z[0]) > 0 and np.exp(-z[-1]) == 0
        n = w["smallest_normals"]
        assert n[0] == np.float32(R.TINY) and np.all(np.diff(R.bits(n)) == 1)
        t = w["up_to_2^-120"]
        assert t[0] == np.float32(R.TINY) and t[-1] == np.float32(2.0 ** -120) and np.all(np.diff(R.bits(t)) == 1024)
    sp = R.specials()
    want = [0x0, 0x1, 0x00800000, 0x7F7FFFFF, 0x7F800000]
    assert sorted(R.bits(sp).tolist()) == sorted(want + [v | 0x80000000 for v in want] + list(R.NAN_PATTERNS))
    assert np.isnan(sp).sum() == 3
    # subnormals are in the grid (biased exponent 0), the smallest among them and zero included
    g = R.grid()
    assert g[0] == 0 and R.bits(g)[1] == 1 and (g[:4096] < np.float32(R.TINY)).all()


@pytest.mark.parametrize("name", ["tanh", "sigmoid", "softplus", "ff_softplus", "elu", "sigmoid_f"])
def test_yardstick_distances_are_the_recorded_ones(name):
    x = R.input_set()
    where = (np.abs(x) <= 87) if name == "sigmoid_f" else None
    ulps, at, tiny_abs, _ = R.distance(R.yard32(name, x), R.ref64(name, x), x, where)
    print(f"yardstick {name}: {ulps:.4f} ulp at z = {at!r}; below 2^-126: {tiny_abs:.3e} absolute")
    rec = R.RECORDED[name]
    assert abs(ulps - rec[0]) <= 0.01 and abs(at - rec[1]) <= 1e-4 * abs(rec[1]), (ulps, at, rec)
    assert tiny_abs <= 2.2e-45                                       # one step of the subnormal grid
    y = R.yard32(name, x)
    assert np.isfinite(y[np.isfinite(x)]).all()


@pytest.mark.parametrize("name", ["sigmoid", "softplus"])
def test_yardstick_derivatives_are_the_recorded_ones(name):
    x = R.input_set()
    fin = np.isfinite(x)
    y = R.yard32(name, x)
    d = R.yard_dy32(name, y)
    ulps, at, _, _ = R.distance(d, R.dy64(name, y), x)
    absd = float(np.abs(d.astype(np.float64) - R.true_dz64(name, x))[fin].max())
    print(f"yardstick {name} dy: {ulps:.4f} ulp at z = {at!r}; from the true derivative: {absd:.3e} absolute")
    rec = R.RECORDED[name + "_dy"]
    assert abs(ulps - rec[0]) <= 0.01 and abs(at - rec[1]) <= 1e-4 * abs(rec[1]), (ulps, at, rec)
    assert abs(absd - rec[2]) <= 0.01 * rec[2], (absd, rec)


def test_the_tanh_restatement_has_the_properties_the_device_is_held_to():
    """tanh_fast as restated on the CPU (exp2 and the reciprocal correctly rounded): what the GPU test then asks of the device's own."""
    x = R.input_set()
    y = R.tanh_fast32(x)
    nn = ~np.isnan(x)
    assert np.isnan(y[~nn]).all()                                    # a NaN stays a NaN (all three patterns)
    assert (np.abs(y[nn]) <= 1).all()
    big = nn & (np.abs(x) >= np.float32(9.1))
    assert np.array_equal(y[big], np.sign(x[big]).astype(np.float32))
    ok, at = R.monotone(x, y)
    assert ok, at
    nz = nn & (x != 0)
    assert np.array_equal(R.bits(R.tanh_fast32(-x[nz])), R.bits(-y[nz]))      # odd, bit for bit
    # the formula's zero: x + x * (x^2 * p) with p < 0 gives +0 for BOTH zeros (harmless: the two compare equal; stated so that no one finds it by surprise)
    assert R.bits(R.tanh_fast32(np.float32([0.0, -0.0]))).tolist() == [0, 0]
