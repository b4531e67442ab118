"""The fp32 input set of the element-wise sweeps (tests/test_gpu_elementwise.py), its fp64 references and its fp32 yardsticks.  No GPU, no
randomness beyond default_rng(0): two calls build the same arrays.

The set: a GRID over every binade (subnormals included), WINDOWS holding every float (or every 64th / 1024th) around the places where the
device functions of csrc/rnde_device.h, rnde_latent.h and rnde_ffjord.h change path -- tanh_fast's seam at 0.55 and its clamp at 9.1, where
1 + exp(-z) rounds to 1, where expf goes subnormal, to zero and overflows, and the smallest normals -- and the SPECIAL values.  Every part
is there with both signs.

References are numpy fp64 (tanh, exp, log1p, expm1).  A yardstick is the numpy float32 restatement of the formula include/rnde.h documents for
an activation: what plain fp32 arithmetic with a good libm gives, the measure of "as close to fp64 as fp32 is".  Distances are in ulps of the
fp64 result rounded to fp32; where the fp64 result is below 2^-126 the distance is absolute (a kernel may flush subnormals, a CPU does not)."""
import functools

import numpy as np

TINY = 2.0 ** -126
CODES = {"identity": 0, "tanh": 1, "relu": 2, "sigmoid": 3, "softplus": 4, "elu": 5}
# the selectors of rnde_debug_elementwise (include/rnde.h: rnde_elementwise_fn)
FN = {"tanh_fast": 0, "tanh_fast2_x": 1, "tanh_fast2_y": 2, "pre_fwd": 3, "pre_bwd": 4, "act_fwd": 5, "act_dy": 6, "act_d2y": 7, "tanh_f": 8,
      "sigmoid_f": 9, "ff_softplus": 10}
NAN_PATTERNS = (0x7FC00000, 0xFFC00000, 0x7FA00000)      # quiet NaN of both signs, and a signalling pattern


def f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def float_range(lo, hi, stride=1):
    """Every stride-th float32 from float32(lo) to float32(hi), both included when the stride lands on them (0 < lo < hi), increasing."""
    ia, ib = int(np.float32(lo).view(np.uint32)), int(np.float32(hi).view(np.uint32))
    return f32(np.arange(ia, ib + 1, stride, dtype=np.int64).astype(np.uint32))


def grid():
    """Biased exponents 0..254, 4096 mantissas each: the first 64, the last 64, 3968 drawn from default_rng(0).  Positive half."""
    rng = np.random.default_rng(0)
    mid = rng.integers(64, 2 ** 23 - 64, size=(255, 3968), dtype=np.int64)
    lo = np.tile(np.arange(64, dtype=np.int64), (255, 1))
    hi = np.tile(np.arange(2 ** 23 - 64, 2 ** 23, dtype=np.int64), (255, 1))
    m = np.concatenate([lo, mid, hi], axis=1)
    e = np.arange(255, dtype=np.int64)[:, None] << 23
    return f32((e | m).ravel().astype(np.uint32))


def windows():
    """name -> positive floats, increasing."""
    min_normal = 0x00800000
    return {
        "seam_0.55": float_range(0.5499, 0.5501),
        "clamp_9.1": float_range(9.09, 9.11),
        "one_plus_t_rounds_to_one": float_range(16.5, 17.5, 64),
        "exp_goes_subnormal": float_range(87.0, 89.5, 64),
        "exp_goes_to_zero": float_range(103.0, 104.5, 64),
        "smallest_normals": f32(np.arange(min_normal, min_normal + 4096, dtype=np.int64).astype(np.uint32)),
        "up_to_2^-120": float_range(2.0 ** -126, 2.0 ** -120, 1024),
    }


def specials():
    """+-0, +-min subnormal, +-min normal, +-FLT_MAX, +-Inf, the three NaN patterns."""
    pos = [0x00000000, 0x00000001, 0x00800000, 0x7F7FFFFF, 0x7F800000]
    return f32(np.array(pos + [b | 0x80000000 for b in pos] + list(NAN_PATTERNS), dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def input_set():
    """The whole set as one read-only float32 array: grid, -grid, every window, every window negated, specials."""
    g = grid()
    w = np.concatenate(list(windows().values()))
    x = np.concatenate([g, -g, w, -w, specials()])
    x.setflags(write=False)
    return x


def _f64(a):
    with np.errstate(invalid="ignore"):      # (a signalling NaN pattern raises "invalid" when it is widened)
        return np.asarray(a, dtype=np.float64)


# ---- fp64 references ------------------------------------------------------------------------------------------------------------------
def ref64(name, z):
    """The activation `name` at the fp32 points z, in fp64 (NaN and +-Inf go where the formula's limit is)."""
    z = _f64(z)
    with np.errstate(all="ignore"):
        if name == "identity":
            return z.copy()
        if name == "tanh":
            return np.tanh(z)
        if name == "relu":
            return np.where(z < 0, 0.0, z)
        t = np.exp(-np.abs(z))
        if name in ("sigmoid", "sigmoid_f"):
            return np.where(z >= 0, 1 / (1 + t), t / (1 + t)) + 0 * z      # (+ 0 z: NaN stays)
        if name in ("softplus", "ff_softplus"):
            return np.log1p(t) + np.where(np.isnan(z), z, np.maximum(z, 0))
        if name == "elu":
            return np.where(z > 0, z, np.expm1(np.minimum(z, 0))) + np.where(np.isnan(z), z, 0)
    raise KeyError(name)


def dy64(name, y):
    """The derivative from the output y, by the formula include/rnde.h documents, in fp64."""
    y = _f64(y)
    with np.errstate(all="ignore"):
        return {"identity": lambda: np.ones_like(y), "tanh": lambda: 1 - y * y, "relu": lambda: (y > 0).astype(np.float64),
                "sigmoid": lambda: y * (1 - y), "softplus": lambda: -np.expm1(-y), "elu": lambda: np.where(y > 0, 1.0, y + 1)}[name]()


def d2y64(name, y):
    y = _f64(y)
    with np.errstate(all="ignore"):
        s = -np.expm1(-y)
        return {"identity": lambda: np.zeros_like(y), "tanh": lambda: -2 * y * (1 - y * y), "relu": lambda: np.zeros_like(y),
                "sigmoid": lambda: y * (1 - y) * (1 - 2 * y), "softplus": lambda: s * (1 - s), "elu": lambda: np.where(y > 0, 0.0, y + 1)}[name]()


def true_dz64(name, z):
    """The derivative at the pre-activation z, in fp64 (what act_dy approximates from a rounded output)."""
    z = _f64(z)
    with np.errstate(all="ignore"):
        if name == "sigmoid":
            s = ref64("sigmoid", z)
            return s * ref64("sigmoid", -z)
        if name == "softplus":
            return ref64("sigmoid", z)
        if name == "tanh":
            return 1 / np.cosh(z) ** 2
        if name == "elu":
            return np.where(z > 0, 1.0, np.exp(np.minimum(z, 0)))
    raise KeyError(name)


# ---- fp32 yardsticks ------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf on float32 arrays, one rounding: the product of two floats is exact in fp64; the sum is formed in fp64 ROUNDED TO ODD (TwoSum
    gives the rounding error; an inexact sum with an even last bit moves to its odd neighbour on the error's side), and a value rounded to
    odd at 53 bits rounds to 24 bits as the exact value does."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.broadcast_to(np.asarray(c, np.float64), p.shape)
    with np.errstate(all="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def tanh_fast32(x):
    """tanh_fast of csrc/rnde_device.h restated in numpy float32, with exp2 and the reciprocal correctly rounded (the device has v_exp_f32 and
    v_rcp_f32 there).  np.minimum keeps a NaN, as the device's clamp does."""
    one = np.float32(1)
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        ax, x2 = np.minimum(np.abs(x), np.float32(9.1)), x * x
        p = np.full_like(x, -0.00671552)
        for c in (0.02136713, -0.05391917, 0.13333165, -0.33333332):
            p = _fma(p, x2, np.float32(c))
        small = _fma(x, x2 * p, x)
        L = np.float32(2.8853900817779268)
        Llo = np.float32(2.8853900817779268 - float(L))
        yh = ax * L
        yl = _fma(ax, L, -yh) + ax * Llo
        e = np.exp2(yh.astype(np.float64)).astype(np.float32)
        e = _fma(e, yl * np.float32(0.6931471805599453), e)
        dd = e + one
        r = (1.0 / dd.astype(np.float64)).astype(np.float32)
        r = _fma(_fma(-dd, r, one), r, r)
        big = _fma(np.float32(-2), r, one)
        return np.where(ax < np.float32(0.55), small, np.copysign(big, x)).astype(np.float32)


def yard32(name, z):
    """The formula of include/rnde.h in numpy float32."""
    z = np.asarray(z, dtype=np.float32)
    one = np.float32(1)
    with np.errstate(all="ignore"):
        if name == "tanh":
            return tanh_fast32(z)
        if name == "sigmoid_f":                                   # rnde_latent.h says 1 / (1 + exp(-x))
            return (one / (one + np.exp(-z))).astype(np.float32)
        t = np.exp(-np.abs(z))
        if name == "sigmoid":
            return np.where(z >= 0, one / (one + t), t / (one + t)).astype(np.float32)
        if name in ("softplus", "ff_softplus"):                   # (rnde_ffjord.h runs the same function)
            y = (np.log1p(t) + np.maximum(z, np.float32(0))).astype(np.float32)
            mid = (z > 0) & (z < np.float32(0.5))                  # there: the fp64 value rounded once
            return np.where(mid, np.log1p(np.exp(z.astype(np.float64))).astype(np.float32), y)
        if name == "elu":
            return np.where(z > 0, z, np.expm1(np.minimum(z, np.float32(0)))).astype(np.float32)
    raise KeyError(name)


def yard_dy32(name, y):
    """The documented derivative from the output, in numpy float32, every operation rounded on its own."""
    y = np.asarray(y, dtype=np.float32)
    one = np.float32(1)
    with np.errstate(all="ignore"):
        return {"tanh": lambda: one - y * y, "sigmoid": lambda: y * (one - y), "softplus": lambda: -np.expm1(-y),
                "elu": lambda: np.where(y > 0, one, y + one)}[name]().astype(np.float32)


def yard_d2y32(name, y):
    y = np.asarray(y, dtype=np.float32)
    one, two = np.float32(1), np.float32(2)
    with np.errstate(all="ignore"):
        s = -np.expm1(-y)
        return {"tanh": lambda: -two * y * (one - y * y), "sigmoid": lambda: y * (one - y) * (one - two * y), "softplus": lambda: s * (one - s),
                "elu": lambda: np.where(y > 0, np.float32(0), y + one)}[name]().astype(np.float32)


# ---- distances ------------------------------------------------------------------------------------------------------------------------
def distance(y, ref, x, where=None):
    """(max ulp distance, its argument, max absolute distance where |ref| < 2^-126, its argument) of the fp32 values y from the fp64
    values ref, over the points of `where` (default: every point with a finite x).  An ulp is that of ref rounded to fp32.  A NaN or
    infinite y at a finite ref counts as infinitely far."""
    y64, ref, x = _f64(y), _f64(ref), np.asarray(x, np.float32)
    m = np.isfinite(x) & np.isfinite(ref) if where is None else np.asarray(where) & np.isfinite(ref)
    with np.errstate(all="ignore"):
        d = np.abs(y64 - ref)
        d = np.where(np.isfinite(y64), d, np.inf)
        r32 = np.clip(ref, -3.4028234663852886e38, 3.4028234663852886e38).astype(np.float32)
        ulps = d / np.spacing(np.abs(r32)).astype(np.float64)
    tiny = m & (np.abs(ref) < TINY)
    norm = m & ~tiny
    out = []
    for sel, v in ((norm, ulps), (tiny, d)):
        if sel.any():
            i = np.flatnonzero(sel)[np.argmax(v[sel])]
            out += [float(v[i]), float(x[i])]
        else:
            out += [0.0, float("nan")]
    return tuple(out)


def monotone(x, y):
    """y non-decreasing along increasing x, over the points where x is not a NaN (-0 and +0 are one point: their values must compare equal)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    keep = ~np.isnan(x)
    o = np.argsort(x[keep], kind="stable")
    xs, ys = x[keep][o], y[keep][o]
    if np.isnan(ys).any():
        return False, float(xs[np.flatnonzero(np.isnan(ys))[0]])
    with np.errstate(invalid="ignore"):      # (inf - inf along a run of infinite values)
        bad = np.flatnonzero(~(ys[1:] >= ys[:-1]))
    return (bad.size == 0), (float(xs[bad[0] + 1]) if bad.size else None)


# What the yardsticks measure on input_set() (test_elementwise_host.py holds them to these figures, so that a changed set is noticed):
# max ulp distance from fp64 and the z it is reached at; for the two derivatives also the max absolute distance from the true derivative at z.
RECORDED = {
    "tanh": (1.61, 0.55008), "sigmoid": (2.99, -9.0928), "softplus": (2.80, -0.99509), "ff_softplus": (2.80, -0.99509), "elu": (2.20, -0.011302),
    "sigmoid_f": (3.29, -16.678),                 # (on [-87, 87])
    "sigmoid_dy": (1.50, -0.00077198, 8.84e-8), "softplus_dy": (2.14, -4.5136, 9.32e-8),
}
SIZES = {"grid": 2088960, "seam_0.55": 3357, "clamp_9.1": 20972, "one_plus_t_rounds_to_one": 8193, "exp_goes_subnormal": 5121,
         "exp_goes_to_zero": 3073, "smallest_normals": 4096, "up_to_2^-120": 49153, "specials": 13, "all": 2276903}
