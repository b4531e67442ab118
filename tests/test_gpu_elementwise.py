"""The element-wise device functions themselves (rnde_debug_elementwise, include/rnde.h) over fp32: every binade, every threshold the code
has (0.55, 9.1, where 1 + exp(-z) rounds to 1, where expf goes subnormal / to zero / overflows), saturation, +-0, subnormals, +-Inf and
NaN -- the inputs the chains of the other tests never reach.  The set, the fp64 references and the fp32 yardsticks are those of
tests/elementwise_ref.py (checked without a GPU in tests/test_elementwise_host.py); it is uploaded once.

Distances are in ulps of the fp64 result rounded to fp32; where the fp64 result is below 2^-126 an absolute 2^-126 is allowed instead (the
tests do not depend on the kernels' denormal mode).  "As close to fp64 as fp32 is" = max(4 x the yardstick's own maximum on the same set,
4 ulp), the factor every parity test of this project uses.  Every test prints what it measured, with the argument."""
import ctypes as C

import numpy as np
import pytest
import torch

from regneuralde_jl_amd import _lib
from tests import elementwise_ref as R

pytestmark = pytest.mark.gpu

TANH_ULP = 3.0      # the project's own 1.65 (exact exp2 / division) plus the ~1 ulp it allows v_exp_f32 / v_rcp_f32, rounded up


class Probe:
    def __init__(self):
        self.L = _lib.lib()
        self.x = R.input_set()
        self.xd = torch.from_numpy(self.x.copy()).cuda()
        self.other = np.roll(self.x, 7919)                       # the other lane of tanh_fast2: a different value (NaN and Inf among them)
        self.od = torch.from_numpy(self.other.copy()).cuda()
        self.nan = np.isnan(self.x)
        self.fin = np.isfinite(self.x)
        self._cache = {}

    def run(self, fn, code=0, a=None, b=None):
        """out = fn(a[, b]) on the device: a, b numpy float32 arrays or device tensors (default: the input set)."""
        ad = self.xd if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda())
        bd = None if b is None else (b if torch.is_tensor(b) else torch.from_numpy(np.ascontiguousarray(b, np.float32)).cuda())
        out = torch.empty_like(ad)
        torch.cuda.current_stream().synchronize()
        _lib.check(None, self.L.rnde_debug_elementwise(R.FN[fn], code, ad.data_ptr(), bd.data_ptr() if bd is not None else None, ad.numel(),
                                                       out.data_ptr(), None))
        return out

    def on_set(self, fn, code=0):
        """fn over the input set (computed once per module, read-only)."""
        k = (fn, code)
        if k not in self._cache:
            two = fn in ("tanh_fast2_x", "tanh_fast2_y")
            y = self.run(fn, code, b=self.od if two else None).cpu().numpy()
            y.setflags(write=False)
            self._cache[k] = y
        return self._cache[k]


@pytest.fixture(scope="module")
def S():
    return Probe()


def _report(what, ulps, at, tiny_abs, tiny_at):
    print(f"{what}: max {ulps:.3f} ulp at {at!r}; where fp64 is below 2^-126: {tiny_abs:.3e} absolute at {tiny_at!r}")


def test_probe_refuses_what_it_does_not_serve(S):
    L = S.L
    out = torch.full((4,), 7.0, device="cuda")
    a = torch.zeros(4, device="cuda")
    for fn, code, n in ((-1, 0, 4), (11, 0, 4), (R.FN["act_fwd"], 6, 4), (R.FN["act_fwd"], -1, 4), (R.FN["pre_fwd"], 3, 4), (R.FN["tanh_fast"], 1, 4),
                        (R.FN["tanh_fast"], 0, -1)):
        assert L.rnde_debug_elementwise(fn, code, a.data_ptr(), a.data_ptr(), n, out.data_ptr(), None) == _lib.BAD_ARG, (fn, code, n)
        assert b"rnde_debug_elementwise" in L.rnde_last_error(None)
    assert L.rnde_debug_elementwise(R.FN["pre_bwd"], 1, a.data_ptr(), None, 4, out.data_ptr(), None) == _lib.BAD_ARG      # a cotangent is needed
    assert L.rnde_debug_elementwise(R.FN["tanh_fast"], 0, None, None, 0, None, None) == _lib.OK                           # n = 0: touches nothing
    assert L.rnde_debug_elementwise(R.FN["tanh_fast"], 0, a.data_ptr(), None, 0, out.data_ptr(), None) == _lib.OK
    assert (out.cpu() == 7.0).all()
    # more points than one pass of the grid covers, and an odd count: the grid-stride loop ends where it should
    n = 2048 * 256 * 2 + 37
    z = torch.linspace(-3, 3, n + 3, device="cuda")
    o = torch.full((n + 3,), 7.0, device="cuda")
    assert L.rnde_debug_elementwise(R.FN["act_fwd"], 0, z.data_ptr(), None, n, o.data_ptr(), None) == _lib.OK
    assert torch.equal(o[:n], z[:n]) and (o[n:] == 7.0).all()


TANH_VARIANTS = [("tanh_fast", 0), ("tanh_fast2_x", 0), ("tanh_fast2_y", 0), ("tanh_f", 0), ("pre_fwd", 1), ("act_fwd", 1)]


@pytest.mark.parametrize("fn,code", TANH_VARIANTS, ids=[f"{f}{c or ''}" for f, c in TANH_VARIANTS])
def test_tanh(S, fn, code):
    """Every way the kernels evaluate tanh: tanh_fast, each lane of tanh_fast2 (the other lane fed another value), the latent code's tanh_f,
    and tanh_fast as pre_fwd(RNDE_PRE_TANH) / act_fwd(RNDE_ACT_TANH) reach it."""
    x, y = S.x, S.on_set(fn, code)
    ulps, at, tiny_abs, tiny_at = R.distance(y, R.ref64("tanh", x), x)
    _report(f"{fn}({code})", ulps, at, tiny_abs, tiny_at)
    # a NaN stays a NaN: quiet of both signs and the signalling pattern (once tanh_fast(NaN) was 1.0: fminf drops a NaN)
    assert np.isnan(y[S.nan]).all() and S.nan.sum() == 3, y[S.nan]
    assert ulps <= TANH_ULP, (ulps, at)
    assert tiny_abs <= R.TINY, (tiny_abs, tiny_at)
    nn = ~S.nan
    assert (np.abs(y[nn]) <= 1).all()
    ok, where = R.monotone(x, y)
    assert ok, f"not monotone at {where!r}"                         # the sorted set: both windows, every float of them, included
    big = nn & (np.abs(x) >= np.float32(9.1))                       # +-Inf among them
    assert np.array_equal(R.bits(y[big]), R.bits(np.copysign(np.float32(1), x[big])))
    # odd, bit for bit: the set holds -x for every x, at a fixed offset inside each part; compare through a lookup by bit pattern
    order = np.argsort(R.bits(x[nn]), kind="stable")
    bx, by = R.bits(x[nn])[order], R.bits(y[nn])[order]
    nz = (bx & 0x7FFFFFFF) != 0
    j = np.searchsorted(bx, bx[nz] ^ np.uint32(0x80000000))
    assert np.array_equal(bx[j], bx[nz] ^ np.uint32(0x80000000))
    assert np.array_equal(by[j], by[nz] ^ np.uint32(0x80000000))
    # the formula's zero is x + x (x^2 p): +0 for both zeros.  Stated on purpose; what is required is that it compares equal to 0.
    zero = nn & (x == 0)
    assert zero.sum() >= 4 and (y[zero] == 0).all()
    # one function, bit for bit, however it is reached (the headers' "bit-identical to it", "as the stage engine evaluates it")
    y0 = S.on_set("tanh_fast")
    assert np.array_equal(R.bits(y[nn]), R.bits(y0[nn])), f"{fn} differs from tanh_fast at {x[nn][np.flatnonzero(R.bits(y[nn]) != R.bits(y0[nn]))[:4]]!r}"


def test_tanh_device_against_the_cpu_restatement(S):
    """How far the hardware exp2 / rcp move tanh_fast from its restatement with both correctly rounded (reported; the bound is test_tanh's)."""
    x, y = S.x, S.on_set("tanh_fast")
    yr = R.tanh_fast32(x)
    nn = ~S.nan
    diff = np.abs(R.bits(y[nn]).astype(np.int64) - R.bits(yr[nn]).astype(np.int64))
    diff = np.where((y[nn] == 0) & (yr[nn] == 0), 0, diff)
    i = int(np.argmax(diff))
    print(f"tanh_fast device vs restatement: {int((diff != 0).sum())} of {diff.size} differ, at most {int(diff[i])} steps (x = {x[nn][i]!r})")
    u_dev = R.distance(y, R.ref64("tanh", x), x)[0]
    u_cpu = R.distance(yr, R.ref64("tanh", x), x)[0]
    print(f"tanh_fast max ulp: device {u_dev:.3f}, restatement {u_cpu:.3f}")
    small = nn & (np.abs(x) < np.float32(0.55)) & (np.abs(x) >= np.float32(R.TINY))
    assert np.array_equal(R.bits(y[small]), R.bits(yr[small]))      # the polynomial branch is fma and mul only: the same bits on both


ACTS = ["relu", "sigmoid", "softplus", "elu", "ff_softplus"]


def _act_on_set(S, name):
    return S.on_set("ff_softplus") if name == "ff_softplus" else S.on_set("act_fwd", R.CODES[name])


@pytest.mark.parametrize("name", ACTS)
def test_act_fwd(S, name):
    x, y = S.x, _act_on_set(S, name)
    fin, nn = S.fin, ~S.nan
    assert np.isnan(y[S.nan]).all(), y[S.nan]
    if name == "relu":
        with np.errstate(invalid="ignore"):
            want = np.where(x < 0, np.float32(0), x)
        assert np.array_equal(R.bits(y[nn]), R.bits(want[nn]))
        return
    ref = R.ref64(name, x)
    ulps, at, tiny_abs, tiny_at = R.distance(y, ref, x)
    yu, yat, ytiny, _ = R.distance(R.yard32(name, x), ref, x)
    _report(f"{name} device", ulps, at, tiny_abs, tiny_at)
    print(f"{name} yardstick: max {yu:.3f} ulp at {yat!r}; below 2^-126: {ytiny:.3e}")
    assert ulps <= max(4 * yu, 4.0), (ulps, at, yu)
    assert tiny_abs <= R.TINY, (tiny_abs, tiny_at)
    assert np.isfinite(y[fin]).all(), x[fin][~np.isfinite(y[fin])][:4]      # softplus / elu at FLT_MAX included
    if name in ("sigmoid", "elu"):                                   # (softplus: test_softplus_is_monotone)
        ok, where = R.monotone(x, y)
        assert ok, f"{name} not monotone at {where!r}"
    pinf, ninf = y[x == np.inf], y[x == -np.inf]
    if name == "sigmoid":
        assert (y[nn] >= 0).all() and (y[nn] <= 1).all()
        assert (pinf == 1).all() and (ninf == 0).all()
    elif name in ("softplus", "ff_softplus"):
        assert (y[nn] >= np.maximum(x[nn], 0)).all()
        assert (pinf == np.inf).all() and (ninf == 0).all()
    else:
        assert (y[nn] >= -1).all() and (y[x == 0] == 0).all() and (x == 0).sum() >= 4
        assert (pinf == np.inf).all() and (ninf == -1).all()


@pytest.mark.parametrize("name", ["softplus", "ff_softplus"])
def test_softplus_is_monotone(S, name):
    """softplus non-decreasing over the sorted set.  The form log1p(exp(-|z|)) + max(z, 0) alone does not have this property in fp32 (measured
    on one MI355X, and the numpy float32 restatement reverses too): 1226 neighbouring pairs of the set stepped DOWN, each by one ulp, all with
    0 < z < 0.5 (first at z = 4.13e-8: 0.69314724 -> 0.6931472) -- below 0.5 exp(-z), and with it the log1p term, moves in steps larger than the
    steps of z.  softplus_f (csrc/rnde_device.h) takes the fp64 value rounded once on (0, 0.5); z <= 0 and z >= 0.5 keep the form and its bits."""
    x, y = S.x, _act_on_set(S, name)
    keep = ~S.nan
    o = np.argsort(x[keep], kind="stable")
    xs, ys = x[keep][o], y[keep][o]
    with np.errstate(invalid="ignore"):
        bad = np.flatnonzero(~(ys[1:] >= ys[:-1]))
    if bad.size:
        steps = R.bits(ys[bad]).astype(np.int64) - R.bits(ys[bad + 1]).astype(np.int64)
        print(f"{name}: {bad.size} reversals, at most {int(steps.max())} ulp, z in [{xs[bad].min()!r}, {xs[bad].max()!r}]")
    ok, where = R.monotone(x, y)
    assert ok, f"{name} not monotone at {where!r} ({bad.size} reversals in the set)"


def test_identity_and_tanh_codes_at_the_specials(S):
    """Codes 0 and 1 of act_fwd: +-Inf to the limit, NaN to NaN (tanh's sweep is test_tanh)."""
    x = S.x
    y = S.on_set("act_fwd", 0)
    assert np.array_equal(R.bits(y), R.bits(x))                      # identity: every bit, the NaN payloads too
    t = S.on_set("act_fwd", 1)
    assert (t[x == np.inf] == 1).all() and (t[x == -np.inf] == -1).all() and np.isnan(t[S.nan]).all()


DERIV = ["tanh", "sigmoid", "softplus", "elu"]


@pytest.mark.parametrize("name", DERIV)
def test_act_dy_and_d2y_from_the_device_output(S, name):
    """act_dy / act_d2y fed the device's own act_fwd output y, (a) against the documented formula in fp64 ON THAT y, in ulps, and (b) act_dy
    against the true derivative at z, absolutely: a derivative taken from a saturated output is exact only to the output's rounding.  Both
    yardsticks are the numpy float32 formulas fed their own float32 forward."""
    x, fin = S.x, S.fin
    code = R.CODES[name]
    y = S.on_set("act_fwd", code)
    yd = torch.from_numpy(y.copy()).cuda()
    d = S.run("act_dy", code, a=yd).cpu().numpy()
    d2 = S.run("act_d2y", code, a=yd).cpu().numpy()
    yy = R.yard32(name, x)
    for what, dev, f64, yard in (("dy", d, R.dy64, R.yard_dy32), ("d2y", d2, R.d2y64, R.yard_d2y32)):
        ulps, at, tiny_abs, tiny_at = R.distance(dev, f64(name, y), x)
        yu, yat, _, _ = R.distance(yard(name, yy), f64(name, yy), x)
        _report(f"{name} {what} device", ulps, at, tiny_abs, tiny_at)
        print(f"{name} {what} yardstick: max {yu:.3f} ulp at {yat!r}")
        assert np.isfinite(dev[fin]).all()                           # zero or tiny at saturation, never NaN or Inf
        assert ulps <= max(4 * yu, 4.0), (what, ulps, at, yu)
        assert tiny_abs <= R.TINY, (what, tiny_abs, tiny_at)
    true = R.true_dz64(name, x)
    a_dev = np.abs(d.astype(np.float64) - true)[fin]
    a_yard = float(np.abs(R.yard_dy32(name, yy).astype(np.float64) - true)[fin].max())
    i = int(np.argmax(a_dev))
    print(f"{name} dy from the true derivative: device {a_dev[i]:.3e} at z = {x[fin][i]!r}; yardstick {a_yard:.3e}")
    assert a_dev[i] <= 4 * a_yard, (a_dev[i], a_yard)


def test_act_dy_exact_values(S):
    one = np.float32(1)
    for name, yv, want in (("tanh", [1.0, -1.0], [0.0, 0.0]), ("relu", [0.0, -0.0], [0.0, 0.0]), ("elu", [0.0, -0.0], [1.0, 1.0]),
                           ("relu", [np.float32(R.TINY), 3.0], [1.0, 1.0]), ("identity", [5.0, -5.0], [1.0, 1.0]),
                           ("sigmoid", [1.0, 0.0], [0.0, 0.0]), ("softplus", [0.0, np.inf], [0.0, 1.0])):
        got = S.run("act_dy", R.CODES[name], a=np.float32(yv)).cpu().numpy()
        assert np.array_equal(R.bits(np.abs(got)), R.bits(np.float32(want))), (name, yv, got)
    for name in ("identity", "relu"):                                # no second derivative
        assert (S.run("act_d2y", R.CODES[name], a=np.float32([-2.0, 0.0, 3.0])).cpu().numpy() == 0).all()
    assert (S.run("act_d2y", R.CODES["elu"], a=np.float32([0.5, 3.0])).cpu().numpy() == 0).all()
    assert one == S.run("act_d2y", R.CODES["elu"], a=np.float32([0.0])).cpu().numpy()[0]


def test_pre_maps(S):
    """pre_fwd / pre_bwd: selector 0 passes through, 2 is the cube as written -- (g g) g and v ((3 g) g), products only, so nothing can be
    contracted: bit for bit -- and 1's derivative is v (1 - a a) with a the device's own tanh_fast(g)."""
    x, nn = S.x, ~S.nan
    rng = np.random.default_rng(1)
    v = rng.standard_normal(x.size).astype(np.float32)
    vd = torch.from_numpy(v).cuda()
    assert np.array_equal(R.bits(S.on_set("pre_fwd", 0)), R.bits(x))
    assert np.array_equal(R.bits(S.run("pre_bwd", 0, b=vd).cpu().numpy()), R.bits(v))
    with np.errstate(all="ignore"):
        cube = (x * x) * x
        dcube = v * ((np.float32(3) * x) * x)
    got, dgot = S.on_set("pre_fwd", 2), S.run("pre_bwd", 2, b=vd).cpu().numpy()
    assert np.isnan(got[S.nan]).all() and np.isnan(dgot[S.nan]).all()
    assert np.array_equal(R.bits(got[nn]), R.bits(cube[nn]))
    ok = ~np.isnan(dcube)                                            # (0 * Inf where 3 g g overflows against a zero cotangent: NaN on both)
    assert np.isnan(dgot[~ok]).all() and np.array_equal(R.bits(dgot[ok]), R.bits(dcube[ok]))
    a = S.on_set("tanh_fast")
    g1 = S.run("pre_bwd", 1, b=vd).cpu().numpy()
    assert np.isnan(g1[S.nan]).all()
    one = np.float32(1)
    plain = v * (one - a * a)                                        # each operation rounded, or 1 - a a as one fma: the compiler may contract
    fused = v * R._fma(-a, a, one)
    assert np.array_equal(R.bits(g1[nn]), R.bits(plain[nn])) or np.array_equal(R.bits(g1[nn]), R.bits(fused[nn]))
    sat = nn & (np.abs(x) >= np.float32(9.1))
    assert (g1[sat] == 0).all()                                      # a saturated tanh passes no cotangent, and no NaN


def test_sigmoid_f(S):
    """The latent encoder's sigmoid (exp2 with a split argument, one Newton step on the reciprocal, the argument clamped to +-87)."""
    x, y = S.x, S.on_set("sigmoid_f")
    nn = ~S.nan
    assert np.isnan(y[S.nan]).all(), y[S.nan]                        # (once 1.0: fminf / fmaxf drop a NaN)
    inside = S.fin & (np.abs(x) <= 87)
    ref = R.ref64("sigmoid_f", x)
    ulps, at, tiny_abs, tiny_at = R.distance(y, ref, x, inside)
    yu, yat, _, _ = R.distance(R.yard32("sigmoid_f", x), ref, x, inside)
    _report("sigmoid_f device on [-87, 87]", ulps, at, tiny_abs, tiny_at)
    print(f"sigmoid_f yardstick 1 / (1 + exp(-x)): max {yu:.3f} ulp at {yat!r}")
    assert ulps <= max(4 * yu, 4.0), (ulps, at, yu)
    assert tiny_abs <= R.TINY
    assert (y[nn] >= 0).all() and (y[nn] <= 1).all()
    ok, where = R.monotone(x, y)
    assert ok, f"not monotone at {where!r}"


# ---- the same edges through the real kernels ------------------------------------------------------------------------------------------------
# The chains of the other tests have Glorot weights and inputs in (-1.3, 1.3): their pre-activations stay inside a few units.  Here the first
# layer is scaled until a good share of them is saturated (|z| > 20) while a share still sits below tanh_fast's seam, and a NaN is put where
# the error estimate does not see it directly: into a parameter in front of a tanh.

SAT_SCALE = 30.0
# (shape, activation) -> seed, picked on the CPU for the precondition below (and, for relu / elu, for test_gpu_activations' kink margin).
SAT_SEEDS = {("small_td", a): 3 for a in ("tanh", "relu", "sigmoid", "softplus", "elu")}
SAT_SEEDS.update({("wide", "tanh"): 1, ("wide", "sigmoid"): 1, ("wide", "relu"): 3374, ("wide", "softplus"): 1702, ("wide", "elu"): 2322})
# "wide" with softplus or elu in BOTH layers: the second layer reads unbounded outputs of a x30 layer, and its pre-activations are large too.  The
# best of 3000 seeds has 4.5 % of the pre-activations below 0.55 (relu: one seed in 6000 reaches 5.1 %), so these two cases ask for 4 %.
SAT_SMALL_SHARE = {("wide", "softplus"): 0.04, ("wide", "elu"): 0.04}


def _sat_case(shape, act, B=8):
    from tests.act_ref import chain64, params
    from tests.test_gpu_activations import SHAPES, _acts
    dims, _, td, pre = SHAPES[shape]
    acts = _acts(shape, act)
    rng = np.random.default_rng(SAT_SEEDS[shape, act])
    p = params(dims, td, rng, bias=0.3)
    p[:(dims[0] + (1 if td else 0)) * dims[1] + dims[1]] *= SAT_SCALE
    u = rng.uniform(-1.3, 1.3, (B, dims[0])).astype(np.float32)
    pa = []
    ref = chain64(dims, acts, td, pre, torch.from_numpy(p).double(), torch.from_numpy(u).double(), 0.3, pa).numpy()
    z = torch.cat([a.reshape(-1) for a in pa]).abs()
    return dims, acts, td, pre, p, u, ref, pa, float((z > 20).double().mean()), float((z < 0.55).double().mean())


@pytest.mark.parametrize("act", ["tanh", "relu", "sigmoid", "softplus", "elu"])
@pytest.mark.parametrize("shape", ["small_td", "wide"])
@pytest.mark.parametrize("col_tile", [64, 0], ids=["one-wave", "four-wave"])
def test_chain_feval_at_saturation(act, shape, col_tile):
    """rnde_debug_feval with the first layer scaled by 30, against the fp64 chain, at test_feval_matches_fp64's tolerance."""
    from tests.act_ref import rel
    from tests.test_gpu_activations import _cfg, _kink_free
    from tests.util import Node
    dims, acts, td, pre, p, u, ref, pa, big, small = _sat_case(shape, act)
    print(f"{shape} {act}: {100 * big:.1f} % of the pre-activations above 20, {100 * small:.1f} % below 0.55")
    assert big >= 0.10 and small >= SAT_SMALL_SHARE.get((shape, act), 0.05), (big, small)
    _kink_free(act, pa)
    node = Node(_cfg(dims, acts, u.shape[0], time_dep=td, pre_act=pre, col_tile=col_tile, regularize=0))
    got = node.feval(u, p, 0.3)
    node.close()
    assert np.isfinite(got).all()
    assert rel(got, ref) <= 2e-6, rel(got, ref)


# seeds for which the fp32 restatement on the CPU stays 1e-5 or closer to the fp64 one (a x30 layer makes the two steps of 0.5 stiff: some seeds
# amplify fp32 rounding to 1e-2, which says nothing about the kernels)
REV_SEEDS = {"tanh": 39, "sigmoid": 26, "softplus": 36}


@pytest.mark.parametrize("act", sorted(REV_SEEDS))
@pytest.mark.parametrize("col_tile", [64, 0], ids=["one-wave", "four-wave"])
def test_chain_reverse_at_saturation(act, col_tile):
    """Two replayed steps of 0.5 and their reverse (test_replay_forward_and_reverse's method) with the first layer scaled by 30: the saturated
    derivatives are zero or tiny, never NaN or Inf; x-bar and p-bar against autograd at that test's 1e-3."""
    from oracle.oracle import Oracle, make_arch
    from tests.act_ref import chain64, params, rel, rk_replay64
    from tests.test_gpu_activations import _cfg
    from tests.util import Node
    dims, td, B = [3, 9, 3], True, 6
    acts = [act, act]
    rng = np.random.default_rng(REV_SEEDS[act])
    p, x = params(dims, td, rng, bias=0.3), rng.uniform(-1.0, 1.0, (B, dims[0])).astype(np.float32)
    p[:(dims[0] + 1) * dims[1] + dims[1]] *= SAT_SCALE
    ubar = rng.standard_normal(x.shape).astype(np.float32)
    dtp, acc = [0.5, 0.5], [1, 1]
    tab = Oracle(make_arch(dims, ["tanh", "tanh"], td), np.float64, solver="Tsit5").tableau()
    node = Node(_cfg(dims, acts, B, time_dep=td, regularize=1, track_ctrl=0, track_initdt=0, max_attempts=16, col_tile=col_tile))
    got = node.forward_replay(x, p, dtp, acc, keep_tape=True)
    assert got["nattempts"] == 2
    att = [(float(s[0]), float(s[1]), int(s[3])) for s in got["steps"]]
    assert [a[2] for a in att] == acc
    P, X = torch.from_numpy(p).double().requires_grad_(True), torch.from_numpy(x).double().requires_grad_(True)
    pa = []
    u = rk_replay64(lambda v, t: chain64(dims, acts, td, 0, P, v, t, pa), X, att, tab)
    z = torch.cat([a.reshape(-1) for a in pa]).abs()
    assert float((z > 20).double().mean()) >= 0.10
    xb, pb, _ = node.backward(ubar)
    node.close()
    gx, gp = torch.autograd.grad(u, (X, P), torch.from_numpy(ubar).double())
    print(f"{act}: u {rel(got['u'], u.detach().numpy()):.2e}, x-bar {rel(xb, gx.numpy()):.2e}, p-bar {rel(pb, gp.numpy()):.2e}")
    assert np.isfinite(got["u"]).all() and np.isfinite(xb).all() and np.isfinite(pb).all()
    assert rel(xb, gx.numpy()) <= 1e-3 and rel(pb, gp.numpy()) <= 1e-3


def _stage_case(B, w1_scale=1.0):
    from tests.util import arch_mnist, glorot_params
    D, H = 8, 50
    rng = np.random.default_rng(D * 100 + H)
    arch = arch_mnist(D, H)
    p = glorot_params(arch, rng, np.float32, 3.0)
    p = (p + 0.05 * rng.standard_normal(p.shape)).astype(np.float32)
    p[:(D + 1) * H] *= np.float32(w1_scale)                          # W1 (the time column with it)
    x = rng.uniform(0, 1, (B, D)).astype(np.float32)
    return arch, p, x, D, H


@pytest.mark.parametrize("matrix_mode", [0, 1])
def test_stage_feval_at_saturation(matrix_mode):
    """The stage engine (tanh_fast2 on pairs) at test_stage_engine_geometry_corners' first shape with W1 scaled by 20: rnde_debug_feval in both
    matrix modes against the fp64 oracle, within that test's forward bound."""
    from tests.test_gpu_forward import _cfg
    from tests.util import Node, Oracle
    arch, p, x, D, H = _stage_case(21, 20.0)
    r64, r32 = Oracle(arch, np.float64).f_eval(p, x, 0.37), Oracle(arch, np.float32).f_eval(p, x, 0.37)
    node = Node(_cfg(arch, 21, reltol=1e-3, abstol=1e-3, col_tile=16), matrix_mode=matrix_mode)
    got = node.feval(x, p, 0.37)
    node.close()
    spread = np.abs(r32 - r64).max()
    err = np.abs(got - r64).max()
    print(f"matrix mode {matrix_mode}: |f - fp64| {err:.2e}, the fp32 oracle's {spread:.2e}")
    assert np.isfinite(got).all()
    assert err <= 3e-5 * max(1.0, np.abs(r64).max()) + 4 * spread


# A NaN in a parameter in front of a tanh layer: every other entry, and x, finite.  RNDE_ERR_NONFINITE is raised from the error estimate and the
# step size only, so the NaN has to get THROUGH the tanh to be seen: while tanh_fast(NaN) was 1.0 these solves finished "successfully".
NONFINITE = 4


def _poison(p, where, n_w, n_b):
    """a copy of p with one NaN: in the first layer's weights (an entry in their middle) or in its bias"""
    q = p.copy()
    q[n_w // 2 if where == "weight" else n_w + n_b // 2] = np.nan
    assert np.isnan(q).sum() == 1
    return q


def _raises_nonfinite(call):
    from regneuralde_jl_amd._lib import RndeError
    with pytest.raises(RndeError) as e:
        call()
    assert e.value.status == NONFINITE, e.value


@pytest.mark.parametrize("where", ["weight", "bias"])
@pytest.mark.parametrize("persist", ["1", "0"])
@pytest.mark.parametrize("matrix_mode", [0, 1])
def test_nan_parameter_is_reported_stage_engine(where, persist, matrix_mode, monkeypatch):
    from tests.test_gpu_forward import _cfg
    from tests.util import Node
    monkeypatch.setenv("RNDE_PERSIST", persist)
    arch, p, x, D, H = _stage_case(9)
    node = Node(_cfg(arch, 9, reltol=1e-3, abstol=1e-3, col_tile=16), matrix_mode=matrix_mode)
    assert np.isfinite(node.forward(x, p)["u"]).all()                # the clean solve is an ordinary one
    _raises_nonfinite(lambda: node.forward(x, _poison(p, where, (D + 1) * H, H)))
    node.close()


@pytest.mark.parametrize("where", ["weight", "bias"])
@pytest.mark.parametrize("col_tile", [64, 0], ids=["one-wave", "four-wave"])
def test_nan_parameter_is_reported_chain_engine(where, col_tile):
    from tests.act_ref import params
    from tests.util import Node, make_cfg
    dims = [3, 5, 3]
    rng = np.random.default_rng(8)
    p, x = params(dims, True, rng, bias=0.3), rng.uniform(-1, 1, (9, 3)).astype(np.float32)
    node = Node(make_cfg(dims, ["tanh", "identity"], 9, reltol=1e-3, abstol=1e-3, col_tile=col_tile))
    assert np.isfinite(node.forward(x, p)["u"]).all()
    _raises_nonfinite(lambda: node.forward(x, _poison(p, where, 4 * 5, 5)))
    node.close()


@pytest.mark.parametrize("where", ["weight", "bias"])
def test_nan_parameter_is_reported_tiled_engine(where):
    from tests.act_ref import params
    from tests.test_gpu_node_tiled import make_cfg, tiled
    dims, acts = [2, 128, 128, 2], ["tanh", "tanh", "identity"]      # test_gpu_eval's TDChain(Dense(3, 128), Dense(129, 128), Dense(129, 2)): a state of 2 and the time
    rng = np.random.default_rng(9)
    p, x = params(dims, True, rng, bias=0.3), rng.uniform(-1, 1, (9, 2)).astype(np.float32)
    node = tiled(make_cfg(dims, acts, True, 9, reltol=1e-3, abstol=1e-3, regularize=1, max_attempts=64))
    assert np.isfinite(node.forward(x, p)["u"]).all()
    _raises_nonfinite(lambda: node.forward(x, _poison(p, where, 3 * 128, 128)))
    node.close()


@pytest.mark.parametrize("where", ["weight", "bias"])
@pytest.mark.parametrize("mw", ["1", "0"], ids=["multi-wave", "one-wave"])
def test_nan_parameter_is_reported_sde_layer(where, mw, monkeypatch):
    from tests.test_gpu_nsde import _cfg, _setup
    from tests.util import NsdeNode
    monkeypatch.setenv("RNDE_SDE_MW", mw)
    drift, diff, p, x, noise = _setup("small", 7, 5, 400)             # drift 3 -> 5 (tanh) -> 3; test_solve_matches_oracle_on_the_same_noise's case
    node = NsdeNode(_cfg(drift, diff, 7, reltol=0.05, abstol=0.05, solver="SOSRI", max_attempts=399))
    ok = node.forward(x, p, noise, check=False)
    assert ok["rc"] == 0 and np.isfinite(ok["u"]).all()
    bad = node.forward(x, _poison(p, where, 3 * 5, 5), noise, check=False)
    assert bad["rc"] == NONFINITE, bad["rc"]
    node.close()


@pytest.mark.parametrize("where", ["weight", "bias"])
def test_nan_parameter_is_reported_ffjord_chain_engine(where):
    from tests import ffjord_chain_ref as CR
    from tests.test_gpu_ffjord_chain import _layer
    dims, acts, B = [2, 10, 2], ["tanh", "identity"], 9                # test_gpu_ffjord_chain's smallest shape
    p, x, e, _ = CR.draw(dims, True, B, 1, 1.0)
    ff = _layer(dims, acts, True, B, p, regularize=True, tol=1e-3)
    with torch.no_grad():
        logpx = ff(x.to("cuda:0"), ff.p, e.to("cuda:0"))[0]
    assert torch.isfinite(logpx).all()
    q = torch.from_numpy(_poison(p.numpy().astype(np.float32), where, 3 * 10, 10)).to("cuda:0")
    with torch.no_grad():
        _raises_nonfinite(lambda: ff(x.to("cuda:0"), q, e.to("cuda:0")))
