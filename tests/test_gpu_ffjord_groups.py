"""Several TrackedFFJORD batches ("groups") in one launch (rnde_ffjord_reserve_groups / rnde_ffjord_forward_groups / rnde_ffjord_group_steps,
include/rnde.h; TrackedFFJORD.logpx_batches and loglikelihood(..., groups=k)), through the C ABI and through the layer.

The yardstick is the single call: a group's logpx, NFE and whole (dt, accepted) log must EQUAL those of rnde_ffjord_forward (or
_forward_exact) on that batch alone with the same p, e and span -- torch.equal / ==, no tolerance.  The single calls here hold at most 9
tiles and meet on one XCD; the group launch is at agent scope whatever its size, so equality also pins that the two forms of the meeting
form the same sums.

Shapes: the smallest that can go wrong.  ConcatSquash MLPDynamics(2, 16) on engine="tiled" (engine 1) and the TD chain [3, 10, 3] with tanh
through rnde_ffjord_create_chain (engine 2), reltol = abstol = 1e-4, max_attempts = 300.  Groups of 16, 40 and 23 columns are 1, 3 and 2
tiles, the last two padded.

The groups that finish apart (SPLIT): parameters from glorot_params(2, 16, seed 9, scale 8), batches of 24, 40 and 16 columns drawn behind
them, the middle one scaled by 4.  tests/ffjord_ref.solve (fp64) takes 23, 38 and 18 attempts with 0, 4 and 0 rejections there, and no EEst
comes closer to 1 than 0.237, so the fp32 controller takes the same decisions; the test asserts on the device's own single-call logs that
the lengths differ and that a group rejects before it compares anything."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import ffjord_chain_ref as CR
from tests import ffjord_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, MAX_ATT = 1e-4, 300
OK, BAD_ARG = 0, 1                          # rnde_status (RNDE_ERR_MAX_ATTEMPTS: _lib.MAX_ATTEMPTS)
SIZES = [16, 40, 23]
CHAIN = ([3, 10, 3], ["tanh", "identity"])
NO_CAPACITY = "no group capacity"


def _L():
    from regneuralde_jl_amd import _lib
    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _layer(dyn, max_batch=64, seed=9, scale=8.0, max_attempts=MAX_ATT, engine="tiled", p=None):
    """(layer, rng): dyn "cs" = MLPDynamics(2, 16), "chain" = the TD chain [3, 10, 3]; the rng stands behind the parameter draw."""
    import regneuralde_jl_amd as rn
    if dyn == "cs":
        m = rn.ffjord.MLPDynamics(2, 16, generator=torch.Generator().manual_seed(seed))
        ff = rn.TrackedFFJORD(m, [0.0, 1.0], True, False, "Tsit5", reltol=TOL, abstol=TOL, max_batch=max_batch, max_attempts=max_attempts, engine=engine)
        rng = np.random.default_rng(seed)
        ff.p = torch.from_numpy(R.glorot_params(2, 16, rng, scale=scale)).to(DEV) if p is None else p
        return ff, rng
    dims, acts = CHAIN
    pp, _, _, rng = CR.draw(dims, True, 1, seed, 2.0)
    model = rn.TDChain(*[rn.Dense(dims[l] + 1, dims[l + 1], acts[l]) for l in range(len(acts))])
    ff = rn.TrackedFFJORD(model, [0.0, 1.0], True, False, "Tsit5", reltol=TOL, abstol=TOL, max_batch=max_batch, max_attempts=max_attempts, engine="tiled")
    assert ff.p.numel() == pp.numel()
    ff.p = pp.to(DEV) if p is None else p
    return ff, rng


def _draw(rng, sizes, D, mult=None):
    mult = mult or [1.0] * len(sizes)
    xs, es = [], []
    for B, m in zip(sizes, mult):
        xs.append((torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)) * np.float32(m)).to(DEV))
        es.append(torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(DEV))
    return xs, es


def _single(ff, x, e, exact):
    """rnde_ffjord_forward / _forward_exact on one batch, untaped: (logpx, NFE, the (dt, accepted) log)."""
    lib, h = _L(), ff._handle().h
    B = x.shape[0]
    logpx = torch.full((B,), float("nan"), device=DEV)
    nfe, nsv, sv = C.c_int64(), C.c_int32(), (C.c_float * (ff.max_attempts + 1))()
    if exact:
        st = lib.lib().rnde_ffjord_forward_exact(h, x.data_ptr(), ff.p.data_ptr(), B, 0.0, 1.0, logpx.data_ptr(), None, C.byref(nfe), sv, C.byref(nsv), 0, _stream())
    else:
        st = lib.lib().rnde_ffjord_forward(h, x.data_ptr(), ff.p.data_ptr(), e.data_ptr(), B, 0.0, 1.0, 0, logpx.data_ptr(), None, C.byref(nfe), sv,
                                           C.byref(nsv), 0, _stream())
    lib.check_ffjord(h, st)
    n = C.c_int32()
    lib.check_ffjord(h, lib.lib().rnde_ffjord_steps(h, None, 0, C.byref(n)))
    arr = (C.c_float * max(2 * n.value, 1))()
    lib.check_ffjord(h, lib.lib().rnde_ffjord_steps(h, arr, n.value, C.byref(n)))
    return logpx.cpu(), int(nfe.value), list(arr[:2 * n.value])


def _groups(ff, xs, es, exact, acc=None, sizes=None, sum_ptr=None, cnt_ptr=None, n_groups=None, drop_e=False, give_e=False):
    """rnde_ffjord_forward_groups: (status, message, [logpx], [NFE], [group status], [(dt, accepted) logs])."""
    lib, h = _L(), ff._handle().h
    sizes = [int(x.shape[0]) for x in xs] if sizes is None else sizes
    n = len(sizes) if n_groups is None else n_groups
    x = torch.cat(xs).contiguous()
    e = None if (exact and not give_e) or drop_e else torch.cat(es).contiguous()
    logpx = torch.full((x.shape[0],), float("nan"), device=DEV)
    Bs, nfe, gst = (C.c_int32 * max(n, len(sizes)))(*sizes), (C.c_int64 * max(n, 1))(), (C.c_int32 * max(n, 1))(*([-1] * max(n, 1)))
    if acc is not None:
        sum_ptr, cnt_ptr = acc.data_ptr(), acc.data_ptr() + 8
    st = lib.lib().rnde_ffjord_forward_groups(h, x.data_ptr(), ff.p.data_ptr(), e.data_ptr() if e is not None else None, n, Bs, 0.0, 1.0, int(exact),
                                              logpx.data_ptr(), nfe, gst, sum_ptr, cnt_ptr, _stream())
    msg = lib.lib().rnde_ffjord_last_error(h).decode()
    torch.cuda.synchronize()
    logs = []
    if st == OK or st == lib.MAX_ATTEMPTS:
        for g in range(n):
            logs.append(ff.group_steps(g))
    return st, msg, list(torch.split(logpx.cpu(), sizes)) if st in (OK, lib.MAX_ATTEMPTS) else None, list(nfe)[:n], list(gst)[:n], logs


def _reserve(ff, g, c):
    lib, h = _L(), ff._handle().h
    st = lib.lib().rnde_ffjord_reserve_groups(h, g, c)
    return st, lib.lib().rnde_ffjord_last_error(h).decode()


def _assert_equal(single, got, what):
    """single: [(logpx, NFE, log)] per group; got: _groups' result"""
    st, msg, lps, nfes, gst, logs = got
    assert st == OK, (what, st, msg)
    assert gst == [OK] * len(single), (what, gst)
    for g, (lp, nfe, log) in enumerate(single):
        assert torch.isfinite(lp).all() and torch.equal(lp, lps[g]), (what, g, float((lp - lps[g]).abs().max()))
        assert nfe == nfes[g] and nfe == 3 + 6 * (len(log) // 2), (what, g, nfe, nfes[g])
        assert log == logs[g], (what, g, len(log) // 2, len(logs[g]) // 2)


# ---- the shared inputs and their single-call results (computed once, never changed) ----
@functools.lru_cache(maxsize=None)
def _case1(dyn, exact):
    ff, rng = _layer(dyn)
    xs, es = _draw(rng, SIZES, ff.in_dims, [1.0, 2.0, 1.0])
    return ff, xs, es, [_single(ff, x, e, exact) for x, e in zip(xs, es)]


@functools.lru_cache(maxsize=None)
def _split():
    ff, rng = _layer("cs")
    xs, es = _draw(rng, [24, 40, 16], 2, [1.0, 4.0, 1.0])
    return ff, xs, es, [_single(ff, x, e, False) for x, e in zip(xs, es)]


# ---- 1. bit equality with single calls ----
@pytest.mark.parametrize("exact", [False, True], ids=["hutchinson", "exact"])
@pytest.mark.parametrize("dyn", ["cs", "chain"])
def test_three_groups_equal_three_single_calls(dyn, exact):
    ff, xs, es, single = _case1(dyn, exact)
    assert _L().lib().rnde_ffjord_engine(ff._handle().h) == (1 if dyn == "cs" else 2)
    assert _reserve(ff, 3, 96)[0] == OK and ff.group_capacity() == (3, 96)
    _assert_equal(single, _groups(ff, xs, es, exact), (dyn, exact))
    print(dyn, "exact" if exact else "hutchinson", "attempts per group:", [len(s[2]) // 2 for s in single])
    # the single call on the handle is what it was, behind a group call too
    again = _single(ff, xs[1], es[1], exact)
    assert torch.equal(again[0], single[1][0]) and again[1:] == single[1][1:]


# ---- 2. groups that finish apart ----
@pytest.mark.parametrize("order", [[0, 1, 2], [1, 2, 0], [2, 0, 1]], ids=["short-long-short", "long-first", "long-last"])
def test_groups_that_finish_apart(order):
    ff, xs, es, single = _split()
    n_att = [len(s[2]) // 2 for s in single]
    rejected = [sum(1 for a in s[2][1::2] if a == 0.0) for s in single]
    print("attempts", n_att, "rejected", rejected)
    assert len(set(n_att)) == 3 and max(n_att) >= min(n_att) + 10, n_att      # (not vacuous: the groups leave the launch at different times)
    assert max(rejected) >= 1 and min(rejected) == 0, rejected
    assert _reserve(ff, 3, 96)[0] == OK
    _assert_equal([single[i] for i in order], _groups(ff, [xs[i] for i in order], [es[i] for i in order], False), order)


# ---- 3. more than 32 tiles in one launch ----
def test_more_than_32_tiles():
    ff, rng = _layer("cs", max_batch=144)
    xs, es = _draw(rng, [144] * 4, 2, [1.0, 2.0, 0.5, 3.0])
    single = [_single(ff, x, e, False) for x, e in zip(xs, es)]
    assert _reserve(ff, 4, 4 * 144)[0] == OK
    _assert_equal(single, _groups(ff, xs, es, False), "36 tiles")
    print("attempts per group:", [len(s[2]) // 2 for s in single])


# ---- 4. one group; the capacity is the switch ----
def test_one_group_equals_the_plain_call_and_release_switches_off():
    ff, xs, es, single = _case1("cs", False)
    fresh, _ = _layer("cs")
    st0, msg0 = _groups(fresh, xs[:1], es[:1], False)[:2]
    assert st0 == BAD_ARG and NO_CAPACITY in msg0 and fresh.group_capacity() == (0, 0)
    assert _reserve(ff, 1, 48)[0] == OK and ff.group_capacity() == (1, 48)
    _assert_equal(single[1:2], _groups(ff, xs[1:2], es[1:2], False), "one group")
    assert _reserve(ff, 0, 0)[0] == OK and ff.group_capacity() == (0, 0)
    st, msg = _groups(ff, xs[1:2], es[1:2], False)[:2]
    assert st == BAD_ARG and msg == msg0
    again = _single(ff, xs[1], es[1], False)         # a handle without a capacity runs what it ran
    assert torch.equal(again[0], single[1][0]) and again[1:] == single[1][1:]


# ---- 5. the sum ----
def test_sum_and_count_accumulate_in_double_and_repeat_bit_for_bit():
    ff, xs, es, single = _case1("cs", False)
    assert _reserve(ff, 3, 96)[0] == OK
    runs = []
    for _ in range(2):
        acc = torch.zeros(2, dtype=torch.float64, device=DEV)
        a = _groups(ff, xs, es, False, acc=acc)
        b = _groups(ff, xs[::-1], es[::-1], False, acc=acc)
        assert a[0] == OK and b[0] == OK
        host = acc.cpu()
        ref = float(np.sum(np.concatenate([lp.numpy().astype(np.float64) for lp in a[2] + b[2]])))
        got = float(host[0])
        print("sum", got, "numpy", ref, "relative", abs(got - ref) / abs(ref))
        assert abs(got - ref) <= 1e-12 * abs(ref)
        assert int(host.view(torch.int64)[1]) == 2 * sum(SIZES)
        runs.append(host.view(torch.int64).clone())
    assert torch.equal(runs[0], runs[1])


# ---- 6. a failing group ----
def test_a_failing_group_is_named_and_leaves_the_others_and_the_sum_alone():
    lib = _L()
    ff0, xs, es, single = _split()
    n_att = [len(s[2]) // 2 for s in single]
    cap = max(n_att) - 1
    assert sorted(n_att)[1] <= cap, n_att                # only the longest group runs out
    long_g = n_att.index(max(n_att))
    ff, _ = _layer("cs", max_attempts=cap, p=ff0.p)
    assert _reserve(ff, 3, 96)[0] == OK
    acc = torch.tensor([1.5, 0.0], dtype=torch.float64, device=DEV)
    before = acc.cpu().view(torch.int64).clone()
    st, msg, lps, nfes, gst, logs = _groups(ff, xs, es, False, acc=acc)
    assert st == lib.MAX_ATTEMPTS and f"group {long_g}" in msg and "max_attempts" in msg, (st, msg)
    assert gst == [lib.MAX_ATTEMPTS if g == long_g else OK for g in range(3)], gst
    assert torch.equal(acc.cpu().view(torch.int64), before)
    for g in range(3):
        if g != long_g:
            assert torch.equal(lps[g], single[g][0]) and logs[g] == single[g][2]
        else:
            assert logs[g] == single[g][2][:2 * cap]
    # the next call on the handle succeeds: the two short groups alone, equal to their single calls
    keep = [g for g in range(3) if g != long_g]
    _assert_equal([single[g] for g in keep], _groups(ff, [xs[g] for g in keep], [es[g] for g in keep], False, acc=acc), "behind a failure")
    host = acc.cpu()
    assert int(host.view(torch.int64)[1]) == sum(int(xs[g].shape[0]) for g in keep) and float(host[0]) != 1.5


# ---- 7. refusals by name, before any launch ----
def test_refusals_name_the_limit():
    lib = _L()
    ff, xs, es, single = _case1("cs", False)
    wg, _ = _layer("cs", engine="workgroup")
    st, msg = _reserve(wg, 3, 96)
    assert st == BAD_ARG and "one-workgroup engine" in msg and "rnde_ffjord_create_tiled" in msg
    st, msg = _groups(wg, xs, es, False)[:2]
    assert st == BAD_ARG and "one-workgroup engine" in msg
    fresh, _ = _layer("cs")
    st, msg = _groups(fresh, xs, es, False)[:2]
    assert st == BAD_ARG and NO_CAPACITY in msg and "rnde_ffjord_reserve_groups" in msg
    for g, c, frag in ((17, 96, "max_groups must be 1..16"), (3, 2, "max_columns must be max_groups..4096"), (3, 4097, "max_columns must be max_groups..4096")):
        st, msg = _reserve(fresh, g, c)
        assert st == BAD_ARG and frag in msg, msg
    assert _reserve(fresh, 2, 96)[0] == OK
    st, msg = _groups(fresh, xs, es, False)[:2]
    assert st == BAD_ARG and "n_groups must be 1..2" in msg and "got 3" in msg
    assert _reserve(fresh, 3, 80)[0] == OK and fresh.group_capacity() == (3, 80)
    st, msg = _groups(fresh, xs, es, False)[:2]
    assert st == BAD_ARG and "need 6 tiles" in msg and "reservation holds 5" in msg
    assert _reserve(fresh, 3, 96)[0] == OK
    st, msg = _groups(fresh, xs, es, False, sizes=[16, 0, 23])[:2]
    assert st == BAD_ARG and "group 1: B must be 1..64" in msg and "got 0" in msg
    st, msg = _groups(fresh, xs, es, False, sizes=[16, 65, 23])[:2]
    assert st == BAD_ARG and "group 1: B must be 1..64" in msg and "got 65" in msg
    st, msg = _groups(fresh, xs, es, False, drop_e=True)[:2]
    assert st == BAD_ARG and "e_dev is required unless exact" in msg
    st, msg = _groups(fresh, xs, es, True, give_e=True)[:2]
    assert st == BAD_ARG and "e_dev must be NULL with exact" in msg
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    for kw in ({"sum_ptr": acc.data_ptr()}, {"cnt_ptr": acc.data_ptr() + 8}):
        st, msg = _groups(fresh, xs, es, False, **kw)[:2]
        assert st == BAD_ARG and "sum_dev and count_dev come together" in msg
    assert torch.equal(acc.cpu(), torch.zeros(2, dtype=torch.float64))
    # a handle that holds a tape keeps its reservation as it is
    x, e = xs[0], es[0]
    logpx, nfe, nsv, sv = torch.empty(16, device=DEV), C.c_int64(), C.c_int32(), (C.c_float * (MAX_ATT + 1))()
    h = fresh._handle().h
    lib.check_ffjord(h, lib.lib().rnde_ffjord_forward(h, x.data_ptr(), fresh.p.data_ptr(), e.data_ptr(), 16, 0.0, 1.0, 0, logpx.data_ptr(), None, C.byref(nfe),
                                                      sv, C.byref(nsv), 1, _stream()))
    st, msg = _reserve(fresh, 0, 0)
    assert st == BAD_ARG and "holds a tape" in msg and fresh.group_capacity() == (3, 96)
    # nothing above launched anything: the fresh handle's first group call is the single calls'
    _assert_equal(single, _groups(fresh, xs, es, False), "behind the refusals")


# ---- 8. the layer ----
def test_layer_logpx_batches_and_loglikelihood():
    import regneuralde_jl_amd as rn
    ff, rng = _layer("cs")
    sizes = [40, 40, 40, 40, 40, 40, 23]
    batches = [rng.standard_normal((B, 2)).astype(np.float32) for B in sizes]
    SEED = 0x5EED
    ff._seed = SEED
    ll = rn.ffjord.loglikelihood(ff, batches, groups=3)
    assert ff.group_capacity() == (3, 3 * 48)
    ff._seed = SEED
    lps, nfes = [], []
    for i in range(0, 7, 3):
        a, b = ff.logpx_batches([torch.from_numpy(x).to(DEV) for x in batches[i:i + 3]])
        lps += a; nfes += b
    assert [tuple(lp.shape) for lp in lps] == [(B,) for B in sizes] and len(nfes) == 7
    mean = float(np.sum(np.concatenate([lp.cpu().numpy().astype(np.float64) for lp in lps]))) / sum(sizes)
    print("loglikelihood", ll, "float64 mean", mean, "relative", abs(ll - mean) / abs(mean))
    assert abs(ll - mean) <= 1e-12 * abs(mean)
    ff._seed = SEED
    with torch.no_grad():
        for i, x in enumerate(batches):
            lp, _, _, nfe, _ = ff(torch.from_numpy(x).to(DEV))
            assert torch.equal(lp, lps[i]) and nfe == nfes[i], i
    # groups = 1 is the loop it was: one solve and one float(logpx.sum()) per batch
    ff._seed = SEED
    one = rn.ffjord.loglikelihood(ff, batches)
    ff._seed = SEED
    assert rn.ffjord.loglikelihood(ff, batches, groups=1) == one
    ff._seed = SEED
    total = 0.0
    with torch.no_grad():
        for x in batches:
            total += float(ff(torch.from_numpy(x).to(DEV))[0].sum())
    assert one == total / sum(sizes)
    # the exact trace, and the refusal of an engine without tiles
    ex = rn.ffjord.loglikelihood(ff, batches, exact=True, groups=3)
    lpe = []
    for i in range(0, 7, 3):
        lpe += ff.logpx_batches([torch.from_numpy(x).to(DEV) for x in batches[i:i + 3]], exact=True)[0]
    with torch.no_grad():
        assert torch.equal(lpe[6], ff(torch.from_numpy(batches[6]).to(DEV), exact=True)[0])
    mean = float(np.sum(np.concatenate([lp.cpu().numpy().astype(np.float64) for lp in lpe]))) / sum(sizes)
    assert abs(ex - mean) <= 1e-12 * abs(mean)
    wg, _ = _layer("cs", engine="workgroup")
    with pytest.raises(ValueError, match="tiled"):
        rn.ffjord.loglikelihood(wg, batches, groups=3)


# ---- 9. stale and uninitialised memory (the pattern of tests/test_gpu_memory_independence.py) ----
@pytest.mark.parametrize("dyn,exact", [("cs", False), ("cs", True), ("chain", False)], ids=["cs", "cs-exact", "chain"])
def test_group_workspaces_do_not_depend_on_what_memory_held(monkeypatch, dyn, exact):
    lib = _L().lib()
    _, xs, es, single = _case1(dyn, exact)
    p = _case1(dyn, exact)[0].p
    # (b) every fresh allocation filled with NaN bytes: the reservation's eight owners (nine with the exact trace's scratch on engine 1)
    c0 = (int(lib.rnde_debug_poison_allocs()), int(lib.rnde_debug_poison_bytes()))
    monkeypatch.setenv("RNDE_POISON", "1")
    ff, _ = _layer(dyn, p=p)
    assert _reserve(ff, 3, 96)[0] == OK
    c1 = (int(lib.rnde_debug_poison_allocs()), int(lib.rnde_debug_poison_bytes()))
    rows = ff.in_dims + 1
    assert c1[0] - c0[0] >= 8 and c1[1] - c0[1] >= 10 * rows * 96 * 4 + 3 * MAX_ATT * 64, (c0, c1)
    _assert_equal(single, _groups(ff, xs, es, exact), "poisoned reservation")
    monkeypatch.delenv("RNDE_POISON")
    # (c) a reservation that has just served other inputs under other parameters, every reserved tile in use
    ff, rng = _layer(dyn, seed=77, scale=4.0)
    assert _reserve(ff, 3, 96)[0] == OK
    dx, de = _draw(rng, [32, 48, 16], ff.in_dims, [3.0, 3.0, 3.0])
    assert _groups(ff, dx, de, exact)[0] == OK
    ff.p = p
    _assert_equal(single, _groups(ff, xs, es, exact), "dirty reservation")
