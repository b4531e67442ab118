"""Bit-for-bit A/B of the tile driver (csrc/rnde_tile_driver.h) against another build of the library, usually the parent commit's:

    python tools/ab_tile_bits.py [--parent regneuralde.jl_amd/lib/librnde_parent.so] [--new regneuralde.jl_amd/lib/librnde.so]

Each library (selected with RNDE_LIB, as tools/build_variant.sh places variants) runs the same seeded cases in a fresh child process of its own,
one after the other, each under its own `timeout`; the script stops at the first nonzero exit, and a child ends at the first call the
library does not serve (a refusal, a HIP error, a meeting that timed out): nothing is caught, nothing more is launched.  Every array the cases return -- end states,
saved states, step logs, saved values, p-bar, x-bar, tspan-bar, logpx, the regulariser rows, samples, feval outputs -- is compared with
numpy.array_equal.  Success is reported only if, by the FIRST library's own step logs, every engine (1: ConcatSquash, 2: Dense chain FFJORD,
4: tiled NeuralODE) had a case with a rejected attempt and a case above 32 tiles (the agent-scope meeting).  The verdict goes under "bits" into
profiles/tile_driver_three.json (other keys of the file are kept).

Cases.  NeuralODE (engine 4): [3, 7, 3] TD at B = 5 and 513 (33 tiles), [6, 80, 72, 6] with relu / softplus / tanh at B = 17 and 37,
[70, 96, 70] TD at B = 17 (state rows above 64); per shape a taped forward + backward with RNDE_REG_ERR and a nonzero saved-value cotangent under
tracking (0, 0), (1, 0), (1, 1), saveat (the start, two interior times, the end) under (0, 0) and (1, 1), save_everystep, the replay of a log
that holds a rejection, feval at t = 0 and 0.71; and the vetted naturally rejecting case of tests/test_gpu_node_tiled.py (pad_td_rej).
FFJORD (engines 1, 2): ConcatSquash (2, 16) and (43, 100), TD [2, 10, 2] and [5, 12, 9, 5], each at B = 17, 37, 513; per case a taped forward +
backward, the kinetic pair, the exact-trace pair, track_ctrl on (free-running and along a log with a rejection), sample, feval (Hutchinson,
exact, kinetic); and the vetted naturally rejecting cases of tests/test_gpu_ffjord_track.py (td2-B5, cs-B5) under track_ctrl.  tol = 1e-5.
The host-side paths beside the single tiled solve: the one-workgroup engine (engine 0, ConcatSquash (2, 16) at B = 17: forward + backward and
the kinetic pair); rnde_ffjord_forward_groups with three unequal groups (B = 1, 17, 37), probe and exact, adding into the sum / count
accumulators, on ConcatSquash (2, 16) and TD [2, 10, 2]; rnde_ffjord_nll_grad in modes 0, 1 and 2 on engines 1 and 2 and modes 0 and 2 on
engine 0, at B = 37.  --key names the key of the output file that takes the verdict ("bits" by default).
The handles, inputs and vetted cases are those of the GPU suites (tests/test_gpu_node_tiled*.py, tests/test_gpu_ffjord_track.py, tests/act_ref.py,
tests/ffjord_ref.py), imported from there: the tool moves with them.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOL = 1e-5
REPLAY_DTP, REPLAY_ACC = [0.25, 0.5, 0.25, 0.25, 0.25], [1, 0, 1, 1, 1]
SAVEAT = np.array([0.0, 0.3, 0.31, 1.0], dtype=np.float32)


def scaled_params(dims, td, rng, factors):
    from tests.act_ref import params
    p = params(dims, td, rng, bias=0.3)
    o = 0
    for l, f in enumerate(factors):
        n = (dims[l] + (1 if td else 0)) * dims[l + 1] + dims[l + 1]
        p[o:o + n] *= f
        o += n
    return p


# ---- engine 4 ----------------------------------------------------------------------------------------------------------------------------------

NODE_SHAPES = [("n3", [3, 7, 3], ["tanh", "identity"], True, (60.0, 0.3), (5, 513)),
               ("n6", [6, 80, 72, 6], ["relu", "softplus", "tanh"], False, (8.0, 1.0, 0.3), (17, 37)),
               ("n70", [70, 96, 70], ["tanh", "tanh"], True, (30.0, 0.1), (17,))]


def node_case(out, logs, name, dims, acts, td, p, x):
    from regneuralde_jl_amd import _lib
    from tests.test_gpu_node_tiled import make_cfg, tiled
    from tests.test_gpu_node_tiled_saveat import _everystep
    from tests.test_gpu_node_tiled_track import set_tracking
    B, D = x.shape
    node = tiled(make_cfg(dims, acts, td, B, reltol=TOL, abstol=TOL, regularize=1, max_attempts=128))
    _lib.check(node.h, node.L.rnde_node_tiled_reserve_saveat(node.h, 129))
    rng = np.random.default_rng(77)
    ubar = rng.uniform(0.5, 1.5, (B, D)).astype(np.float32)
    ubar_sv = rng.uniform(0.5, 1.5, (B, len(SAVEAT), D)).astype(np.float32)

    def keep(tag, fwd, bwd=None):
        for k in ("u", "steps", "saveval"):
            out[f"{name}/{tag}/{k}"] = fwd[k]
        logs.append((4, B, fwd["steps"]))
        if bwd is not None:
            for k, v in zip(("x_bar", "p_bar", "tspan_bar"), bwd):
                out[f"{name}/{tag}/{k}"] = v

    for flags in ((0, 0), (1, 0), (1, 1)):
        set_tracking(node, *flags)
        f = node.forward(x, p, keep_tape=True)
        keep(f"taped{flags}", f, node.backward(ubar, rng.uniform(0.5, 1.5, len(f["saveval"])).astype(np.float32)))
    for flags in ((0, 0), (1, 1)):
        set_tracking(node, *flags)
        f = node.forward_saveat(x, p, SAVEAT, keep_tape=True)
        keep(f"saveat{flags}", f, node.backward(ubar_sv, np.ones(len(f["saveval"]), np.float32)))
    st, n, times, u = _everystep(node, x, p, 1, 129, keep_tape=True)
    _lib.check(node.h, st)
    out[f"{name}/everystep/u"], out[f"{name}/everystep/times"] = u, times
    for k, v in zip(("x_bar", "p_bar", "tspan_bar"), node.backward(rng.uniform(0.5, 1.5, u.shape).astype(np.float32), None)):
        out[f"{name}/everystep/{k}"] = v
    f = node.forward_replay(x, p, REPLAY_DTP, REPLAY_ACC, keep_tape=True)      # (tracking is (1, 1) here)
    keep("replay", f, node.backward(ubar, np.ones(len(f["saveval"]), np.float32)))
    for t in (0.0, 0.71):
        out[f"{name}/feval{t}"] = node.feval(x, p, t)
    node.close()


def node_cases(out, logs):
    from tests.test_gpu_node_tiled import adaptive_case
    for key, dims, acts, td, factors, batches in NODE_SHAPES:
        for B in batches:
            rng = np.random.default_rng(1000 + B)
            p = scaled_params(dims, td, rng, factors)
            x = rng.uniform(-1.0, 1.0, (B, dims[0])).astype(np.float32)
            node_case(out, logs, f"{key}-B{B}", dims, acts, td, p, x)
    dims, acts, td, p, x = adaptive_case("pad_td_rej")
    node_case(out, logs, "pad_td_rej", dims, acts, td, p, x)


# ---- engines 1 and 2 ---------------------------------------------------------------------------------------------------------------------------

FF_DYN = [("cs2", ("cs", 2, 16), (5.0, 2.0)), ("cs43", ("cs", 43, 100), (1.0, 1.0)),
          ("td2", ("chain", [2, 10, 2], ["tanh", "identity"], True), (30.0, 0.3)),
          ("td5", ("chain", [5, 12, 9, 5], ["tanh", "softplus", "identity"], True), (30.0, 1.0, 0.3))]


def ff_inputs(dyn, recipe, B):
    import torch
    from tests import ffjord_ref as R
    rng = np.random.default_rng(2000 + B)
    if dyn[0] == "chain":
        D = dyn[1][0]
        p = scaled_params(dyn[1], dyn[3], rng, recipe)
        x = rng.uniform(-1.0, 1.0, (B, D)).astype(np.float32)
    else:
        D = dyn[1]
        p = R.glorot_params(dyn[1], dyn[2], rng, recipe[0])
        x = (rng.standard_normal((B, D)) * recipe[1]).astype(np.float32)
    e = rng.standard_normal((B, D)).astype(np.float32)
    g = (rng.standard_normal(B) * 0.02 / B).astype(np.float32)
    return tuple(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for v in (p, x, e, g))


def ff_case(out, logs, name, dyn, p, x, e, g, full=True):
    import torch
    from tests.test_gpu_ffjord_track import DEV, Handle
    engine = 2 if dyn[0] == "chain" else 1
    B, D = x.shape
    chk = lambda hd, st: hd.rn._lib.check_ffjord(hd.h, st)

    def pair(tag, hd, fwd, sv_bar):
        logpx, sv, log = fwd
        pb, xb = hd.backward(g, sv_bar)
        out[f"{name}/{tag}/logpx"], out[f"{name}/{tag}/saveval"] = logpx.cpu().numpy(), sv
        out[f"{name}/{tag}/steps"] = np.array(log, dtype=np.float32)
        out[f"{name}/{tag}/p_bar"], out[f"{name}/{tag}/x_bar"] = pb.numpy(), xb.numpy()
        logs.append((engine, B, np.array([[t, dt, 0.0, acc] for t, dt, acc in log], dtype=np.float32)))

    hd = Handle(dyn, B, regularize=1, track=0)
    if full:
        pair("taped", hd, hd.forward(x, p, e), 0.7)
        pair("exact", hd, hd.forward(x, p, None), 0.7)
    hd.set_track(1)
    pair("tracked", hd, hd.forward(x, p, e), 0.7)
    pair("tracked_replay", hd, hd.forward(x, p, e, list(zip(REPLAY_DTP, REPLAY_ACC))), 0.7)
    if full:
        xd, pd, ed = hd.x, hd.p, hd.e
        xs = torch.empty_like(xd)
        chk(hd, hd.L.rnde_ffjord_sample(hd.h, pd.data_ptr(), xd.data_ptr(), B, 0.0, 1.0, 0, xs.data_ptr(), None))
        out[f"{name}/sample"] = xs.cpu().numpy()
        for tag, exact in (("feval_hutch", 0), ("feval_exact", 1)):
            o = torch.empty(B * (D + 1), device=DEV)
            chk(hd, hd.L.rnde_ffjord_debug_feval(hd.h, xd.data_ptr(), pd.data_ptr(), ed.data_ptr(), B, 0.71, exact, o.data_ptr(), None))
            torch.cuda.synchronize()
            out[f"{name}/{tag}"] = o.cpu().numpy()
    hd.close()
    if not full:
        return
    hk = Handle(dyn, B, regularize=0)      # (the kinetic rows are served on a regularize = 0 handle)
    xd, pd, ed, gd = (v.to(DEV).contiguous() for v in (x, p, e, g))
    logpx, reg, nfe = torch.empty(B, device=DEV), torch.empty(2 * B, device=DEV), C.c_int64()
    chk(hk, hk.L.rnde_ffjord_forward_kinetic(hk.h, xd.data_ptr(), pd.data_ptr(), ed.data_ptr(), B, 0.0, 1.0, 0, logpx.data_ptr(), reg.data_ptr(), None,
                                             C.byref(nfe), 1, None))
    rb = torch.full((2 * B,), 0.01 / B, device=DEV)
    pb, xb = torch.empty_like(pd), torch.empty_like(xd)
    chk(hk, hk.L.rnde_ffjord_backward_kinetic(hk.h, gd.data_ptr(), rb.data_ptr(), pb.data_ptr(), xb.data_ptr(), None))
    o = torch.empty(B * (D + 3), device=DEV)
    chk(hk, hk.L.rnde_ffjord_debug_feval_kinetic(hk.h, xd.data_ptr(), pd.data_ptr(), ed.data_ptr(), B, 0.71, o.data_ptr(), None))
    torch.cuda.synchronize()
    for k, v in (("logpx", logpx), ("reg", reg), ("p_bar", pb), ("x_bar", xb), ("feval", o)):
        out[f"{name}/kinetic/{k}"] = v.cpu().numpy()
    out[f"{name}/kinetic/nfe"] = np.array([nfe.value])
    hk.close()


def ff_cases(out, logs):
    from tests.test_gpu_ffjord_track import CASES, _inputs
    for key, dyn, recipe in FF_DYN:
        for B in (17, 37, 513):
            ff_case(out, logs, f"{key}-B{B}", dyn, *ff_inputs(dyn, recipe, B))
    for key in ("td2-B5", "cs-B5"):
        ff_case(out, logs, key, CASES[key][0], *_inputs(key), full=False)


def ff_steps(hd, entry, *lead):
    """The (dt, accepted) export of rnde_ffjord_steps / rnde_ffjord_group_steps (lead: the group)."""
    n = C.c_int32()
    hd.rn._lib.check_ffjord(hd.h, entry(hd.h, *lead, None, 0, C.byref(n)))
    arr = (C.c_float * max(2 * n.value, 1))()
    hd.rn._lib.check_ffjord(hd.h, entry(hd.h, *lead, arr, n.value, C.byref(n)))
    return np.array(arr[:2 * n.value], dtype=np.float32)


def ff_engine0_case(out, logs, name, dyn, p, x, e, g):
    """The one-workgroup engine: a taped forward + backward (regularize = 1, a nonzero saved-value cotangent) and the kinetic pair."""
    import torch
    from tests.test_gpu_ffjord_track import DEV, Handle
    B = x.shape[0]
    hd = Handle(dyn, B, regularize=1, engine0=True)
    logpx, sv, log = hd.forward(x, p, e)
    pb, xb = hd.backward(g, 0.7)
    for k, v in (("logpx", logpx.cpu().numpy()), ("saveval", sv), ("steps", np.array(log, dtype=np.float32)), ("p_bar", pb.numpy()), ("x_bar", xb.numpy())):
        out[f"{name}/taped/{k}"] = v
    logs.append((0, B, np.array([[t, dt, 0.0, acc] for t, dt, acc in log], dtype=np.float32)))
    hd.close()
    hk = Handle(dyn, B, regularize=0, engine0=True)
    chk = lambda st: hk.rn._lib.check_ffjord(hk.h, st)
    xd, pd, ed, gd = (v.to(DEV).contiguous() for v in (x, p, e, g))
    logpx, reg, nfe = torch.empty(B, device=DEV), torch.empty(2 * B, device=DEV), C.c_int64()
    chk(hk.L.rnde_ffjord_forward_kinetic(hk.h, xd.data_ptr(), pd.data_ptr(), ed.data_ptr(), B, 0.0, 1.0, 0, logpx.data_ptr(), reg.data_ptr(), None, C.byref(nfe), 1, None))
    rb = torch.full((2 * B,), 0.01 / B, device=DEV)
    pb, xb = torch.empty_like(pd), torch.empty_like(xd)
    chk(hk.L.rnde_ffjord_backward_kinetic(hk.h, gd.data_ptr(), rb.data_ptr(), pb.data_ptr(), xb.data_ptr(), None))
    torch.cuda.synchronize()
    for k, v in (("logpx", logpx), ("reg", reg), ("p_bar", pb), ("x_bar", xb)):
        out[f"{name}/kinetic/{k}"] = v.cpu().numpy()
    out[f"{name}/kinetic/nfe"], out[f"{name}/kinetic/steps"] = np.array([nfe.value]), ff_steps(hk, hk.L.rnde_ffjord_steps)
    hk.close()


GROUP_SIZES = (1, 17, 37)


def ff_groups_case(out, name, dyn, recipe):
    """rnde_ffjord_forward_groups with three unequal groups, probe and exact, adding into the sum / count accumulators (twice: they accumulate)."""
    import torch
    from tests.test_gpu_ffjord_track import DEV, Handle
    n, cols = len(GROUP_SIZES), sum(GROUP_SIZES)
    p, x, e, _ = ff_inputs(dyn, recipe, cols)
    hd = Handle(dyn, max(GROUP_SIZES), regularize=1)
    chk = lambda st: hd.rn._lib.check_ffjord(hd.h, st)
    chk(hd.L.rnde_ffjord_reserve_groups(hd.h, n, 16 * sum((b + 15) // 16 for b in GROUP_SIZES)))
    xd, pd, ed = (v.to(DEV).contiguous() for v in (x, p, e))
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)      # (the sum, then the count's eight bytes)
    for tag, exact in (("probe", 0), ("exact", 1), ("probe_again", 0)):
        logpx = torch.full((cols,), float("nan"), device=DEV)
        Bs, nfe, gst = (C.c_int32 * n)(*GROUP_SIZES), (C.c_int64 * n)(), (C.c_int32 * n)(*([-1] * n))
        chk(hd.L.rnde_ffjord_forward_groups(hd.h, xd.data_ptr(), pd.data_ptr(), None if exact else ed.data_ptr(), n, Bs, 0.0, 1.0, exact, logpx.data_ptr(), nfe, gst,
                                            acc.data_ptr(), acc.data_ptr() + 8, None))
        torch.cuda.synchronize()
        out[f"{name}/{tag}/logpx"], out[f"{name}/{tag}/nfe"], out[f"{name}/{tag}/status"] = logpx.cpu().numpy(), np.array(list(nfe)), np.array(list(gst))
        out[f"{name}/{tag}/sum_count_bytes"] = acc.cpu().numpy().view(np.uint8)
        for gi in range(n):
            out[f"{name}/{tag}/steps{gi}"] = ff_steps(hd, hd.L.rnde_ffjord_group_steps, gi)
    hd.close()


def ff_nll_grad_case(out, name, dyn, recipe, B, modes, engine0=False):
    """rnde_ffjord_nll_grad: mode 0 (probe) and 1 (exact) on a regularize = 1 handle with lambda_r, mode 2 (kinetic rows) on a regularize = 0 one."""
    import torch
    from tests.test_gpu_ffjord_track import DEV, Handle
    p, x, e, _ = ff_inputs(dyn, recipe, B)
    xd, pd, ed = (v.to(DEV).contiguous() for v in (x, p, e))
    for mode in modes:
        hd = Handle(dyn, B, regularize=0 if mode == 2 else 1, engine0=engine0)
        pb, xb, lp, terms = torch.full_like(pd, float("nan")), torch.full_like(xd, float("nan")), torch.full((B,), float("nan"), device=DEV), torch.full((3,), float("nan"), device=DEV)
        reg, nfe = C.c_float(float("nan")), C.c_int64(-1)
        lam = (0.0, 0.01, 0.02) if mode == 2 else (0.5, 0.0, 0.0)
        st = hd.L.rnde_ffjord_nll_grad(hd.h, xd.data_ptr(), pd.data_ptr(), None if mode == 1 else ed.data_ptr(), B, 0.0, 1.0, 0, mode, *lam, pb.data_ptr(), xb.data_ptr(),
                                       lp.data_ptr(), terms.data_ptr(), C.byref(reg), C.byref(nfe), None)
        hd.rn._lib.check_ffjord(hd.h, st)
        torch.cuda.synchronize()
        for k, v in (("p_bar", pb), ("x_bar", xb), ("logpx", lp), ("terms", terms)):
            out[f"{name}/mode{mode}/{k}"] = v.cpu().numpy()
        out[f"{name}/mode{mode}/reg_nfe"] = np.array([reg.value, nfe.value], dtype=np.float64)
        out[f"{name}/mode{mode}/steps"] = ff_steps(hd, hd.L.rnde_ffjord_steps)
        hd.close()


def ff_host_side_cases(out, logs):
    """What the host-side paths beside the single tiled solve need: engine 0, the group call, the one-call training step."""
    cs, td = FF_DYN[0], FF_DYN[2]
    ff_engine0_case(out, logs, "e0-cs2-B17", cs[1], *ff_inputs(cs[1], cs[2], 17))
    for key, dyn, recipe in (cs, td):
        ff_groups_case(out, f"groups-{key}", dyn, recipe)
        ff_nll_grad_case(out, f"nll-{key}-B37", dyn, recipe, 37, (0, 1, 2))
    ff_nll_grad_case(out, "nll-e0-cs2-B37", cs[1], cs[2], 37, (0, 2), engine0=True)


def child(path):
    out, logs = {}, []
    node_cases(out, logs)
    ff_cases(out, logs)
    ff_host_side_cases(out, logs)
    for i, (engine, B, steps) in enumerate(logs):
        out[f"_log/{i:04d}/e{engine}/B{B}"] = steps
    np.savez(path, **out)
    print(f"{os.environ.get('RNDE_LIB')}: {len(out)} arrays, {len(logs)} step logs", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "regneuralde.jl_amd", "lib", "librnde_parent.so"))
    ap.add_argument("--new", default=os.path.join(ROOT, "regneuralde.jl_amd", "lib", "librnde.so"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child")
    ap.add_argument("--workdir", help="where the two children leave their arrays (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_driver_three.json"))
    ap.add_argument("--key", default="bits", help="the key of --out that takes the verdict")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not a.workdir:      # (the children's arrays are of no use once compared)
        with tempfile.TemporaryDirectory(prefix="ab_tile_bits_") as tmp:
            a.workdir = tmp
            return compare(a)
    os.makedirs(a.workdir, exist_ok=True)
    return compare(a)


def compare(a):
    got = {}
    for side, lib in (("parent", a.parent), ("new", a.new)):      # one after the other, a fresh process each
        path = os.path.join(a.workdir, f"ab_tile_bits_{side}.npz")
        env = dict(os.environ, RNDE_LIB=os.path.abspath(lib))
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", path], env=env, cwd=ROOT)
        if r.returncode != 0:
            print(f"{side} ({lib}): exit status {r.returncode}; stopping")
            return r.returncode
        got[side] = dict(np.load(path))
    P, N = got["parent"], got["new"]
    differing = sorted(k for k in P if k not in N or not np.array_equal(P[k], N[k])) + sorted(k for k in N if k not in P)
    cover = {}
    for k, steps in P.items():
        if not k.startswith("_log/"):
            continue
        _, _, engine, B = k.split("/")
        c = cover.setdefault(engine, dict(logs=0, with_rejection=0, above_32_tiles=0))
        c["logs"] += 1
        c["with_rejection"] += int(len(steps) > 0 and bool((steps[:, 3] == 0).any()))
        c["above_32_tiles"] += int((int(B[1:]) + 15) // 16 > 32)
    covered = all(e in cover and cover[e]["with_rejection"] > 0 and cover[e]["above_32_tiles"] > 0 for e in ("e1", "e2", "e4"))
    res = dict(how="tools/ab_tile_bits.py: numpy.array_equal per array, one child process per library", parent=os.path.basename(a.parent),
               new=os.path.basename(a.new), arrays=len(P), differing=differing, coverage_by_parent_step_logs=cover, covered=covered,
               equal=not differing and covered)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc[a.key] = res
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "differing"}), flush=True)
    for k in differing[:40]:
        print("differs:", k)
    if not covered:
        print("NOT REPORTED AS EQUAL: the parent's step logs lack a rejected attempt or a launch above 32 tiles on some engine")
    return 0 if res["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
