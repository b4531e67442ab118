"""Bit-for-bit A/B of the ODE forward solve (csrc/rnde.hip: prepare, the three solve forms, the epilogue, the debug entries) and the three ODE
reverse passes (csrc/rnde_reverse.hip: stage engine, one-wave chain, multi-wave chain), against another build of the library, usually the parent
commit's:

    python tools/ab_node_bits.py [--parent regneuralde.jl_amd/lib/librnde_parent.so] [--new regneuralde.jl_amd/lib/librnde.so]

The method is tools/ab_tile_bits.py's: each library (selected with RNDE_LIB) runs the same seeded cases in a fresh child process of its own, one
after the other, each under its own `timeout`; the script stops at the first nonzero exit, and a child ends at the first call the library does
not serve: nothing is caught, nothing more is launched.  Every array the cases return -- u, saved states, step log, saved values, x-bar, p-bar,
tspan-bar -- is compared with numpy.array_equal.  Success is reported only if, by the FIRST library's own step logs, every engine (stage,
chain1 = one wave per 16 columns, chainmw = four waves) had a case with a rejected attempt.  The verdict, the array count and the per-engine
rejection evidence go to profiles/forward_plan_bits.json (profiles/reverse_plan_bits.json is the record of the reverse cases alone, from
before the forward cases were added).

Cases (the handles and inputs are those of the GPU suites -- tests/test_gpu_forward.py, tests/test_gpu_chain.py, tests/test_gpu_activations.py,
tests/golden/make_golden.py -- imported from there: the tool moves with them); every case is a taped forward and its backward with a nonzero
saved-value cotangent under tracking (1, 1):
  stage, headline geometry   [784, 100, 784], B = 19 (two column tiles, the last one padded), tol 1e-3, scale 3: regularize 0..4 without saveat and
                             1, 2, 3 with saveat = linspace(0, 1, 13) (the four EX instantiations of the bf16x3 attempt kernel), each under RNDE_X3
                             default / 0 and RNDE_PERSIST default / 0 (read at creation: a handle each)
  stage, side stream         the B = 16 case at the reference tolerance (tests/golden/mnist_B16_reftol_x3.npz's inputs); n_att >= 8 is asserted, so
                             the weight-gradient groups underneath the sweep run
  stage, pre-reduction       B = 2048 at tol 1e-3: 7 * 128 = 896 partials, the threshold of rnde_bpart_reduce_kernel
  stage, generic kernels     kinds small (B = 12) and test_node (B = 5) with act[1] identity and tanh; the rough cases of
                             tests/test_gpu_forward.py (weight scale >= 8) and a replay along a log with a rejected attempt
  chain, layouts 64 and 65   latent (B = 4, 70), chain3 (B = 19), small (B = 12): regularize 1..4; saveat of 49 points and of [0.1, 0.5, 0.9]; a
                             replay along a log with a rejected attempt; the latent shape with and without RNDE_CHAIN_GENERIC
  chain, other activation    softplus on [3, 9, 3] (tests/test_gpu_activations.py's replay shape), both layouts: the ALT / LAT = 2 kernels
  multi-wave only            DP5 (chain3, B = 19) and DOP853 (latent, B = 70); RNDE_CHAIN_BSWEEP default and 0
Forward cases (forward_cases; the same shapes).  Each asserts, in the child and so first of all by the FIRST library, that the path it is there
for was taken -- from the step log, rnde_node_one_launch_solves and rnde_node_launches_per_attempt -- and leaves that evidence as an array:
  untaped forwards           stage (one-launch solve, with and without RNDE_SOLVE_FOLD; RNDE_STAGE_SOLVE=0: the chunked loop over the persistent
                             attempt kernel; RNDE_PERSIST=0: over the seven-launch kernels), one-wave chain, multi-wave chain (one-launch solve;
                             RNDE_CHAIN_SOLVE=0: chunked)
  forward_everystep          stage (headline and generic kernels), one-wave and multi-wave chain, save_start on and off: count, times, states, log
  rnde_debug_feval/_attempt  all three engines (stage: persistent and seven-launch kernels)
  attempt-limit redo         a taped multi-wave one-launch solve of more than 48 attempts on a fresh handle (the first run ends at the limit of 48,
                             the redo has room for max_attempts), with its backward
  max_attempts               a solve that ends there, each solve form: status, attempt count, message, step log
  more than one chunk        RNDE_PERSIST=0 (stage), the one-wave chain and RNDE_CHAIN_SOLVE=0 (multi-wave, taped): more attempts than the first
                             chunk of a fresh handle (12)
"""
import ctypes as C
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPLAY_DTP, REPLAY_ACC = [0.25, 0.5, 0.25, 0.25, 0.25], [1, 0, 1, 1, 1]
SAVEAT13 = np.linspace(0, 1, 13).astype(np.float32)
SAVEAT49 = np.linspace(0, 1, 49).astype(np.float32)
SAVEAT3 = np.array([0.1, 0.5, 0.9], dtype=np.float32)
# chosen from the parent build's step logs (asserted again by every run): more than the 12 attempts of a fresh handle's first chunk; more than the
# 48 attempts a fresh handle's taped one-launch multi-wave solve has room for
TOL_CHUNKS = dict(reltol=1e-6, abstol=1e-6)
TOL_REDO = dict(reltol=1.4e-8, abstol=1.4e-8)


class Env:
    """Environment switches the library reads when a handle is created (None: unset)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def run(out, logs, engine, name, cfg, x, p, saveat=None, t1=1.0, replay=False, min_attempts=0, one_launch=None):
    """One taped forward and its backward on a fresh handle; every array goes to `out`, the step log to `logs`."""
    from tests.util import Node
    node = Node(cfg)
    if replay:
        f = node.forward_replay(x, p, REPLAY_DTP, REPLAY_ACC, keep_tape=True)
    elif saveat is not None:
        f = node.forward_saveat(x, p, saveat, keep_tape=True)
    else:
        f = node.forward(x, p, 0.0, t1, keep_tape=True)
    assert f["nattempts"] >= min_attempts, (name, f["nattempts"])
    if one_launch is not None:
        evidence(out, name, node, f["nattempts"], one_launch)
    rng = np.random.default_rng(77)
    ubar = rng.uniform(0.5, 1.5, f["u"].shape).astype(np.float32)
    svbar = rng.uniform(0.5, 1.5, len(f["saveval"])).astype(np.float32)
    xb, pb, tb = node.backward(ubar, svbar)
    for k in ("u", "steps", "saveval"):
        out[f"{name}/{k}"] = f[k]
    out[f"{name}/x_bar"], out[f"{name}/p_bar"], out[f"{name}/tspan_bar"] = xb, pb, tb
    logs.append((engine, name, f["steps"]))
    node.close()


def evidence(out, name, node, n_att, one_launch):
    """Which solve form the handle's one forward took, by its own counters: asserted, and left as an array beside the results."""
    got = node.L.rnde_node_one_launch_solves(node.h)
    assert got == one_launch, (name, "one-launch solves", got)
    out[f"_path/{name}"] = np.array([got, n_att, node.L.rnde_node_launches_per_attempt(node.h), node.L.rnde_node_fallback_count(node.h)])


def forward(out, logs, engine, name, cfg, x, p, one_launch, min_attempts=0, expect=0):
    """One untaped rnde_node_forward on a fresh handle, its status not checked but recorded (expect: the status the case is there for)."""
    from regneuralde_jl_amd import _lib
    from tests.util import Node
    node = Node(cfg)
    xd, pd = node.dev(x), node.dev(p)
    u = torch.zeros_like(xd)
    nfe, nsv, natt = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    sv = (C.c_float * (cfg.max_attempts + 1))()
    torch.cuda.current_stream().synchronize()
    st = node.L.rnde_node_forward(node.h, xd.data_ptr(), pd.data_ptr(), x.shape[0], 0.0, 1.0, u.data_ptr(), C.byref(nfe), sv, C.byref(nsv), 0, None)
    assert st == expect, (name, st, node.L.rnde_last_error(node.h))
    steps = (C.c_float * (4 * cfg.max_attempts))()
    node.L.rnde_node_steps(node.h, steps, cfg.max_attempts, C.byref(natt))
    assert natt.value >= min_attempts and natt.value == node.L.rnde_node_last_attempts(node.h), (name, natt.value)
    out[f"{name}/steps"] = np.array(steps[:4 * natt.value], dtype=np.float32).reshape(-1, 4)
    out[f"{name}/status"] = np.array([st, natt.value])
    if st == _lib.OK:
        out[f"{name}/u"], out[f"{name}/nfe"], out[f"{name}/saveval"] = u.cpu().numpy(), np.array([nfe.value]), np.array(sv[:nsv.value], dtype=np.float32)
        evidence(out, name, node, natt.value, one_launch)
        logs.append((engine, name, out[f"{name}/steps"]))
    else:      # (the end state of a solve that stopped at max_attempts is not an output)
        assert st == _lib.MAX_ATTEMPTS and natt.value == cfg.max_attempts, (name, st, natt.value)
        out[f"{name}/message"] = np.frombuffer(node.L.rnde_last_error(node.h), dtype=np.uint8).copy()
    node.close()


def everystep(out, logs, engine, name, cfg, x, p, save_start):
    """rnde_node_forward_everystep on a fresh handle: the count, the times, the saved states, the saved values and the (second solve's) step log."""
    from tests.util import Node
    node = Node(cfg)
    B, D = x.shape
    cap = cfg.max_attempts + 1
    xd, pd = node.dev(x), node.dev(p)
    sol = torch.zeros((B * cap * D,), dtype=torch.float32, device="cuda")
    th, n, nfe, nsv, natt = (C.c_float * cap)(), C.c_int32(-1), C.c_int64(0), C.c_int32(0), C.c_int32(0)
    sv = (C.c_float * cap)()
    torch.cuda.current_stream().synchronize()
    st = node.L.rnde_node_forward_everystep(node.h, xd.data_ptr(), pd.data_ptr(), B, 0.0, 1.0, int(save_start), sol.data_ptr(), cap, th, C.byref(n),
                                            C.byref(nfe), sv, C.byref(nsv), 0, None)
    assert st == 0, (name, st, node.L.rnde_last_error(node.h))
    steps = (C.c_float * (4 * cfg.max_attempts))()
    node.L.rnde_node_steps(node.h, steps, cfg.max_attempts, C.byref(natt))
    steps = np.array(steps[:4 * natt.value], dtype=np.float32).reshape(-1, 4)
    assert n.value == int(steps[:, 3].sum()) + int(save_start), (name, n.value)      # one state per accepted step (and the start)
    out[f"{name}/t"], out[f"{name}/n_nfe"] = np.array(th[:n.value], dtype=np.float32), np.array([n.value, nfe.value])
    out[f"{name}/sol"], out[f"{name}/saveval"], out[f"{name}/steps"] = sol[:B * n.value * D].cpu().numpy(), np.array(sv[:nsv.value], dtype=np.float32), steps
    logs.append((engine, name, steps))
    node.close()


def debug_entries(out, name, cfg, x, p):
    """rnde_debug_feval at x, then rnde_debug_attempt from x with that evaluation as k1."""
    from tests.util import Node
    node = Node(cfg)
    k1 = node.feval(x, p, 0.125)
    k, unew, eest = node.attempt(x, k1, p, 0.125, 0.0625)
    out[f"{name}/feval"], out[f"{name}/k"], out[f"{name}/unew"], out[f"{name}/eest"] = k1, k, unew, np.array([eest], dtype=np.float32)
    node.close()


def forward_cases(out, logs):
    from tests.test_gpu_chain import _cfg as ccfg, _setup as csetup
    from tests.test_gpu_forward import _cfg as scfg, _setup as ssetup
    mn = ssetup("mnist", 19, 3, 3.0)
    sm = ssetup("small", 12, 3, 4.0)
    tn = ssetup("test_node", 5, 3, 3.0)
    l4, l70 = csetup("latent", 4, 4, 1.5), csetup("latent", 70, 4, 1.5)
    tol = dict(reltol=1e-3, abstol=1e-3)

    def stage(a, **kw):
        return scfg(a[0], len(a[2]), **kw)

    def chain(a, lay, **kw):
        return ccfg(a[0], len(a[2]), col_tile=lay, **kw)
    # untaped forwards, every solve form
    forward(out, logs, "stage", "fwd/stage/mnist19/one_launch", stage(mn, regularize=3, **tol), mn[2], mn[1], one_launch=1)
    with Env(RNDE_SOLVE_FOLD="0"):
        forward(out, logs, "stage", "fwd/stage/mnist19/one_launch/fold=0", stage(mn, regularize=3, **tol), mn[2], mn[1], one_launch=1)
    with Env(RNDE_STAGE_SOLVE="0"):
        forward(out, logs, "stage", "fwd/stage/mnist19/stage_solve=0", stage(mn, regularize=3, **tol), mn[2], mn[1], one_launch=0)
    with Env(RNDE_PERSIST="0"):
        forward(out, logs, "stage", "fwd/stage/mnist19/persist=0", stage(mn, regularize=3, **tol), mn[2], mn[1], one_launch=0)
        assert out["_path/fwd/stage/mnist19/persist=0"][2] == 7
        forward(out, logs, "stage", "fwd/stage/small12/persist=0/chunks", stage(sm, regularize=2, **TOL_CHUNKS), sm[2], sm[1], one_launch=0, min_attempts=13)
    forward(out, logs, "stage", "fwd/stage/small12", stage(sm, regularize=2, **tol), sm[2], sm[1], one_launch=0)
    forward(out, logs, "chain1", "fwd/chain1/latent4", chain(l4, 64, regularize=2, **tol), l4[2], l4[1], one_launch=0)
    forward(out, logs, "chain1", "fwd/chain1/latent4/chunks", chain(l4, 64, regularize=2, **TOL_CHUNKS), l4[2], l4[1], one_launch=0, min_attempts=13)
    forward(out, logs, "chainmw", "fwd/chainmw/latent70", chain(l70, 65, regularize=2, **tol), l70[2], l70[1], one_launch=1)
    with Env(RNDE_CHAIN_SOLVE="0"):
        forward(out, logs, "chainmw", "fwd/chainmw/latent70/chain_solve=0", chain(l70, 65, regularize=2, **tol), l70[2], l70[1], one_launch=0)
        run(out, logs, "chainmw", "fwd/chainmw/latent70/chain_solve=0/chunks", chain(l70, 65, regularize=2, **TOL_CHUNKS), l70[2], l70[1], min_attempts=13, one_launch=0)
    # a taped one-launch multi-wave solve beyond the attempt limit of a fresh handle: ends at 48, redone with room for max_attempts
    run(out, logs, "chainmw", "fwd/chainmw/latent70/redo", chain(l70, 65, regularize=2, **TOL_REDO), l70[2], l70[1], min_attempts=49, one_launch=1)
    # a solve that ends at max_attempts, each form
    short = dict(max_attempts=4, regularize=1, **tol)
    forward(out, logs, "stage", "fwd/stage/mnist19/max_attempts", stage(mn, **short), mn[2], mn[1], one_launch=0, expect=2)
    with Env(RNDE_PERSIST="0"):
        forward(out, logs, "stage", "fwd/stage/mnist19/persist=0/max_attempts", stage(mn, **short), mn[2], mn[1], one_launch=0, expect=2)
    forward(out, logs, "chain1", "fwd/chain1/latent4/max_attempts", chain(l4, 64, **short), l4[2], l4[1], one_launch=0, expect=2)
    forward(out, logs, "chainmw", "fwd/chainmw/latent70/max_attempts", chain(l70, 65, **short), l70[2], l70[1], one_launch=0, expect=2)
    # save_everystep
    for start in (0, 1):
        everystep(out, logs, "stage", f"every/stage/mnist19/start={start}", stage(mn, regularize=3, **tol), mn[2], mn[1], start)
        everystep(out, logs, "stage", f"every/stage/test_node5/start={start}", stage(tn, regularize=2, **tol), tn[2], tn[1], start)
        everystep(out, logs, "chain1", f"every/chain1/latent4/start={start}", chain(l4, 64, regularize=2, **tol), l4[2], l4[1], start)
        everystep(out, logs, "chainmw", f"every/chainmw/latent4/start={start}", chain(l4, 65, regularize=2, **tol), l4[2], l4[1], start)
    # the kernel-level entries
    debug_entries(out, "debug/stage/mnist19", stage(mn, **tol), mn[2], mn[1])
    debug_entries(out, "debug/stage/small12", stage(sm, **tol), sm[2], sm[1])
    with Env(RNDE_PERSIST="0"):
        debug_entries(out, "debug/stage/small12/persist=0", stage(sm, **tol), sm[2], sm[1])
    debug_entries(out, "debug/chain1/latent4", chain(l4, 64, **tol), l4[2], l4[1])
    debug_entries(out, "debug/chainmw/latent70", chain(l70, 65, **tol), l70[2], l70[1])


def stage_cases(out, logs):
    from tests.golden.make_golden import devorder_inputs
    from tests.test_gpu_forward import _cfg, _setup
    arch, p, x = _setup("mnist", 19, 3, 3.0)
    for x3 in (None, "0"):
        for persist in (None, "0"):
            with Env(RNDE_X3=x3, RNDE_PERSIST=persist):
                tag = f"stage/mnist19/x3={x3}/persist={persist}"
                for reg in range(5):
                    run(out, logs, "stage", f"{tag}/reg{reg}", _cfg(arch, 19, reltol=1e-3, abstol=1e-3, regularize=reg), x, p)
                for reg in (1, 2, 3):
                    run(out, logs, "stage", f"{tag}/reg{reg}/saveat13", _cfg(arch, 19, reltol=1e-3, abstol=1e-3, regularize=reg), x, p, saveat=SAVEAT13)
    arch, p, x, tol = devorder_inputs("mnist_B16_reftol_devorder")
    run(out, logs, "stage", "stage/mnist16_reftol_side", _cfg(arch, 16, reltol=tol, abstol=tol, max_attempts=96), x.astype(np.float32), p.astype(np.float32),
        min_attempts=8)
    arch, p, x = _setup("mnist", 2048, 3, 3.0)
    run(out, logs, "stage", "stage/mnist2048_prereduce", _cfg(arch, 2048, reltol=1e-3, abstol=1e-3, max_attempts=32), x, p)
    for kind, B, scale in (("small", 12, 4.0), ("test_node", 5, 3.0)):
        arch, p, x = _setup(kind, B, 3, scale)
        for act1 in (0, 1):
            cfg = _cfg(arch, B, reltol=1e-3, abstol=1e-3, regularize=2)
            cfg.act[1] = act1
            run(out, logs, "stage", f"stage/{kind}{B}/act1={act1}", cfg, x, p)
            run(out, logs, "stage", f"stage/{kind}{B}/act1={act1}/replay", cfg, x, p, replay=True)
    for kind, B, tol, scale, t1, seed in (("test_node", 3, 1e-2, 10.0, 3.0, 0), ("small", 6, 1e-2, 15.0, 2.0, 12)):      # (rough: they reject)
        arch, p, x = _setup(kind, B, seed, scale)
        run(out, logs, "stage", f"stage/{kind}{B}/rough", _cfg(arch, B, reltol=tol, abstol=tol), x, p, t1=t1)


def chain_cases(out, logs):
    from tests.act_ref import params
    from tests.test_gpu_activations import REPLAY_SHAPES, _cfg as act_cfg
    from tests.test_gpu_chain import _cfg, _setup
    for lay, engine in ((64, "chain1"), (65, "chainmw")):
        for kind, B, scale in (("latent", 4, 1.5), ("latent", 70, 1.5), ("chain3", 19, 2.0), ("small", 12, 4.0)):
            arch, p, x = _setup(kind, B, 4, scale)
            tag = f"{engine}/{kind}{B}"
            for reg in (1, 2, 3, 4):
                run(out, logs, engine, f"{tag}/reg{reg}", _cfg(arch, B, reltol=1e-3, abstol=1e-3, regularize=reg, col_tile=lay), x, p)
            for sname, sa in (("saveat49", SAVEAT49), ("saveat3", SAVEAT3)):
                run(out, logs, engine, f"{tag}/{sname}", _cfg(arch, B, reltol=1e-3, abstol=1e-3, col_tile=lay), x, p, saveat=sa)
            run(out, logs, engine, f"{tag}/replay", _cfg(arch, B, reltol=1e-3, abstol=1e-3, regularize=2, col_tile=lay), x, p, replay=True)
        arch, p, x = _setup("latent", 4, 4, 1.5)
        with Env(RNDE_CHAIN_GENERIC="1"):
            run(out, logs, engine, f"{engine}/latent4/generic", _cfg(arch, 4, reltol=1e-3, abstol=1e-3, regularize=2, col_tile=lay), x, p)
        dims, td, seed = REPLAY_SHAPES["small"]
        rng = np.random.default_rng(seed)
        pa, xa = params(dims, td, rng, bias=0.3), rng.uniform(-1.0, 1.0, (6, dims[0])).astype(np.float32)
        cfg = act_cfg(dims, ["softplus", "softplus"], 6, time_dep=td, regularize=2, max_attempts=16, col_tile=lay)
        run(out, logs, engine, f"{engine}/softplus", cfg, xa, pa, replay=True)
    arch, p, x = _setup("chain3", 19, 4, 2.0)
    run(out, logs, "chainmw", "chainmw/chain3_19/dp5", _cfg(arch, 19, reltol=1e-3, abstol=1e-3, col_tile=65, solver="DP5"), x, p)
    run(out, logs, "chainmw", "chainmw/chain3_19/dp5/saveat3", _cfg(arch, 19, reltol=1e-3, abstol=1e-3, col_tile=65, solver="DP5"), x, p, saveat=SAVEAT3)
    arch, p, x = _setup("latent", 70, 4, 1.5)
    run(out, logs, "chainmw", "chainmw/latent70/dop853", _cfg(arch, 70, reltol=1e-4, abstol=1e-4, col_tile=65, solver="DOP853"), x, p)
    with Env(RNDE_CHAIN_BSWEEP="0"):
        run(out, logs, "chainmw", "chainmw/latent70/bsweep=0", _cfg(arch, 70, reltol=1e-3, abstol=1e-3, regularize=2, col_tile=65), x, p)
        run(out, logs, "chainmw", "chainmw/latent70/bsweep=0/saveat49", _cfg(arch, 70, reltol=1e-3, abstol=1e-3, col_tile=65), x, p, saveat=SAVEAT49)


def child(path):
    out, logs = {}, []
    forward_cases(out, logs)
    stage_cases(out, logs)
    chain_cases(out, logs)
    for i, (engine, name, steps) in enumerate(logs):
        out[f"_log/{i:04d}/{engine}"] = steps
    np.savez(path, **out)
    print(f"{os.environ.get('RNDE_LIB')}: {len(out)} arrays, {len(logs)} step logs", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "regneuralde.jl_amd", "lib", "librnde_parent.so"))
    ap.add_argument("--new", default=os.path.join(ROOT, "regneuralde.jl_amd", "lib", "librnde.so"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--workdir", help="where the two children leave their arrays (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_plan_bits.json"))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not a.workdir:      # (the children's arrays are of no use once compared)
        with tempfile.TemporaryDirectory(prefix="ab_node_bits_") as tmp:
            a.workdir = tmp
            return compare(a)
    os.makedirs(a.workdir, exist_ok=True)
    return compare(a)


def compare(a):
    got = {}
    for side, lib in (("parent", a.parent), ("new", a.new)):      # one after the other, a fresh process each
        path = os.path.join(a.workdir, f"ab_node_bits_{side}.npz")
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
        c = cover.setdefault(k.split("/")[2], dict(logs=0, with_rejection=0, rejected_attempts=0))
        rejected = int((steps[:, 3] == 0).sum()) if len(steps) else 0
        c["logs"] += 1
        c["with_rejection"] += int(rejected > 0)
        c["rejected_attempts"] += rejected
    covered = all(e in cover and cover[e]["with_rejection"] > 0 for e in ("stage", "chain1", "chainmw"))
    res = dict(how="tools/ab_node_bits.py: numpy.array_equal per array, one child process per library", parent=os.path.basename(a.parent),
               new=os.path.basename(a.new), arrays=len(P), differing=differing, rejections_by_parent_step_logs=cover, covered=covered,
               forward_paths_by_parent={k[len("_path/"):]: dict(zip(("one_launch_solves", "n_att", "launches_per_attempt", "fallbacks"), map(int, v)))
                                        for k, v in P.items() if k.startswith("_path/")},
               equal=not differing and covered)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "differing"}), flush=True)
    for k in differing[:40]:
        print("differs:", k)
    if not covered:
        print("NOT REPORTED AS EQUAL: the first library's step logs lack a rejected attempt on some engine")
    return 0 if res["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
