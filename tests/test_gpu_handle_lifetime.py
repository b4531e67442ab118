"""Every handle gives back what it took: the library counts its live device allocations and their bytes (rnde_debug_live_allocs / _bytes,
csrc/rnde_alloc.h), and a handle that is created, run through every buffer it grows on demand -- a taped forward and its backward, saveat
forwards with 3 and then 9 times, a replay, the classifier head and the one-call step where the engine has them -- and destroyed must leave
both counters where they were.  A create that is refused leaves them unchanged too.  Handles and inputs are those of
tests/test_gpu_memory_independence.py.  (A create that runs out of memory half-way is not provoked on a device: the owners that free a
half-built handle are checked by tests/test_alloc_host.py.)"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from tests import test_gpu_memory_independence as M

pytestmark = pytest.mark.gpu

SAVE3 = np.array([0.0, 0.25, 1.0], dtype=np.float32)
SAVE9 = np.linspace(0.0, 1.0, 9).astype(np.float32)


def _lib():
    from regneuralde_jl_amd import _lib
    return _lib


def _live():
    gc.collect()      # (a handle an earlier test dropped goes now, not in the middle of a case)
    L = _lib().lib()
    return int(L.rnde_debug_live_allocs()), int(L.rnde_debug_live_bytes())


class returns_everything:
    """with returns_everything(): create, run, destroy"""

    def __enter__(self):
        self.before = _live()
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            torch.cuda.synchronize()
            assert _live() == self.before, (self.before, _live())
        return False


def _grew(before):
    now = _live()
    assert now[0] > before[0] and now[1] > before[1], (before, now)


def _node_all(node, x, p):
    """every lazily grown buffer of a rnde_node_create handle: tape and reverse buffers, the saveat table twice, a replay"""
    M._chain_run(node, x, p, None)
    M._chain_run(node, x, p, SAVE3)
    M._chain_run(node, x, p, SAVE9)
    node.forward_replay(x, p, [0.25] * 4, [1] * 4, keep_tape=True)
    node.backward(np.ones_like(x))


# ---- the stage engine -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,B,mb", [("small", 33, 48), ("mnist", 13, 16)], ids=["generic", "mnist-x3"])
def test_stage_engine(kind, B, mb):
    """mnist at max_batch 16: D = 784, H = 100, so the matrix-mode-1 images and the one-launch solve's granules exist"""
    from tests.test_gpu_forward import _cfg, _setup
    from tests.util import Node
    arch, p, x = _setup(kind, B, 3, 3.0)
    with returns_everything() as r:
        node = Node(_cfg(arch, mb, reltol=1e-3, abstol=1e-3, col_tile=16, track_ctrl=1, track_initdt=1))
        _grew(r.before)
        _node_all(node, x, p)
        node.close()


def test_stage_engine_head_and_one_call_step():
    """the layer's handles (classifier head scratch, the one-call step's buffers and event) go with the model"""
    import regneuralde_jl_amd as rn
    with returns_everything() as r:
        g = torch.Generator().manual_seed(5)
        dyn = rn.MLPDynamics(36, 10, generator=g)
        node = rn.TrackedNeuralODE(dyn, [0.0, 1.0], True, True, "Tsit5", save_everystep=False, reltol=1e-3, abstol=1e-3, save_start=False,
                                   max_batch=16, max_attempts=64)
        model = rn.ClassifierNODE(node, rn.Dense(36, 10, "identity", generator=g), device=torch.device("cuda", 0))
        x = torch.rand(16, 36, generator=g).cuda()
        y = torch.eye(10)[torch.randint(0, 10, (16,), generator=g)].cuda()
        rn.fused_loss_and_grad(model, x, y, lam=50.0)                    # forward, head, backward
        rn.fused_loss_and_grad(model, x, y, lam=50.0, sync=False)        # rnde_node_classifier_grad
        torch.cuda.synchronize()
        _grew(r.before)
        del model, node, dyn


# ---- the chain engine ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("col_tile,solver", [(64, "Tsit5"), (0, "Tsit5"), (0, "DOP853")], ids=["one-wave", "multi-wave", "multi-wave-dop853"])
def test_chain_engine(col_tile, solver):
    from tests.test_gpu_chain import _setup
    from tests.test_gpu_forward import _cfg
    from tests.util import Node
    B, mb, scale, _ = M.CHAIN_CASES["chain3"]
    arch, p, x = _setup("chain3", B, 3, scale)
    dop = solver == "DOP853"      # (a table pair has no dense output: no saveat; its reverse is the untracked one)
    with returns_everything() as r:
        node = Node(_cfg(arch, mb, reltol=1e-3, abstol=1e-3, col_tile=col_tile, solver=solver, track_ctrl=0 if dop else 1, track_initdt=0 if dop else 1))
        _grew(r.before)
        if dop:
            M._chain_run(node, x, p, None)
        else:
            _node_all(node, x, p)
        node.close()


# ---- the tiled TrackedNeuralODE engine ------------------------------------------------------------------------------------------------------------

def test_tiled_node():
    dims, acts, td, p, x, _, _, mb = M._node_inputs("pad_td")
    with returns_everything() as r:
        node = M._node_make(dims, acts, td, mb)()      # (reserves 129 saveat rows)
        _grew(r.before)
        _lib().check(node.h, node.L.rnde_node_tiled_reserve_saveat(node.h, 16))
        _lib().check(node.h, node.L.rnde_node_tiled_reserve_saveat(node.h, 129))
        for leg in ("tracked", "saveat-tracked", "everystep"):      # (set_tracking(1, 1) in the tracked legs)
            M._node_run(leg, node, x, p)
        node.close()


# ---- TrackedFFJORD: the three engines ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["tiled-cs2", "chain-td2", "onewg-cs2"])
def test_ffjord(case):
    """a Hutchinson solve and its reverse, then one kinetic forward and its reverse: the buffers the kinetic rows need are allocated again"""
    dyn, B, mb, engine0, recipe = M.FF_CASES[case]
    p, x, e, g = M._ff_inputs(dyn, recipe, B, 31)
    with returns_everything() as r:
        hd = M._ff_make(dyn, mb, engine0, "kinetic")()
        _grew(r.before)
        M._ff_run("hutch", hd, p, x, e, g)
        M._ff_run("kinetic", hd, p, x, e, g)
        hd.close()


# ---- the SDE engine ------------------------------------------------------------------------------------------------------------------------------

def test_sde_engine():
    from tests.test_gpu_nsde import AGGR, _cfg, _setup
    from tests.util import NsdeNode
    B, mb = 7, 20
    drift, diff, p, x, noise = _setup("small", B, 13, 400, 2.0, 0.5)
    with returns_everything() as r:
        node = NsdeNode(_cfg(drift, diff, mb, reltol=0.05, abstol=0.05, solver="SOSRI", regularize=1, max_attempts=399, **AGGR))
        _grew(r.before)
        M._sde_run(node, x, p, noise, None)
        M._sde_run(node, x, p, noise, SAVE3[1:] * 0.5)
        M._sde_run(node, x, p, noise, SAVE9[1:-1])
        node.close()
        drift, diff, p, x, _ = _setup("nsde", 48, 3, 1)      # the library's noise stream (tests/test_gpu_nsde.py: its pool grows on demand)
        node = NsdeNode(_cfg(drift, diff, 48, reltol=0.14, abstol=0.14))
        f = node.forward(x, p, None, seed=7, keep_tape=True)
        node.backward(np.ones_like(f["u"]), np.ones(len(f["saveval"]), np.float32))
        node.close()


def test_sde_engine_head_and_one_call_step(monkeypatch):
    import regneuralde_jl_amd as rn
    B = 16
    with returns_everything() as r:
        g = torch.Generator().manual_seed(21)
        nsde = rn.TrackedNeuralDSDE(rn.Chain(rn.Dense(32, 64, "tanh", g), rn.Dense(64, 32, "identity", g)), rn.Dense(32, 32, "identity", g),
                                    [0.0, 1.0], True, "SOSRI", reltol=0.14, abstol=0.14, max_batch=B, seed=5)
        model = rn.ClassifierNSDE(rn.Dense(784, 32, "identity", g), nsde, rn.Dense(32, 10, "identity", g))
        x = torch.rand(B, 784, generator=g).cuda()
        y = torch.eye(10)[torch.randint(0, 10, (B,), generator=g)].cuda()
        for one_call in ("0", "1"):
            monkeypatch.setenv("RNDE_ONE_CALL", one_call)
            rn.fused_nsde_loss_and_grad(model, x, y, lam=10.0)
        torch.cuda.synchronize()
        _grew(r.before)
        del model, nsde


# ---- the latent caller, the communicator -------------------------------------------------------------------------------------------------------------

def test_latent_caller():
    with returns_everything() as r:
        h = M._Latent(37, 49)
        _grew(r.before)
        h.run(16, 7, 3)
        h.close()


def test_communicator_with_a_coupled_chain_handle():
    from tests.test_gpu_chain import _setup
    from tests.test_gpu_forward import _cfg
    from tests.util import Node
    lib = _lib()
    L = lib.lib()
    B = 32
    arch, p, x = _setup("chain3", B, 21, 2.0)
    with returns_everything() as r:
        comms = (C.c_void_p * 1)()
        assert L.rnde_comm_create_local_group(1, 0, comms) == 0, L.rnde_comm_last_error(None)
        node = Node(_cfg(arch, B, reltol=1e-3, abstol=1e-3, col_tile=65)).own_stream()
        lib.check(node.h, L.rnde_node_set_coupling(node.h, C.c_void_p(comms[0]), B))
        _grew(r.before)
        M._chain_run(node, x, p, None)
        node.close()
        L.rnde_comm_destroy(C.c_void_p(comms[0]))


# ---- refused creates -----------------------------------------------------------------------------------------------------------------------------

def test_a_refused_create_takes_nothing():
    """One refusal per create function, each provoked by an existing test; rnde_node_create and rnde_nsde_create also with one that comes
    after the handle exists (the other creates refuse behind `new` only what their argument checks have already turned away)."""
    import regneuralde_jl_amd as rn
    from tests.test_ffjord_chain_host import _cfg as chain_cfg
    from tests.test_ffjord_tiled_host import _cfg as ff_cfg
    from tests.test_gpu_node_tiled import make_cfg as tiled_cfg
    from tests.util import make_cfg, make_nsde_cfg
    lib = _lib()
    L = lib.lib()
    scfg = make_nsde_cfg([3, 5, 3], ["tanh", "identity"], [3, 3], ["identity"], 4)
    scfg.diff_act[0] = 6
    cases = [(L.rnde_node_create, make_cfg([36, 10, 36], ["tanh", "identity"], 16, col_tile=4)),      # (refused behind `new`: the handle exists)
             (L.rnde_node_create, make_cfg([3, 5, 3], ["tanh", "identity"], 4, time_dep=False, pre_act=3)),
             (L.rnde_node_create_tiled, tiled_cfg([3, 7, 3], ["tanh", "identity"], True, 4097)),
             (L.rnde_nsde_create, scfg),
             (L.rnde_nsde_create, make_nsde_cfg([3, 5, 3], ["tanh", "identity"], [3, 3], ["identity"], 16385)),      # (likewise behind `new`: 257 workgroups)
             (L.rnde_ffjord_create, ff_cfg(rn, 43, 100)),
             (L.rnde_ffjord_create_tiled, ff_cfg(rn, 43, 100, max_batch=4097)),
             (L.rnde_ffjord_create_chain, chain_cfg(rn, [2, 3, 2], True, max_batch=4097)),
             (L.rnde_latent_create, lib.LatentConfig(max_batch=8, max_T=70, device=0))]
    for create, cfg in cases:
        with returns_everything():
            h = C.c_void_p()
            assert create(C.byref(cfg), C.byref(h)) == lib.BAD_ARG and not h.value, create.__name__


# ---- the poison fill reaches every allocation but the meeting places' ---------------------------------------------------------------------------------

def _poison_chain(col_tile):
    from tests.test_gpu_chain import _setup
    from tests.test_gpu_forward import _cfg
    from tests.util import Node
    B, mb, scale, _ = M.CHAIN_CASES["chain3"]
    arch, p, x = _setup("chain3", B, 3, scale)
    return (lambda: Node(_cfg(arch, mb, reltol=1e-3, abstol=1e-3, col_tile=col_tile))), x, p


def _poison_stage():
    from tests.test_gpu_forward import _cfg, _setup
    from tests.util import Node
    arch, p, x = _setup("mnist", 13, 3, 3.0)
    return (lambda: Node(_cfg(arch, 16, reltol=1e-3, abstol=1e-3, col_tile=16))), x, p


def _poison_tiled_node():
    dims, acts, td, p, x, _, _, mb = M._node_inputs("pad_td")
    return M._node_make(dims, acts, td, mb), x, p


# what MeetRes holds on the device (csrc/rnde_meet.h): create() makes the granules, the XCC ids and the abort word; create_granules() the first alone
MEET_CREATE, MEET_GRANULES = 3, 1


@pytest.mark.parametrize("setup,meet_allocs", [(lambda: _poison_chain(64), 0), (lambda: _poison_chain(0), MEET_CREATE), (_poison_stage, MEET_GRANULES),
                                               (_poison_tiled_node, MEET_CREATE)], ids=["one-wave", "multi-wave", "stage-mnist-x3", "tiled-node"])
def test_poison_fills_every_allocation_meetres_does_not_own(setup, meet_allocs, monkeypatch):
    """Create and one untaped forward (nothing is released in between, so the growth of the live count is the number of allocations made).
    The one-wave kernels have no meeting place; the multi-wave chain handle and the tiled handle hold a whole MeetRes; the stage engine at
    D = 784, H = 100 holds the granules of its one-launch solve alone."""
    make, x, p = setup()
    monkeypatch.setenv("RNDE_POISON", "1")
    live0, poison0 = _live(), M._counters()
    node = make()
    node.forward(x, p)
    live1, poison1 = _live(), M._counters()
    node.close()
    assert poison1[0] - poison0[0] == live1[0] - live0[0] - meet_allocs > 0, (live0, live1, poison0, poison1)
    assert _live() == live0
