"""TrackedNeuralODE(engine="tiled") without a device: what the Python layer refuses, the LDS mirror of rnde_node_tiled_lds_bytes as written-down
numbers, and that the default engine's config did not move.  Constructing a layer touches neither the library nor a GPU."""
import pytest
import torch

import regneuralde_jl_amd as rn
from regneuralde_jl_amd import _lib
from regneuralde_jl_amd.node import TILED_LDS_BYTES, check_tiled_served, tiled_lds_bytes


def _chain(dims, acts, td, seed=0):
    g = torch.Generator().manual_seed(seed)
    layers = [rn.Dense(dims[l] + (1 if td else 0), dims[l + 1], acts[l], g) for l in range(len(acts))]
    return rn.TDChain(*layers) if td else rn.Chain(*layers)


def _tiled(dims=(2, 128, 128, 2), acts=("tanh", "tanh", "identity"), td=True, regularize=True, solver="Tsit5", **kw):
    kw.setdefault("track_ctrl", False)
    kw.setdefault("track_initdt", False)
    return rn.TrackedNeuralODE(_chain(list(dims), list(acts), td), [0.0, 1.0], td, regularize, solver, engine="tiled", **kw)


# ---- the LDS mirror ------------------------------------------------------------------------------------------------------------------
# floats = align4(sum_l in_p (out_p + 1) + 2 out_p) + D_p 16 + sum_l out_p 16 + 2 M_p 16 + 128, worked out by hand for each shape
LDS = {
    (3, 7, 3): 4 * ((2 * 16 * 17 + 4 * 16) + 256 + 512 + 512 + 128),                                            # 8064
    (6, 80, 72, 6): 4 * ((16 * 81 + 80 * 81 + 80 * 17 + 2 * (80 + 80 + 16)) + 256 + 176 * 16 + 2 * 80 * 16 + 128),
    (70, 96, 70): 4 * ((80 * 97 + 96 * 81 + 2 * (96 + 80)) + 80 * 16 + 176 * 16 + 2 * 96 * 16 + 128),
    (5, 20, 9, 20, 9, 20, 9, 20, 5): 4 * ((16 * 33 + 3 * (32 * 17 + 16 * 33) + 32 * 17 + 2 * (4 * 32 + 4 * 16)) + 256 + (4 * 32 + 4 * 16) * 16 + 2 * 32 * 16 + 128),
    (2, 128, 128, 2): 120512,
    (64, 192, 64): 146944,
    (64, 256, 64): 192768,
}


@pytest.mark.parametrize("dims", sorted(LDS))
def test_lds_mirror_values(dims):
    assert tiled_lds_bytes(list(dims)) == LDS[dims]


def test_lds_values_are_the_issues_table():
    assert LDS[(3, 7, 3)] == 8064
    assert round(LDS[(2, 128, 128, 2)] / 1000) == 121 and LDS[(2, 128, 128, 2)] // 1024 == 117      # "120 KB" in the issue's table
    assert round(LDS[(64, 192, 64)] / 1000) == 147 and round(LDS[(64, 256, 64)] / 1000) == 193


def test_served_and_refused_widths():
    assert tiled_lds_bytes([2, 128, 128, 2]) <= TILED_LDS_BYTES and tiled_lds_bytes([64, 192, 64]) <= TILED_LDS_BYTES
    _tiled()
    _tiled((64, 192, 64), ("tanh", "identity"), False)
    with pytest.raises(ValueError, match="192768 bytes of LDS"):
        _tiled((64, 256, 64), ("tanh", "identity"), False)


def test_state_rows_above_64_are_served():
    _tiled((70, 96, 70), ("tanh", "tanh"), True)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_track_flags_must_be_passed_as_false():
    m = _chain([3, 7, 3], ["tanh", "identity"], True)
    for kw in ({}, {"track_ctrl": False}, {"track_initdt": False}, {"track_ctrl": True, "track_initdt": False}):
        with pytest.raises(ValueError) as e:
            rn.TrackedNeuralODE(m, [0.0, 1.0], True, True, engine="tiled", **kw)
        assert "track_ctrl" in str(e.value) and "track_initdt" in str(e.value)
    rn.TrackedNeuralODE(m, [0.0, 1.0], True, True, engine="tiled", track_ctrl=False, track_initdt=False)
    # the constructor's defaults stay True
    d = rn.TrackedNeuralODE(m, [0.0, 1.0], True, True)
    assert d.track_ctrl is True and d.track_initdt is True and d.engine is None


def test_unknown_engine_is_refused():
    with pytest.raises(ValueError, match="engine must be one of"):
        rn.TrackedNeuralODE(_chain([3, 7, 3], ["tanh", "identity"], True), [0.0, 1.0], True, True, engine="wide")


@pytest.mark.parametrize("solver", ["AutoTsit5", "DP5", "DOP853"])
def test_other_solvers_are_refused(solver):
    with pytest.raises(ValueError, match="Tsit5"):
        _tiled(solver=solver)


def test_saveat_and_everystep_are_refused():
    with pytest.raises(ValueError, match="saveat"):
        _tiled(saveat=[0.5, 1.0])
    with pytest.raises(ValueError, match="save_everystep"):
        _tiled(save_everystep=True)
    _tiled(save_everystep=False)


def test_stiffness_callback_is_refused():
    node = _tiled()
    assert node.resolve_func(None) is None      # (the default callback: EEst * dt)
    assert node.resolve_func("error_est") == "error_est"
    with pytest.raises(ValueError):
        node.resolve_func("stiff_est")


def test_set_coupling_is_refused():
    with pytest.raises(ValueError, match="set_coupling"):
        _tiled().set_coupling(None, 0)


def test_fused_loss_and_grad_is_refused():
    class M:
        pass
    m = M()
    m.node = _tiled()
    with pytest.raises(ValueError, match="fused_loss_and_grad"):
        rn.fused_loss_and_grad(m, torch.zeros(2, 2), torch.zeros(2, 10))


def test_limits_of_batch_and_attempts():
    with pytest.raises(ValueError, match="4096"):
        _tiled(max_batch=4097)
    with pytest.raises(ValueError, match="8000"):
        _tiled(max_attempts=8001)
    _tiled(max_batch=4096, max_attempts=8000)


def test_check_is_the_constructors():
    node = _tiled()
    check_tiled_served(node)
    node.track_ctrl = True
    with pytest.raises(ValueError):
        check_tiled_served(node)


# ---- the default engine is as it was ---------------------------------------------------------------------------------------------------

def _fields(cfg):
    out = {}
    for name, _ in _lib.NodeConfig._fields_:
        v = getattr(cfg, name)
        out[name] = list(v) if hasattr(v, "__len__") else v
    return out


def test_default_engine_config_is_unchanged():
    """_config() field by field, on one stage-engine model and one chain-engine model: the values written down are what the parent commit builds."""
    stage = rn.TrackedNeuralODE(_chain([784, 100, 784], ["tanh", "tanh"], True), [0.0, 1.0], True, True, "Tsit5", reltol=1.4e-8, abstol=1.4e-8)
    f = _fields(stage._config(0, "error_est"))
    assert f == dict(n_layers=2, dims=[784, 100, 784, 0, 0, 0, 0, 0, 0], act=[1, 1, 0, 0, 0, 0, 0, 0], time_dep=1, pre_act=0, max_batch=512,
                     solver=0, reltol=pytest.approx(1.4e-8), abstol=pytest.approx(1.4e-8), regularize=1, cb_save_start=1, track_ctrl=1,
                     track_initdt=1, max_attempts=128, device=0, col_tile=0, persist=0, wgrad_side_pct=0, stage_generic=0)
    chain = rn.TrackedNeuralODE(_chain([5, 12, 9, 5], ["relu", "tanh", "identity"], False), [0.0, 1.0], False, False, "DP5", max_batch=24,
                                max_attempts=64, track_ctrl=False)
    f = _fields(chain._config(1, None))
    assert f == dict(n_layers=3, dims=[5, 12, 9, 5, 0, 0, 0, 0, 0], act=[2, 1, 0, 0, 0, 0, 0, 0], time_dep=0, pre_act=0, max_batch=24, solver=1,
                     reltol=pytest.approx(1e-3), abstol=pytest.approx(1e-6), regularize=0, cb_save_start=1, track_ctrl=0, track_initdt=1,
                     max_attempts=64, device=1, col_tile=0, persist=0, wgrad_side_pct=0, stage_generic=0)
    # and a tiled layer's config differs in the two track flags only
    t = _fields(_tiled((5, 12, 9, 5), ("relu", "tanh", "identity"), False, regularize=False, max_batch=24, max_attempts=64)._config(1, None))
    f.update(solver=0, track_initdt=0)
    assert t == f
