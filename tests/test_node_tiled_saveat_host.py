"""Saved points on the tiled TrackedNeuralODE engine, what needs no GPU: the layer's tiled_max_saveat keyword (acceptances, refusals, the create
config untouched), the new exports, and the host side of the feature by a stand-alone program (tests/save_host/save_plan_check.cpp) compiled
with the address and undefined-behaviour sanitizers: csrc/rnde_rev_plan.h (the save plan on written-down attempt logs, the chain engines' evaluation
times, the saved-value cotangent gather; the eigen_est cotangent coefficients are checked beside the callback's value, tests/test_fwd_plan_host.py) and the Tsit5 dense-output
weights against the tableau and central differences."""
import ctypes as C
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(3)
    return rn.TDChain(rn.Dense(3, 96, "tanh", g), rn.Dense(97, 2, "identity", g))


def _tiled(**kw):
    import regneuralde_jl_amd as rn
    kw.setdefault("track_ctrl", False)
    kw.setdefault("track_initdt", False)
    return rn.TrackedNeuralODE(_model(), [0, 1], True, True, engine="tiled", max_batch=16, **kw)


def test_keyword_switches_saveat_and_everystep_on():
    node = _tiled(tiled_max_saveat=8, saveat=[0.0, 0.5, 1.0])
    assert node.tiled_max_saveat == 8 and node.return_multiple and not node.save_everystep
    node = _tiled(tiled_max_saveat=8, save_everystep=True)
    assert node.return_multiple and node.save_everystep
    node = _tiled(tiled_max_saveat=1)      # a capacity alone changes nothing about the calls
    assert not node.return_multiple
    assert _tiled().tiled_max_saveat is None


def test_without_the_keyword_the_refusals_are_todays():
    with pytest.raises(ValueError, match="saveat= and save_everystep=True are not served"):
        _tiled(saveat=[0.5, 1.0])
    with pytest.raises(ValueError, match="saveat= and save_everystep=True are not served"):
        _tiled(save_everystep=True)
    with pytest.raises(ValueError, match="saveat= and save_everystep=True are not served"):
        _tiled(saveat=[0.5, 1.0], tiled_max_saveat=None)


def test_keyword_refusals():
    import regneuralde_jl_amd as rn
    with pytest.raises(ValueError, match='tiled_max_saveat.*engine="tiled"'):
        rn.TrackedNeuralODE(_model(), [0, 1], True, True, max_batch=16, tiled_max_saveat=8)
    with pytest.raises(ValueError, match='tiled_max_saveat.*engine="tiled"'):
        rn.TrackedNeuralODE(_model(), [0, 1], True, True, max_batch=16, tiled_max_saveat=8, saveat=[0.5, 1.0])
    for bad in (0, -1, 2.5, "8", True):
        with pytest.raises(ValueError, match="tiled_max_saveat must be an integer >= 1"):
            _tiled(tiled_max_saveat=bad)
    with pytest.raises(ValueError, match="above max_attempts"):
        _tiled(tiled_max_saveat=130, max_attempts=128)
    _tiled(tiled_max_saveat=129, max_attempts=128)
    # the other refusals of the engine are untouched by the keyword
    with pytest.raises(ValueError, match="track_ctrl=False and track_initdt=False"):
        _tiled(tiled_max_saveat=8, track_ctrl=True)


def test_more_save_times_than_the_capacity_raise_before_any_launch():
    node = _tiled(tiled_max_saveat=2, saveat=[0.5, 1.0])
    x = torch.zeros(4, 2)      # (a CPU tensor: the count is checked first; had the call gone on it would raise RuntimeError for the device)
    with pytest.raises(ValueError, match="3 save times are above the layer's tiled_max_saveat = 2"):
        node(x.cuda() if torch.cuda.is_available() else _FakeCuda(x), saveat=[0.25, 0.5, 1.0])
    with pytest.raises(ValueError, match="3 save times"):
        bad = _tiled(tiled_max_saveat=2, saveat=[0.25, 0.5, 1.0])
        bad(x.cuda() if torch.cuda.is_available() else _FakeCuda(x))
    assert not node._handles      # no handle was created: nothing reached the library


class _FakeCuda:
    """What TrackedNeuralODE.__call__ reads of x before it forms the save times (no device here)."""

    def __init__(self, x):
        self._x = x
        self.is_cuda, self.device, self.dtype, self.shape, self.requires_grad = True, x.device, x.dtype, x.shape, False

    def reshape(self, *a):
        return _FakeCuda(self._x.reshape(*a))

    def contiguous(self):
        return self


def test_config_is_unchanged_by_the_keyword():
    a = _tiled(reltol=1e-5, abstol=1e-5)
    b = _tiled(reltol=1e-5, abstol=1e-5, tiled_max_saveat=49, saveat=[0.5, 1.0])
    assert bytes(a._config(0, None)) == bytes(b._config(0, None))


def test_new_exports_exist():
    from regneuralde_jl_amd import _lib
    names = ("rnde_node_tiled_reserve_saveat", "rnde_node_tiled_saveat_capacity")
    assert all(n in _lib.EXPORTS for n in names)
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes is not None
    header = open(os.path.join(ROOT, "include", "rnde.h")).read()
    julia = open(os.path.join(ROOT, "bindings", "julia", "RNDE.jl")).read()
    for n in names:
        assert n + "(" in header and ":" + n in julia
    # without a device: a null handle is refused, not dereferenced
    assert L.rnde_node_tiled_reserve_saveat(None, 4) == _lib.BAD_ARG and L.rnde_node_tiled_saveat_capacity(None) == -1
    # the parity instrument that lets a saving solve run along a given sequence
    assert "rnde_debug_arm_replay" in _lib.EXPORTS and "rnde_debug_arm_replay(" in header and L.rnde_debug_arm_replay(None, None, 0) == _lib.BAD_ARG


def test_save_plan_and_dense_weights_by_a_sanitized_host_program(tmp_path):
    exe = os.path.join(str(tmp_path), "save_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "regneuralde.jl_amd", "csrc"), os.path.join(ROOT, "tests", "save_host", "save_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "save host checks passed" in r.stdout
