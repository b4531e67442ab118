"""The tracked reverse sweep of the tiled TrackedNeuralODE engine, what needs no GPU: the layer's set_tracking refusals, the constructor's pinned
refusals, the create config, the new exports, and the scalar reverses of csrc/rnde_track_rec.h (the initial-step rule, the PI controller's
attempt record) against finite differences, by a stand-alone program (tests/track_host/track_host_check.cpp) compiled with the address and
undefined-behaviour sanitizers."""
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


def test_set_tracking_refusals_need_no_device():
    import regneuralde_jl_amd as rn
    plain = rn.TrackedNeuralODE(_model(), [0, 1], True, True, max_batch=16)
    with pytest.raises(ValueError, match='set_tracking.*engine="tiled"'):
        plain.set_tracking(True, True)
    with pytest.raises(ValueError, match='set_tracking.*engine="tiled"'):
        rn.TrackedNeuralODE(_model(), [0, 1], True, True, max_batch=16, tiled_tracking=(True, True))
    node = _tiled()
    assert node.tiled_tracking == (False, False)
    with pytest.raises(ValueError, match="track_ctrl=False with track_initdt=True"):
        node.set_tracking(False, True)
    with pytest.raises(ValueError, match="track_ctrl=False with track_initdt=True"):
        _tiled(tiled_tracking=(False, True))
    assert node.tiled_tracking == (False, False)
    for pair in ((True, False), (True, True), (False, False)):      # (no handle exists yet: nothing touches a device)
        node.set_tracking(*pair)
        assert node.tiled_tracking == pair
    assert _tiled(tiled_tracking=(True, True)).tiled_tracking == (True, True)


def test_constructor_refusals_are_still_pinned():
    for kw in (dict(track_ctrl=True), dict(track_initdt=True), dict(track_ctrl=True, track_initdt=True)):
        with pytest.raises(ValueError, match="track_ctrl=False and track_initdt=False"):
            _tiled(**kw)
        with pytest.raises(ValueError, match="track_ctrl=False and track_initdt=False"):
            _tiled(tiled_tracking=(True, True), **kw)


def test_config_is_unchanged_by_set_tracking():
    node = _tiled(reltol=1e-5, abstol=1e-5)
    before = bytes(node._config(0, None))
    node.set_tracking(True, True)
    cfg = node._config(0, None)
    assert bytes(cfg) == before and cfg.track_ctrl == 0 and cfg.track_initdt == 0


def test_new_exports_exist():
    from regneuralde_jl_amd import _lib
    names = ("rnde_node_set_tracking", "rnde_node_tracking", "rnde_node_attempts_ext")
    assert all(n in _lib.EXPORTS for n in names)
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes is not None
    header = open(os.path.join(ROOT, "include", "rnde.h")).read()
    julia = open(os.path.join(ROOT, "bindings", "julia", "RNDE.jl")).read()
    for n in names:
        assert n + "(" in header and ":" + n in julia
    assert "RNDE.set_tracking" in open(os.path.join(ROOT, "bindings", "julia", "patch_neural_ode.jl")).read()
    # without a device: a null handle is refused, not dereferenced
    n32 = C.c_int32(0)
    assert L.rnde_node_set_tracking(None, 1, 1) == _lib.BAD_ARG and L.rnde_node_tracking(None, C.byref(n32), C.byref(n32)) == _lib.BAD_ARG
    assert L.rnde_node_attempts_ext(None, None, 0, C.byref(n32)) == _lib.BAD_ARG


def test_initial_step_and_controller_reverse_against_finite_differences(tmp_path):
    exe = os.path.join(str(tmp_path), "track_host_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "regneuralde.jl_amd", "csrc"), os.path.join(ROOT, "tests", "track_host", "track_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "track host checks passed" in r.stdout
