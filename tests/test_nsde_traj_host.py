"""ClassifierNSDE with several trajectories per input behind the C ABI (rnde_nsde_classifier_head_traj / _grad_traj / _predict): what can be
checked without a GPU -- the header declares the three entry points and the built library exports them, the ctypes prototypes have the
header's parameter counts, the Julia stub binds them, and the Python front end refuses bad calls before anything touches a device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rnde_nsde_classifier_head_traj", "rnde_nsde_classifier_grad_traj", "rnde_nsde_classifier_predict"]


def _header():
    src = open(os.path.join(ROOT, "include", "rnde.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _params(name):
    """the parameter list of `name` as the header declares it"""
    m = re.search(r"\brnde_status\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"include/rnde.h does not declare {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_three_entry_points(rnde):
    L = rnde._lib.lib()
    for name in NAMES:
        _params(name)
        assert hasattr(L, name), name
        assert name in rnde._lib.EXPORTS
    assert "stays on the host side" not in open(os.path.join(ROOT, "include", "rnde.h")).read()


def test_ctypes_prototypes_have_the_headers_parameter_counts(rnde):
    import ctypes as C
    L = rnde._lib.lib()
    for name, n in zip(NAMES, (12, 22, 18)):
        params = _params(name)
        assert len(params) == n, (name, params)
        argtypes = getattr(L, name).argtypes
        assert argtypes is not None and len(argtypes) == len(params), name
        for p, a in zip(params, argtypes):      # pointers as pointers, the integers and floats by width
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            elif p.startswith("int32_t"):
                assert a is C.c_int32, (name, p, a)
            elif p.startswith("uint64_t"):
                assert a is C.c_uint64, (name, p, a)
            else:
                assert p.startswith("float") and a is C.c_float, (name, p, a)
    # B, T, n_classes in that order in all three
    for name in NAMES:
        words = [p.split()[-1] for p in _params(name)]
        i = words.index("B")
        assert words[i:i + 3] == ["B", "T", "n_classes"], (name, words)


def test_julia_stub_binds_the_three_entry_points_with_matching_argument_counts():
    src = open(os.path.join(ROOT, "bindings", "julia", "RNDE.jl")).read()
    for name in NAMES:
        m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", src)
        assert m, name
        assert len([t for t in m.group(1).split(",") if t.strip()]) == len(_params(name)), name


def _model(rn, n_classes=10, max_batch=64):
    import torch
    g = torch.Generator().manual_seed(3)
    nsde = rn.TrackedNeuralDSDE(rn.Chain(rn.Dense(8, 16, "tanh", g), rn.Dense(16, 8, "identity", g)), rn.Dense(8, 8, "identity", g), [0.0, 1.0], False,
                                "SOSRI", reltol=0.14, abstol=0.14, max_batch=max_batch)
    model = rn.ClassifierNSDE(rn.Dense(12, 8, "identity", g), nsde, rn.Dense(8, n_classes, "identity", g), device=torch.device("cpu"))

    def no_device(*a, **k):
        raise AssertionError("a refused call must not reach the device")
    nsde._acquire = no_device
    return model, g


def test_predict_refuses_before_any_device_call(rnde):
    import torch
    rn = rnde
    model, g = _model(rn)
    x = torch.rand(4, 12, generator=g)
    with pytest.raises(RuntimeError, match="cuda tensor"):
        model.predict(x, trajectories=2)                                    # a host tensor
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="trajectories"):
            model.predict(x, trajectories=bad)
    with pytest.raises(ValueError, match="max_batch = 64"):
        model.predict(x, trajectories=17)                                   # 4 * 17 = 68 > 64
    many, _ = _model(rn, n_classes=17)
    with pytest.raises(ValueError, match="2 .. 16 classes"):
        many.predict(x, trajectories=2)
    with pytest.raises(ValueError, match="without labels"):
        model.predict(x, trajectories=2, correct=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="cuda tensor"):
        rn.nsde_accuracy(model, [(x, torch.eye(10)[:4])], trajectories=2)
    assert rn.nsde_accuracy(model, [], trajectories=2) == 0.0               # (as classifier.accuracy on no batches)
