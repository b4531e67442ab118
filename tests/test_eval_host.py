"""The evaluation passes of the two ODE experiments behind the C ABI (rnde_node_classifier_predict, rnde_latent_decode_mse): what can be
checked without a GPU -- the header declares both entry points and the built library exports them, the ctypes prototypes have the header's
parameter counts and widths, the Julia stub binds them, and the Python front ends (ClassifierNODE.predict, node_accuracy,
latent_total_loss) refuse bad calls before anything touches a device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rnde_node_classifier_predict", "rnde_latent_decode_mse"]


def _header():
    src = open(os.path.join(ROOT, "include", "rnde.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _params(name):
    """the parameter list of `name` as the header declares it"""
    m = re.search(r"\brnde_status\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"include/rnde.h does not declare {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_and_library_exports_both_entry_points(rnde):
    L = rnde._lib.lib()
    for name in NAMES:
        _params(name)
        assert hasattr(L, name), name
        assert name in rnde._lib.EXPORTS
    assert hasattr(rnde, "node_accuracy") and hasattr(rnde, "latent_total_loss") and hasattr(rnde.ClassifierNODE, "predict")


def test_ctypes_prototypes_have_the_headers_parameter_counts_and_widths(rnde):
    import ctypes as C
    L = rnde._lib.lib()
    for name, n in zip(NAMES, (13, 10)):
        params = _params(name)
        assert len(params) == n, (name, params)
        argtypes = getattr(L, name).argtypes
        assert argtypes is not None and len(argtypes) == len(params), name
        for p, a in zip(params, argtypes):      # pointers as pointers, the integers and floats by width
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
                if issubclass(a, C._Pointer):
                    assert p.startswith("int64_t") and a._type_ is C.c_int64, (name, p, a)
            elif p.startswith("int32_t"):
                assert a is C.c_int32, (name, p, a)
            else:
                assert p.startswith("float") and a is C.c_float, (name, p, a)
    words = [p.split()[-1] for p in _params(NAMES[0])]
    assert words[words.index("B"):words.index("B") + 4] == ["B", "n_classes", "t0", "t1"], words
    words = [p.split()[-1] for p in _params(NAMES[1])]
    assert words[words.index("B"):] == ["B", "T", "mse_out_dev", "sum_dev", "count_dev", "stream"], words


def test_julia_stub_binds_both_entry_points_with_matching_argument_counts():
    src = open(os.path.join(ROOT, "bindings", "julia", "RNDE.jl")).read()
    for name in NAMES:
        m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", src)
        assert m, name
        assert len([t for t in m.group(1).split(",") if t.strip()]) == len(_params(name)), name


def _no_device(*a, **k):
    raise AssertionError("a refused call must not reach the device")


def _classifier(rn, n_classes=10, max_batch=8):
    import torch
    g = torch.Generator().manual_seed(3)
    node = rn.TrackedNeuralODE(rn.MLPDynamics(12, 5, generator=g), [0.0, 1.0], True, True, "Tsit5", reltol=1e-3, abstol=1e-3, max_batch=max_batch,
                               max_attempts=32)
    model = rn.ClassifierNODE(node, rn.Dense(12, n_classes, generator=g), device=torch.device("cpu"))
    node._acquire = _no_device
    return model, g


def test_predict_refuses_before_any_device_call(rnde):
    import torch
    rn = rnde
    model, g = _classifier(rn)
    x = torch.rand(4, 12, generator=g)
    y = torch.eye(10)[:4]
    with pytest.raises(ValueError, match="without labels"):
        model.predict(x, correct=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\(B, C\) = \(4, 10\)"):
        model.predict(x, y=torch.eye(10)[:3])                               # wrong batch
    with pytest.raises(ValueError, match=r"\(B, C\) = \(4, 10\)"):
        model.predict(x, y=torch.eye(9)[:4])                                # wrong class count
    with pytest.raises(TypeError, match="one-element int64"):
        model.predict(x, y=y, correct=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError, match="one-element int64"):
        model.predict(x, y=y, correct=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError, match="float32"):
        model.predict(x.double(), y=y)
    with pytest.raises(TypeError, match="float32"):
        model.predict(x, y=y.double())
    with pytest.raises(ValueError, match="max_batch = 8"):
        model.predict(torch.rand(9, 12, generator=g))
    with pytest.raises(ValueError, match="features per input"):
        model.predict(torch.rand(4, 11, generator=g))
    with pytest.raises(ValueError, match="tspan must increase"):
        model.predict(x, tspan=[1.0, 1.0])
    for c in (1, 17):
        other, _ = _classifier(rn, n_classes=c)
        with pytest.raises(ValueError, match="2 .. 16 classes"):
            other.predict(x)
    with pytest.raises(ValueError, match="same device"):
        model.predict(x, y=y.to("meta"))
    with pytest.raises(RuntimeError, match="cuda tensor"):
        model.predict(x, y=y)                                               # everything right but the device: still no device call
    with pytest.raises(RuntimeError, match="cuda tensor"):
        rn.node_accuracy(model, [(x, y)])
    assert rn.node_accuracy(model, []) == 0.0                               # (as classifier.accuracy on no batches)


def _latent(rn, T=5):
    import torch
    g = torch.Generator().manual_seed(5)
    saveat = [i / (T - 1) for i in range(T)]
    model = rn.build_latent_ode(saveat=saveat, generator=g, device="cpu", reltol=1e-3, abstol=1e-3, max_batch=8, max_attempts=64)
    model.node._acquire = _no_device
    return model, g


def test_latent_total_loss_refuses_before_any_device_call(rnde, monkeypatch):
    import math
    import torch
    rn = rnde
    from regneuralde_jl_amd import timeseries
    monkeypatch.setattr(timeseries, "_LatentHandle", _no_device)
    model, g = _latent(rn)
    B, T = 3, 5
    d, m, t = torch.rand(B, T, 37, generator=g), torch.ones(B, T, 37), torch.zeros(B, T, 1)
    with pytest.raises(ValueError, match="no t_row"):
        rn.latent_total_loss(model, [(d, m)])
    with pytest.raises(ValueError, match="must be \\(data, mask\\)"):
        rn.latent_total_loss(model, [(d,)])
    with pytest.raises(ValueError, match="must both be"):
        rn.latent_total_loss(model, [(d, m[:, :4], t)])
    with pytest.raises(ValueError, match="reference's latent-ODE sizes"):
        rn.latent_total_loss(model, [(d[:, :, :36], m[:, :, :36], t)])
    with pytest.raises(ValueError, match="does not expand"):
        rn.latent_total_loss(model, [(d, m)], t_row=torch.zeros(B, T + 1, 1))
    with pytest.raises(ValueError, match="one save time per observation time"):
        rn.latent_total_loss(model, [(d[:, :4], m[:, :4], t[:, :4])])
    with pytest.raises(ValueError, match="max_batch = 8"):
        rn.latent_total_loss(model, [(torch.rand(9, T, 37, generator=g), torch.ones(9, T, 37))], t_row=torch.zeros(1, T, 1))
    with pytest.raises(ValueError, match=r"eps must be \(B, 20\) = \(3, 20\)"):
        rn.latent_total_loss(model, [(d, m, t)], eps=[torch.zeros(B, 19)])
    with pytest.raises(ValueError, match=r"eps must be \(B, 20\)"):
        rn.latent_total_loss(model, [(d, m, t)], eps=lambda i: torch.zeros(B + 1, 20))
    with pytest.raises(TypeError, match="eps must be None, a list"):
        rn.latent_total_loss(model, [(d, m, t)], eps=torch.zeros(B, 20))
    with pytest.raises(TypeError, match="float32"):
        rn.latent_total_loss(model, [(d.double(), m.double(), t.double())])
    with pytest.raises(TypeError, match="float32"):
        rn.latent_total_loss(model, [(d, m, t)], eps=[torch.zeros(B, 20, dtype=torch.float64)])
    with pytest.raises(RuntimeError, match="cuda tensors"):
        rn.latent_total_loss(model, [(d, m, t)], eps=[torch.zeros(B, 20)])      # everything right but the device
    assert math.isnan(rn.latent_total_loss(model, []))                          # (0 / 0 in the reference)
