"""TrackedFFJORD's exact-trace mode without a GPU: the fp64 restatements' exact trace (D unit probes) against
torch.autograd.functional.jacobian, the package's three refusals (raised before any device call), the two C-ABI entries (declared, exported,
listed, NULL handle refused) and loglikelihood's keyword."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from tests import ffjord_chain_ref as CR
from tests import ffjord_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rnde_ffjord_forward_exact", "rnde_ffjord_forward_exact_replay"]


def test_chain_restatement_exact_trace_is_the_jacobian_trace():
    """TD [5, 12, 9, 5] softplus, sigmoid, tanh: the trace row of rhs(..., e=None) is -tr J with J from autograd, per column, to 1e-12."""
    dims, acts, td, B = [5, 12, 9, 5], ["softplus", "sigmoid", "tanh"], True, 4
    p, x, _, _ = CR.draw(dims, td, B, 11, 1.0)
    p, x = p.double(), x.double()
    from tests import act_ref as A
    for t in (0.0, 0.71):
        got = CR.rhs(dims, acts, td, p, CR.aug(x), t).detach()
        assert got.shape == (B, dims[0] + 1)
        for b in range(B):
            fn = lambda z: A.chain64(dims, acts, td, 0, p, z[None], t)[0]
            J = torch.autograd.functional.jacobian(fn, x[b])
            assert abs(float(got[b, dims[0]]) + float(torch.trace(J))) <= 1e-12
            assert float((got[b, :dims[0]] - fn(x[b])).abs().max()) <= 1e-12


def test_concatsquash_restatement_exact_trace_is_the_jacobian_trace():
    """ConcatSquash (3, 5): the same, for tests/ffjord_ref.rhs(..., e=None)."""
    D, H, B = 3, 5, 4
    rng = __import__("numpy").random.default_rng(11)
    p = torch.from_numpy(R.glorot_params(D, H, rng, 1.0)).double()
    x = torch.from_numpy(rng.standard_normal((B, D))).double()
    for t in (0.0, 0.71):
        got = R.rhs(p, D, H, CR.aug(x), t)
        for b in range(B):
            fn = lambda z: R.mlp(p, D, H, z[None], t)[0][0]
            J = torch.autograd.functional.jacobian(fn, x[b])
            assert abs(float(got[b, D]) + float(torch.trace(J))) <= 1e-12


def _bare_layer(rnde, regularize, engine):
    """A TrackedFFJORD with the fields __call__ reads ahead of its first device call (the constructor moves the parameters to the device)."""
    ff = rnde.ffjord
    layer = object.__new__(ff.TrackedFFJORD)
    layer.model, layer.regularize, layer.engine, layer.chain, layer.in_dims = ff.MLPDynamics(2, 16), regularize, engine, False, 2
    return layer


def test_package_refusals_come_before_any_device_call(rnde):
    ff = rnde.ffjord
    assert "exact" in inspect.signature(ff.TrackedFFJORD.__call__).parameters
    assert "exact" in inspect.signature(ff.loglikelihood).parameters
    x = torch.zeros(4, 2)                                               # (a host tensor: a device call would raise RuntimeError instead)
    with pytest.raises(ValueError, match="exact=True.*no probe"):
        _bare_layer(rnde, False, "tiled")(x, e=torch.zeros(4, 2), exact=True)
    with pytest.raises(ValueError, match="exact=True together with regularize=True"):
        _bare_layer(rnde, False, "tiled")(x, regularize=True, exact=True)
    with pytest.raises(ValueError, match='exact=True is served on engine="tiled" only'):
        _bare_layer(rnde, False, "workgroup")(x, exact=True)
    with pytest.raises(ValueError, match='engine="tiled" only'):        # ({true} layers ignore the regularize keyword, as the plain call does)
        _bare_layer(rnde, True, "workgroup")(x, regularize=True, exact=True)


def test_abi_declares_exports_and_guards_the_exact_entries(rnde):
    """Declared, exported and listed; a NULL handle is BAD_ARG (the engine-0 refusal needs a handle, hence a device: tests/test_gpu_ffjord_exact.py)."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnde.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rnde_[a-z_]+)\s*\(", src))
    L = rnde._lib.lib()
    for name in NEW:
        assert name in declared and hasattr(L, name) and name in rnde._lib.EXPORTS, name
    f = (C.c_float * 8)()
    BAD = rnde._lib.BAD_ARG
    assert L.rnde_ffjord_forward_exact(None, None, None, 1, 0.0, 1.0, None, None, None, None, None, 0, None) == BAD
    assert L.rnde_ffjord_forward_exact_replay(None, None, None, 1, 0.0, 1.0, f, 1, None, None, None, None, None, 0, None) == BAD
    assert L.rnde_ffjord_forward_exact_replay(None, None, None, 1, 0.0, 1.0, None, 0, None, None, None, None, None, 0, None) == BAD
    jl = open(os.path.join(ROOT, "bindings", "julia", "RNDE.jl")).read()
    for name in NEW:
        assert re.search(r"ccall\(\(:" + name + r", LIB\)", jl), name
