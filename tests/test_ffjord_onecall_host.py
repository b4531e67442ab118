"""The one-call FFJORD training step without a GPU: the two C-ABI entries (declared, exported, listed, NULL handle refused), the Julia
sources' ccalls, and the package wrapper's refusals, raised before any device call."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rnde_ffjord_nll_grad", "rnde_adam_wd_step"]


def test_header_declares_and_the_library_exports_both_entries(rnde):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnde.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rnde_[a-z_]+)\s*\(", src))
    L = rnde._lib.lib()
    for name in NEW:
        assert name in declared and hasattr(L, name) and name in rnde._lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    assert len(L.rnde_ffjord_nll_grad.argtypes) == 19 and len(L.rnde_adam_wd_step.argtypes) == len(L.rnde_adam_step.argtypes) + 1
    f, n = (C.c_float * 4)(), C.c_int64()
    assert L.rnde_ffjord_nll_grad(None, None, None, None, 1, 0.0, 1.0, 0, 0, 0.0, 0.0, 0.0, None, None, None, None, f, C.byref(n), None) == rnde._lib.BAD_ARG
    assert L.rnde_adam_wd_step(None, None, None, None, 4, 1, 1e-2, 0.9, 0.999, 1e-8, 1.0, 1e-5, None) == rnde._lib.BAD_ARG


def test_the_header_states_the_seed_formulas():
    """The tests on the device rebuild the seeds from these lines."""
    hdr = open(os.path.join(ROOT, "include", "rnde.h")).read()
    own = open(os.path.join(ROOT, "regneuralde.jl_amd", "csrc", "rnde_ffjord_loss.h")).read()
    for text in (hdr, own):
        for line in ("logpx_bar[b] = -1.0f / (float)B", "reg_bar[0][b] = lambda_k / (float)B", "reg_bar[1][b] = lambda_j / (float)B",
                     "saveval_bar[i] = lambda_r / (float)n", "(float)((double)lambda_r * sum(saveval) / n)"):
            assert line in text, line


def test_julia_sources_call_both_entries():
    d = os.path.join(ROOT, "bindings", "julia")
    src = open(os.path.join(d, "RNDE.jl")).read()
    called = set(re.findall(r"ccall\(\(:(\w+), LIB\)", src))
    assert set(NEW) <= called
    assert re.search(r"^function ffjord_nll_grad\(", src, flags=re.M) and re.search(r"^function adam_wd_step!\(", src, flags=re.M)
    patch = open(os.path.join(d, "patch_ffjord.jl")).read()
    assert "RNDE.ffjord_nll_grad(" in patch and "RNDE.adam_wd_step!(" in patch and "update_parameters!(ps, gs, opt)" in patch


def _bare_layer(rnde, regularize, engine):
    """A TrackedFFJORD with the fields the wrapper reads ahead of its first device call (the constructor moves the parameters to the device)."""
    ff = rnde.ffjord
    layer = object.__new__(ff.TrackedFFJORD)
    layer.model, layer.regularize, layer.engine, layer.chain, layer.in_dims = ff.MLPDynamics(2, 16), regularize, engine, False, 2
    return layer


def test_wrapper_refusals_come_before_any_device_call(rnde):
    fused = rnde.fused_ffjord_loss_and_grad
    assert fused is rnde.ffjord.fused_ffjord_loss_and_grad
    assert list(inspect.signature(fused).parameters) == ["ff", "x", "p", "e", "lam_r", "kinetic", "exact", "need_x_grad"]
    assert inspect.signature(rnde.FluxADAM.__init__).parameters["one_launch"].default is False
    x = torch.zeros(4, 2)                                               # (a host tensor: a device call would raise RuntimeError instead)
    with pytest.raises(ValueError, match=r"kinetic=\(lam_k, lam_j\).*regularize=True layer"):
        fused(_bare_layer(rnde, True, "tiled"), x, kinetic=(0.01, 0.05))
    with pytest.raises(ValueError, match='exact=True is served on engine="tiled" only'):
        fused(_bare_layer(rnde, False, "workgroup"), x, exact=True)
    with pytest.raises(ValueError, match="exact=True.*takes no probe"):
        fused(_bare_layer(rnde, False, "tiled"), x, e=torch.zeros(4, 2), exact=True)
    with pytest.raises(ValueError, match="lam_r.*regularize=False layer"):
        fused(_bare_layer(rnde, False, "tiled"), x, lam_r=1.0e2)


def test_training_tools_take_the_switch():
    for tool in ("train_ffjord_gaussian.py", "train_ffjord_tabular.py"):
        src = open(os.path.join(ROOT, "tools", tool)).read()
        assert '"--one-call"' in src and "fused_ffjord_loss_and_grad" in src and "one_launch" in src, tool
