"""TrackedFFJORD{false} with regularize = true, without a GPU: the fp64 restatement of the kinetic right-hand side against
torch.autograd.functional.jacobian, the five C-ABI entries (declared, exported, listed, NULL handle refused), and the limits."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import ffjord_kinetic_ref as K
from tests import ffjord_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rnde_ffjord_forward_kinetic", "rnde_ffjord_forward_kinetic_replay", "rnde_ffjord_backward_kinetic", "rnde_ffjord_debug_feval_kinetic",
       "rnde_ffjord_step_log"]


def test_restatement_rows_are_the_kinetic_energy_and_the_jacobian_norm():
    """lambda1's rate is |f|^2 and lambda2's is |e' J|^2 with J from torch.autograd.functional.jacobian, per column; f and the trace row are
    those of the plain restatement."""
    D, H, B = 3, 5, 4
    p, x, e, _ = K.draw(D, H, B, 11, 1.0)
    p, x, e = p.double(), x.double(), e.double()
    for t in (0.0, 0.71):
        got = K.rhs_kinetic(p, D, H, K.aug(x, 3), t, e)
        assert got.shape == (B, D + 3)
        assert torch.equal(got[:, :D + 1], R.rhs(p, D, H, K.aug(x, 1), t, e))
        for b in range(B):
            fn = lambda z: R.mlp(p, D, H, z[None], t)[0][0]
            J = torch.autograd.functional.jacobian(fn, x[b])
            assert abs(float(got[b, D + 1]) - float((fn(x[b]) ** 2).sum())) <= 1e-12
            assert abs(float(got[b, D + 2]) - float(((e[b] @ J) ** 2).sum())) <= 1e-12
            assert abs(float(got[b, D]) + float(e[b] @ J @ e[b])) <= 1e-12


def test_abi_declares_exports_and_guards_the_kinetic_entries(rnde):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnde.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rnde_[a-z_]+)\s*\(", src))
    L = rnde._lib.lib()
    for name in NEW:
        assert name in declared and hasattr(L, name) and name in rnde._lib.EXPORTS, name
    n, f = C.c_int32(), (C.c_float * 8)()
    BAD = rnde._lib.BAD_ARG
    assert L.rnde_ffjord_forward_kinetic(None, None, None, None, 1, 0.0, 1.0, 0, None, None, None, None, 0, None) == BAD
    assert L.rnde_ffjord_forward_kinetic_replay(None, None, None, None, 1, 0.0, 1.0, 0, f, 1, None, None, None, None, 0, None) == BAD
    assert L.rnde_ffjord_backward_kinetic(None, None, None, None, None, None) == BAD
    assert L.rnde_ffjord_debug_feval_kinetic(None, None, None, None, 1, 0.0, None, None) == BAD
    assert L.rnde_ffjord_step_log(None, f, 2, C.byref(n)) == BAD


def test_kinetic_limits_and_create_still_refuses_kinetic_reg(rnde):
    ff = rnde.ffjord
    ff.check_kinetic_served(ff.MLPDynamics(61, 64), "workgroup")
    ff.check_kinetic_served(ff.MLPDynamics(43, 100), "tiled")
    ff.check_kinetic_served(ff.MLPDynamics(64, 112), "tiled")
    with pytest.raises(ValueError, match=r"kinetic energy.*in_dims \+ 3 <= 64"):
        ff.check_kinetic_served(ff.MLPDynamics(62, 16), "workgroup")
    with pytest.raises(ValueError, match="limit of 64"):
        ff.check_kinetic_served(ff.MLPDynamics(43, 100), "workgroup")
    with pytest.raises(ValueError, match="hidden <= 112"):
        ff.check_kinetic_served(ff.MLPDynamics(43, 113), "tiled")
    with pytest.raises(ValueError, match="kinetic energy"):           # check_served keeps its behaviour
        ff.check_served(ff.MLPDynamics(2, 16), regularize_kinetic=True)
    L = rnde._lib.lib()
    for create in (L.rnde_ffjord_create, L.rnde_ffjord_create_tiled):
        cfg = rnde._lib.FfjordConfig()
        cfg.in_dims, cfg.hidden, cfg.max_batch, cfg.max_attempts, cfg.kinetic_reg = 2, 16, 64, 64, 1
        cfg.reltol = cfg.abstol = 1e-5
        h = C.c_void_p()
        assert create(C.byref(cfg), C.byref(h)) == rnde._lib.BAD_ARG and not h.value
        assert b"kinetic energy" in L.rnde_ffjord_last_error(None)
