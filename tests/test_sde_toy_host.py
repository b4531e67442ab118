"""CPU checks of the toy-problem pieces (reference experiments/sde_toy_problem.jl): the data fixture, the Chain's leading-map probe, the ABI."""
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sde_demo")


def _read(name):
    head, vals = [], []
    for line in open(os.path.join(GOLDEN, name + ".txt")):
        if line.startswith("#"):
            head.append(line)
            continue
        bits, dec = line.split()
        vals.append((int(bits, 16), float(dec)))
    return head, vals


@pytest.mark.parametrize("name", ["sde_data", "sde_data_vars"])
def test_fixture_is_self_consistent(name):
    head, vals = _read(name)
    assert any("sde_demo.bson" in h and re.search(r"sha256 [0-9a-f]{64}", h) for h in head)
    assert "# size 2 30\n" in head and len(vals) == 60
    for bits, dec in vals:
        f32 = struct.unpack("<f", struct.pack("<I", bits))[0]
        assert f32 == dec and struct.unpack("<f", struct.pack("<f", dec))[0] == dec
    if name == "sde_data":
        assert [d for _, d in vals[:2]] == [2.0, 0.0]          # u0 = (2, 0): the first column of the data is the initial state
    else:
        assert all(d >= 0 for _, d in vals) and [d for _, d in vals[:2]] == [0.0, 0.0]


def test_chain_probe_classifies_the_leading_map():
    import math
    import torch
    import regneuralde_jl_amd as rn
    from regneuralde_jl_amd.layers import PRE_ACT
    assert rn.pre_act_of(torch.tanh) == "tanh" and rn.pre_act_of(lambda x: x ** 3) == "cube" and rn.pre_act_of(lambda x: x * x * x) == "cube"
    for f in (lambda x: x ** 2, lambda x: x, lambda x: torch.sin(x), lambda x: 1.0001 * x ** 3):
        with pytest.raises(ValueError):
            rn.pre_act_of(f)
    c = rn.Chain(lambda x: x ** 3, rn.Dense(2, 50, "tanh"), rn.Dense(50, 2))
    assert c.pre_act == "cube" and c.dims() == [2, 50, 2] and len(c.layers) == 2 and rn.destructure(c).numel() == 2 * 50 + 50 + 50 * 2 + 2
    assert PRE_ACT[rn.Chain(torch.tanh, rn.Dense(3, 3)).pre_act] == 1 and PRE_ACT[rn.Chain(rn.Dense(3, 3), pre_act=True).pre_act] == 1
    assert PRE_ACT[c.pre_act] == 2 and PRE_ACT[rn.Chain(rn.Dense(3, 3)).pre_act] == 0
    with pytest.raises(ValueError):
        rn.Chain(lambda x: x ** 2, rn.Dense(2, 2))
    with pytest.raises(ValueError):
        rn.Chain(rn.Dense(2, 2), lambda x: x ** 3)
    # the host-side chain evaluation (timeseries.py) applies the cube for "cube", never tanh
    from regneuralde_jl_amd.timeseries import _apply_chain
    x = torch.tensor([[0.5, -2.0]])
    p = rn.destructure(rn.Chain(rn.Dense(2, 2)))
    y = _apply_chain(rn.Chain(lambda v: v ** 3, rn.Dense(2, 2)), p, x)
    W = p[:4].view(2, 2)
    assert torch.allclose(y, (x ** 3) @ W + p[4:]) and not math.isclose(float(y[0, 0]), float((torch.tanh(x) @ W + p[4:])[0, 0]))


def test_toy_helpers_refuse_host_tensors():
    """The kernels read every pointer on the GPU: host tensors are a ValueError before anything is launched."""
    import torch
    import regneuralde_jl_amd as rn
    sol, dm, dv = torch.zeros(4, 3, 2), torch.zeros(3, 2), torch.zeros(3, 2)
    with pytest.raises(ValueError):
        rn.moment_loss(sol, dm, dv)


def test_header_declares_and_exports_the_new_entry_points():
    from regneuralde_jl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rnde.h")).read()
    for name in ("rnde_nsde_set_pre_act", "rnde_moment_loss", "rnde_nsde_moment_grad", "rnde_adabelief_step"):
        assert re.search(r"rnde_status\s+" + name + r"\(", hdr), name
        assert name in _lib.EXPORTS
    assert "RNDE_PRE_NONE = 0" in hdr and "RNDE_PRE_TANH = 1" in hdr and "RNDE_PRE_CUBE = 2" in hdr
