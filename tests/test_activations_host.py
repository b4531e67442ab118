"""The Dense activations of include/rnde.h (rnde_act) without a GPU: the derivative-from-output identities the reverse kernels rely on, the
Python names and the codes of the header, the Julia binding's names and codes, and the refusal of an unknown name."""
import os
import re

import pytest
import torch

from tests.act_ref import CODES, NEW, act_dy, act_fwd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_codes():
    src = open(os.path.join(ROOT, "include", "rnde.h")).read()
    body = re.search(r"typedef enum \{([^}]*)\} rnde_act;", src).group(1)
    return {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"RNDE_ACT_(\w+)\s*=\s*(\d+)", body)}


@pytest.mark.parametrize("name", ("tanh",) + NEW)
def test_derivative_from_output_matches_autograd(name):
    """act_dy(y = act(z)) equals d act / dz by autograd in fp64, on a grid with |z| near 0 and beyond 20 (away from the kinks of relu / elu at 0,
    where the one-sided values are pinned separately below)."""
    z = torch.cat([torch.linspace(-30, 30, 2001), torch.tensor([-1e-6, -1e-3, 1e-3, 1e-6, 20.5, -20.5, 25.0, -25.0])]).double()
    if name in ("relu", "elu"):
        z = z[z != 0]
    z.requires_grad_(True)
    y = act_fwd(name, z)
    (dz,) = torch.autograd.grad(y.sum(), z)
    want, got = dz.detach(), act_dy(name, y.detach())
    assert torch.isfinite(y).all() and torch.isfinite(got).all()
    err = (got - want).abs() / torch.clamp(want.abs(), min=1e-300)
    # (relative: sigmoid's derivative from y loses digits only where y (1 - y) cancels, i.e. where it is tiny in absolute terms)
    assert float(((got - want).abs()).max()) <= 1e-12 and float(err[want.abs() > 1e-8].max()) <= 1e-6, name


def test_forward_formulas_are_the_textbook_maps():
    z = torch.linspace(-25, 25, 1001).double()
    assert torch.allclose(act_fwd("relu", z), torch.relu(z), rtol=0, atol=0)
    assert torch.allclose(act_fwd("sigmoid", z), torch.sigmoid(z), rtol=1e-15, atol=1e-300)
    assert torch.allclose(act_fwd("softplus", z), torch.nn.functional.softplus(z, threshold=1e9), rtol=1e-14, atol=1e-300)
    assert torch.allclose(act_fwd("elu", z), torch.nn.functional.elu(z), rtol=1e-14, atol=1e-300)
    # one-sided values at the kinks: relu' and elu' at y = 0 are the left derivatives (0 and 1)
    assert float(act_dy("relu", torch.zeros(1).double())) == 0.0 and float(act_dy("elu", torch.zeros(1).double())) == 1.0


def test_python_names_map_to_the_header_codes():
    from regneuralde_jl_amd.layers import ACT, act_code
    hdr = _header_codes()
    assert hdr == {"identity": 0, "tanh": 1, "relu": 2, "sigmoid": 3, "softplus": 4, "elu": 5}
    assert ACT == hdr == CODES
    for name, code in hdr.items():
        assert act_code(name) == code


@pytest.mark.parametrize("name", ["swish", "gelu", "Relu", None, 2])
def test_unknown_name_is_a_value_error(name):
    import regneuralde_jl_amd as rn
    from regneuralde_jl_amd.layers import act_code
    with pytest.raises(ValueError, match="relu"):
        act_code(name)
    g = torch.Generator().manual_seed(0)
    with pytest.raises(ValueError, match="not served"):
        rn.TrackedNeuralODE(rn.Chain(rn.Dense(2, 4, name, g), rn.Dense(4, 2, "identity", g)), [0.0, 1.0], False, False)
    with pytest.raises(ValueError, match="not served"):
        rn.TrackedNeuralDSDE(rn.Chain(rn.Dense(2, 4, "tanh", g), rn.Dense(4, 2, "identity", g)), rn.Dense(2, 2, name, g), [0.0, 1.0], False)


def test_new_names_are_accepted_by_the_layers():
    """Constructing the layers with the new names needs no GPU (the handle is made at the first call)."""
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(0)
    for name in NEW:
        node = rn.TrackedNeuralODE(rn.Chain(rn.Dense(2, 4, name, g), rn.Dense(4, 2, "identity", g)), [0.0, 1.0], False, False)
        cfg = node._config(0, None)
        assert cfg.act[0] == CODES[name] and cfg.act[1] == 0
        sde = rn.TrackedNeuralDSDE(rn.Chain(rn.Dense(2, 4, name, g), rn.Dense(4, 2, "identity", g)), rn.Dense(2, 2, name, g), [0.0, 1.0], False)
        cfg = sde._config(0)
        assert cfg.drift_act[0] == CODES[name] and cfg.diff_act[0] == CODES[name]


def test_julia_binding_names_and_codes_match_the_header():
    """bindings/julia cannot run here: RNDE.jl declares the six codes with the header's values, recognises NNlib's functions by identity, and
    both patch files go through that one helper (no inline tanh / identity test is left)."""
    d = os.path.join(ROOT, "bindings", "julia")
    mod, ode, sde = (open(os.path.join(d, f)).read() for f in ("RNDE.jl", "patch_neural_ode.jl", "patch_neural_sde.jl"))
    m = re.search(r"^const (ACT_\w+(?:, ACT_\w+)*) = (Int32\(\d+\)(?:, Int32\(\d+\))*)$", mod, flags=re.M)
    names = [n[len("ACT_"):].lower() for n in m.group(1).split(", ")]
    codes = [int(v) for v in re.findall(r"Int32\((\d+)\)", m.group(2))]
    assert dict(zip(names, codes)) == _header_codes()
    fn = {"identity": "identity", "tanh": "tanh", "relu": "Flux.relu", "sigmoid": "Flux.σ", "softplus": "Flux.softplus", "elu": "Flux.elu"}
    for name, f in fn.items():
        assert re.search(r"f === " + re.escape(f) + r" && return ACT_" + name.upper() + r"\b", mod), name
    assert re.search(r"^import Flux\b", mod, flags=re.M)
    assert "_act_code(σ) = RNDE.act_code(σ)" in ode and "_act_code(l.σ)" in ode
    assert "RNDE.act_code(l.σ)" in sde
    assert "σ === tanh" not in ode and "l.σ === tanh" not in sde
