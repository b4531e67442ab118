"""Host-side mirrors of the Flux pieces the hot path is built from.

Dense / TDChain / MLPDynamics only describe shapes and hold initial parameters; the arithmetic
runs in librnde.so.  Layout rule (reference src/models/neural_ode.jl:12, Flux.destructure): the
flat parameter vector is [vec(W_1) column-major (out x in); b_1; vec(W_2); b_2; ...].
A Julia D x B column-major matrix is a torch tensor of shape (B, D), contiguous.
"""
import math

import torch


class Dense:
    """Flux.Dense(in, out, act): W is out x in, Glorot-uniform, zero bias (Flux 0.11 defaults)."""

    def __init__(self, n_in, n_out, act="identity", generator=None):
        self.n_in, self.n_out, self.act = n_in, n_out, act
        lim = math.sqrt(6.0 / (n_in + n_out))
        # stored as (in, out) row-major == (out x in) column-major
        self.W = (torch.rand(n_in, n_out, generator=generator) * 2 - 1) * lim
        self.b = torch.zeros(n_out)


class TDChain:
    """reference src/models/basic.jl:1-35: every layer sees vcat(x, t)."""
    time_dep = True
    pre_act = False

    def __init__(self, *layers):
        self.layers = list(layers)

    def dims(self):
        d = [self.layers[0].n_in - 1]
        for l in self.layers:
            d.append(l.n_out)
        return d


# Dense activations the kernels serve (include/rnde.h: rnde_act), by name: NNlib's identity, tanh, relu, σ, softplus and elu (alpha = 1).
# Each derivative is a function of the layer's output (what the reverse pass keeps); swish / gelu and the like are not served.
ACT = {"identity": 0, "tanh": 1, "relu": 2, "sigmoid": 3, "softplus": 4, "elu": 5}


def act_code(name):
    """rnde_act code of a Dense layer's activation name; ValueError for a name the kernels do not serve."""
    try:
        return ACT[name]
    except (KeyError, TypeError):
        raise ValueError(f"Dense activation {name!r} is not served: one of {list(ACT)}") from None


def MLPDynamics(n_in, hidden, generator=None):
    """reference experiments/mnist_node.jl:41-54: Dense(in+1, hidden, tanh) -> Dense(hidden+1, in, tanh)."""
    return TDChain(Dense(n_in + 1, hidden, "tanh", generator), Dense(hidden + 1, n_in, "tanh", generator))


# The leading element-wise maps the kernels apply in front of a Dense chain (include/rnde.h: rnde_pre_act), by name
PRE_ACT = {None: 0, False: 0, "tanh": 1, True: 1, "cube": 2}
_PRE_PROBES = (-1.5, -0.3, 0.0, 0.7, 2.0)      # (bindings/julia/RNDE.jl::pre_act_code: the same points, fp64, the same pointwise 1e-9 test)
_PRE_WANT = {"tanh": math.tanh, "cube": lambda v: v * v * v}


def pre_act_of(f):
    """Name of a leading element-wise callable as the reference writes it -- `x -> tanh.(x)` (experiments/latent_ode.jl:114) or `x -> x .^ 3`
    (experiments/sde_toy_problem.jl:45): its values at a few fixed points are matched against tanh and the cube (the rule node.py::reg_code applies
    to callbacks; the same rule as bindings/julia/RNDE.jl::pre_act_code).  Raises ValueError for anything else: a map the kernels do not apply must
    not be replaced by another one silently."""
    x = torch.tensor(_PRE_PROBES, dtype=torch.float64)
    try:
        got = [float(v) for v in torch.as_tensor(f(x), dtype=torch.float64).reshape(-1)]
    except Exception as e:
        raise ValueError(f"leading element of the Chain: calling it on a tensor failed ({e})") from e
    if len(got) == len(_PRE_PROBES):
        for name, want in _PRE_WANT.items():
            if all(abs(g - want(p)) <= 1e-9 * max(1.0, abs(want(p))) for g, p in zip(got, _PRE_PROBES)):
                return name
    raise ValueError(f"leading element of the Chain is neither tanh nor x -> x ** 3 (the element-wise maps the kernels apply): on {_PRE_PROBES} it "
                     f"returned {got}")


class Chain:
    """Time-independent Flux.Chain of Dense layers, optional leading element-wise map: tanh (experiments/latent_ode.jl:113-124) or the cube
    (experiments/sde_toy_problem.jl:45).  The map is given as the reference writes it -- a leading callable, Chain(lambda x: x ** 3, Dense(2, 50,
    "tanh"), Dense(50, 2)) -- or as pre_act = True (tanh) / "tanh" / "cube".  It is kept in `pre_act`, not in `layers` (it has no parameters:
    destructure and dims() see the Dense layers only)."""
    time_dep = False

    def __init__(self, *layers, pre_act=False):
        layers = list(layers)
        if layers and callable(layers[0]) and not isinstance(layers[0], Dense):
            if pre_act:
                raise ValueError("Chain: a leading callable and pre_act together")
            pre_act = pre_act_of(layers.pop(0))
        if not all(isinstance(l, Dense) for l in layers):
            raise ValueError("Chain: an optional leading element-wise map (tanh or x -> x ** 3), then Dense layers only")
        if pre_act not in PRE_ACT:
            raise ValueError(f"pre_act: one of {list(PRE_ACT)}")
        self.layers = layers
        self.pre_act = pre_act

    def dims(self):
        d = [self.layers[0].n_in]
        for l in self.layers:
            d.append(l.n_out)
        return d


def LatentGenDynamics(latent=20, hidden=50, depth=8, generator=None):
    """reference experiments/latent_ode.jl:113-124 (gen_dynamics): x -> tanh.(x), then `depth` Dense layers alternating
    latent -> hidden -> latent, all tanh, time independent."""
    dims = [latent if i % 2 == 0 else hidden for i in range(depth + 1)]
    return Chain(*[Dense(dims[i], dims[i + 1], "tanh", generator) for i in range(depth)], pre_act=True)


def destructure(model):
    """Flux.destructure(model)[1]: flat fp32 parameter vector."""
    parts = []
    for l in model.layers:
        parts.append(l.W.reshape(-1))
        parts.append(l.b.reshape(-1))
    return torch.cat(parts).to(torch.float32).contiguous()
