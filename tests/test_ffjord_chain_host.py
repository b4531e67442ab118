"""TrackedFFJORD's default dynamics for Dense chains, without a GPU: the parameter count and the struct layout of the C ABI, every refusal
(at the ABI and in the package), and the restatements of tests/ffjord_chain_ref.py against something independent."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import act_ref as A
from tests import ffjord_chain_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOS = [([2, 10, 2], True, 64), ([5, 40, 24, 5], False, 1349), ([5, 40, 24, 5], True, 1418), ([48, 64, 64, 48], True, 10592), (CR.LATENT, False, 8280)]


def _model(rnde, dims, td, acts=None):
    acts = acts or ["tanh"] * (len(dims) - 1)
    layers = [rnde.Dense(dims[l] + (1 if td else 0), dims[l + 1], acts[l]) for l in range(len(dims) - 1)]
    return rnde.TDChain(*layers) if td else rnde.Chain(*layers)


def _cfg(rnde, dims, td, acts=None, **kw):
    c = rnde._lib.FfjordChainConfig()
    c.n_layers = len(dims) - 1
    for i, d in enumerate(dims):
        c.dims[i] = d
    for i, a in enumerate(acts or [1] * (len(dims) - 1)):
        c.act[i] = a
    c.time_dep, c.max_batch, c.max_attempts, c.reltol, c.abstol = int(td), 64, 100, 1e-5, 1e-5
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("dims,td,count", GEOS)
def test_param_count_is_destructure_length(rnde, dims, td, count):
    got = rnde._lib.lib().rnde_ffjord_chain_param_count(C.byref(_cfg(rnde, dims, td)))
    assert got == count == rnde.destructure(_model(rnde, dims, td)).numel()
    assert len(A.params(dims, td, np.random.default_rng(0))) == count


def test_struct_layout_agrees_between_c_ctypes_and_julia(rnde, tmp_path):
    """One layout, three descriptions (as tests/test_abi.py does for the node and nsde structs)."""
    exe = os.path.join(str(tmp_path), "abi_check_ffjord_chain")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_c", "abi_check_ffjord_chain.c"), "-o", exe])
    fields, size = [], None
    for line in subprocess.check_output([exe], text=True).splitlines():
        w = line.split()
        assert w[0] == "rnde_ffjord_chain_config"
        if w[1] == "sizeof":
            size = int(w[2])
        else:
            fields.append((w[1], int(w[2]), int(w[3])))
    py = rnde._lib.FfjordChainConfig
    want = ["n_layers", "dims", "act", "time_dep", "regularize", "max_batch", "solver", "reltol", "abstol", "cb_save_start", "max_attempts", "device"]
    assert [f[0] for f in fields] == want == [f[0] for f in py._fields_]
    assert C.sizeof(py) == size
    for name, off, nbytes in fields:
        d = getattr(py, name)
        assert (d.offset, d.size) == (off, nbytes), name
    src = open(os.path.join(ROOT, "bindings", "julia", "RNDE.jl")).read()
    body = re.search(r"\nstruct FfjordChainConfig\b[^\n]*\n(.*?)\nend\n", src, flags=re.S).group(1)
    jl = []
    for line in body.splitlines():
        for decl in line.split("#")[0].split(";"):
            m = re.match(r"\s*(\w+)::(.+?)\s*$", decl)
            if m:
                jl.append((m.group(1), m.group(2)))
    nbytes = {"Int32": 4, "Float32": 4, "NTuple{9,Int32}": 36, "NTuple{8,Int32}": 32}
    assert [f[0] for f in jl] == want
    off = 0
    for (name, ty), (_, coff, cbytes) in zip(jl, fields):
        assert (off, nbytes[ty]) == (coff, cbytes), name
        off += nbytes[ty]
    assert off == size
    for sym in ("rnde_ffjord_create_chain", "rnde_ffjord_chain_param_count"):
        assert f"(:{sym}, LIB)" in src, sym


def test_abi_refusals_name_the_limit(rnde):
    """Every refusal of rnde_ffjord_create_chain comes before a device is needed and names its limit; the ConcatSquash creates keep
    refusing dynamics = 1 by name and point at the new entry."""
    L = rnde._lib.lib()
    cases = [(_cfg(rnde, [2, 65, 2], True), b"limit of 64"),                     # a layer output above 64
             (_cfg(rnde, [2, 65, 65, 2], False), b"limit of 64"),                # ... and a layer input
             (_cfg(rnde, [64, 8, 64], False), b"64 rows"),                       # the state [z; l]
             (_cfg(rnde, [2, 3, 4], True), b"dims[0] must equal"),
             (_cfg(rnde, [2, 3, 2], True, [1, 6]), b"rnde_act"),
             (_cfg(rnde, [2, 3, 2], True, [-1, 0]), b"rnde_act"),
             (_cfg(rnde, [2, 3, 2], True, solver=1), b"Tsit5"),
             (_cfg(rnde, [60] + [64] * 7 + [60], False), b"bytes of LDS"),
             (_cfg(rnde, [2, 3, 2], True, max_batch=4097), b"4096"),
             (_cfg(rnde, [2, 3, 2], True, max_attempts=8001), b"8000"),
             (_cfg(rnde, [2, 3, 2], True, n_layers=9), b"RNDE_MAX_LAYERS"),
             (_cfg(rnde, [2, 3, 2], True, n_layers=0), b"RNDE_MAX_LAYERS")]
    for cfg, msg in cases:
        h = C.c_void_p()
        assert L.rnde_ffjord_create_chain(C.byref(cfg), C.byref(h)) == rnde._lib.BAD_ARG and not h.value
        assert msg in L.rnde_ffjord_last_error(None), (msg, L.rnde_ffjord_last_error(None))
    h = C.c_void_p()
    cfg = _cfg(rnde, [60] + [64] * 7 + [60], False)
    assert L.rnde_ffjord_create_chain(C.byref(cfg), C.byref(h)) == rnde._lib.BAD_ARG
    need = re.search(rb"need (\d+) bytes of LDS, above the limit of (\d+) bytes", L.rnde_ffjord_last_error(None))
    assert need and int(need.group(2)) == 160 * 1024 and int(need.group(1)) == rnde.ffjord.chain_lds_bytes([60] + [64] * 7 + [60]) > 160 * 1024
    # the geometries that must be served pass every check that needs no device
    if not torch.cuda.is_available():
        for dims, td, _ in GEOS + [([5, 12, 9, 5], True, 0)]:
            h = C.c_void_p()
            cfg = _cfg(rnde, dims, td)
            assert L.rnde_ffjord_create_chain(C.byref(cfg), C.byref(h)) == rnde._lib.NO_DEVICE, (dims, L.rnde_ffjord_last_error(None))
    old = rnde._lib.FfjordConfig()
    old.in_dims, old.hidden, old.dynamics, old.max_batch, old.max_attempts, old.reltol, old.abstol = 2, 16, 1, 64, 100, 1e-5, 1e-5
    for create in (L.rnde_ffjord_create, L.rnde_ffjord_create_tiled):
        h = C.c_void_p()
        assert create(C.byref(old), C.byref(h)) == rnde._lib.BAD_ARG and not h.value
        msg = L.rnde_ffjord_last_error(None)
        assert b"Tracker.forward" in msg and b"rnde_ffjord_create_chain" in msg


def test_package_refusals_name_the_limit(rnde):
    ff = rnde.ffjord
    td, ch = _model(rnde, [2, 10, 2], True), _model(rnde, [2, 10, 2], False)
    with pytest.raises(ValueError, match="Tracker.forward"):                      # a chain model on the default engine
        ff.TrackedFFJORD(td, [0.0, 1.0], True, False)
    with pytest.raises(ValueError, match="Tracker.forward"):                      # a Chain called as m(z, t)
        ff.TrackedFFJORD(ch, [0.0, 1.0], True, False, engine="tiled")
    with pytest.raises(ValueError, match="TDChain"):
        ff.TrackedFFJORD(td, [0.0, 1.0], False, False, engine="tiled")
    with pytest.raises(ValueError, match="leading element-wise map"):
        ff.TrackedFFJORD(rnde.Chain(rnde.Dense(2, 10, "tanh"), rnde.Dense(10, 2), pre_act=True), [0.0, 1.0], False, False, engine="tiled")
    with pytest.raises(ValueError, match="forw_n_back"):
        ff.TrackedFFJORD(td, [0.0, 1.0], True, False, engine="tiled", dynamics="forw_n_back")
    with pytest.raises(ValueError, match="limit of 64"):
        ff.TrackedFFJORD(_model(rnde, [2, 65, 2], True), [0.0, 1.0], True, False, engine="tiled")
    with pytest.raises(ValueError, match="limit of 64"):
        ff.TrackedFFJORD(_model(rnde, [64, 8, 64], False), [0.0, 1.0], False, False, engine="tiled")
    with pytest.raises(ValueError, match="bytes of LDS"):
        ff.TrackedFFJORD(_model(rnde, [60] + [64] * 7 + [60], False), [0.0, 1.0], False, False, engine="tiled")
    with pytest.raises(ValueError, match="ends in 4"):
        ff.TrackedFFJORD(_model(rnde, [2, 3, 4], True), [0.0, 1.0], True, False, engine="tiled")
    with pytest.raises(ValueError, match="not served"):
        ff.TrackedFFJORD(_model(rnde, [2, 3, 2], True, ["swish", "identity"]), [0.0, 1.0], True, False, engine="tiled")
    with pytest.raises(ValueError, match="limit of 64"):                          # the kinetic rows need D + 3 <= 64
        ff.check_kinetic_served(_model(rnde, [62, 8, 62], False), "tiled")
    ff.check_kinetic_served(_model(rnde, [61, 8, 61], False), "tiled")
    ff.check_served(_model(rnde, [48, 64, 64, 48], True), engine="tiled")


@pytest.mark.parametrize("dims,td,acts", [([2, 10, 2], True, ["tanh", "identity"]), ([5, 12, 9, 5], False, ["sigmoid", "softplus", "tanh"]),
                                          ([5, 12, 9, 5], True, ["elu", "relu", "tanh"])])
def test_restatement_against_the_full_jacobian(dims, td, acts):
    """e . eJ against e' J e, the exact trace against trace(J), and the kinetic rows, with J from torch.autograd.functional.jacobian."""
    D, B, t = dims[0], 6, 0.37
    p, x, e, _ = CR.draw(dims, td, B, 3, 2.0)
    P, X, E = p.double(), x.double(), e.double()
    hut, ex = CR.rhs(dims, acts, td, P, CR.aug(X), t, E).detach(), CR.rhs(dims, acts, td, P, CR.aug(X), t).detach()
    kin = CR.rhs_kinetic(dims, acts, td, P, CR.aug(X, 3), t, E).detach()
    for b in range(B):
        J = torch.autograd.functional.jacobian(lambda z: A.chain64(dims, acts, td, 0, P, z[None], t)[0], X[b])
        f = A.chain64(dims, acts, td, 0, P, X[b:b + 1], t)[0]
        assert torch.allclose(hut[b, :D], f, rtol=1e-12, atol=1e-14) and torch.allclose(ex[b, :D], f, rtol=1e-12, atol=1e-14)
        assert abs(float(hut[b, D]) + float(E[b] @ J @ E[b])) <= 1e-12 * max(1.0, abs(float(hut[b, D])))
        assert abs(float(ex[b, D]) + float(torch.trace(J))) <= 1e-12 * max(1.0, abs(float(ex[b, D])))
        assert torch.equal(kin[b, :D + 1], hut[b])
        assert abs(float(kin[b, D + 1]) - float(f @ f)) <= 1e-12 * float(f @ f)
        eJ = E[b] @ J
        assert abs(float(kin[b, D + 2]) - float(eJ @ eJ)) <= 1e-12 * max(float(eJ @ eJ), 1e-30)


@pytest.mark.parametrize("name", list(A.CODES))
def test_second_derivative_from_the_output(name):
    """The hand formulas for phi'' (from the output y) against autograd of act_dy(act_fwd(z)); relu / elu away from the kink."""
    z = torch.linspace(-6.0, 6.0, 241, dtype=torch.float64)
    z = z[z.abs() > 1e-3].clone().requires_grad_(True)
    y = A.act_fwd(name, z)
    d = A.act_dy(name, y)
    want = torch.autograd.grad(d.sum(), z, allow_unused=True)[0] if d.requires_grad else None
    want = torch.zeros_like(z) if want is None else want
    got = CR.d2y(name, y.detach())
    assert float((got - want).abs().max()) <= 1e-12
