"""The neural-SDE toy problem of reference experiments/sde_toy_problem.jl on the device: AdaBelief (rnde_adabelief_step), the moment-matching
loss (rnde_moment_loss), the fused training step (rnde_nsde_moment_grad) and the layer with the x -> x .^ 3 drift."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sde_demo")


def _fixture(name):
    """(T, D) float32 tensor of the Julia D x T fixture (the bit patterns are the values)."""
    rows, size = [], None
    for line in open(os.path.join(GOLDEN, name + ".txt")):
        if line.startswith("# size"):
            size = [int(v) for v in line.split()[2:]]
        elif not line.startswith("#"):
            rows.append(int(line.split()[0], 16))
    v = np.array(rows, dtype=np.uint32).view(np.float32)
    return torch.from_numpy(v.reshape(size[1], size[0]).copy())


def _toy(regularize, seed=5, B=100):
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(seed)
    nsde = rn.TrackedNeuralDSDE(rn.Chain(lambda x: x ** 3, rn.Dense(2, 50, "tanh", g), rn.Dense(50, 2, "identity", g)), rn.Dense(2, 2, "identity", g),
                                [0.0, 1.0 + float(np.finfo(np.float32).eps)], regularize, "SOSRI", saveat=torch.linspace(0, 1, 30), reltol=0.3, abstol=0.3,
                                max_batch=B)
    u0 = torch.tensor([[2.0, 0.0]]).repeat(B, 1).cuda()
    return nsde, u0


def test_adabelief_matches_the_recurrence():
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(1)
    p = torch.randn(1000, generator=g).cuda()
    ref = p.double().clone()
    opt = rn.FluxAdaBelief([p], eta=0.01, beta=(0.9, 0.999), eps=1e-8)
    m = torch.zeros_like(ref)
    s = torch.zeros_like(ref)
    for _ in range(5):
        grad = torch.randn(1000, generator=g).cuda()
        p.grad = grad.clone()
        opt.step()
        gd = grad.double()
        m = 0.9 * m + 0.1 * gd
        s = 0.999 * s + 0.001 * (gd - m) ** 2
        ref = ref - 0.01 * m / (s.sqrt() + 1e-8)
    torch.cuda.synchronize()
    assert (p.double() - ref).abs().max() <= 1e-6 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("B,T,D", [(2, 5, 3), (100, 30, 2), (100, 1, 2), (37, 4, 7)])
def test_moment_loss_matches_fp64(B, T, D):
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(B + T)
    sol = (torch.randn(B, T, D, generator=g) * 0.7 + 1.0).cuda()
    dm, dv = torch.randn(T, D, generator=g).cuda(), torch.rand(T, D, generator=g).cuda()
    s = sol.double().clone().requires_grad_(True)
    l2m = ((dm.double() - s.mean(dim=0)) ** 2).mean()
    l2v = ((dv.double() - s.var(dim=0, unbiased=True)) ** 2).mean()
    gref = torch.autograd.grad(l2m + l2v, s)[0]
    so = sol.clone().requires_grad_(True)
    out = rn.moment_loss(so, dm, dv)
    assert abs(out[0].item() - l2m.item()) <= 1e-6 * max(l2m.item(), 1e-12) + 1e-12
    assert abs(out[1].item() - l2v.item()) <= 1e-6 * max(l2v.item(), 1e-12) + 1e-12
    (out[0] + out[1]).backward()
    assert (so.grad.double() - gref).abs().max() <= 1e-5 * gref.abs().max()
    # separate weights split the kernel's cotangent exactly
    so.grad = None
    out = rn.moment_loss(so, dm, dv)
    (2.0 * out[0] + 0.5 * out[1]).backward()
    s2 = sol.double().clone().requires_grad_(True)
    gw = torch.autograd.grad(2.0 * ((dm.double() - s2.mean(dim=0)) ** 2).mean() + 0.5 * ((dv.double() - s2.var(dim=0)) ** 2).mean(), s2)[0]
    assert (so.grad.double() - gw).abs().max() <= 1e-5 * gw.abs().max()
    # the same bits on a second run
    again = rn.moment_loss(sol, dm, dv)
    assert torch.equal(again, out.detach())


@pytest.mark.parametrize("regularize", [False, True])
def test_fused_step_matches_the_composed_path(regularize):
    """fused_moment_loss_and_grad == layer saveat call + moment_loss + autograd (+ 0.2 * sum(saveval)), on the same noise pool, to 1e-6 relative."""
    import regneuralde_jl_amd as rn
    dm, dv = _fixture("sde_data").cuda(), _fixture("sde_data_vars").cuda()
    nsde, u0 = _toy(regularize)
    noise = torch.randn(300, 2, 100, 2, generator=torch.Generator().manual_seed(2)).cuda()
    p = nsde.p.cuda().requires_grad_(True)
    sol, nfe1, nfe2, sv = nsde(u0, p, func=None, noise=noise)
    l2 = rn.moment_loss(sol, dm, dv)
    reg = 0.2 * sv.saveval.sum() if regularize else torch.zeros((), device="cuda")
    (l2[0] + l2[1] + reg).backward()
    q = nsde.p.cuda().clone()
    loss, l2m, l2v, reg_f, n1, n2 = rn.fused_moment_loss_and_grad(nsde, u0, dm, dv, c=0.2, p=q, noise=noise)
    torch.cuda.synchronize()
    assert (n1, n2) == (nfe1, nfe2)
    assert abs(l2m.item() - l2[0].item()) <= 1e-6 * l2[0].item() and abs(l2v.item() - l2[1].item()) <= 1e-6 * l2[1].item()
    reg = float(reg.detach())
    assert abs(reg_f - reg) <= 1e-6 * max(abs(reg), 1e-12)
    assert (q.grad - p.grad).abs().max() <= 1e-6 * p.grad.abs().max()


def test_short_toy_run_is_finite_and_counts_like_the_composed_path():
    """20 iterations of the toy loop (AdaBelief(0.01), fused steps, library noise) stay finite; each step's NFE is that of the composed path
    on the same parameters and the same seed."""
    import regneuralde_jl_amd as rn
    dm, dv = _fixture("sde_data").cuda(), _fixture("sde_data_vars").cuda()
    nsde, u0 = _toy(True)
    p = nsde.p.cuda()
    opt = rn.FluxAdaBelief([p], eta=0.01)
    for it in range(20):
        seed = nsde.seed
        with torch.no_grad():
            _, nfe_c, _, _ = nsde(u0, p.clone())            # composed path: the layer call with the seed the fused step will use
        nsde.seed = seed
        loss, l2m, l2v, reg, n1, n2 = rn.fused_moment_loss_and_grad(nsde, u0, dm, dv, c=0.2, p=p)
        assert n1 == nfe_c
        opt.step()
        assert torch.isfinite(loss).item() and np.isfinite(reg)
    assert torch.isfinite(p).all()


def test_refusals():
    import regneuralde_jl_amd as rn
    from regneuralde_jl_amd import _lib
    from tests.util import NsdeNode, make_nsde_cfg
    with pytest.raises(ValueError):
        rn.Chain(lambda x: x ** 2, rn.Dense(2, 50, "tanh"), rn.Dense(50, 2))
    # data left on the host (the fixtures load there) is refused, never handed to a kernel
    dm, dv = _fixture("sde_data"), _fixture("sde_data_vars")
    nsde, u0 = _toy(False)
    with pytest.raises(ValueError):
        rn.moment_loss(torch.zeros(100, 30, 2, device="cuda"), dm, dv.cuda())
    with pytest.raises(ValueError):
        rn.moment_loss(torch.zeros(100, 30, 2, device="cuda"), dm.cuda(), dv)
    with pytest.raises(ValueError):
        rn.fused_moment_loss_and_grad(nsde, u0, dm, dv.cuda(), p=nsde.p.cuda())
    with pytest.raises(ValueError):
        rn.fused_moment_loss_and_grad(nsde, u0, dm.cuda(), dv.cuda(), p=nsde.p)
    node = NsdeNode(make_nsde_cfg([2, 5, 2], ["tanh", "identity"], [2, 2], ["identity"], 4, regularize=0))
    assert node.L.rnde_nsde_set_pre_act(node.h, 2, 0) == _lib.OK
    assert node.L.rnde_nsde_set_pre_act(node.h, 3, 0) == _lib.BAD_ARG
    rng = np.random.default_rng(0)
    p = rng.standard_normal(node.P).astype(np.float32) * 0.3
    node.forward(rng.standard_normal((4, 2)).astype(np.float32), p, rng.standard_normal((200, 2, 4, 2)).astype(np.float32), keep_tape=True)
    assert node.L.rnde_nsde_set_pre_act(node.h, 0, 0) == _lib.BAD_ARG       # a tape is held
    node.backward(np.zeros((4, 2), np.float32))
    assert node.L.rnde_nsde_set_pre_act(node.h, 0, 0) == _lib.OK
    node.close()
