"""ClassifierNSDE with several trajectories per input on the device: rnde_nsde_classifier_head_traj, rnde_nsde_classifier_grad_traj and
rnde_nsde_classifier_predict (csrc/rnde_head_traj.h), and their Python front end (ClassifierNSDE.predict, nsde_accuracy,
fused_nsde_loss_and_grad with trajectories > 1).

Layout everywhere: row t * B + b of a (B * T, D) tensor (= column t * B + b of the Julia D x (B T) array) is trajectory t of input b.
Shapes: the generic solve kernels on `small` of tests/test_gpu_nsde.py (D = 3) with C = 4, and the reference geometry (D = 32) with C = 10
and C = 16; (B, T) from one column to 170 (not a multiple of the 16-column tile: workgroups of the solve straddle trajectories).
Tolerance 0.14, explicit noise pools."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BT = [(1, 1), (5, 3), (16, 2), (17, 10)]
CASES = [("small", 4, b, t) for b, t in BT] + [("nsde", 10, b, t) for b, t in BT] + [("nsde", 16, 5, 3)]
IDS = [f"{k}-C{c}-B{b}-T{t}" for k, c, b, t in CASES]
N_POOL = 128
LAM = 10.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _case(kind, n_classes, B, T, seed=31, mb=None, **kw):
    """handle + inputs: x (B, D) NOT repeated, p2, p3 in the Flux.destructure(Dense(D, C)) layout, one-hot and soft labels, a noise pool for B T columns"""
    from tests.test_gpu_nsde import _cfg, _setup
    from tests.util import NsdeNode
    drift, diff, p2, xall, noise = _setup(kind, B * T, seed, N_POOL)
    D = drift.dims[0]
    rng = np.random.default_rng(seed + 1)
    p3 = (0.5 * rng.standard_normal(n_classes * D + n_classes)).astype(np.float32)
    y1 = np.eye(n_classes, dtype=np.float32)[rng.integers(0, n_classes, B)]
    ys = rng.uniform(0.0, 1.5, (B, n_classes)).astype(np.float32)      # neither one-hot nor summing to 1
    node = NsdeNode(_cfg(drift, diff, mb or B * T, **kw))
    return dict(node=node, D=D, C=n_classes, B=B, T=T, x=np.ascontiguousarray(xall[:B]), p2=p2, p3=p3, y=y1, y_soft=ys, noise=noise)


def head_traj(node, u, p3, y, B, T, n_classes):
    from regneuralde_jl_amd import _lib
    ud, pd, yd = _dev(u), _dev(p3), _dev(y)
    z = torch.full((B, n_classes), float("nan"), device="cuda")
    ubar, p3bar, ce = torch.full_like(ud, float("nan")), torch.full_like(pd, float("nan")), torch.full((1,), float("nan"), device="cuda")
    _lib.check_nsde(node.h, node.L.rnde_nsde_classifier_head_traj(node.h, ud.data_ptr(), pd.data_ptr(), yd.data_ptr(), B, T, n_classes, z.data_ptr(),
                                                                  ubar.data_ptr(), p3bar.data_ptr(), ce.data_ptr(), None))
    torch.cuda.synchronize()
    return dict(z=z, ubar=ubar, p3bar=p3bar, ce=ce, u=ud, p3=pd, y=yd)


def grad_traj(node, c, y=None, lam=LAM, t1=1.0):
    from regneuralde_jl_amd import _lib
    B, T = c["B"], c["T"]
    xd, p2d, p3d, yd, nd = _dev(c["x"]), _dev(c["p2"]), _dev(c["p3"]), _dev(c["y"] if y is None else y), _dev(c["noise"])
    p2bar, p3bar, xbar = torch.full_like(p2d, float("nan")), torch.full_like(p3d, float("nan")), torch.full_like(xd, float("nan"))
    ce = torch.full((1,), float("nan"), device="cuda")
    reg, n1, n2 = C.c_float(0), C.c_int64(0), C.c_int64(0)
    _lib.check_nsde(node.h, node.L.rnde_nsde_classifier_grad_traj(
        node.h, xd.data_ptr(), p2d.data_ptr(), p3d.data_ptr(), yd.data_ptr(), B, T, c["C"], 0.0, t1, nd.data_ptr(), nd.shape[0], 0, lam,
        p2bar.data_ptr(), p3bar.data_ptr(), xbar.data_ptr(), ce.data_ptr(), C.byref(reg), C.byref(n1), C.byref(n2), None))
    torch.cuda.synchronize()
    return dict(nfe=np.array([n1.value, n2.value]), ce=ce.cpu().numpy(), reg=np.array([reg.value], np.float32), p2bar=p2bar.cpu().numpy(),
                p3bar=p3bar.cpu().numpy(), xbar=xbar.cpu().numpy())


def predict(node, c, y=None, correct=None, p3=None):
    from regneuralde_jl_amd import _lib
    B, T = c["B"], c["T"]
    xd, p2d, p3d, nd = _dev(c["x"]), _dev(c["p2"]), _dev(c["p3"] if p3 is None else p3), _dev(c["noise"])
    yd = None if y is None else _dev(y)
    if yd is not None and correct is None:
        correct = torch.zeros(1, dtype=torch.int64, device="cuda")
    z = torch.full((B, c["C"]), float("nan"), device="cuda")
    n1, n2 = C.c_int64(0), C.c_int64(0)
    _lib.check_nsde(node.h, node.L.rnde_nsde_classifier_predict(
        node.h, xd.data_ptr(), p2d.data_ptr(), p3d.data_ptr(), yd.data_ptr() if yd is not None else None, B, T, c["C"], 0.0, 1.0, nd.data_ptr(),
        nd.shape[0], 0, z.data_ptr(), correct.data_ptr() if yd is not None else None, C.byref(n1), C.byref(n2), None))
    torch.cuda.synchronize()
    return z.cpu().numpy(), np.array([n1.value, n2.value]), correct


def _first_argmax_matches(z, y):
    return int((np.argmax(z, axis=1) == np.argmax(y, axis=1)).sum())      # numpy's argmax is the first index of the maximum, as Julia's


# ---- 1. the head against fp64 ------------------------------------------------------------------------------------------------------------------

def _head64(u, p3, y, B, T, n_classes, D):
    """the formulas of csrc/rnde_head_traj.h in float64"""
    u, p3, y = u.astype(np.float64), p3.astype(np.float64), y.astype(np.float64)
    W = p3[: n_classes * D].reshape(D, n_classes).T                 # C x D: W[i, d] = p3[d * C + i]
    b3 = p3[n_classes * D:]
    u3 = u.reshape(T, B, D)
    z = (u3 @ W.T + b3).mean(axis=0)
    mag = (np.abs(u3)[:, :, None, :] * np.abs(W)[None, None, :, :]).sum(axis=(0, 3)) + T * np.abs(b3)      # sum_t sum_d |W_id u_d,tb| + T |b_i|
    m = z.max(axis=1, keepdims=True)
    logp = z - (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))
    ce = -(y * logp).sum() / B
    delta = (np.exp(logp) * y.sum(axis=1, keepdims=True) - y) / B
    ubar = np.tile(delta @ W / T, (T, 1))
    Wbar = np.einsum("tbd,bi->di", u3, delta) / T                    # (D, C): p3bar[d * C + i]
    return dict(z=z, zmag=mag / T, ce=np.array([ce]), ubar=ubar, p3bar=np.concatenate([Wbar.reshape(-1), delta.sum(axis=0)]))


def _head_torch32(ud, p3d, yd, B, T, n_classes, D):
    """the fp32 expression the trajectory branch of fused_nsde_loss_and_grad ran before this head existed, on the same device tensors"""
    W3, b3 = p3d[: D * n_classes].view(D, n_classes), p3d[D * n_classes:]
    z = torch.addmm(b3, ud, W3).view(T, B, n_classes).mean(dim=0)
    logp = torch.log_softmax(z, dim=1)
    ce = -(yd * logp).sum() / B
    dz = ((torch.exp(logp) * yd.sum(dim=1, keepdim=True) - yd) / (B * T)).repeat(T, 1)
    p3bar = torch.cat([(ud.t() @ dz).reshape(-1), dz.sum(dim=0)])
    ubar = (dz @ W3.t()).contiguous()
    return dict(ce=ce.reshape(1), ubar=ubar, p3bar=p3bar)


@pytest.mark.parametrize("kind,n_classes,B,T", CASES, ids=IDS)
def test_head_against_fp64(kind, n_classes, B, T):
    """Averaged logits within the derived bound (D + T + 3) 2^-24 (sum_t sum_d |W_id u_d,tb| + T |b_i|) / T, which holds for any order of the
    sums (D roundings of the dot product, one of the bias, T - 1 of the trajectory sum, one of the division, and 2 to spare).  ce, u-bar and
    p3-bar go through expf / logf: each one's distance from fp64 is at most four times that of the torch fp32 expression on the same device
    tensors (floor: 4 ulp of the output's largest magnitude).  On the device's own u (the solve of the repeated input), with one-hot labels
    and with labels that are neither one-hot nor sum to 1."""
    c = _case(kind, n_classes, B, T)
    node, D = c["node"], c["D"]
    u = node.forward(np.tile(c["x"], (T, 1)), c["p2"], c["noise"])["u"]
    for what in ("y", "y_soft"):
        got = head_traj(node, u, c["p3"], c[what], B, T, n_classes)
        r64 = _head64(u, c["p3"], c[what], B, T, n_classes, D)
        r32 = _head_torch32(got["u"], got["p3"], got["y"], B, T, n_classes, D)
        z = got["z"].cpu().numpy().astype(np.float64)
        bound = (D + T + 3) * 2.0 ** -24 * r64["zmag"]
        print(f"{kind} C={n_classes} B={B} T={T} {what}: logits |z - z64| max {np.abs(z - r64['z']).max():.3e}, smallest bound {bound.min():.3e}, "
              f"largest ratio {(np.abs(z - r64['z']) / bound).max():.3f}")
        assert (np.abs(z - r64["z"]) <= bound).all()
        for k in ("ce", "ubar", "p3bar"):
            dev = got[k].cpu().numpy().astype(np.float64).reshape(r64[k].shape)
            ref32 = r32[k].cpu().numpy().astype(np.float64).reshape(r64[k].shape)
            d_dev, d_32 = np.abs(dev - r64[k]).max(), np.abs(ref32 - r64[k]).max()
            floor = 4.0 * float(np.spacing(np.float32(np.abs(r64[k]).max())))
            print(f"    {k}: device - fp64 {d_dev:.3e}, torch fp32 - fp64 {d_32:.3e}, floor {floor:.3e}")
            assert np.isfinite(dev).all() and d_dev <= max(4.0 * d_32, floor), (k, d_dev, d_32, floor)
    node.close()


def test_head_at_one_trajectory_agrees_with_the_one_trajectory_head():
    """T = 1: the same formulas as rnde_nsde_classifier_head (one-hot labels: sum_i y_i = 1) -- to rounding, not bit for bit."""
    from regneuralde_jl_amd import _lib
    c = _case("nsde", 10, 37, 1)
    node = c["node"]
    u = node.forward(c["x"], c["p2"], c["noise"])["u"]
    got = head_traj(node, u, c["p3"], c["y"], 37, 1, 10)
    z = torch.empty((37, 10), device="cuda")
    ubar, p3bar, ce = torch.empty_like(got["u"]), torch.empty_like(got["p3"]), torch.empty(1, device="cuda")
    _lib.check_nsde(node.h, node.L.rnde_nsde_classifier_head(node.h, got["u"].data_ptr(), got["p3"].data_ptr(), got["y"].data_ptr(), 37, 10, z.data_ptr(),
                                                             ubar.data_ptr(), p3bar.data_ptr(), ce.data_ptr(), None))
    torch.cuda.synchronize()
    for a, b in ((got["z"], z), (got["ubar"], ubar), (got["p3bar"], p3bar), (got["ce"], ce)):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))
    node.close()


# ---- 2. the one-call step is the composition of its parts, bit for bit ------------------------------------------------------------------------

@pytest.mark.parametrize("kind,n_classes,B,T", CASES, ids=IDS)
def test_grad_traj_is_the_composition_bit_for_bit(kind, n_classes, B, T):
    """rnde_nsde_classifier_grad_traj on x against rnde_nsde_forward (taped) on the explicitly repeated x with the same pool, then
    rnde_nsde_classifier_head_traj, then rnde_nsde_backward: NFE, ce, reg, p2-bar, p3-bar the same bits; x-bar the float32 sum of the
    unfolded cotangent over t = 0 .. T - 1 in that order; and the call repeats itself bit for bit."""
    c = _case(kind, n_classes, B, T)
    node = c["node"]
    one = grad_traj(node, c)
    f = node.forward(np.tile(c["x"], (T, 1)), c["p2"], c["noise"], keep_tape=True)
    hd = head_traj(node, f["u"], c["p3"], c["y"], B, T, n_classes)
    sv = f["saveval"]
    assert len(sv) > 0
    s = 0.0
    for v in sv:                                                   # lambda * mean(saveval), summed in double in the order of the values
        s += float(v)
    reg = np.float32(float(np.float32(LAM)) * s / len(sv))
    svbar = np.full(len(sv), np.float32(LAM) / np.float32(len(sv)), np.float32)
    xb, p2bar = node.backward(hd["ubar"].cpu().numpy(), svbar)
    assert np.array_equal(one["nfe"], [f["nfe1"], f["nfe2"]])
    assert np.array_equal(one["ce"], hd["ce"].cpu().numpy()) and np.isfinite(one["ce"]).all()
    assert one["reg"][0] == reg
    assert np.array_equal(one["p2bar"], p2bar) and np.array_equal(one["p3bar"], hd["p3bar"].cpu().numpy())
    xb3 = xb.reshape(T, B, -1)
    fold = xb3[0].copy()
    for t in range(1, T):
        fold = (fold + xb3[t]).astype(np.float32)
    assert np.array_equal(one["xbar"], fold) and np.isfinite(fold).all() and np.abs(fold).max() > 0
    again = grad_traj(node, c)
    for k in one:
        assert np.array_equal(one[k], again[k]), k
    node.close()


# ---- 3. the evaluation call ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,n_classes,B,T", CASES, ids=IDS)
def test_predict_logits_and_count(kind, n_classes, B, T):
    """Logits: the bits of logits_out of rnde_nsde_classifier_head_traj on the untaped rnde_nsde_forward of the repeated input.  The counter:
    numpy's first-index argmax comparison on the returned logits, and twice that after a second call (it accumulates)."""
    c = _case(kind, n_classes, B, T)
    node = c["node"]
    # labels that agree with the prediction for about half of the inputs, so that the count is neither 0 nor B by construction
    z0 = predict(node, c)[0]
    y = np.eye(n_classes, dtype=np.float32)[np.where(np.arange(B) % 2 == 0, np.argmax(z0, axis=1), (np.argmax(z0, axis=1) + 1) % n_classes)]
    z, nfe, correct = predict(node, c, y=y)
    f = node.forward(np.tile(c["x"], (T, 1)), c["p2"], c["noise"], keep_tape=False)
    hd = head_traj(node, f["u"], c["p3"], y, B, T, n_classes)
    assert np.array_equal(z, hd["z"].cpu().numpy()) and np.isfinite(z).all()
    assert np.array_equal(nfe, [f["nfe1"], f["nfe2"]])
    want = _first_argmax_matches(z, y)
    assert want == (B + 1) // 2
    assert correct.dtype == torch.int64 and int(correct.item()) == want
    predict(node, c, y=y, correct=correct)
    assert int(correct.item()) == 2 * want
    node.close()


def test_ties_take_the_first_index():
    """u = 0, W3 = 0 and a bias whose maximum is repeated: the averaged logits are tied exactly, the predicted class is the FIRST of them
    (Julia's argmax, src/metrics.jl:2), and so is the target of a label column whose maximum is repeated."""
    B, T, n_classes = 5, 3, 4
    c = _case("small", n_classes, B, T)
    node, D = c["node"], c["D"]
    p3 = np.concatenate([np.zeros(n_classes * D), [0.3, 0.7, 0.7, 0.1]]).astype(np.float32)
    hd = head_traj(node, np.zeros((B * T, D), np.float32), p3, c["y"], B, T, n_classes)
    z = hd["z"].cpu().numpy()
    assert np.array_equal(z[:, 1], z[:, 2]) and (np.argmax(z, axis=1) == 1).all() and np.allclose(z, p3[-n_classes:], rtol=1e-6)
    first = np.tile(np.eye(n_classes, dtype=np.float32)[1], (B, 1))
    second = np.tile(np.eye(n_classes, dtype=np.float32)[2], (B, 1))
    tied = np.tile(np.array([0.0, 0.5, 0.5, 0.0], np.float32), (B, 1))           # its first largest entry is class 1
    late = np.tile(np.array([0.0, 0.0, 0.5, 0.5], np.float32), (B, 1))           # class 2
    for y, want in ((first, B), (second, 0), (tied, B), (late, 0)):
        zp, _, correct = predict(node, c, y=y, p3=p3)                             # W3 = 0: the logits are the bias whatever the solve returns
        assert np.array_equal(zp, z)
        assert int(correct.item()) == want == _first_argmax_matches(zp, y)
    node.close()


def test_limits_are_refused_with_a_message_that_names_them():
    from regneuralde_jl_amd import _lib
    c = _case("small", 4, 5, 3, mb=20)
    node = c["node"]

    def refused(call, text, **kw):
        with pytest.raises(_lib.RndeError) as e:
            call(node, {**c, **kw})
        assert e.value.status == _lib.BAD_ARG and text in str(e.value), str(e.value)
    for call in (grad_traj, predict):
        refused(call, "max_batch (20)", T=5)                       # 5 * 5 = 25 columns
        refused(call, "trajectories >= 1", T=0)
        refused(call, "n_classes <= 16", C=17)
        refused(call, "2 <= n_classes", C=1)
    with pytest.raises(_lib.RndeError) as e:
        head_traj(node, np.zeros((25, 3), np.float32), c["p3"], c["y"], 5, 5, 4)
    assert e.value.status == _lib.BAD_ARG and "max_batch (20)" in str(e.value)
    xd = _dev(c["x"])
    n1 = C.c_int64(0)
    st = node.L.rnde_nsde_classifier_predict(node.h, xd.data_ptr(), xd.data_ptr(), xd.data_ptr(), None, 5, 3, 4, 0.0, 1.0, None, 0, 0, xd.data_ptr(),
                                             xd.data_ptr(), C.byref(n1), C.byref(n1), None)
    assert st == _lib.BAD_ARG and b"without y_dev" in node.L.rnde_nsde_last_error(node.h)
    node.close()


# ---- 4. the Python front end -------------------------------------------------------------------------------------------------------------------

def _model(B, T, seed=5, nsde_seed=0, max_batch=None):
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(seed)
    nsde = rn.TrackedNeuralDSDE(rn.Chain(rn.Dense(32, 64, "tanh", g), rn.Dense(64, 32, "identity", g)), rn.Dense(32, 32, "identity", g),
                                [0.0, 1.0], True, "SOSRI", reltol=0.14, abstol=0.14, max_batch=max_batch or B * T, seed=nsde_seed)
    return rn.ClassifierNSDE(rn.Dense(784, 32, "identity", g), nsde, rn.Dense(32, 10, "identity", g)), g


def test_predict_matches_the_layer_call():
    """ClassifierNSDE.predict against model(x, trajectories = T, noise = noise) on the same pool: the same average (atol 1e-6, as
    test_classifier_nsde_trajectories allows for it), the same NFE, no graph.

    The images have ONE lit pixel each, so the pre-layer product x W1 + b1 has a single rounding whatever the order of its sums.  predict runs
    that product on B rows and the layer call on B T rows, and torch's GEMM over K = 784 picks its algorithm by the row count: on dense random
    images its rows differ by 2.0e-6 between 8 and 24 rows (|h| <= 2.2), the solve carries that to 5.7e-6 in u and 2.4e-6 in the logits
    (measured; printed below), which says nothing about the library call.  On the same u the device's averaged logits are 1.1e-7 from fp64, the
    torch expression 4.4e-7."""
    B, T = 8, 3
    model, g = _model(B, T)
    x = torch.zeros(B, 784)
    x[torch.arange(B), torch.randint(0, 784, (B,), generator=g)] = 1.0
    x = x.cuda()
    noise = torch.randn(257, 2, B * T, 32, generator=g).cuda()
    with torch.no_grad():
        z_ref, a, b, _ = model(x, trajectories=T, func="error_est", noise=noise)
    z, n1, n2 = model.predict(x, trajectories=T, noise=noise)
    assert z.shape == (B, 10) and not z.requires_grad and (n1, n2) == (a, b)
    print(f"predict vs layer call, one-pixel images: max |dz| {float((z - z_ref).abs().max()):.3e}")
    assert torch.allclose(z, z_ref, atol=1e-6)
    y = torch.eye(10)[torch.randint(0, 10, (B,), generator=g)].cuda()
    z2, _, _, correct = model.predict(x, trajectories=T, y=y, noise=noise)
    assert torch.equal(z2, z) and correct.dtype == torch.int64 and correct.is_cuda
    assert int(correct.item()) == int((z.argmax(1) == y.argmax(1)).sum())
    xd = torch.rand(B, 784, generator=g).cuda()
    with torch.no_grad():
        zr = model(xd, trajectories=T, func="error_est", noise=noise)[0]
    print(f"predict vs layer call, dense images (torch's pre-layer GEMM differs between {B} and {B * T} rows): max |dz| "
          f"{float((model.predict(xd, trajectories=T, noise=noise)[0] - zr).abs().max()):.3e}")


def test_nsde_accuracy_is_the_host_count_with_one_counter():
    import regneuralde_jl_amd as rn
    B, T = 8, 3
    m1, g = _model(B, T, nsde_seed=41)
    m2, _ = _model(B, T, nsde_seed=41)
    batches = []
    for _ in range(3):
        x = torch.rand(B, 784, generator=g).cuda()
        batches.append((x, torch.eye(10)[torch.randint(0, 10, (B,), generator=g)].cuda()))
    hits = 0
    for x, y in batches:                                           # (the library's noise stream: the same seeds in the same order in both models)
        z = m2.predict(x, trajectories=T)[0]
        hits += int((z.cpu().numpy().argmax(1) == y.cpu().numpy().argmax(1)).sum())
    acc = rn.nsde_accuracy(m1, batches, trajectories=T)
    assert acc == hits / (3 * B)


def test_fused_step_with_trajectories_agrees_with_the_torch_chain(monkeypatch):
    """fused_nsde_loss_and_grad(trajectories = 3) through rnde_nsde_classifier_grad_traj (RNDE_ONE_CALL = 1) against the chain of torch products
    it replaces (RNDE_ONE_CALL = 0) in fresh models with the same seed: the tolerances of test_fused_nsde_step_matches_autograd."""
    import regneuralde_jl_amd as rn
    B, T = 16, 3
    m1, g = _model(B, T, seed=9, nsde_seed=77)
    m2, _ = _model(B, T, seed=9, nsde_seed=77)
    x = torch.rand(B, 784, generator=g).cuda()
    y = torch.eye(10)[torch.randint(0, 10, (B,), generator=g)].cuda()
    monkeypatch.setenv("RNDE_ONE_CALL", "0")
    loss1, ce1, reg1, a1, b1 = rn.fused_nsde_loss_and_grad(m1, x, y, trajectories=T, lam=10.0)
    monkeypatch.setenv("RNDE_ONE_CALL", "1")
    loss2, ce2, reg2, a2, b2 = rn.fused_nsde_loss_and_grad(m2, x, y, trajectories=T, lam=10.0)
    torch.cuda.synchronize()
    assert (a1, b1) == (a2, b2)
    assert abs(float(loss1) - float(loss2)) <= 1e-5 * max(1.0, abs(float(loss1)))
    for p, q in zip(m1.trainable(), m2.trainable()):
        assert torch.allclose(p.grad, q.grad, rtol=1e-4, atol=1e-6 * float(p.grad.abs().max())), float((p.grad - q.grad).abs().max())


# ---- 5. the evaluation size --------------------------------------------------------------------------------------------------------------------

def test_predict_at_the_evaluation_size():
    """B = 512 inputs x 10 trajectories = 5,120 columns (experiments/mnist_nsde.jl:154-155), D = 32, C = 10: finite logits, and the NFE counters
    of rnde_nsde_forward on the explicitly repeated input with the same pool."""
    B, T = 512, 10
    model, g = _model(B, T, seed=6)
    x = torch.rand(B, 784, generator=g).cuda()
    noise = torch.randn(N_POOL, 2, B * T, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    z, n1, n2 = model.predict(x, trajectories=T, noise=noise)
    assert z.shape == (B, 10) and bool(torch.isfinite(z).all())
    with torch.no_grad():
        h = model._dense(x, model.p1, model.pre_shape).repeat(T, 1).contiguous()
        _, a, b, _ = model.nsde(h, model.p2.detach(), noise=noise)
    assert (n1, n2) == (a, b) and n1 > 2


# ---- 6. independence of uninitialised and stale device memory ---------------------------------------------------------------------------------

def test_the_three_calls_on_poisoned_and_on_dirty_workspaces(monkeypatch):
    """As tests/test_gpu_memory_independence.py: the three calls give the same bits on a fresh handle, on a handle created and run under
    RNDE_POISON = 1, and on a handle whose workspaces served a larger, different call before (more columns, more classes, a longer span)."""
    from tests.test_gpu_memory_independence import three_ways
    from tests.test_gpu_nsde import _cfg, _nets
    from tests.util import NsdeNode
    mb = 64
    c = _case("small", 4, 5, 3, mb=mb)
    c["node"].close()
    big = _case("small", 7, 16, 4, seed=977, mb=mb)
    big["node"].close()
    drift, diff = _nets("small")
    make = lambda: NsdeNode(_cfg(drift, diff, mb, max_attempts=127))

    def S(node):
        out = {"g_" + k: v for k, v in grad_traj(node, c, y=c["y_soft"]).items()}
        z, nfe, correct = predict(node, c, y=c["y"])
        out.update(z=z, nfe=nfe, correct=correct)
        f = node.forward(np.tile(c["x"], (c["T"], 1)), c["p2"], c["noise"])
        hd = head_traj(node, f["u"], c["p3"], c["y_soft"], c["B"], c["T"], c["C"])
        out.update({"h_" + k: hd[k] for k in ("z", "ubar", "p3bar", "ce")})
        return out

    def dirty(node):
        grad_traj(node, big, t1=1.25)
        predict(node, big, y=big["y"])

    A = ((mb + 15) // 16) * 4 * 64
    three_ways(monkeypatch, make, S, dirty, 8, (2 * 127 + 8) * 2 * A * 4)


def test_trajectory_workspaces_are_released_with_the_handle():
    """The workspaces of the three calls belong to the handle's owners (csrc/rnde_alloc.h): created, run and destroyed, a handle leaves the
    library's live-allocation counters where they were."""
    import gc
    from regneuralde_jl_amd import _lib
    gc.collect()
    L = _lib.lib()
    before = (int(L.rnde_debug_live_allocs()), int(L.rnde_debug_live_bytes()))
    c = _case("small", 4, 5, 3)
    grad_traj(c["node"], c)
    predict(c["node"], c, y=c["y"])
    during = (int(L.rnde_debug_live_allocs()), int(L.rnde_debug_live_bytes()))
    assert during[0] > before[0] and during[1] > before[1]
    c["node"].close()
    assert (int(L.rnde_debug_live_allocs()), int(L.rnde_debug_live_bytes())) == before

