"""The evaluation passes of the two ODE experiments on the device (include/rnde.h: rnde_node_classifier_predict, rnde_latent_decode_mse;
ClassifierNODE.predict, node_accuracy, latent_total_loss).

Classifier (reference src/metrics.jl:2-18 around src/models/supervised_classification.jl:40-46): the untaped solve is that of
rnde_node_forward(keep_tape = 0) on a second handle of the same config (NFE equal; the end state is compared through the logits, the workspace
is the handle's own), and the logits are the BITS rnde_classifier_head computes from that end state -- on every engine the untaped forward
serves: the stage engine in both matrix modes, the chain engine, the tiled engine (rnde_classifier_head takes a tiled handle: no fallback
to a tolerance was needed).  Every output buffer starts as NaN.
Shapes: B = 1, 17 (no multiple of the 16-column tile), 40 (three tiles); C = 10 (the compile-time instantiation), 2 and 16 (the generic
one, its smallest and its cap).

Latent (reference experiments/latent_ode.jl:271-292): rnde_latent_decode_mse against fp64 numpy with the fp32 torch expression as the
yardstick, latent_total_loss against the torch composition of LatentTimeSeriesModel.__call__ and the masked error."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


# ---- classifier ------------------------------------------------------------------------------------------------------------------------------

def _layer(engine_key, max_batch):
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(11)
    if engine_key in ("stage0", "stage1"):
        dyn = rn.MLPDynamics(784, 100, generator=g)
        return rn.TrackedNeuralODE(dyn, [0.0, 1.0], True, True, "Tsit5", reltol=1e-3, abstol=1e-3, max_batch=max_batch, max_attempts=64,
                                   matrix_mode=int(engine_key[-1]))
    if engine_key == "chain":
        dyn = rn.TDChain(rn.Dense(4, 8, "tanh", g), rn.Dense(9, 3, "tanh", g))
        return rn.TrackedNeuralODE(dyn, [0.0, 1.0], True, True, "Tsit5", reltol=1e-3, abstol=1e-3, max_batch=max_batch, max_attempts=64)
    assert engine_key == "tiled"
    dyn = rn.TDChain(rn.Dense(3, 128, "tanh", g), rn.Dense(129, 128, "tanh", g), rn.Dense(129, 2, "identity", g))
    return rn.TrackedNeuralODE(dyn, [0.0, 1.0], True, True, "Tsit5", reltol=1e-5, abstol=1e-5, max_batch=max_batch, max_attempts=128, engine="tiled",
                               track_ctrl=False, track_initdt=False)


def _handle(layer):
    """a raw C-ABI handle of the layer's config (EEst * dt callback), matrix mode applied"""
    from regneuralde_jl_amd import _lib
    from regneuralde_jl_amd.node import _Handle
    h = _Handle(layer._config(0, "error_est"), layer.engine)
    if layer.matrix_mode is not None:
        _lib.check(h.ptr, _lib.lib().rnde_node_set_matrix_mode(h.ptr, int(layer.matrix_mode)))
    return h


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _predict(h, x, p2, p3, Cn, y=None, correct=None, check=True):
    from regneuralde_jl_amd import _lib
    B = x.shape[0]
    z = _nan(B, Cn)
    nfe = C.c_int64(-1)
    st = _lib.lib().rnde_node_classifier_predict(h.ptr, x.data_ptr(), p2.data_ptr(), p3.data_ptr(), y.data_ptr() if y is not None else None, B, Cn,
                                                 0.0, 1.0, z.data_ptr(), correct.data_ptr() if correct is not None else None, C.byref(nfe), None)
    if check:
        _lib.check(h.ptr, st)
    torch.cuda.synchronize()
    return st, z, int(nfe.value)


def _inputs(engine_key, B, Cn):
    layer = _layer(engine_key, B)
    D = layer.model.dims()[0]
    g = torch.Generator().manual_seed(100 * B + Cn)
    x = torch.rand(B, D, generator=g).cuda()
    p2 = layer.p.cuda()
    lim = math.sqrt(6.0 / (D + Cn))
    p3 = torch.cat([((torch.rand(D, Cn, generator=g) * 2 - 1) * lim).reshape(-1), torch.rand(Cn, generator=g) - 0.5]).cuda()
    return layer, D, x, p2, p3


def _run_case(engine_key, B, Cn):
    """predict without labels on one handle; rnde_node_forward(keep_tape = 0) + rnde_classifier_head on a second one of the same config"""
    from regneuralde_jl_amd import _lib
    L = _lib.lib()
    layer, D, x, p2, p3 = _inputs(engine_key, B, Cn)
    hp, hr = _handle(layer), _handle(layer)
    _, z, nfe = _predict(hp, x, p2, p3, Cn)
    u, nfe_r = _nan(B, D), C.c_int64(-1)
    _lib.check(hr.ptr, L.rnde_node_forward(hr.ptr, x.data_ptr(), p2.data_ptr(), B, 0.0, 1.0, u.data_ptr(), C.byref(nfe_r), None, None, 0, None))
    yy = torch.zeros(B, Cn, device="cuda"); yy[:, 0] = 1.0
    zh, ubar, p3bar, ce = _nan(B, Cn), _nan(B, D), _nan(p3.numel()), _nan(1)
    _lib.check(hr.ptr, L.rnde_classifier_head(hr.ptr, u.data_ptr(), p3.data_ptr(), yy.data_ptr(), B, Cn, zh.data_ptr(), ubar.data_ptr(), p3bar.data_ptr(),
                                              ce.data_ptr(), None))
    torch.cuda.synchronize()
    return dict(layer=layer, hp=hp, hr=hr, x=x, p2=p2, p3=p3, z=z, nfe=nfe, u=u, nfe_ref=int(nfe_r.value), z_head=zh)


_case = functools.lru_cache(maxsize=None)(_run_case)

CASES = [("stage0", 1, 10), ("stage0", 17, 10), ("stage0", 40, 10), ("stage1", 1, 10), ("stage1", 17, 10), ("stage1", 40, 10),
         ("stage0", 17, 2), ("stage0", 17, 16), ("stage1", 17, 2), ("stage1", 17, 16),
         ("chain", 1, 10), ("chain", 17, 10), ("tiled", 17, 10)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


@pytest.mark.parametrize("engine_key,B,Cn", CASES)
def test_solve_is_the_untaped_forward_and_logits_are_the_training_heads_bits(engine_key, B, Cn):
    """Tests 1 and 2 of the issue: NFE equal to rnde_node_forward(keep_tape = 0) on a second handle; the logits, as int32 views, equal to
    rnde_classifier_head's on that forward's end state -- which also pins the internal end state to the forward's (a differing u would have
    to give the same C logits in all B columns)."""
    c = _case(engine_key, B, Cn)
    assert c["nfe"] == c["nfe_ref"] and c["nfe"] > 3, (c["nfe"], c["nfe_ref"])
    assert torch.isfinite(c["u"]).all() and torch.isfinite(c["z"]).all() and torch.isfinite(c["z_head"]).all()
    assert np.array_equal(_bits(c["z"]), _bits(c["z_head"])), float((c["z"] - c["z_head"]).abs().max())
    # and against fp64: the worst-case bound of a 784-term (D-term) fp32 sum, so that both being wrong together would show
    W = c["p3"][:-Cn].view(-1, Cn).double().cpu().numpy(); b = c["p3"][-Cn:].double().cpu().numpy()
    u = c["u"].double().cpu().numpy()
    ref = u @ W + b
    bound = 16 * U * (np.abs(u) @ np.abs(W) + np.abs(b))
    assert (np.abs(c["z"].double().cpu().numpy() - ref) <= bound).all()


def _labels(z, Cn):
    """one-hot at the predicted class (numpy's first argmax) for even b, at (pred + 1) mod C for odd b"""
    pred = z.cpu().numpy().argmax(1)
    B = len(pred)
    cls = np.where(np.arange(B) % 2 == 0, pred, (pred + 1) % Cn)
    y = np.zeros((B, Cn), dtype=np.float32)
    y[np.arange(B), cls] = 1.0
    return torch.from_numpy(y).cuda()


@pytest.mark.parametrize("engine_key,B,Cn", [("stage0", 17, 10), ("stage1", 40, 10), ("stage0", 17, 2), ("stage1", 17, 16), ("chain", 1, 10), ("chain", 17, 10),
                                             ("tiled", 17, 10)])
def test_count_adds_the_first_argmax_matches(engine_key, B, Cn):
    c = _case(engine_key, B, Cn)
    y = _labels(c["z"], Cn)
    correct = torch.zeros(1, dtype=torch.int64, device="cuda")
    _, z1, nfe1 = _predict(c["hp"], c["x"], c["p2"], c["p3"], Cn, y=y, correct=correct)
    assert int(correct.item()) == (B + 1) // 2
    assert nfe1 == c["nfe"] and np.array_equal(_bits(z1), _bits(c["z"]))              # the counting variant writes the same logits
    _predict(c["hp"], c["x"], c["p2"], c["p3"], Cn, y=y, correct=correct)
    assert int(correct.item()) == 2 * ((B + 1) // 2)                                   # ADDED, not stored
    # soft labels: neither one-hot nor normalised
    g = torch.Generator().manual_seed(7 + B)
    ys = (torch.rand(B, Cn, generator=g) * 1.5)
    want = int((c["z"].cpu().numpy().argmax(1) == ys.numpy().argmax(1)).sum())
    soft = torch.zeros(1, dtype=torch.int64, device="cuda")
    _predict(c["hp"], c["x"], c["p2"], c["p3"], Cn, y=ys.cuda(), correct=soft)
    assert int(soft.item()) == want


@pytest.mark.parametrize("engine_key,B,Cn", [("stage0", 17, 10), ("chain", 17, 16)])
def test_ties_take_the_first_index(engine_key, B, Cn):
    layer, D, x, p2, p3 = _inputs(engine_key, B, Cn)
    W = p3[:-Cn].view(D, Cn).clone(); b = p3[-Cn:].clone()
    W[:, 3] = W[:, 1]
    b[1] = b[3] = 50.0                                                                # (the other biases are within 0.5 and W u is of order 1: the bias decides; asserted below)
    p3t = torch.cat([W.reshape(-1), b]).contiguous()
    h = _handle(layer)
    _, z, _ = _predict(h, x, p2, p3t, Cn)
    zn = z.cpu().numpy()
    assert (zn[:, 1] == zn[:, 3]).all() and (zn[:, 1] == zn.max(1)).all()              # the condition: classes 1 and 3 tie for the largest logit
    for cls, want in ((1, B), (3, 0)):
        y = torch.zeros(B, Cn, device="cuda"); y[:, cls] = 1.0
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        _predict(h, x, p2, p3t, Cn, y=y, correct=cnt)
        assert int(cnt.item()) == want, (cls, int(cnt.item()))


def test_without_labels_the_counter_is_untouched_and_a_counter_without_labels_is_refused():
    from regneuralde_jl_amd import _lib
    c = _case("stage1", 17, 10)
    poison = torch.full((4,), 0x5555555555555555, dtype=torch.int64, device="cuda")
    _, z, _ = _predict(c["hp"], c["x"], c["p2"], c["p3"], 10)                           # y = NULL, correct = NULL
    assert np.array_equal(_bits(z), _bits(c["z"])) and (poison == 0x5555555555555555).all()
    st, z2, _ = _predict(c["hp"], c["x"], c["p2"], c["p3"], 10, y=None, correct=poison, check=False)
    assert st == _lib.BAD_ARG and len(_lib.lib().rnde_last_error(c["hp"].ptr)) > 0
    assert (poison == 0x5555555555555555).all() and torch.isnan(z2).all()               # refused before anything was launched
    # the limits, each named by the message
    L = _lib.lib()
    for kw, word in ((dict(B=18), "max_batch"), (dict(Cn=1), "n_classes"), (dict(Cn=17), "n_classes"), (dict(t1=0.0), "t1 > t0")):
        B, Cn, t1 = kw.get("B", 17), kw.get("Cn", 10), kw.get("t1", 1.0)
        nfe = C.c_int64(0)
        st = L.rnde_node_classifier_predict(c["hp"].ptr, c["x"].data_ptr(), c["p2"].data_ptr(), c["p3"].data_ptr(), None, B, Cn, 0.0, t1, z2.data_ptr(), None,
                                            C.byref(nfe), None)
        assert st == _lib.BAD_ARG and word in L.rnde_last_error(c["hp"].ptr).decode(), (kw, L.rnde_last_error(c["hp"].ptr))


def _classifier(B):
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(21)
    node = rn.TrackedNeuralODE(rn.MLPDynamics(784, 100, generator=g), [0.0, 1.0], True, True, "Tsit5", reltol=1e-3, abstol=1e-3, max_batch=B,
                               max_attempts=64)
    post = rn.Dense(784, 10, generator=g)
    post.b = torch.rand(10, generator=g) - 0.5
    return rn.ClassifierNODE(node, post, device="cuda"), g


def test_a_pending_tape_survives_predict():
    import regneuralde_jl_amd as rn
    B = 16
    grads = []
    for with_predict in (False, True):
        model, g = _classifier(B)
        x = torch.rand(B, 784, generator=g).cuda()
        y = torch.eye(10)[torch.randint(0, 10, (B,), generator=g)].cuda()
        loss, _, _, nfe = rn.loss_function(x, y, model, lam=100.0)
        if with_predict:
            z, nfe_p, cnt = model.predict(x)
            assert cnt is None and tuple(z.shape) == (B, 10) and nfe_p > 3 and torch.isfinite(z).all()
        loss.backward()
        torch.cuda.synchronize()
        grads.append((model.p2.grad.clone(), model.p3.grad.clone()))
    for a, b in zip(*grads):
        assert torch.isfinite(a).all() and np.array_equal(_bits(a), _bits(b))


def test_node_accuracy_equals_accuracy_on_ragged_batches():
    import regneuralde_jl_amd as rn
    model, g = _classifier(40)
    batches = []
    for B in (40, 17, 1):
        x = torch.rand(B, 784, generator=g).cuda()
        z, _, _ = model.predict(x)
        batches.append((x, _labels(z, 10)))
        with torch.no_grad():
            zt, _, _ = model(x)
        # the torch GEMM associates differently: the worst-case bound of the D-term fp32 sum on both sides (as test_fused_head_step_matches_autograd allows)
        u, _, _ = model.node(x.reshape(B, -1), model.p2.detach())
        W = model.p3.detach()[:7840].view(784, 10).double(); b = model.p3.detach()[7840:].double()
        bound = 16 * U * (u.double().abs() @ W.abs() + b.abs())
        assert ((z.double() - zt.double()).abs() <= bound).all(), float((z - zt).abs().max())
    want = rn.accuracy(model, batches)
    got = rn.node_accuracy(model, batches)
    assert got == want == (20 + 9 + 1) / 58.0, (got, want)


# ---- latent ------------------------------------------------------------------------------------------------------------------------------------

LATENT_SHAPES = [(1, 1), (3, 5), (17, 49), (5, 64)]


def _latent_case(B, T):
    rng = np.random.default_rng(1000 * B + T)
    x = np.zeros((B, T, 75), dtype=np.float32)
    x[:, :, :37] = rng.standard_normal((B, T, 37))
    x[:, :, 37:74] = rng.uniform(size=(B, T, 37)) < 0.3                                # Bernoulli(0.3)
    x[:, :, 74] = np.abs(rng.standard_normal((B, T))) * 0.02
    x[0, :, 37:74] = 0.0                                                               # sample 0: exactly one observed entry
    x[:, 0, 37] = 1.0                                                                  # entry (0, 0) of every sample observed: none is empty
    lim = np.sqrt(6.0 / 57)
    p4 = np.concatenate([rng.uniform(-lim, lim, 20 * 37), rng.uniform(-0.05, 0.05, 37)]).astype(np.float32)
    res = (0.5 * rng.standard_normal((B, T, 20))).astype(np.float32)
    return x, p4, res


def _mse_fp64(x, p4, res):
    """(mse_b, mag_b) in fp64: latent_ode.jl:281-286, and the same expression over the absolute values of every term, per observed entry"""
    x, p4, res = x.astype(np.float64), p4.astype(np.float64), res.astype(np.float64)
    W, b = p4[:740].reshape(20, 37), p4[740:]
    data, mask = x[:, :, :37], x[:, :, 37:74]
    M = mask.sum((1, 2))
    d = (res @ W + b) * mask - data * mask
    absd = (np.abs(res) @ np.abs(W) + np.abs(b) + np.abs(data)) * mask
    return (d ** 2).sum((1, 2)) / M, (absd ** 2).sum((1, 2)) / M


def _mse_torch32(x, p4, res):
    """the fp32 torch expression of latent_ode.jl:278-286 on the same tensors (the decoder as LatentTimeSeriesModel.__call__ applies it)"""
    xd, pd, rd = (torch.from_numpy(a).cuda() for a in (x, p4, res))
    B, T, _ = x.shape
    result = (rd.reshape(B * T, 20) @ pd[:740].view(20, 37) + pd[740:]).reshape(B, T, 37)
    d, m = xd[:, :, :37], xd[:, :, 37:74]
    return (((result * m - d * m) ** 2).sum(dim=(1, 2)) / m.sum(dim=(1, 2))).double().cpu().numpy()


def _decode_mse(x, p4, res, calls=1):
    from regneuralde_jl_amd import _lib
    L = _lib.lib()
    B, T, _ = x.shape
    h = C.c_void_p()
    cfg = _lib.LatentConfig(max_batch=B, max_T=T, device=0)
    _lib.check_latent(None, L.rnde_latent_create(C.byref(cfg), C.byref(h)))
    xd, pd, rd = (torch.from_numpy(a).cuda() for a in (x, p4, res))
    mse = _nan(B)
    acc = torch.zeros(2, dtype=torch.int64, device="cuda")                               # [sum (fp64) | count (int64)]
    torch.cuda.synchronize()
    for _ in range(calls):
        _lib.check_latent(h, L.rnde_latent_decode_mse(h, rd.data_ptr(), pd.data_ptr(), xd.data_ptr(), B, T, mse.data_ptr(), acc.data_ptr(), acc.data_ptr() + 8, None))
    torch.cuda.synchronize()
    host = acc.cpu()
    out = mse.cpu().numpy(), float(host[:1].view(torch.float64).item()), int(host[1].item())
    # neither accumulator: only mse; one without the other: refused
    m2 = _nan(B)
    _lib.check_latent(h, L.rnde_latent_decode_mse(h, rd.data_ptr(), pd.data_ptr(), xd.data_ptr(), B, T, m2.data_ptr(), None, None, None))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(m2), _bits(mse))
    assert L.rnde_latent_decode_mse(h, rd.data_ptr(), pd.data_ptr(), xd.data_ptr(), B, T, m2.data_ptr(), acc.data_ptr(), None, None) == _lib.BAD_ARG
    assert len(L.rnde_latent_last_error(h)) > 0
    assert L.rnde_latent_decode_mse(h, rd.data_ptr(), pd.data_ptr(), xd.data_ptr(), B + 1, T, m2.data_ptr(), None, None, None) == _lib.BAD_ARG
    L.rnde_latent_destroy(h)
    return out


@functools.lru_cache(maxsize=None)
def _decode_mse_cached(B, T):
    return _decode_mse(*_latent_case(B, T), calls=2)


def _floor(T, mag):
    return (37 * T + 21) * U * mag                                                       # the worst-case summation bound of n = 37 T + 21 fp32 terms


@pytest.mark.parametrize("B,T", LATENT_SHAPES)
def test_decode_mse_against_fp64(B, T):
    """Per sample |device - fp64| <= max(4 |fp32 torch - fp64|, n 2^-24 mag_b), n = 37 T + 21 terms (37 T squared residuals, 20 products and the bias
    of the decoder), mag_b the same expression over the absolute values of every term per observed entry.  Observed on one MI355X: the largest ratio
    of the device's distance to that allowance is 0.003 (shapes (1, 1) and (3, 5); below 0.0005 at (17, 49) and (5, 64)); relative distances from
    fp64 4.1e-8, 1.3e-7, 2.5e-7, 7.2e-8 against 4.1e-8, 4.5e-8, 2.5e-7, 7.2e-8 for the torch expression.  The test prints the figures."""
    x, p4, res = _latent_case(B, T)
    assert (x[0, :, 37:74].sum() == 1) and (x[:, :, 37:74].sum((1, 2)) >= 1).all()
    mse, acc_sum, acc_count = _decode_mse_cached(B, T)
    ref, mag = _mse_fp64(x, p4, res)
    t32 = _mse_torch32(x, p4, res)
    assert np.isfinite(mse).all()
    allow = np.maximum(4 * np.abs(t32 - ref), _floor(T, mag))
    dist = np.abs(mse.astype(np.float64) - ref)
    print(f"decode_mse B={B} T={T}: largest device distance / allowance {float((dist / allow).max()):.3f}; largest relative distance {float((dist / ref).max()):.2e} "
          f"(torch fp32: {float((np.abs(t32 - ref) / ref).max()):.2e})")
    assert (dist <= allow).all(), (dist / allow).max()
    s = 0.0
    for v in mse:
        s += float(v)                                                                    # fp64, increasing b
    assert acc_sum == s + s and acc_count == 2 * B                                       # two calls: exactly twice the index-order sum
    again = _decode_mse(x, p4, res, calls=2)
    assert np.array_equal(again[0].view(np.int32), mse.view(np.int32)) and again[1] == acc_sum and again[2] == acc_count      # the same bits run to run


def test_latent_total_loss_matches_the_torch_composition():
    """Two batches, (17, 49) and (3, 49), explicit eps.  Allowance: test 8's per-sample allowance (4 x its floor) summed over the samples, plus the
    decoder's sensitivity to the saved states' fp32 differences between the two encoders: each side's z0 is within 5e-6 of the largest entry of
    fp64 (tests/test_gpu_latent.py:76, the tolerance stated in its line 6), so the two differ by at most 1e-5 max|z0|; the solve and the tanh
    dynamics carry that to res with the margin of 4 the project uses elsewhere, delta_res = 4e-5 max(|z0|, |res|); the decoder turns it into
    delta_pred <= delta_res max_i sum_j |W_ji|, and mse_b moves by at most (2 sum |d| mask delta_pred + n_obs delta_pred^2) / M_b.
    Observed on one MI355X: |difference| 8.3e-9 at a value of 1.853 against an allowance of 7.2e-3, NFE 33 for both batches on both paths."""
    import regneuralde_jl_amd as rn
    g = torch.Generator().manual_seed(12)
    T = 49
    grid = torch.linspace(0, 1, T)
    model = rn.build_latent_ode(saveat=grid.tolist(), generator=g, reltol=1e-3, abstol=1e-3, max_batch=17, max_attempts=64)
    with torch.no_grad():
        model.p3.mul_(1.5)                                                               # (truncation-dominated regime, as in test_latent_time_series_model_end_to_end)
    batches, epss = [], []
    for B in (17, 3):
        data = torch.randn(B, T, 37, generator=g).cuda()
        mask = (torch.rand(B, T, 37, generator=g) < 0.3).float().cuda()
        mask[:, 0, 0] = 1.0
        t_row = torch.full((B, T, 1), 1.0 / (T - 1)).cuda(); t_row[:, -1] = 0.0
        batches.append((data, mask, t_row))
        epss.append(torch.randn(B, 20, generator=g).cuda())
    got = rn.latent_total_loss(model, batches, eps=epss)
    nfe_dev = list(model.last_eval_nfe)
    got_callable = rn.latent_total_loss(model, [b[:2] for b in batches], t_row=batches[0][2][:1], eps=lambda i: epss[i])
    assert got_callable == got                                                           # (t_row by keyword, eps by callable: the same bits)
    # the torch composition: model.__call__ with the same eps, then latent_ode.jl:281-286
    total, allow, count, nfe_t = 0.0, 0.0, 0, []
    inner = model.node
    seen = {}

    class Spy:
        def __call__(self, z0, p3, **kw):
            res, nfe, sv = inner(z0, p3, **kw)
            seen.update(z0=z0.detach(), res=res.detach())
            return res, nfe, sv
    real_randn = torch.randn
    for (data, mask, t_row), e in zip(batches, epss):
        try:
            torch.randn = lambda *a, **k: e.clone()
            model.node = Spy()
            with torch.no_grad():
                result, _, _, nfe, _ = model(torch.cat([data, mask, t_row], dim=2))
        finally:
            torch.randn = real_randn
            model.node = inner
        nfe_t.append(nfe)
        d64 = (result.double() * mask.double() - data.double() * mask.double())
        M = mask.double().sum(dim=(1, 2))
        total += float(((d64 ** 2).sum(dim=(1, 2)) / M).sum())
        count += data.shape[0]
        W = model.p4.detach()[:740].view(20, 37).double(); b = model.p4.detach()[740:].double()
        res = seen["res"].double()
        absd = (res.abs() @ W.abs() + b.abs() + data.double().abs()) * mask.double()
        floor = (37 * T + 21) * U * (absd ** 2).sum(dim=(1, 2)) / M
        dres = 4e-5 * max(float(seen["z0"].abs().max()), float(res.abs().max()))
        dpred = dres * float(W.abs().sum(dim=0).max())
        sens = (2 * d64.abs().sum(dim=(1, 2)) * dpred + M * dpred ** 2) / M
        allow += float((4 * floor + sens).sum())
    want = total / count
    print(f"latent_total_loss {got:.9g} torch composition {want:.9g} |diff| {abs(got - want):.3e} allowance {allow / count:.3e} nfe {nfe_dev}")
    assert nfe_dev == nfe_t
    assert math.isfinite(got) and abs(got - want) <= allow / count, (got, want, allow / count)


# ---- memory independence ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine_key,B,Cn", [("stage1", 17, 10), ("chain", 17, 10), ("tiled", 17, 10)])
def test_predict_does_not_depend_on_uninitialised_memory(monkeypatch, engine_key, B, Cn):
    from regneuralde_jl_amd import _lib
    L = _lib.lib()
    monkeypatch.delenv("RNDE_POISON", raising=False)
    a = _case(engine_key, B, Cn)
    c0 = int(L.rnde_debug_poison_allocs())
    monkeypatch.setenv("RNDE_POISON", "1")
    b = _run_case(engine_key, B, Cn)                                                     # fresh handles, every allocation filled with NaN bytes
    monkeypatch.delenv("RNDE_POISON")
    assert int(L.rnde_debug_poison_allocs()) > c0
    assert b["nfe"] == a["nfe"] and torch.isfinite(b["z"]).all()
    assert np.array_equal(_bits(b["z"]), _bits(a["z"])) and np.array_equal(_bits(b["z_head"]), _bits(a["z"]))


@pytest.mark.parametrize("B,T", [(3, 5), (17, 49)])
def test_decode_mse_does_not_depend_on_uninitialised_memory(monkeypatch, B, T):
    from regneuralde_jl_amd import _lib
    L = _lib.lib()
    monkeypatch.delenv("RNDE_POISON", raising=False)
    a = _decode_mse_cached(B, T)
    c0 = int(L.rnde_debug_poison_allocs())
    monkeypatch.setenv("RNDE_POISON", "1")
    b = _decode_mse(*_latent_case(B, T), calls=2)
    monkeypatch.delenv("RNDE_POISON")
    assert int(L.rnde_debug_poison_allocs()) > c0
    assert np.isfinite(b[0]).all() and np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and a[1:] == b[1:]
