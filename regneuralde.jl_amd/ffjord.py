"""TrackedFFJORD (reference src/models/ffjord.jl) with the ConcatSquash MLPDynamics of experiments/ffjord_gaussian.jl:48-107, the `solve`
calls replaced by librnde.so (rnde_ffjord_*: one launch per adaptive solve, one per reverse sweep).

    model = MLPDynamics(2, 16)
    ffjord = TrackedFFJORD(model, [0.0, 1.0], True, True, "Tsit5", reltol=1.4e-8, abstol=1.4e-8, max_batch=1024)
    logpx, l1, l2, nfe, sv = ffjord(x)          # x: (B, D) cuda tensor == Julia D x B; sv.saveval: tensor ({true}) or None
    xs = sample(ffjord, 2, nsamples=1024)

    logpx, ke, jn, nfe, _ = ffjord(x, regularize=True)   # {false} layers: the kinetic energy and Jacobian norm rows (RNODE), differentiable

Served: the call methods of ffjord.jl -- TrackedFFJORD{false} with regularize = false or true (the state [z; l; lambda1; lambda2],
d lambda1 / dt = sum f^2, d lambda2 / dt = sum eJ^2, under the same controller) and TrackedFFJORD{true} (EEst * dt saved per accepted
step) -- and sample(), on one of two engines:
    engine="workgroup" (default): the whole batch in one workgroup, widths in_dims + 1 <= 64 and hidden <= 64;
    engine="tiled": one workgroup per 16 columns, layer products on the matrix cores, in_dims <= 64 and hidden <= 112 (the tabular
                    experiment's MLPDynamics(43, 100)), max_batch <= 4096.
The regularize = true rows add two state rows: engine="workgroup" serves them for in_dims + 3 <= 64, engine="tiled" at its own limits.
The default dynamics (dynamics = nothing, ffjord.jl:21-27: Tracker.forward through any Flux model, then back(e)) are served for Dense chains
on engine="tiled": a layers.TDChain with time_dep=True or a layers.Chain (no leading map) with time_dep=False, up to 8 layers, no layer output
and no layer input above 64 (the time row apart), any of the six Dense activations (rnde_ffjord_create_chain):

    model = TDChain(Dense(3, 10, "tanh"), Dense(11, 2))
    ffjord = TrackedFFJORD(model, [0.0, 1.0], True, False, "Tsit5", reltol=1.4e-3, abstol=1.4e-3, engine="tiled")   # p = destructure(model)

Exact trace (an extension: the reference evaluates -tr J only inside sample()): ffjord(x, exact=True) solves [z; l] with dl / dt = -tr J, so
logpx carries no probe and no variance; same 5-tuple, differentiable (the reverse sweep costs about D + 1 Hutchinson ones).  On
engine="tiled" only, without e, and not together with the kinetic rows; loglikelihood(model, batches, exact=True) reports with it.

Tracked step controller (track_ctrl=True; engine="tiled" and regularize=True): the reverse pass differentiates the PI controller as well, as
the reference's Tracker tape does (track_ctrl = 1, track_initdt = 0 of TrackedNeuralODE), so the gradient of the regulariser sum(EEst * dt)
sees dt's dependence on the parameters.  The default (False) treats step sizes and times as constants.

Refused with a message that names the limit: any other dynamics, a chain model on engine="workgroup", and widths above the engine's limit.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from . import layers as _layers

MAX_WIDTH = 64
TILED_MAX_IN, TILED_MAX_HIDDEN, TILED_MAX_BATCH = 64, 112, 4096
ENGINES = ("workgroup", "tiled")
CHAIN_MAX_WIDTH, CHAIN_LDS_BYTES = 64, 160 * 1024


def _glorot(rows, cols, gen):
    """Flux.glorot_uniform(rows, cols): U(-l, l), l = sqrt(6 / (rows + cols))."""
    lim = math.sqrt(6.0 / (rows + cols))
    return (torch.rand(rows, cols, generator=gen, dtype=torch.float64) * 2 - 1).mul_(lim).to(torch.float32)


class ConcatSquashLinear:
    """(W x + b) .* sig(gw t) + (bw t + bb) (ffjord_gaussian.jl:48-82).  Parameters as Flux holds them: W (out, in), b / bw / bb / gw (out,)."""

    def __init__(self, in_dims, out_dims, generator=None):
        self.in_dims, self.out_dims = in_dims, out_dims
        self.W = _glorot(out_dims, in_dims, generator)
        self.b = torch.zeros(out_dims)
        self.bw = _glorot(out_dims, 1, generator).reshape(-1)
        self.bb = torch.zeros(out_dims)
        self.gw = _glorot(out_dims, 1, generator).reshape(-1)

    def param_count(self):
        return self.out_dims * self.in_dims + 4 * self.out_dims

    def flat(self):
        """Flux.destructure order: layer_W (column-major), layer_B, bias_W, bias_B, gate_W."""
        return torch.cat([self.W.t().reshape(-1), self.b, self.bw, self.bb, self.gw])


class MLPDynamics:
    """The experiments' MLPDynamics(in_dims, hsize): ConcatSquashLinear in -> h -> h -> in, softplus between them (ffjord_gaussian.jl:84-96)."""

    def __init__(self, in_dims, hsize, generator=None):
        self.in_dims, self.hidden = in_dims, hsize
        self.layers = [ConcatSquashLinear(in_dims, hsize, generator), ConcatSquashLinear(hsize, hsize, generator),
                       ConcatSquashLinear(hsize, in_dims, generator)]

    def param_count(self):
        return sum(l.param_count() for l in self.layers)

    def destructure(self):
        return torch.cat([l.flat() for l in self.layers]).to(torch.float32).contiguous()


def param_count(in_dims, hidden):
    """Length of Flux.destructure(MLPDynamics(in_dims, hidden)) (from the library when it is built, else the same formula here)."""
    return (hidden * in_dims + 4 * hidden) + (hidden * hidden + 4 * hidden) + (in_dims * hidden + 4 * in_dims)


def is_chain(model):
    """A Dense chain of layers.py: the models the default dynamics (Tracker.forward, then back) are served for."""
    return isinstance(model, (_layers.Chain, _layers.TDChain))


def chain_lds_bytes(dims):
    """LDS bytes of a tile of the chain kernels (rnde_ffjordc.h::FcDyn::lds_floats): padded weights with the t column and bias vectors, the input
    and the probe, every layer's output, two VJP vectors, reduction scratch."""
    pad = lambda n: (n + 15) // 16 * 16
    n = len(dims) - 1
    w = sum(pad(dims[l]) * (pad(dims[l + 1]) + 1) + 2 * pad(dims[l + 1]) for l in range(n))
    mp = max(pad(d) for d in dims)
    return 4 * ((w + 3) // 4 * 4 + 2 * pad(dims[0]) * 16 + sum(pad(dims[l + 1]) * 16 for l in range(n)) + 2 * mp * 16 + 128)


def check_chain_served(model, time_dep, engine="workgroup", kinetic=False):
    """ValueError naming the limit for a Dense-chain model under the default dynamics."""
    if engine != "tiled":
        raise ValueError("TrackedFFJORD: the default forw_n_back (TDChain / Dense dynamics through Tracker.forward) is served on engine=\"tiled\" only; "
                         f"got engine={engine!r}")
    td = isinstance(model, _layers.TDChain)
    if time_dep and not td:
        raise ValueError("TrackedFFJORD: time_dep = true calls m(z, t) inside Tracker.forward, and a Chain takes one argument; pass a TDChain, or "
                         "time_dep=False")
    if td and not time_dep:
        raise ValueError("TrackedFFJORD: a TDChain reads t at every layer; time_dep=False would call it with one argument")
    if getattr(model, "pre_act", False):
        raise ValueError("TrackedFFJORD: a leading element-wise map in front of the Dense chain is not served")
    if not model.layers or len(model.layers) > _lib.MAX_LAYERS:
        raise ValueError(f"TrackedFFJORD chain dynamics: 1..{_lib.MAX_LAYERS} Dense layers; got {len(model.layers)}")
    dims = model.dims()
    for l, lay in enumerate(model.layers):
        if lay.n_in != dims[l] + (1 if td else 0):
            raise ValueError(f"TrackedFFJORD chain dynamics: layer {l + 1} takes {lay.n_in} inputs where the chain hands it {dims[l] + (1 if td else 0)}")
        _layers.act_code(lay.act)
    if dims[0] != dims[-1]:
        raise ValueError(f"TrackedFFJORD chain dynamics: the chain must map {dims[0]} rows to {dims[0]} rows; it ends in {dims[-1]}")
    rows = dims[0] + (3 if kinetic else 1)
    if max(dims) > CHAIN_MAX_WIDTH or rows > CHAIN_MAX_WIDTH:
        raise ValueError(f"TrackedFFJORD chain dynamics: widths above the limit of {CHAIN_MAX_WIDTH} are not served (no layer's output, no layer's "
                         f"input -- its time row apart -- and not the {rows} state rows; got dims = {dims})")
    need = chain_lds_bytes(dims)
    if need > CHAIN_LDS_BYTES:
        raise ValueError(f"TrackedFFJORD chain dynamics: the resident weights and the activations of a tile need {need} bytes of LDS, above the "
                         f"limit of {CHAIN_LDS_BYTES} bytes")


def check_served(model, regularize_kinetic=False, engine="workgroup"):
    """ValueError naming the limit for what the kernels of `engine` do not serve."""
    if engine not in ENGINES:
        raise ValueError(f"TrackedFFJORD: engine must be one of {ENGINES}; got {engine!r}")
    if is_chain(model):
        return check_chain_served(model, isinstance(model, _layers.TDChain), engine, kinetic=bool(regularize_kinetic))
    if not isinstance(model, MLPDynamics):
        raise ValueError("TrackedFFJORD: only the ConcatSquash MLPDynamics of experiments/ffjord_gaussian.jl (dynamics = forw_n_back) is served; "
                         "the default forw_n_back (TDChain / Dense dynamics through Tracker.forward) is not")
    if engine == "workgroup" and (model.in_dims + 1 > MAX_WIDTH or model.hidden > MAX_WIDTH):
        raise ValueError(f"TrackedFFJORD: widths above the chain engine's limit of {MAX_WIDTH} are not served (in_dims + 1 <= 64 and hidden <= 64; "
                         f"got in_dims = {model.in_dims}, hidden = {model.hidden}; engine=\"tiled\" serves wider models)")
    if engine == "tiled" and (model.in_dims > TILED_MAX_IN or model.hidden > TILED_MAX_HIDDEN):
        raise ValueError(f"TrackedFFJORD tiled engine: widths above its LDS limit are not served (in_dims <= {TILED_MAX_IN} and hidden <= "
                         f"{TILED_MAX_HIDDEN}; got in_dims = {model.in_dims}, hidden = {model.hidden})")
    if regularize_kinetic:
        raise ValueError("TrackedFFJORD{false} with regularize = true (kinetic energy and Jacobian norm rows) is not served")


def check_track_ctrl_served(engine, regularize):
    """ValueError naming the reason track_ctrl=True is not served (rnde_ffjord_set_track_ctrl's refusals, before a device is needed)."""
    if engine != "tiled":
        raise ValueError("TrackedFFJORD track_ctrl: the one-workgroup engine does not differentiate the step controller; "
                         f"track_ctrl=True needs engine=\"tiled\" (got engine={engine!r})")
    if not regularize:
        raise ValueError("TrackedFFJORD track_ctrl: a regularize = false layer has no saved value EEst * dt, and without one the tracked and the "
                         "constant-step sweep agree to O(tol) (2e-10 to 2e-6 relative, measured with the fp64 oracle); track_ctrl=True needs "
                         "regularize=True")


def check_kinetic_served(model, engine="workgroup"):
    """ValueError naming the limit for the {false} method's regularize = true rows (kinetic energy, Jacobian norm) on `engine`: the limits
    of check_served with two more state rows."""
    if is_chain(model):
        return check_chain_served(model, isinstance(model, _layers.TDChain), engine, kinetic=True)
    check_served(model, engine=engine)
    if engine == "workgroup" and model.in_dims + 3 > MAX_WIDTH:
        raise ValueError(f"TrackedFFJORD{{false}} with regularize = true (kinetic energy and Jacobian norm rows): the chain engine's limit of "
                         f"{MAX_WIDTH} rows holds in_dims + 3 <= 64 and hidden <= 64 (got in_dims = {model.in_dims}, hidden = {model.hidden}; "
                         f"engine=\"tiled\" serves in_dims <= {TILED_MAX_IN} and hidden <= {TILED_MAX_HIDDEN})")


class SavedValues:
    def __init__(self, saveval):
        self.saveval = saveval


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _Handle:
    """One rnde_ffjord handle.  A handle holds ONE tape: `gen` counts the taped forwards run on it, `busy` is set while a taped forward
    waits for its backward (or for its graph to be dropped)."""

    def __init__(self, cfg, engine="workgroup", track_ctrl=False):
        self.h = C.c_void_p()
        if isinstance(cfg, _lib.FfjordChainConfig):
            create = _lib.lib().rnde_ffjord_create_chain
        else:
            create = _lib.lib().rnde_ffjord_create_tiled if engine == "tiled" else _lib.lib().rnde_ffjord_create
        _lib.check_ffjord(None, create(C.byref(cfg), C.byref(self.h)))
        self.gen, self.busy = 0, False
        if track_ctrl:
            _lib.check_ffjord(self.h, _lib.lib().rnde_ffjord_set_track_ctrl(self.h, 1))

    def __del__(self):
        try:
            if self.h:
                _lib.lib().rnde_ffjord_destroy(self.h)
        except Exception:
            pass


class _TapeToken:
    """Lifetime of one taped forward: it lives in the autograd node's ctx and hands its handle back to the layer's pool after the backward
    pass, or when the graph is dropped without one (an inference call with tracking on)."""

    def __init__(self, hd):
        self.hd, self.gen, self.done = hd, hd.gen, False

    def finish(self):
        if not self.done:
            self.done = True
            self.hd.busy = False

    def __del__(self):
        try:
            self.finish()
        except Exception:
            pass


MAX_TAPES = 4     # taped forwards that may wait for their backward at the same time, per layer


class _Solve(torch.autograd.Function):
    """The {false} / {true} forward and its reverse.  e = None: the exact-trace forward (rnde_ffjord_forward_exact / _replay, no probe); the tape
    remembers that it is exact, so the reverse pass is the same call of rnde_ffjord_backward."""

    @staticmethod
    def forward(ctx, x, p, e, layer, t0, t1, steps, keep):
        L = _lib.lib()
        hd = layer._taped_handle() if keep else layer._handle()
        h = hd.h
        B = x.shape[0]
        logpx = torch.empty(B, device=x.device, dtype=torch.float32)
        nfe = C.c_int64()
        sv = (C.c_float * (layer.max_attempts + 1))()
        nsv = C.c_int32()
        if keep:
            hd.busy, hd.gen = True, hd.gen + 1
        arr = None if steps is None else (C.c_float * len(steps))(*steps)
        if e is None and steps is None:
            st = L.rnde_ffjord_forward_exact(h, x.data_ptr(), p.data_ptr(), B, t0, t1, logpx.data_ptr(), None, C.byref(nfe), sv, C.byref(nsv), keep,
                                             _stream(x.device))
        elif e is None:
            st = L.rnde_ffjord_forward_exact_replay(h, x.data_ptr(), p.data_ptr(), B, t0, t1, arr, len(steps) // 2, logpx.data_ptr(), None,
                                                    C.byref(nfe), sv, C.byref(nsv), keep, _stream(x.device))
        elif steps is None:
            st = L.rnde_ffjord_forward(h, x.data_ptr(), p.data_ptr(), e.data_ptr(), B, t0, t1, 0, logpx.data_ptr(), None, C.byref(nfe), sv, C.byref(nsv),
                                       keep, _stream(x.device))
        else:
            st = L.rnde_ffjord_forward_replay(h, x.data_ptr(), p.data_ptr(), e.data_ptr(), B, t0, t1, 0, arr, len(steps) // 2, logpx.data_ptr(), None,
                                              C.byref(nfe), sv, C.byref(nsv), keep, _stream(x.device))
        layer._last = hd
        if st != _lib.OK:
            hd.busy = False
            _lib.check_ffjord(h, st)
        ctx.layer, ctx.nsv = layer, nsv.value
        ctx.token = _TapeToken(hd) if keep else None
        ctx.save_for_backward(x, p, e)
        layer.last_nfe = int(nfe.value)
        saveval = torch.tensor(list(sv[:nsv.value]), dtype=torch.float32, device=x.device)
        return logpx, saveval

    @staticmethod
    def backward(ctx, g_logpx, g_sv):
        x, p, e = ctx.saved_tensors
        tok = ctx.token
        if tok is None:
            raise RuntimeError("TrackedFFJORD: this forward was not taped (it ran with grad disabled or with no input requiring grad)")
        if tok.done or tok.hd.gen != tok.gen:
            raise RuntimeError("TrackedFFJORD: the tape of this forward has been released (a second backward through the same graph)")
        L, h = _lib.lib(), tok.hd.h
        g_logpx = (torch.zeros(x.shape[0], device=x.device) if g_logpx is None else g_logpx).contiguous().float()
        svb = None
        if g_sv is not None and ctx.nsv:
            svb = (C.c_float * ctx.nsv)(*g_sv.detach().float().cpu().tolist())
        pb = torch.empty_like(p)
        xb = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        st = L.rnde_ffjord_backward(h, g_logpx.data_ptr(), svb, pb.data_ptr(), xb.data_ptr() if xb is not None else None, _stream(x.device))
        ctx.layer._last_bwd = tok.hd
        tok.finish()
        _lib.check_ffjord(h, st)
        return xb, pb, None, None, None, None, None, None


class _SolveKinetic(torch.autograd.Function):
    """The {false} method called with regularize = true: (logpx, lambda1, lambda2) from one solve over D + 3 rows, one reverse sweep for all
    three cotangents.  Shares the layer's tape pool with _Solve."""

    @staticmethod
    def forward(ctx, x, p, e, layer, t0, t1, steps, keep):
        L = _lib.lib()
        hd = layer._taped_handle() if keep else layer._handle()
        h = hd.h
        B = x.shape[0]
        logpx = torch.empty(B, device=x.device, dtype=torch.float32)
        reg = torch.empty(2, B, device=x.device, dtype=torch.float32)
        nfe = C.c_int64()
        if keep:
            hd.busy, hd.gen = True, hd.gen + 1
        if steps is None:
            st = L.rnde_ffjord_forward_kinetic(h, x.data_ptr(), p.data_ptr(), e.data_ptr(), B, t0, t1, 0, logpx.data_ptr(), reg.data_ptr(), None,
                                               C.byref(nfe), keep, _stream(x.device))
        else:
            arr = (C.c_float * len(steps))(*steps)
            st = L.rnde_ffjord_forward_kinetic_replay(h, x.data_ptr(), p.data_ptr(), e.data_ptr(), B, t0, t1, 0, arr, len(steps) // 2,
                                                      logpx.data_ptr(), reg.data_ptr(), None, C.byref(nfe), keep, _stream(x.device))
        layer._last = hd
        if st != _lib.OK:
            hd.busy = False
            _lib.check_ffjord(h, st)
        ctx.layer = layer
        ctx.token = _TapeToken(hd) if keep else None
        ctx.save_for_backward(x, p, e)
        layer.last_nfe = int(nfe.value)
        return logpx, reg[0].clone(), reg[1].clone()

    @staticmethod
    def backward(ctx, g_logpx, g_l1, g_l2):
        x, p, e = ctx.saved_tensors
        tok = ctx.token
        if tok is None:
            raise RuntimeError("TrackedFFJORD: this forward was not taped (it ran with grad disabled or with no input requiring grad)")
        if tok.done or tok.hd.gen != tok.gen:
            raise RuntimeError("TrackedFFJORD: the tape of this forward has been released (a second backward through the same graph)")
        L, h, B = _lib.lib(), tok.hd.h, x.shape[0]
        zeros = lambda: torch.zeros(B, device=x.device)                    # (an unused output's None gradient counts as zeros)
        g_logpx = (zeros() if g_logpx is None else g_logpx).contiguous().float()
        gr = torch.stack([zeros() if g is None else g.float() for g in (g_l1, g_l2)]).contiguous()
        pb = torch.empty_like(p)
        xb = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        st = L.rnde_ffjord_backward_kinetic(h, g_logpx.data_ptr(), gr.data_ptr(), pb.data_ptr(), xb.data_ptr() if xb is not None else None,
                                            _stream(x.device))
        ctx.layer._last_bwd = tok.hd
        tok.finish()
        _lib.check_ffjord(h, st)
        return xb, pb, None, None, None, None, None, None


class TrackedFFJORD:
    """TrackedFFJORD(model, tspan, time_dep, regularize, solver; reltol, abstol, ...) (ffjord.jl:1-51).  regularize selects the call
    method: False -> TrackedFFJORD{false} (returns logpx, 0, 0, nfe, None; called with regularize=True: logpx, lambda1, lambda2, nfe, None with
    the kinetic energy and the Jacobian norm rows, differentiable), True -> TrackedFFJORD{true} (returns logpx, 0, 0, nfe, sv with
    sv.saveval = EEst * dt per accepted step, differentiable).  Called with exact=True (engine="tiled"; no e, no kinetic rows): the same
    5-tuple with logpx from the exact trace -tr J instead of the Hutchinson estimate, differentiable.  engine: "workgroup" (default) or "tiled" (see the module docstring).
    track_ctrl=True (engine="tiled", regularize=True): the reverse pass differentiates the step controller too (every handle of the layer)."""

    def __init__(self, model, tspan, time_dep, regularize, solver="Tsit5", *, reltol=1.4e-8, abstol=1.4e-8, max_batch=1024, max_attempts=4096,
                 cb_save_start=True, device=0, dynamics=None, engine="workgroup", track_ctrl=False, **kwargs):
        if dynamics is not None and dynamics != "forw_n_back":
            raise ValueError("TrackedFFJORD: only dynamics = forw_n_back of the ConcatSquash MLPDynamics is served")
        self.chain = is_chain(model)
        if self.chain:
            if engine not in ENGINES:
                raise ValueError(f"TrackedFFJORD: engine must be one of {ENGINES}; got {engine!r}")
            if dynamics is not None:
                raise ValueError("TrackedFFJORD: dynamics = forw_n_back is the ConcatSquash MLPDynamics' own VJP; a Dense chain goes through the "
                                 "default dynamics (dynamics=None)")
            check_chain_served(model, bool(time_dep), engine)
        else:
            check_served(model, engine=engine)
        if engine == "tiled" and int(max_batch) > TILED_MAX_BATCH:
            raise ValueError(f"TrackedFFJORD tiled engine: max_batch above {TILED_MAX_BATCH} is not served (one meeting holds 256 resident tiles)")
        self.engine = engine
        if track_ctrl:
            check_track_ctrl_served(engine, bool(regularize))
        self.track_ctrl = bool(track_ctrl)
        if solver != "Tsit5":
            raise ValueError("TrackedFFJORD: only Tsit5 is served")
        self.model, self.tspan, self.time_dep, self.regularize = model, (float(tspan[0]), float(tspan[1])), bool(time_dep), bool(regularize)
        self.reltol, self.abstol, self.max_batch, self.max_attempts = float(reltol), float(abstol), int(max_batch), int(max_attempts)
        self.cb_save_start, self.device = bool(cb_save_start), int(device)
        self.in_dims = model.dims()[0] if self.chain else model.in_dims
        self.p = (_layers.destructure(model) if self.chain else model.destructure()).cuda(self.device)
        self.n_params = self.p.numel()
        self._h = None          # untaped calls: inference, sample, steps of those, feval
        self._pool = []         # handles for taped forwards (one tape each)
        self._last = self._last_bwd = None
        self.last_nfe = 0
        self._seed = 0x5EED

    def config(self):
        if self.chain:
            cfg, dims = _lib.FfjordChainConfig(), self.model.dims()
            cfg.n_layers = len(self.model.layers)
            for i, d in enumerate(dims):
                cfg.dims[i] = d
            for i, l in enumerate(self.model.layers):
                cfg.act[i] = _layers.act_code(l.act)
            cfg.time_dep, cfg.regularize, cfg.max_batch, cfg.solver = int(self.time_dep), int(self.regularize), self.max_batch, 0
            cfg.reltol, cfg.abstol, cfg.cb_save_start, cfg.max_attempts, cfg.device = self.reltol, self.abstol, int(self.cb_save_start), self.max_attempts, self.device
            return cfg
        cfg = _lib.FfjordConfig()
        cfg.in_dims, cfg.hidden, cfg.dynamics, cfg.time_dep = self.in_dims, self.model.hidden, 0, int(self.time_dep)
        cfg.regularize, cfg.kinetic_reg, cfg.max_batch, cfg.solver = int(self.regularize), 0, self.max_batch, 0
        cfg.reltol, cfg.abstol, cfg.cb_save_start, cfg.max_attempts, cfg.device = self.reltol, self.abstol, int(self.cb_save_start), self.max_attempts, self.device
        return cfg

    def _handle(self):
        if self._h is None:
            self._h = _Handle(self.config(), self.engine, self.track_ctrl)
        return self._h

    def _taped_handle(self):
        for hd in self._pool:
            if not hd.busy:
                return hd
        if len(self._pool) >= MAX_TAPES:
            raise RuntimeError(f"TrackedFFJORD: {MAX_TAPES} taped forwards are waiting for their backward pass; run backward (or drop the graphs) "
                               "before taping more")
        self._pool.append(_Handle(self.config(), self.engine, self.track_ctrl))
        return self._pool[-1]

    def _fused_handle(self):
        """The handle of fused_ffjord_loss_and_grad: its own, so that a one-call step leaves the tape pool and the untaped handle alone."""
        if getattr(self, "_fh", None) is None:
            self._fh = _Handle(self.config(), self.engine, self.track_ctrl)
        return self._fh

    def draw_normal(self, rows, cols, device):
        """(cols, rows) standard normals from the library's stream (a fresh seed per call: the reference's CUDA.randn default argument)."""
        out = torch.empty(cols, rows, device=device, dtype=torch.float32)
        self._seed += 1
        _lib.check(None, _lib.lib().rnde_normal_fill(out.data_ptr(), out.numel(), self._seed, 0x46464A4F, _stream(device)))
        return out

    def __call__(self, x, p=None, e=None, regularize=False, steps=None, exact=False):
        kinetic = bool(regularize) and not self.regularize      # ({true} never passes the keyword on: ffjord.jl:119)
        if exact:
            if e is not None:
                raise ValueError("TrackedFFJORD: exact=True evaluates -tr J and takes no probe; call it without e")
            if kinetic:
                raise ValueError("TrackedFFJORD: exact=True together with regularize=True on a {false} layer (kinetic energy and Jacobian norm "
                                 "rows) is not served: the Jacobian norm row is defined on the probe")
            if self.engine != "tiled":
                raise ValueError("TrackedFFJORD: exact=True is served on engine=\"tiled\" only (the tiled engine's solve and reverse sweep); "
                                 f"got engine={self.engine!r}")
        if kinetic:
            check_kinetic_served(self.model, self.engine)
        p = self.p if p is None else p
        if not (x.is_cuda and p.is_cuda):
            raise RuntimeError("TrackedFFJORD runs on the device only: x and p must be cuda tensors")
        x = x.contiguous().float()
        if x.dim() != 2 or x.shape[1] != self.in_dims:
            raise ValueError(f"x must be (B, {self.in_dims})")
        if exact:
            p = p.contiguous()
            if p.numel() != self.n_params:
                raise ValueError(f"p must hold {self.n_params} parameters; got {p.numel()}")
            keep = torch.is_grad_enabled() and (x.requires_grad or p.requires_grad)
            logpx, saveval = _Solve.apply(x, p, None, self, self.tspan[0], self.tspan[1], steps, keep)
            zero = torch.zeros(x.shape[0], device=x.device)
            return logpx, zero, zero, self.last_nfe, (SavedValues(saveval) if self.regularize else None)
        if e is None:
            e = self.draw_normal(self.in_dims, x.shape[0], x.device)
        elif tuple(e.shape) != tuple(x.shape) or not e.is_cuda:
            raise ValueError(f"e must be a cuda tensor of x's shape {tuple(x.shape)} (B, D); got {tuple(e.shape)}")
        e = e.contiguous().float()
        p = p.contiguous()
        if p.numel() != self.n_params:
            raise ValueError(f"p must hold {self.n_params} parameters; got {p.numel()}")
        # tape only when a gradient can be asked for: an inference call must not occupy (or replace) a tape
        keep = torch.is_grad_enabled() and (x.requires_grad or p.requires_grad)
        if kinetic:
            logpx, l1, l2 = _SolveKinetic.apply(x, p, e, self, self.tspan[0], self.tspan[1], steps, keep)
            return logpx, l1, l2, self.last_nfe, None
        logpx, saveval = _Solve.apply(x, p, e, self, self.tspan[0], self.tspan[1], steps, keep)
        zero = torch.zeros(x.shape[0], device=x.device)
        return logpx, zero, zero, self.last_nfe, (SavedValues(saveval) if self.regularize else None)

    # ---- several batches per launch (rnde_ffjord_reserve_groups / rnde_ffjord_forward_groups; engine="tiled") ----
    def reserve_groups(self, max_groups, max_columns):
        """Capacity of the untaped handle for group calls of up to max_groups batches and ceil(max_columns / 16) tiles; (0, 0) releases it.
        The library's message (RndeError) when the device does not hold that many tiles or the engine has none."""
        h = self._handle().h
        _lib.check_ffjord(h, _lib.lib().rnde_ffjord_reserve_groups(h, int(max_groups), int(max_columns)))

    def group_capacity(self):
        """(max_groups, max_columns) of the untaped handle; (0, 0) without a reservation."""
        a, b = C.c_int32(), C.c_int32()
        h = self._handle().h
        _lib.check_ffjord(h, _lib.lib().rnde_ffjord_group_capacity(h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _grow_groups(self, n_groups, sizes):
        """The reservation a call of these batches needs: every batch its own tiles.  Grows, never shrinks."""
        need_g, need_c = n_groups, 16 * sum((b + 15) // 16 for b in sizes)
        have_g, have_c = self.group_capacity()
        if need_g > have_g or need_c > have_c:
            self.reserve_groups(max(need_g, have_g), max(need_c, have_c))

    @torch.no_grad()
    def _forward_groups(self, xs, p, es, exact, acc=None):
        """One group call: logpx (sum B,), the NFEs.  acc: a (2,) float64 cuda tensor whose first entry takes the sum of logpx and whose
        second, read as an int64, the column count (the library's sum_dev / count_dev)."""
        p = (self.p if p is None else p).contiguous()
        if p.numel() != self.n_params or not p.is_cuda:
            raise ValueError(f"p must be a cuda tensor of {self.n_params} parameters")
        sizes = [int(x.shape[0]) for x in xs]
        for x in xs:
            if not x.is_cuda or x.dim() != 2 or x.shape[1] != self.in_dims:
                raise ValueError(f"every batch must be a cuda tensor of shape (B, {self.in_dims})")
        dev = xs[0].device
        x = torch.cat([x.float() for x in xs]).contiguous()
        e = None
        if not exact:
            for x_g, e_g in zip(xs, es):
                if tuple(e_g.shape) != tuple(x_g.shape) or not e_g.is_cuda:
                    raise ValueError(f"every probe must be a cuda tensor of its batch's shape; got {tuple(e_g.shape)} for {tuple(x_g.shape)}")
            e = torch.cat([v.float() for v in es]).contiguous()
        self._grow_groups(len(xs), sizes)
        hd = self._handle()
        n = len(xs)
        logpx = torch.empty(x.shape[0], device=dev, dtype=torch.float32)
        Bs, nfe, st = (C.c_int32 * n)(*sizes), (C.c_int64 * n)(), (C.c_int32 * n)()
        sum_ptr = acc.data_ptr() if acc is not None else None
        cnt_ptr = acc.data_ptr() + 8 if acc is not None else None
        rc = _lib.lib().rnde_ffjord_forward_groups(hd.h, x.data_ptr(), p.data_ptr(), e.data_ptr() if e is not None else None, n, Bs, self.tspan[0],
                                                  self.tspan[1], int(bool(exact)), logpx.data_ptr(), nfe, st, sum_ptr, cnt_ptr, _stream(dev))
        self.last_group_status = list(st)
        _lib.check_ffjord(hd.h, rc)
        return logpx, [int(v) for v in nfe]

    def logpx_batches(self, xs, p=None, es=None, exact=False):
        """logpx of several independent batches from ONE launch: xs a list of (B_g, D) cuda tensors -> (list of logpx tensors, list of NFEs),
        each bit for bit what self(x_g, p, e_g)[0] gives for that batch alone.  es=None draws the probes with draw_normal per batch, in
        order, so a seeded layer gives the probes the loop over single calls gives.  exact=True: the exact trace, no probes.  Untaped."""
        if self.engine != "tiled":
            raise ValueError(f"TrackedFFJORD: several batches per launch are served on engine=\"tiled\" only; got engine={self.engine!r}")
        xs = list(xs)
        if not xs:
            return [], []
        if exact and es is not None:
            raise ValueError("TrackedFFJORD: exact=True evaluates -tr J and takes no probes; call it without es")
        if not exact:
            es = [self.draw_normal(self.in_dims, x.shape[0], x.device) for x in xs] if es is None else list(es)
            if len(es) != len(xs):
                raise ValueError(f"es must hold one probe per batch; got {len(es)} for {len(xs)} batches")
        logpx, nfe = self._forward_groups(xs, p, es, exact)
        self.last_nfe = nfe[-1]
        return list(torch.split(logpx, [int(x.shape[0]) for x in xs])), nfe

    def group_steps(self, g):
        """[(dt, accepted), ...] of every attempt of group g of the last group call (rnde_ffjord_group_steps), flattened."""
        h, n = self._handle().h, C.c_int32()
        _lib.check_ffjord(h, _lib.lib().rnde_ffjord_group_steps(h, int(g), None, 0, C.byref(n)))
        arr = (C.c_float * max(2 * n.value, 1))()
        _lib.check_ffjord(h, _lib.lib().rnde_ffjord_group_steps(h, int(g), arr, n.value, C.byref(n)))
        return list(arr[:2 * n.value])

    def steps(self):
        """[(dt, accepted), ...] of every attempt of the last solve (rnde_ffjord_steps), flattened."""
        h, n = (self._last or self._handle()).h, C.c_int32()
        _lib.check_ffjord(h, _lib.lib().rnde_ffjord_steps(h, None, 0, C.byref(n)))
        arr = (C.c_float * max(2 * n.value, 1))()
        _lib.check_ffjord(h, _lib.lib().rnde_ffjord_steps(h, arr, n.value, C.byref(n)))
        return list(arr[:2 * n.value])

    def step_log(self):
        """(n, 4) array of (t, dt, EEst, accepted) per attempt of the last solve (rnde_ffjord_step_log)."""
        h, n = (self._last or self._handle()).h, C.c_int32()
        _lib.check_ffjord(h, _lib.lib().rnde_ffjord_step_log(h, None, 0, C.byref(n)))
        arr = (C.c_float * max(4 * n.value, 1))()
        _lib.check_ffjord(h, _lib.lib().rnde_ffjord_step_log(h, arr, n.value, C.byref(n)))
        return np.array(arr[:4 * n.value], dtype=np.float32).reshape(-1, 4)

    def timing(self):
        """(solve ms, attempts, accepted) of the last solve and the reverse ms of the last backward (HIP events): (solve, reverse, n, m)."""
        a, b, n, m = C.c_float(), C.c_float(), C.c_int32(), C.c_int32()
        h = (self._last or self._handle()).h
        _lib.check_ffjord(h, _lib.lib().rnde_ffjord_timing(h, C.byref(a), None, C.byref(n), C.byref(m)))
        if self._last_bwd is not None:
            _lib.check_ffjord(self._last_bwd.h, _lib.lib().rnde_ffjord_timing(self._last_bwd.h, None, C.byref(b), None, None))
        return a.value, (b.value if self._last_bwd is not None else -1.0), n.value, m.value

    def feval(self, x, t, e=None, p=None, regularize=False):
        """[f(x, t); -e . eJ] as (B, D + 1) (e = None: the exact trace); regularize=True: [f; -e . eJ; sum f^2; sum eJ^2] as (B, D + 3)."""
        p = self.p if p is None else p
        if regularize:
            check_kinetic_served(self.model, self.engine)
            if e is None or x.dim() != 2 or x.shape[1] != self.in_dims or tuple(e.shape) != tuple(x.shape):
                raise ValueError(f"x and e must be (B, {self.in_dims}) (the kinetic rows use the Hutchinson probe)")
            h = self._handle().h
            out = torch.empty(x.shape[0], self.in_dims + 3, device=x.device)
            _lib.check_ffjord(h, _lib.lib().rnde_ffjord_debug_feval_kinetic(h, x.contiguous().data_ptr(), p.contiguous().data_ptr(),
                                                                            e.contiguous().data_ptr(), x.shape[0], float(t), out.data_ptr(),
                                                                            _stream(x.device)))
            return out
        if x.dim() != 2 or x.shape[1] != self.in_dims or (e is not None and tuple(e.shape) != tuple(x.shape)):
            raise ValueError(f"x and e must be (B, {self.in_dims})")
        h = self._handle().h
        out = torch.empty(x.shape[0], self.in_dims + 1, device=x.device)
        _lib.check_ffjord(h, _lib.lib().rnde_ffjord_debug_feval(h, x.contiguous().data_ptr(), p.contiguous().data_ptr(),
                                                                e.contiguous().data_ptr() if e is not None else None, x.shape[0], float(t),
                                                                int(e is None), out.data_ptr(), _stream(x.device)))
        return out


def check_one_call_served(ff, e, lam_r, kinetic, exact):
    """ValueError naming the reason for what rnde_ffjord_nll_grad would refuse (before a device is needed)."""
    if exact and ff.engine != "tiled":
        raise ValueError("fused_ffjord_loss_and_grad: exact=True is served on engine=\"tiled\" only (the tiled engine's solve and reverse sweep); "
                         f"got engine={ff.engine!r}")
    if exact and e is not None:
        raise ValueError("fused_ffjord_loss_and_grad: exact=True evaluates -tr J and takes no probe; call it without e")
    if kinetic is not None:
        if ff.regularize:
            raise ValueError("fused_ffjord_loss_and_grad: kinetic=(lam_k, lam_j) weighs the kinetic energy and Jacobian norm rows, which a "
                             "regularize=True layer ({true}) does not have: its method never passes regularize on (ffjord.jl:119)")
        if exact:
            raise ValueError("fused_ffjord_loss_and_grad: exact=True together with the kinetic rows is not served: the Jacobian norm row is "
                             "defined on the probe")
        if len(kinetic) != 2:
            raise ValueError("fused_ffjord_loss_and_grad: kinetic is None or the pair (lam_k, lam_j)")
        check_kinetic_served(ff.model, ff.engine)
    if float(lam_r) != 0.0 and not ff.regularize:
        raise ValueError("fused_ffjord_loss_and_grad: lam_r weighs the saved values EEst * dt, which a regularize=False layer ({false}) does not "
                         "have; lam_r must be 0 there")


def fused_ffjord_loss_and_grad(ff, x, p=None, e=None, lam_r=0.0, kinetic=None, exact=False, need_x_grad=False):
    """The gradient of the experiments' loss_function (ffjord_tabular.jl:143-147, ffjord_gaussian.jl:142-146) in ONE library call,
    rnde_ffjord_nll_grad: the taped solve, the loss terms and the reverse sweep's seeds on the device, the reverse sweep -- no torch loss, no
    autograd, no read-back of the cotangents.

        loss = -mean(logpx) + lam_r * mean(sv.saveval) + lam_k * mean(lambda1) + lam_j * mean(lambda2)

    lam_r: {true} layers; kinetic=(lam_k, lam_j): the {false} method's regularize = true rows; exact=True: the exact trace (engine="tiled", no
    e).  e=None: the library's probe draw (a fresh seed per call).  Sets p.grad (and x.grad with need_x_grad=True); returns
    (nll, reg, lam1_mean, lam2_mean, nfe): nll and the two means are 0-dim device tensors that are not read back, reg = lam_r * mean(saveval)
    is the host float the library computes from the step log.  Runs on one handle of its own (ff._fused_handle()): the autograd tape pool
    and the handle of the untaped calls are not touched."""
    check_one_call_served(ff, e, lam_r, kinetic, exact)
    p = ff.p if p is None else p
    if not (x.is_cuda and p.is_cuda):
        raise RuntimeError("fused_ffjord_loss_and_grad runs on the device only: x and p must be cuda tensors")
    xd = x.detach().contiguous().float()
    if xd.dim() != 2 or xd.shape[1] != ff.in_dims:
        raise ValueError(f"x must be (B, {ff.in_dims})")
    pd = p.detach().contiguous()
    if pd.numel() != ff.n_params:
        raise ValueError(f"p must hold {ff.n_params} parameters; got {pd.numel()}")
    if e is not None:
        if tuple(e.shape) != tuple(xd.shape) or not e.is_cuda:
            raise ValueError(f"e must be a cuda tensor of x's shape {tuple(xd.shape)} (B, D); got {tuple(e.shape)}")
        e = e.detach().contiguous().float()
    hd = ff._fused_handle()
    mode = 1 if exact else (2 if kinetic is not None else 0)
    lam_k, lam_j = (float(kinetic[0]), float(kinetic[1])) if kinetic is not None else (0.0, 0.0)
    pb = torch.empty_like(pd)
    xb = torch.empty_like(xd) if need_x_grad else None
    terms = torch.empty(3, device=xd.device, dtype=torch.float32)
    reg, nfe = C.c_float(), C.c_int64()
    ff._seed += 1
    st = _lib.lib().rnde_ffjord_nll_grad(hd.h, xd.data_ptr(), pd.data_ptr(), e.data_ptr() if e is not None else None, xd.shape[0], ff.tspan[0],
                                         ff.tspan[1], ff._seed, mode, float(lam_r), lam_k, lam_j, pb.data_ptr(),
                                         xb.data_ptr() if xb is not None else None, None, terms.data_ptr(), C.byref(reg), C.byref(nfe),
                                         _stream(xd.device))
    ff._last = ff._last_bwd = hd
    _lib.check_ffjord(hd.h, st)
    ff.last_nfe = int(nfe.value)
    p.grad = pb.view_as(p)
    if need_x_grad:
        x.grad = xb.view_as(x)
    return terms[0], float(reg.value), terms[1], terms[2], ff.last_nfe


@torch.no_grad()
def sample(ffjord, indims, p=None, nsamples=1, z=None):
    """sample(ffjord, indims, p; nsamples) (ffjord.jl:160-167): z ~ N(0, I), solved from t1 back to t0 with the exact trace.  Returns x (nsamples, D)."""
    if indims != ffjord.in_dims:
        raise ValueError("indims must equal the model's in_dims")
    p = ffjord.p if p is None else p
    hd = ffjord._handle()
    h = hd.h
    dev = p.device
    if z is None:
        z = ffjord.draw_normal(indims, nsamples, dev)
    elif z.dim() != 2 or z.shape[1] != indims or not z.is_cuda:
        raise ValueError(f"z must be a cuda tensor of shape (nsamples, {indims}); got {tuple(z.shape)}")
    z = z.contiguous().float()
    out = torch.empty(z.shape[0], indims, device=dev)
    _lib.check_ffjord(h, _lib.lib().rnde_ffjord_sample(h, p.contiguous().data_ptr(), z.data_ptr(), z.shape[0], ffjord.tspan[0], ffjord.tspan[1], 0,
                                                       out.data_ptr(), _stream(dev)))
    ffjord._last = hd
    return out


@torch.no_grad()
def loglikelihood(model, batches, p=None, exact=False, groups=1):
    """src/metrics.jl:20-33: sum of logpx over the batches / the number of columns.  exact=True: logpx from the exact trace (no probe).
    groups=k > 1 (engine="tiled"): up to k consecutive batches share a launch (logpx_batches: every batch keeps its own solve, bit for bit;
    the last call of a data set may carry fewer), the sum is kept on the device in double and read back once per data set.  The capacity
    is reserved on first use from k and the largest batch; the library's message is raised when the device does not hold that many tiles."""
    groups = int(groups)
    if groups < 1:
        raise ValueError(f"loglikelihood: groups must be at least 1; got {groups}")
    if groups > 1:
        if model.engine != "tiled":
            raise ValueError(f"loglikelihood: groups > 1 is served on engine=\"tiled\" only; got engine={model.engine!r}")
        acc, pending = None, []

        def flush():
            es = None if exact else [model.draw_normal(model.in_dims, x.shape[0], x.device) for x in pending]
            model._forward_groups(pending, p, es, exact, acc)
            pending.clear()
        for xb in batches:
            x = torch.as_tensor(xb, dtype=torch.float32).cuda(model.device)
            if acc is None:
                acc = torch.zeros(2, dtype=torch.float64, device=x.device)      # (the sum, and the column count as an int64)
            pending.append(x)
            if len(pending) == groups:
                flush()
        if pending:
            flush()
        if acc is None:
            raise ZeroDivisionError("loglikelihood: no batches")      # (as the groups=1 path's 0.0 / 0)
        host = acc.cpu()          # the one read-back of the data set
        return float(host[0]) / int(host.view(torch.int64)[1])
    total, n = 0.0, 0
    for xb in batches:
        x = torch.as_tensor(xb, dtype=torch.float32).cuda(model.device)
        total += float((model(x, p, exact=True) if exact else model(x, p))[0].sum())
        n += x.shape[0]
    return total / n


class _Loader:
    """Flux.Data.DataLoader(X; batchsize, shuffle): (B, D) float32 batches; a shuffling loader draws a new order each pass (seeded)."""

    def __init__(self, X, batchsize, shuffle, seed):
        self.X, self.batchsize, self.shuffle = X, batchsize, shuffle
        self.rng = np.random.default_rng(seed)

    def __len__(self):
        return (self.X.shape[0] + self.batchsize - 1) // self.batchsize

    def __iter__(self):
        idx = self.rng.permutation(self.X.shape[0]) if self.shuffle else np.arange(self.X.shape[0])
        for i in range(0, len(idx), self.batchsize):
            yield self.X[idx[i:i + self.batchsize]]


def load_gaussian_mixture(batchsize, train_test_split=0.75, *, nsamples=1000, ngaussians=6, dim=2, radius=5.0, sigma=0.1, noise=0.3, seed=0):
    """src/dataset.jl:159-199: ngaussians isotropic gaussians (std sigma) on a circle of `radius`, plus N(0, noise^2) noise, nsamples // ngaussians
    each; shuffled, split train / test.  The reference's distribution and shapes from a seeded numpy generator (not its draws)."""
    if dim != 2:
        raise ValueError("the reference generator places the means on a circle: dim = 2")
    rng = np.random.default_rng(seed)
    per = nsamples // ngaussians
    X = np.empty((per * ngaussians, dim), dtype=np.float32)
    theta = np.float32(0.0)
    for i in range(ngaussians):
        theta = np.float32(theta + np.float32(2 * np.pi / ngaussians))
        mu = np.array([np.cos(theta) * radius, np.sin(theta) * radius], dtype=np.float32)
        samples = mu[None, :] + sigma * rng.standard_normal((per, dim))
        X[i * per:(i + 1) * per] = (samples + noise * rng.standard_normal((per, dim))).astype(np.float32)
    X = X[rng.permutation(X.shape[0])]
    ntrain = int(math.floor(train_test_split * X.shape[0]))
    return _Loader(X[:ntrain].copy(), batchsize, True, seed + 1), _Loader(X[ntrain:].copy(), batchsize, False, seed + 2)


def load_miniboone(batchsize, path, train_test_split=0.8, seed=0):
    """src/dataset.jl:33-56: MiniBooNE from a (N, 43) array file (miniboone.npy), each feature standardised with its mean and its corrected
    standard deviation, the samples shuffled, then split train / test.  Returns (train loader, test loader) of (B, 43) float32 batches."""
    X = np.load(path).astype(np.float64)
    if X.ndim != 2:
        raise ValueError(f"expected a 2-d array (samples, features); got shape {X.shape}")
    X = (X - X.mean(0, keepdims=True)) / X.std(0, ddof=1, keepdims=True)
    rng = np.random.default_rng(seed)
    X = X[rng.permutation(X.shape[0])].astype(np.float32)
    ntrain = int(math.floor(train_test_split * X.shape[0]))
    return _Loader(X[:ntrain].copy(), batchsize, True, seed + 1), _Loader(X[ntrain:].copy(), batchsize, False, seed + 2)
