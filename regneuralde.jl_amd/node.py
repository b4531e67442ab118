"""TrackedNeuralODE: the reference's DE layer (src/models/neural_ode.jl), same constructor and
call contract, with the `solve` call replaced by librnde.so (hand-written gfx950 kernels).

    node = TrackedNeuralODE(model, [0.0, 1.0], True, regularize, "Tsit5",
                            save_everystep=False, reltol=1.4e-8, abstol=1.4e-8, save_start=False)
    u, nfe, sv = node(x, p)            # x: (B, D) cuda tensor == Julia D x B;  sv.saveval: tensor or None

With `saveat=` (constructor keyword or per-call override, neural_ode.jl:35-46) the {R,true} methods run
(neural_ode.jl:79-108,:146-180): `u` is then the (B, T, D) tensor whose memory is exactly the Julia
D x T x B array of diffeqsol_to_3dtrackedarray (src/utils.jl:17-19).

`func` is the caller's closure `(u, t, integrator) -> value` as the reference passes it (mnist_node.jl:134) -- it is evaluated on two
mock integrators and RECOGNISED as one of the reference's callbacks (mnist_node.jl:67,:74-79,:88-97; `reg_code` below), the library
computes the value inside its kernels -- or that callback's name ('error_est' / 'stiff_est' / 'error_stiff_est').  Anything else raises.
Differences from the Julia layer that are inherent to the host language:
`save_everystep=True` (a result whose length is data dependent; no reference call site uses it): `rnde_node_forward_everystep`, the state
after every accepted step (and the initial one with save_start=True), (B, n, D) with n known after the call.

`engine="tiled"` (opt-in; `rnde_node_create_tiled`) serves Dense chains wider than 64 whose padded weights fit LDS (`tiled_lds_bytes(dims)` <=
160 KB): Tsit5, EEst*dt or no callback; the end state, and with `tiled_max_saveat=n` (the capacity every handle of the layer reserves,
`rnde_node_tiled_reserve_saveat`) also `saveat=` of up to n times and `save_everystep=True`.  By default its gradient treats step sizes and times as constants, and the layer must be
built with `track_ctrl=False, track_initdt=False` (they describe the create config); `set_tracking(True, True)` or the constructor keyword
`tiled_tracking=(True, True)` then switches its handles to the tracked reverse sweep (`rnde_node_set_tracking`): the controller and the initial
step are differentiated and `last_tspan_bar` carries the real cotangent.  `check_tiled_served` raises a ValueError that names the limit for
everything else the engine does not serve.
"""
import ctypes as C

import torch

from . import _lib
from .layers import PRE_ACT, act_code, destructure

_FUNCS = {None: 1, "none": 0, "error_est": 1, "stiff_est": 2, "error_stiff_est": 3, "stiff_est_dt": 4}      # None: the layer's default callback (neural_ode.jl:116)
_FUNC_NAMES = {0: "none", 1: "error_est", 2: "stiff_est", 3: "error_stiff_est", 4: "stiff_est_dt"}
TSIT5_STABILITY_SIZE = 3.5068     # OrdinaryDiffEq.alg_stability_size(Tsit5()): what mnist_node.jl:73,:86 divides by
SOSRI2_STABILITY_SIZE = 10.6      # StochasticDiffEq.alg_stability_size(SOSRI2()): mnist_nsde.jl:55


class MockIntegrator:
    """What a saving callback reads off the integrator (neural_ode.jl:116; mnist_node.jl:67,:76,:89-91)."""

    def __init__(self, EEst, dt, eigen_est):
        self.EEst, self.dt, self.eigen_est = EEst, dt, eigen_est


_PROBES = ((2.0, 3.0, 5.0), (0.5, 0.25, -7.0))


def reg_code(func, stability_size):
    """rnde_reg code (include/rnde.h) of a caller's callback `func(u, t, integrator)`: its values on two mock integrators are matched against
    the reference's callbacks -- 0 (neural_ode.jl:54), EEst*dt (mnist_node.jl:67), |eigen_est|/stability_size (:74-79), EEst*dt +
    0.1*eigen_est/stability_size (:88-97), |eigen_est*dt| (test/test_node.jl:75).  The same rule as bindings/julia/RNDE.jl::reg_code.  Raises ValueError for anything else: a
    regulariser the kernels do not compute must not be replaced by another one silently."""
    got = [float(func(None, 0.0, MockIntegrator(*m))) for m in _PROBES]
    s = float(stability_size)
    want = {0: lambda e, d, g: 0.0, 1: lambda e, d, g: e * d, 2: lambda e, d, g: abs(g) / s, 3: lambda e, d, g: e * d + 0.1 * g / s,
            4: lambda e, d, g: abs(g * d)}      # 4: the reference's own test, func = abs(integrator.eigen_est * integrator.dt) (test/test_node.jl:75,:84)
    for code in (0, 1, 2, 3, 4):
        if all(abs(v - want[code](*m)) <= 1e-4 * abs(want[code](*m)) + 1e-7 for v, m in zip(got, _PROBES)):
            return code
    raise ValueError("func is none of the callbacks librnde.so computes (EEst*dt, |eigen_est|/stability_size, EEst*dt + "
                     f"0.1*eigen_est/stability_size, |eigen_est*dt|, 0): on (EEst, dt, eigen_est) = {_PROBES[0]} and {_PROBES[1]} it returned {got}")


def effective_reg(code, composite):
    """The callback code a (func, solver) pair runs with, or an error: integrator.eigen_est is filled by the composite solvers only
    (AutoTsit5(Tsit5()), AutoSOSRI2(SOSRI2()): mnist_node.jl:81,:99, mnist_nsde.jl:60).  Under a plain solver it keeps its INITIAL value -- 1, not 0
    [RECALL] -- so the reference would record a constant there (|1| / stability_size, EEst*dt + 0.1 / stability_size), which no experiment does and the
    kernels do not reproduce: every callback that reads eigen_est is refused under a plain solver, the blend included (round 5 mapped the blend to
    EEst*dt, i.e. assumed eigen_est = 0: a constant offset of the saved values)."""
    if composite or code in (0, 1):
        return code
    raise ValueError("func reads integrator.eigen_est, which only the composite solvers (AutoTsit5 / AutoSOSRI2) fill; with a plain solver "
                     "the reference records its initial value, a constant -- build the layer with the composite solver")


class SavedValues:
    """DiffEqCallbacks.SavedValues as returned by the regularised call (neural_ode.jl:126,:143)."""

    def __init__(self, saveval):
        self.saveval = saveval


ENGINES = (None, "tiled")      # None: rnde_node_create's own routing (stage engine / chain engine); "tiled": rnde_node_create_tiled
TILED_LDS_BYTES = 160 * 1024
TILED_MAX_BATCH, TILED_MAX_ATTEMPTS = 4096, 8000


def tiled_lds_bytes(dims):
    """LDS bytes of a tile of the tiled engine (rnde_node_tiled_lds_bytes; rnde_node_tile.h::NtDyn::lds_floats): padded weights with the t column
    and bias vectors, the input, every layer's output, two VJP vectors, reduction scratch.  The solve and the reverse sweep share the layout."""
    pad = lambda n: (n + 15) // 16 * 16
    n = len(dims) - 1
    w = sum(pad(dims[l]) * (pad(dims[l + 1]) + 1) + 2 * pad(dims[l + 1]) for l in range(n))
    mp = max(pad(d) for d in dims)
    return 4 * ((w + 3) // 4 * 4 + pad(dims[0]) * 16 + sum(pad(dims[l + 1]) * 16 for l in range(n)) + 2 * mp * 16 + 128)


def check_tiled_served(layer):
    """ValueError naming the limit or the alternative for what engine="tiled" does not serve (include/rnde.h: rnde_node_create_tiled)."""
    if layer.track_ctrl is not False or layer.track_initdt is not False:
        raise ValueError('TrackedNeuralODE(engine="tiled"): the reverse sweep of the tiled engine treats step sizes and times as constants; pass '
                         "track_ctrl=False and track_initdt=False to ask for that gradient (the defaults, True, differentiate the controller and the "
                         "initial step, which only the default engines do)")
    if layer.solver != "Tsit5":
        raise ValueError(f'TrackedNeuralODE(engine="tiled"): solver must be "Tsit5"; got {layer.solver!r} (AutoTsit5, DP5 and DOP853 run on the default engines)')
    if ("saveat" in layer.kwargs or layer.kwargs.get("save_everystep", False)) and layer.tiled_max_saveat is None:
        raise ValueError('TrackedNeuralODE(engine="tiled"): saveat= and save_everystep=True are not served (the end state only); use the default engine')
    if getattr(layer.model, "pre_act", False):
        raise ValueError('TrackedNeuralODE(engine="tiled"): a leading element-wise map (pre_act) is not served; use the default engine')
    if layer.col_tile != 0:
        raise ValueError('TrackedNeuralODE(engine="tiled"): col_tile must be 0')
    if layer.matrix_mode not in (None, 0):
        raise ValueError('TrackedNeuralODE(engine="tiled"): matrix_mode 1 (bf16x3) is not served; its layer products are the fp32-input MFMA')
    dims = layer.model.dims()
    if not 1 <= len(dims) - 1 <= _lib.MAX_LAYERS:
        raise ValueError(f'TrackedNeuralODE(engine="tiled"): 1..{_lib.MAX_LAYERS} Dense layers; got {len(dims) - 1}')
    if dims[0] != dims[-1]:
        raise ValueError('TrackedNeuralODE(engine="tiled"): the chain must map the state to its own width (dims[0] == dims[-1])')
    if layer.max_batch > TILED_MAX_BATCH:
        raise ValueError(f'TrackedNeuralODE(engine="tiled"): max_batch above {TILED_MAX_BATCH} is not served (256 resident tiles of 16 columns meet)')
    if layer.max_attempts > TILED_MAX_ATTEMPTS:
        raise ValueError(f'TrackedNeuralODE(engine="tiled"): max_attempts above {TILED_MAX_ATTEMPTS} is not served (meeting tags)')
    need = tiled_lds_bytes(dims)
    if need > TILED_LDS_BYTES:
        raise ValueError(f'TrackedNeuralODE(engine="tiled"): the resident weights and the activations of a tile need {need} bytes of LDS, above the '
                         f"limit of {TILED_LDS_BYTES} bytes")


class _Handle:
    def __init__(self, cfg, engine=None):
        self.ptr = C.c_void_p()
        create = _lib.lib().rnde_node_create_tiled if engine == "tiled" else _lib.lib().rnde_node_create
        st = create(C.byref(cfg), C.byref(self.ptr))
        _lib.check(None, st)
        self.busy = False
        self.tracking = (False, False)      # engine="tiled": the pair this handle runs under (rnde_node_set_tracking)

    def __del__(self):
        try:
            if self.ptr:
                _lib.lib().rnde_node_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


class _TapeToken:
    """Lifetime of one taped forward.  It lives in the autograd node's ctx: when the graph is dropped WITHOUT a backward pass
    (the reference's per-epoch `_, nfe, _ = node(dummy)` with tracking on, experiments/mnist_node.jl:236) the token dies with
    it, releases the tape and hands the handle back to the pool -- otherwise every such call would pin a handle and its
    max_attempts arena (~4 GB at B = 512) for good."""

    def __init__(self, h, release):
        self.h, self.release, self.done = h, release, False

    def finish(self):
        if not self.done:
            self.done = True
            self.h.busy = False

    def __del__(self):
        try:
            if not self.done:
                self.done = True
                if self.h.ptr:
                    self.release(self.h.ptr)
                self.h.busy = False
        except Exception:
            pass


MAX_HANDLES_PER_KEY = 4   # simultaneously pending (taped, not yet back-propagated) forwards per layer, device and callback


def _check_f32(name, t):
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype}): the C ABI reads raw fp32 memory; convert explicitly, "
                        "as the reference does with eltype(p)")


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, layer, t0, t1, keep_tape, saveat):
        h = layer._acquire(x, keep_tape)
        L = _lib.lib()
        B, D = x.shape
        nfe = C.c_int64(0)
        nsv = C.c_int32(0)
        sv_host = (C.c_float * (layer.max_attempts + 1))()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if saveat is None:
            u = torch.empty_like(x)
            st = L.rnde_node_forward(h.ptr, x.data_ptr(), p.data_ptr(), B, t0, t1, u.data_ptr(), C.byref(nfe), sv_host,
                                     C.byref(nsv), 1 if keep_tape else 0, C.c_void_p(stream))
        elif saveat == "everystep":      # save_everystep = true: every accepted step's end (neural_ode.jl:10-11); the count comes back with the call
            cap = layer.max_attempts + 1
            buf = torch.empty((B, cap, D), dtype=torch.float32, device=x.device)
            # the library writes D x n x B column-major = (B, n, D) rows of the n it finds: ask with the capacity as the time stride is n, not cap --
            # so the call goes into a scratch of the full capacity first and the (B, n, D) block is what it filled
            th = (C.c_float * cap)()
            nout = C.c_int32(0)
            st = L.rnde_node_forward_everystep(h.ptr, x.data_ptr(), p.data_ptr(), B, t0, t1, 1 if layer.kwargs.get("save_start", True) else 0,
                                               buf.data_ptr(), cap, th, C.byref(nout), C.byref(nfe), sv_host, C.byref(nsv), 1 if keep_tape else 0,
                                               C.c_void_p(stream))
            _lib.check(h.ptr, st)
            n = nout.value
            u = buf.reshape(-1)[: B * n * D].reshape(B, n, D).clone()
            layer.last_times = [float(th[i]) for i in range(n)]
        else:
            T = len(saveat)
            u = torch.empty((B, T, D), dtype=torch.float32, device=x.device)
            sa = (C.c_float * T)(*saveat)
            st = L.rnde_node_forward_saveat(h.ptr, x.data_ptr(), p.data_ptr(), B, t0, t1, sa, T, u.data_ptr(), C.byref(nfe),
                                            sv_host, C.byref(nsv), 1 if keep_tape else 0, C.c_void_p(stream))
        _lib.check(h.ptr, st)
        layer.last_nfe = int(nfe.value)
        saveval = torch.tensor(list(sv_host[:nsv.value]), dtype=torch.float32, device=x.device)
        ctx.layer, ctx.h, ctx.nsv = layer, h, nsv.value
        if keep_tape:
            h.busy = True
            ctx.token = _TapeToken(h, L.rnde_node_release_tape)
        return u, saveval

    @staticmethod
    def backward(ctx, u_bar, sv_bar):
        layer, h = ctx.layer, ctx.h
        L = _lib.lib()
        u_bar = u_bar.contiguous().to(torch.float32)
        x_bar = torch.empty((u_bar.shape[0], u_bar.shape[-1]), dtype=torch.float32, device=u_bar.device)
        p_bar = torch.empty(layer.P, dtype=torch.float32, device=u_bar.device)
        svb = None
        if ctx.nsv and sv_bar is not None:
            svb = (C.c_float * ctx.nsv)(*sv_bar.detach().to("cpu", torch.float32).tolist())
        tsb = (C.c_float * 2)()
        stream = torch.cuda.current_stream(u_bar.device).cuda_stream
        st = L.rnde_node_backward(h.ptr, u_bar.data_ptr(), svb, x_bar.data_ptr(), p_bar.data_ptr(), tsb, C.c_void_p(stream))
        ctx.token.finish()
        _lib.check(h.ptr, st)
        layer.last_tspan_bar = (tsb[0], tsb[1])
        return x_bar, p_bar, None, None, None, None, None


class TrackedNeuralODE:
    """Mirror of reference src/models/neural_ode.jl:1-33 (struct + constructor) and :48-180 (call methods)."""

    def __init__(self, model, tspan, time_dep, regularize, solver="Tsit5", *, max_batch=512, max_attempts=128,
                 cb_save_start=True, track_ctrl=True, track_initdt=True, col_tile=0, matrix_mode=None, engine=None, tiled_tracking=(False, False),
                 tiled_max_saveat=None, **kwargs):
        if engine not in ENGINES:
            raise ValueError(f"engine must be one of {ENGINES}; got {engine!r}")
        self.engine = engine
        # engine="tiled": the saveat capacity every handle of the layer reserves (rnde_node_tiled_reserve_saveat); None: saving calls are refused
        if tiled_max_saveat is not None:
            if engine != "tiled":
                raise ValueError('TrackedNeuralODE: tiled_max_saveat is served with engine="tiled" only; the default engines take saveat= and '
                                 "save_everystep=True without a reservation")
            if isinstance(tiled_max_saveat, bool) or not isinstance(tiled_max_saveat, int) or tiled_max_saveat < 1:
                raise ValueError(f'TrackedNeuralODE(engine="tiled"): tiled_max_saveat must be an integer >= 1 or None; got {tiled_max_saveat!r}')
            if tiled_max_saveat > int(max_attempts) + 1:
                raise ValueError(f'TrackedNeuralODE(engine="tiled"): tiled_max_saveat = {tiled_max_saveat} is above max_attempts + 1 = '
                                 f"{int(max_attempts) + 1} (what save_everystep with save_start can need)")
        self.tiled_max_saveat = tiled_max_saveat
        if solver not in ("Tsit5", "AutoTsit5", "DP5", "DOP853"):
            raise ValueError("solver: the reference's call sites use Tsit5() / AutoTsit5(Tsit5()) only; DP5 (a second 7-stage pair) and DOP853 "
                             "(a 13-stage table) run on the tableau-as-data kernels (Dense chains of width <= 64)")
        self.solver = solver
        self.model = model
        for l in model.layers:
            act_code(l.act)                              # (an activation the kernels do not serve is refused here, not at the first call)
        self.p = destructure(model)                      # Flux.destructure (neural_ode.jl:12)
        self.tspan = [float(tspan[0]), float(tspan[1])]
        self.time_dep = bool(time_dep)
        self.regularize = bool(regularize)
        self.kwargs = dict(kwargs)                       # reltol, abstol, save_everystep, save_start, saveat
        self.return_multiple = bool(kwargs.get("save_everystep", False)) or ("saveat" in kwargs)  # neural_ode.jl:11
        self.save_everystep = bool(kwargs.get("save_everystep", False)) and "saveat" not in kwargs      # (saveat given: it decides what is saved)
        if bool(time_dep) != bool(model.time_dep):
            raise ValueError("time_dep must match the model (TDChain => True)")
        self.max_batch, self.max_attempts = int(max_batch), int(max_attempts)
        self.cb_save_start, self.track_ctrl, self.track_initdt, self.col_tile = cb_save_start, track_ctrl, track_initdt, col_tile
        # which unit forms the Dense-layer products of the one-launch solve (include/rnde.h: rnde_node_set_matrix_mode): None = the library's default
        # (bf16x3 on the matrix cores where the kernels serve the shape, RNDE_X3 overrides), 0 = fp32-input MFMA, 1 = bf16x3
        self.matrix_mode = matrix_mode
        self.P = self.p.numel()
        if engine == "tiled":      # (opt-in: Dense chains wider than 64 on the tile layout; refusals need no device)
            check_tiled_served(self)
        self._handles = {}
        self._coupling = None
        self.tiled_tracking = (False, False)
        if tuple(tiled_tracking) != (False, False):
            self.set_tracking(*tiled_tracking)
        self.last_nfe = None
        self.last_times = None                            # save_everystep: the times of the states the last call returned
        self.last_tspan_bar = None

    # -- C-ABI config -------------------------------------------------------------------------
    def _config(self, device_index, func):
        cfg = _lib.NodeConfig()
        dims = self.model.dims()
        cfg.n_layers = len(self.model.layers)
        for i, d in enumerate(dims):
            cfg.dims[i] = d
        for i, l in enumerate(self.model.layers):
            cfg.act[i] = act_code(l.act)
        cfg.time_dep = int(self.time_dep)
        cfg.pre_act = PRE_ACT[getattr(self.model, "pre_act", False)]
        cfg.max_batch = self.max_batch
        cfg.solver = _lib.ODE_SOLVER[self.solver]
        cfg.reltol = float(self.kwargs.get("reltol", 1e-3))   # OrdinaryDiffEq defaults when not given
        cfg.abstol = float(self.kwargs.get("abstol", 1e-6))
        cfg.regularize = _FUNCS[func] if self.regularize else 0
        cfg.cb_save_start = int(self.cb_save_start)
        cfg.track_ctrl = int(self.track_ctrl)
        cfg.track_initdt = int(self.track_initdt)
        cfg.max_attempts = self.max_attempts
        cfg.device = device_index
        cfg.col_tile = self.col_tile
        return cfg

    def _acquire(self, x, keep_tape, func=None):
        key = (x.device.index or 0, bool(keep_tape), self._func)
        hs = self._handles.setdefault(key, [])
        for h in hs:
            if not h.busy:
                self._apply_tracking(h)      # (a handle that was pending while set_tracking ran takes the layer's pair when it is next handed out)
                return h
        if len(hs) >= MAX_HANDLES_PER_KEY:
            raise RuntimeError(f"{len(hs)} taped forwards of this layer are pending without a backward pass; each owns a tape of "
                               "max_attempts records.  Run them under torch.no_grad() (NFE probes), call backward, or drop the graphs")
        h = _Handle(self._config(x.device.index or 0, self._func), self.engine)
        if self.matrix_mode is not None:
            _lib.check(h.ptr, _lib.lib().rnde_node_set_matrix_mode(h.ptr, int(self.matrix_mode)))
        if self._coupling is not None:
            _lib.check(h.ptr, _lib.lib().rnde_node_set_coupling(h.ptr, self._coupling[0], self._coupling[1]))
        if self.tiled_max_saveat is not None:      # (a fresh handle holds no tape)
            _lib.check(h.ptr, _lib.lib().rnde_node_tiled_reserve_saveat(h.ptr, int(self.tiled_max_saveat)))
        self._apply_tracking(h)
        hs.append(h)
        return h

    def set_coupling(self, comm, global_batch):
        """SURVEY 8e mode 2 (include/rnde.h: rnde_node_set_coupling): ONE step-size controller for all shards of a minibatch split by
        columns over `world` layers.  `comm`: an rnde_comm* (ctypes void pointer: `GradientAllReducer.comm` across processes,
        rnde_comm_create_local_group inside one); None switches back to independent controllers.  Every rank must make the same calls."""
        if self.engine == "tiled":
            raise ValueError('TrackedNeuralODE(engine="tiled"): set_coupling is not served (one controller over several shards runs on the default engines)')
        self._coupling = None if comm is None else (comm, int(global_batch))
        for hs in self._handles.values():
            for h in hs:
                _lib.check(h.ptr, _lib.lib().rnde_node_set_coupling(h.ptr, comm, int(global_batch) if comm is not None else 0))

    def set_tracking(self, track_ctrl, track_initdt=False):
        """Which reverse sweep the taped forwards of an engine="tiled" layer get (include/rnde.h: rnde_node_set_tracking): (False, False) the
        default, step sizes and times constants; (True, False) the step-size controller differentiated; (True, True) the initial step as well
        -- the reference's gradient.  Applies at once to every handle that is not pending (the tape of a finished backward is released for it),
        to a pending one -- a taped forward waiting for its backward keeps the setting it ran under -- when it is next handed out, and to every
        handle created later."""
        if self.engine != "tiled":
            raise ValueError('TrackedNeuralODE.set_tracking: served with engine="tiled" only; the default engines take track_ctrl / track_initdt '
                             "in the constructor")
        ctrl, initdt = bool(track_ctrl), bool(track_initdt)
        if initdt and not ctrl:
            raise ValueError("TrackedNeuralODE.set_tracking: track_ctrl=False with track_initdt=True is not served: with the controller a constant "
                             "the first proposed step reaches nothing (the settings are (False, False), (True, False) and (True, True))")
        self.tiled_tracking = (ctrl, initdt)
        for hs in self._handles.values():
            for h in hs:
                if not h.busy:
                    self._apply_tracking(h)

    def _apply_tracking(self, h):
        """Bring a handle that is not pending to the layer's pair.  A handle whose backward has run still holds its tape on the library's side
        (rnde_node_backward may be called again on it), and the library refuses to switch a handle that holds one: nothing of this layer waits
        for that tape any more, so it is released first."""
        if h.tracking == self.tiled_tracking:
            return
        L = _lib.lib()
        _lib.check(h.ptr, L.rnde_node_release_tape(h.ptr))
        _lib.check(h.ptr, L.rnde_node_set_tracking(h.ptr, int(self.tiled_tracking[0]), int(self.tiled_tracking[1])))
        h.tracking = self.tiled_tracking

    @staticmethod
    def _saveat_times(saveat, ts):
        """What OrdinaryDiffEq saves for `saveat`: a vector as given (must lie in [t0, t1], increasing); a number s is the
        range t0:s:t1 plus t1 (save_start = save_end = true for a Number)."""
        if isinstance(saveat, (int, float)):
            s, out, k = float(saveat), [], 0
            if s <= 0:
                raise ValueError("saveat step must be positive")
            while ts[0] + k * s < ts[1]:
                out.append(ts[0] + k * s)
                k += 1
            out.append(ts[1])
            return out
        v = [float(t) for t in (saveat.detach().cpu().reshape(-1).tolist() if torch.is_tensor(saveat) else list(saveat))]
        if not v:
            raise ValueError("saveat is empty")
        if any(b <= a for a, b in zip(v, v[1:])) or v[0] < ts[0] or v[-1] > ts[1]:
            raise ValueError("saveat must be strictly increasing inside tspan")
        return v

    def resolve_func(self, func):
        """The name of the library callback a call's `func` selects (None when the layer does not regularise): a closure `(u, t, integrator) -> value`
        as the reference passes it (mnist_node.jl:134) is recognised, not called per step; names pass through."""
        if not self.regularize:
            return None
        if callable(func):
            func = _FUNC_NAMES[reg_code(func, TSIT5_STABILITY_SIZE)]
        if func not in _FUNCS:
            raise ValueError("func must be a callback (u, t, integrator) -> value or one of None/'error_est', 'stiff_est', "
                             "'error_stiff_est' (the three callbacks of experiments/mnist_node.jl:62-103), 'stiff_est_dt' (test/test_node.jl:75)")
        effective_reg(_FUNCS[func], self.solver == "AutoTsit5")      # names and closures alike: a callback that reads eigen_est needs the composite solver
        if self.engine == "tiled" and _FUNCS[func] > 1:
            raise ValueError('TrackedNeuralODE(engine="tiled"): the stiffness callbacks are not served; func is None / "error_est" (EEst * dt)')
        return func

    # -- call operator ------------------------------------------------------------------------
    def __call__(self, x, p=None, func=None, tspan=None, saveat=None):
        """(x, p = n.p; func, tspan, saveat) -> (res, nfe, sv)   [neural_ode.jl:48-54,:76,:110-119,:143]"""
        if saveat is not None and not self.return_multiple:
            raise ValueError("saveat override on a layer built without saveat: the reference dispatches on the constructor "
                             "keyword (neural_ode.jl:11), build the layer with saveat=")
        if not x.is_cuda:
            raise RuntimeError("TrackedNeuralODE runs on the MI355X only: x must be a cuda tensor (no CPU fallback)")
        p = self.p if p is None else p
        if p.device != x.device:
            if p is self.p:
                self.p = p = self.p.to(x.device)
            else:
                raise RuntimeError("p and x must live on the same device")
        _check_f32("p", p)
        _check_f32("x", x)
        x2 = x.reshape(x.shape[0], -1).contiguous()
        ts = self.tspan if tspan is None else [float(tspan[0]), float(tspan[1])]   # _convert_tspan, utils.jl:21-23
        self._func = self.resolve_func(func)
        keep = torch.is_grad_enabled() and (x2.requires_grad or p.requires_grad)
        times = None
        if self.return_multiple and self.save_everystep and saveat is None:
            times = "everystep"
        elif self.return_multiple:      # update_saveat! (neural_ode.jl:35-46): a per-call override, the stored one otherwise
            times = self._saveat_times(self.kwargs["saveat"] if saveat is None else saveat, ts)
            if self.engine == "tiled" and len(times) > self.tiled_max_saveat:      # (before any launch; the library refuses it too)
                raise ValueError(f'TrackedNeuralODE(engine="tiled"): {len(times)} save times are above the layer\'s tiled_max_saveat = '
                                 f"{self.tiled_max_saveat}")
        u, saveval = _Solve.apply(x2, p.contiguous(), self, ts[0], ts[1], keep, times)
        sv = SavedValues(saveval) if self.regularize else None
        return u, self.last_nfe, sv
