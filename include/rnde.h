/*
 * rnde.h -- C ABI of librnde.so: the MI355X (gfx950) drop-in for the adaptive
 * Runge-Kutta integration behind RegNeuralDE.jl's TrackedNeuralODE call operator.
 *
 * What each entry point replaces in the reference (paths relative to the reference root):
 *   rnde_node_create    TrackedNeuralODE(model, tspan, time_dep, regularize, solver; kw...)
 *                       src/models/neural_ode.jl:10-33 (constructor; Flux.destructure at :12)
 *   rnde_node_forward   (n::TrackedNeuralODE{R,Z})(x, p; func, tspan, saveat)
 *                       src/models/neural_ode.jl:48-77 ({false,false}), :110-144 ({true,false}):
 *                       everything between ODEProblem construction (:128-129) and the unpacking
 *                       of sol.u[end] / sol.destats.nf / sv (:138-143), i.e. the `solve` call
 *                       (:131-137) that lives in OrdinaryDiffEq/DiffEqBase/DiffEqCallbacks.
 *   rnde_node_backward  the reverse sweep Tracker.gradient performs over that solve
 *                       (experiments/mnist_node.jl:229-232) because
 *                       sensealg = SensitivityADPassThrough() (neural_ode.jl:134).
 *   rnde_node_release_tape / rnde_node_destroy   Julia GC of the Tracker tape / the layer.
 *
 * All arrays are fp32, column-major, exactly as Julia holds them: x and u are D x B
 * (element (r,c) at c*D + r); p is the Flux.destructure vector
 * [vec(W1) (out x in_ext, column-major); b1; vec(W2); b2; ...] (neural_ode.jl:12).
 * Pointers named *_dev are DEVICE (HBM) pointers owned by the caller; the library keeps no
 * caller pointer after a call returns.  `stream` is a hipStream_t (0 = default stream); calls
 * are asynchronous on that stream except where they return host scalars (they synchronise
 * the stream before returning those).  One in-flight call per handle; handles are independent.
 * No exceptions cross this boundary: every function returns an rnde_status.
 */
#ifndef RNDE_H
#define RNDE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNDE_MAX_LAYERS 8

typedef enum {
    RNDE_OK = 0,
    RNDE_ERR_BAD_ARG = 1,       /* shape / config not supported                               */
    RNDE_ERR_MAX_ATTEMPTS = 2,  /* solver hit max_attempts (reference: maxiters, never checked) */
    RNDE_ERR_DT_UNDERFLOW = 3,  /* dt <= dtmin                                                 */
    RNDE_ERR_NONFINITE = 4,     /* NaN/Inf in EEst or dt                                       */
    RNDE_ERR_HIP = 5,           /* HIP runtime error, see rnde_last_error                      */
    RNDE_ERR_NO_TAPE = 6,       /* backward without a recorded forward                         */
    RNDE_ERR_NO_DEVICE = 7      /* no gfx950 device visible                                    */
} rnde_status;

/* rnde_node_config.act[l], rnde_nsde_config.drift_act[l] / diff_act[l]: the activation of Dense layer l (Flux's Dense(in, out, sigma)), NNlib's
 * identity, tanh, relu, sigma, softplus and elu (alpha = 1).  The kernels compute, in fp32, with t = exp(-|z|):
 *   relu      z < 0 ? 0 : z                                   (max(z, 0); a NaN stays NaN)
 *   sigmoid   z >= 0 ? 1 / (1 + t) : t / (1 + t)
 *   softplus  log1p(t) + max(z, 0); on 0 < z < 1/2, where that form is not monotone in fp32, log1p(exp(z)) in fp64, rounded once
 *   elu       z > 0 ? z : expm1(z)
 * and tanh with a polynomial / exp2 formula of at most 1.65 ulp (1.62 measured on the device, hardware exp2 and reciprocal included, over every
 * binade and every float around its two seams).  On that set every one of them is monotone, and a NaN comes out of every one as a NaN (tests/test_gpu_elementwise.py).  Each derivative is taken from the layer's OUTPUT y, which is what the reverse pass
 * keeps: tanh 1 - y^2, relu y > 0 ? 1 : 0, sigmoid y (1 - y), softplus -expm1(-y), elu y > 0 ? 1 : y + 1.  An activation whose derivative needs the
 * pre-activation (swish, gelu) is not served.  These are the textbook formulas; agreement with NNlib's own code at rounding level is not pinned
 * (it has not been compared).  Any other code is RNDE_ERR_BAD_ARG at create.  Where each is served: every Dense chain of width <= 64 (the chain
 * engine, the SDE layer).  The stage engine (the two-layer TDChain form with act[0] = tanh, col_tile 0 / 16) serves identity or tanh in act[1] and
 * refuses the rest by name.  The kernels with compile-time shapes (the latent-ODE widths, the SDE layer's 32 -> 64 -> 32 drift) serve identity
 * and tanh: a chain with any other activation runs a separately compiled variant of the generic kernels. */
typedef enum { RNDE_ACT_IDENTITY = 0, RNDE_ACT_TANH = 1, RNDE_ACT_RELU = 2, RNDE_ACT_SIGMOID = 3, RNDE_ACT_SOFTPLUS = 4, RNDE_ACT_ELU = 5 } rnde_act;
/* rnde_node_config.pre_act (and rnde_nsde_set_pre_act): the element-wise map in front of the first Dense layer.  RNDE_PRE_TANH is the
 * leading tanh of experiments/latent_ode.jl:114, RNDE_PRE_CUBE the leading x -> x .^ 3 of experiments/sde_toy_problem.jl:45.  Any other value
 * is RNDE_ERR_BAD_ARG at create.  The kernels with compile-time shapes that skip the generic chain evaluation (the SDE layer's 32 -> 64 -> 32
 * drift, rnde_nsde_config.generic = 0) apply no map: a handle with a nonzero selector runs the generic kernels instead. */
typedef enum { RNDE_PRE_NONE = 0, RNDE_PRE_TANH = 1, RNDE_PRE_CUBE = 2 } rnde_pre_act;
/* RNDE_SOLVER_TSIT5: every reference call site (experiments/mnist_node.jl:62-103, latent_ode.jl:131-136), all engines.
 * RNDE_SOLVER_DP5: Dormand-Prince 5(4), the second 7-stage first-same-as-last pair, through the tableau-as-data kernels of the chain
 * engine (Dense chains of width <= 64; callbacks none / EEst*dt): there a pair of that shape is a table, not a kernel. */
/* RNDE_SOLVER_DOP853: Hairer's 8(5,3) pair as a 13-stage first-same-as-last TABLE (csrc/rk_tables.h, generated from scipy's coefficients;
 * linear fifth-order error estimate, controller exponents for order 8): the same kernels with stage count, tape layout and evaluation
 * counts read from the table -- what a Verner pair (Vern7, 10 stages + the closing evaluation) would be once its
 * coefficients are at hand.  End state only (no dense output in the table); callbacks none / EEst*dt; NFE = 3 + 12 per attempted step. */
typedef enum { RNDE_SOLVER_TSIT5 = 0, RNDE_SOLVER_DP5 = 1, RNDE_SOLVER_DOP853 = 2 } rnde_solver;
/* func passed to the layer call (neural_ode.jl:116; experiments/mnist_node.jl:67,:74-79,:88-97) */
typedef enum { RNDE_REG_NONE = 0, RNDE_REG_ERR = 1, RNDE_REG_STIFF = 2, RNDE_REG_ERR_STIFF = 3,
               RNDE_REG_STIFF_DT = 4   /* |eigen_est * dt|: the callback of the reference's own test (test/test_node.jl:75,:84; the comment at src/models/neural_ode.jl:115) */
} rnde_reg;

typedef struct {
    /* dynamics: Dense chain; time_dep = TDChain semantics (src/models/basic.jl:16-23,
     * experiments/mnist_node.jl:51-54): a row of t is appended to every layer input */
    int32_t n_layers;
    int32_t dims[RNDE_MAX_LAYERS + 1]; /* dims[0] = dims[n_layers] = D */
    int32_t act[RNDE_MAX_LAYERS];
    int32_t time_dep;
    int32_t pre_act;       /* rnde_pre_act: leading tanh (experiments/latent_ode.jl:114) or cube (sde_toy_problem.jl:45) */
    int32_t max_batch;     /* largest B any call will pass */
    int32_t solver;        /* rnde_solver */
    float   reltol, abstol;
    int32_t regularize;    /* rnde_reg: which value the saving callback records per accepted step */
    int32_t cb_save_start; /* 1: callback also fires at init (value 0 for RNDE_REG_ERR) -- SURVEY.md B.5 */
    int32_t track_ctrl;    /* 1: reverse pass differentiates dt_next = dt/q through the PI controller */
    int32_t track_initdt;  /* 1: reverse pass differentiates the initial-step heuristic */
    int32_t max_attempts;  /* tape capacity in attempted steps */
    int32_t device;        /* HIP device ordinal */
    int32_t col_tile;      /* 0 = auto; MNIST form: 16 (stage engine, the only engine of that form since round 4); small-width chains:
                            * 64 (chain engine: 16 columns per wave) */
    /* tuning (0 = default everywhere, so a zero-initialised tail keeps the defaults) */
    int32_t persist;        /* stage engine: 0 = one launch per attempted step where the shape allows, -1 = always the 7-launch kernels */
    int32_t wgrad_side_pct; /* share (per cent of the attempts) of the parameter-gradient GEMMs run beside the reverse sweep on the CUs
                             * it leaves idle: 0 = default (30), -1 = none */
    int32_t stage_generic;  /* 1 = never use the instantiations with the MNIST geometry (D = 784, H = 100) as compile-time constants */
} rnde_node_config;

typedef struct rnde_node rnde_node;
typedef struct rnde_comm rnde_comm;   /* gradient collective, see rnde_comm_* below */

const char* rnde_version(void);
/* Debugging aid.  With the environment variable RNDE_POISON set (read per allocation), every device allocation of the library -- of every
 * engine and layer below, create-time and grown while a handle runs -- is filled with 0xFF bytes (NaN as float), so that a read of memory
 * nothing wrote shows up as NaN instead of depending on what the allocator hands back.  The two readers return how many allocations and
 * how many bytes were filled since the library was loaded (0 while the variable was never set): a test that creates a handle under the
 * variable checks that they grew. */
int64_t     rnde_debug_poison_allocs(void);
int64_t     rnde_debug_poison_bytes(void);
/* How many device allocations of the library are live, and their bytes (every engine and layer below, whatever RNDE_POISON says; pinned host
 * memory is not counted).  A handle that is created, run and destroyed leaves both where they were. */
int64_t     rnde_debug_live_allocs(void);
int64_t     rnde_debug_live_bytes(void);
const char* rnde_last_error(const rnde_node* h); /* h may be NULL: last create error */
int32_t     rnde_param_count(const rnde_node_config* cfg);

rnde_status rnde_node_create(const rnde_node_config* cfg, rnde_node** out);
void        rnde_node_destroy(rnde_node* h);

/* The tiled engine (opt-in; rnde_node_create never selects it): the same layer for Dense chains WIDER than the chain engine's 64, on the tile
 * layout of TrackedFFJORD's chain dynamics -- one workgroup of four waves per 16 batch columns, the padded weights resident in LDS, the whole
 * adaptive Tsit5 solve in one launch (the tiles meet once per attempt), the reverse sweep in one launch with no meeting.
 * Serves: 1..8 Dense layers, Chain or TDChain (time_dep), the six rnde_act activations in any layer, dims[0] == dims[n_layers], pre_act =
 *   RNDE_PRE_NONE, col_tile = 0, Tsit5, regularize RNDE_REG_NONE or RNDE_REG_ERR (cb_save_start honoured), max_batch <= 4096 (256 resident
 *   tiles), max_attempts <= 8000.
 * Widths are limited by BYTES, not rows: rnde_node_tiled_lds_bytes(cfg) -- padded weights (in_p x (out_p + 1) floats per layer, plus the t
 *   column and the bias), the input tile, every layer's output and two VJP vectors ([rows_p][16] each), 128 floats of scratch -- must not
 *   exceed 163840 (160 KB); the solve and the reverse sweep share the layout.  [2,128,128,2] needs 120512 bytes, [64,192,64] 146944 (served);
 *   [64,256,64] needs 192768 and is refused with that count in the message.  The state may have more than 64 rows where the bytes allow.
 *   rnde_node_tiled_lds_bytes needs no device; -1 for a malformed shape.
 * CONSTANT STEP SIZES IN THE REVERSE BY DEFAULT: rnde_node_backward on this engine differentiates the recorded Runge-Kutta program with step
 *   sizes and times as constants (the cotangent of a saved value EEst * dt reaches the stages through EEst) and returns tspan_bar = (0, 0).
 *   That is track_ctrl = track_initdt = 0, and rnde_node_create_tiled REFUSES a config with either flag set: nobody gets the constant-step
 *   gradient without asking for it.  rnde_node_set_tracking (below) switches the handle to the tracked sweep AFTER creation: the PI
 *   controller, the clamps and (track_initdt) the initial-step rule are differentiated too, one meeting of the tiles per reversed attempt,
 *   and tspan_bar is the real cotangent.  With regularize = RNDE_REG_ERR the constant-step gradient of sum EEst * dt is 40-94 % away from
 *   the tracked one.
 * Calls served on such a handle: rnde_node_forward, _forward_replay, _backward, _release_tape, _steps, _attempts_ext, _set_tracking,
 *   _tracking, _timing (solve, reverse sweep, tile reduction; always recorded), _last_attempts, rnde_debug_feval, rnde_node_forward_host / _backward_host, rnde_node_destroy,
 *   rnde_node_tiled_reserve_saveat / _saveat_capacity; and, once a saveat capacity is reserved (below), rnde_node_forward_saveat /
 *   _everystep with the D x n x B backward that follows them, and rnde_debug_arm_replay.
 * Refused with RNDE_ERR_BAD_ARG and a message naming the entry: rnde_node_forward_saveat / _everystep on a handle without a saveat capacity
 *   (every fresh handle), rnde_debug_attempt, rnde_bench_*,
 *   rnde_node_set_coupling, rnde_node_set_matrix_mode(h, 1), rnde_node_classifier_grad, rnde_node_backward_async; a tape pool
 *   (rnde_tapes_create) holds rnde_node_create instances only.  A meeting of the solve or of the tracked reverse sweep that times out is
 *   RNDE_ERR_HIP with a message that says which; nothing falls back to other arithmetic. */
rnde_status rnde_node_create_tiled(const rnde_node_config* cfg, rnde_node** out);
int64_t     rnde_node_tiled_lds_bytes(const rnde_node_config* cfg);

/* Which reverse sweep the taped forwards of a TILED handle get, set after creation (any regularize).  (0, 0): the default, step sizes and
 * times constants, bit for bit the sweep of a handle that was never switched.  (1, 0): the step-size controller and the clamps to t1 are
 * differentiated, the first proposed step is a constant.  (1, 1): the initial-step rule as well -- the reference's gradient (its Tracker
 * tapes the solver's scalar arithmetic).  The tape remembers the setting of its forward; rnde_node_backward runs the sweep the tape asks
 * for and tspan_bar_host receives (t0-bar, t1-bar) from a tracked tape, (0, 0) otherwise.  A tracked replay tape is differentiated as if
 * the controller had produced the sequence.  Refused with RNDE_ERR_BAD_ARG and a message, before any launch: (0, 1) (with the controller
 * a constant the first step reaches nothing), values other than 0 / 1, a handle of rnde_node_create (those engines take cfg.track_ctrl /
 * cfg.track_initdt), a handle that holds a tape, and -- when tracking is first switched on with max_batch above 512 -- a device that does
 * not hold max_batch / 16 workgroups of the tracked sweep at once.  rnde_node_tracking reads the setting back (a handle of
 * rnde_node_create: its config's flags). */
rnde_status rnde_node_set_tracking(rnde_node* h, int32_t track_ctrl, int32_t track_initdt);
rnde_status rnde_node_tracking(const rnde_node* h, int32_t* ctrl_out, int32_t* initdt_out);

/* Saved points on a TILED handle, switched on after creation by a capacity: room for up to max_saveat save times per call (the device copy
 * of the times, the tape's own copy, one range of save indices per attempt for the reverse sweep).  On a handle with a capacity
 * rnde_node_forward_saveat is served as described below -- times increasing inside [t0, t1], a first time equal to t0 yields x, output
 * D x n_saveat x B -- by the one-launch solve: behind the controller of an accepted attempt every tile writes the states of that step's
 * save times (unew itself at the step's end, the Tsit5 dense output inside it); the times never enter the controller, so the attempts are
 * the end-state solve's bit for bit.  rnde_node_forward_everystep runs through it twice (its own description); rnde_node_backward after a
 * taped saving forward takes u_bar_dev D x n x B and runs the sweep the tape's tracking setting asks for: (0, 0) with step sizes and times
 * constants and tspan_bar = (0, 0), tracked with the cotangents of theta = (ts - t) / dt in the attempt's sums and the real tspan_bar.
 * n_saveat (or the step ends of _everystep) above the capacity: RNDE_ERR_BAD_ARG naming both numbers.  End-state calls on the handle are
 * the kernels and the bits of a handle that never reserved.  max_saveat = 0 releases: the handle refuses saving calls again exactly as a
 * fresh one.  Refused by name with RNDE_ERR_BAD_ARG, before any launch: a handle of rnde_node_create (its engines need no reservation), a
 * handle that holds a tape, max_saveat < 0 or above cfg.max_attempts + 1, and -- max_batch above 512 -- a device that does not hold
 * max_batch / 16 workgroups of the saving kernels at once.  rnde_node_tiled_saveat_capacity: the capacity, 0 for a tiled handle without
 * one, -1 for NULL or a handle of rnde_node_create. */
rnde_status rnde_node_tiled_reserve_saveat(rnde_node* h, int32_t max_saveat);
int32_t     rnde_node_tiled_saveat_capacity(const rnde_node* h);

/* Forward solve on [t0,t1].  u_out_dev: D x B.  saveval_host (may be NULL when regularize==0):
 * room for max_attempts+1 floats.  keep_tape != 0 records what rnde_node_backward needs.
 * nfe_out = sol.destats.nf (neural_ode.jl:72,:142).  Synchronises `stream` before returning. */
rnde_status rnde_node_forward(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B,
                              float t0, float t1, float* u_out_dev, int64_t* nfe_out,
                              float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape,
                              void* stream);

/* The {R,true} call methods (reference src/models/neural_ode.jl:79-108, :146-180 and update_saveat! :35-46): same
 * solve, returning the state at every time of `saveat` (increasing, inside [t0,t1]) from the Tsit5 dense output.
 * u_saved_dev: D x n_saveat x B, column-major, exactly what diffeqsol_to_3dtrackedarray builds (src/utils.jl:17-19).
 * With a taped saveat forward, rnde_node_backward takes u_bar_dev of that same D x n_saveat x B shape. */
rnde_status rnde_node_forward_saveat(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B,
                                     float t0, float t1, const float* saveat_host, int32_t n_saveat,
                                     float* u_saved_dev, int64_t* nfe_out, float* saveval_host,
                                     int32_t* n_saveval_out, int32_t keep_tape, void* stream);

/* save_everystep = true (reference src/models/neural_ode.jl:10-11: the other way to `return_multiple`): the state after every accepted step, and
 * the initial state first when save_start != 0 -- sol_out_dev: D x n x B, column-major, n <= capacity returned in *n_out together with the times
 * (t_host_out: room for `capacity` floats, may be NULL).  The number of steps is known only after the solve, so the call solves twice (the step
 * sequence, then the same solve saving at those step ends: u_new itself, no interpolation); the rest as rnde_node_forward_saveat, including the
 * backward call afterwards (u_bar_dev: D x n x B).  More accepted steps than `capacity`: RNDE_ERR_BAD_ARG with *n_out set to the room needed. */
rnde_status rnde_node_forward_everystep(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1,
                                        int32_t save_start, float* sol_out_dev, int32_t capacity, float* t_host_out, int32_t* n_out,
                                        int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape, void* stream);

/* Parity instrument: the same solve along a GIVEN sequence of attempts.  steps_host holds n_steps pairs
 * (dt_proposed, accepted != 0): attempt n runs with min(dt_proposed[n], t1 - t) and is accepted or rejected as told, and
 * the solve ends after n_steps attempts; the error estimate, q11 and q of every attempt are still computed and logged
 * (rnde_node_steps), the saving callback still fires per accepted step, the tape is recorded and rnde_node_backward
 * differentiates the recorded program as if the controller had produced the sequence.  At the reference tolerance
 * (reltol = abstol = 1.4e-8, experiments/mnist_node.jl:121-124) the fp32 error estimate sits on its rounding floor, so
 * two fp32 implementations choose different step sequences; replaying ONE sequence (e.g. the fp32 CPU solver's) is how
 * trajectories and gradients are compared element-wise there (tests/test_gpu_replay.py).  Not a reference entry point. */
rnde_status rnde_node_forward_replay(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B,
                                     float t0, float t1, const float* steps_host, int32_t n_steps,
                                     float* u_out_dev, int64_t* nfe_out, float* saveval_host,
                                     int32_t* n_saveval_out, int32_t keep_tape, void* stream);

/* Parity instrument for saved points: the NEXT rnde_node_forward_saveat on this handle runs along the given sequence of attempts (steps_host:
 * n_steps pairs as for rnde_node_forward_replay, copied), then the handle is back to its controller; n_steps = 0 disarms.  Every engine: the
 * solves read the handle's replay state whether they save or not, and rnde_node_forward_replay, which sets it for its own call only, has no
 * saving form.  Not a reference entry point. */
rnde_status rnde_debug_arm_replay(rnde_node* h, const float* steps_host, int32_t n_steps);

/* Reverse pass of the last recorded forward.  u_bar_dev: D x B cotangent of u_out;
 * saveval_bar_host: one cotangent per saveval element (NULL = zeros).
 * Outputs: x_bar_dev (D x B), p_bar_dev (P, overwritten), tspan_bar_host[2] (may be NULL).
 * Synchronises `stream` before returning. */
rnde_status rnde_node_backward(rnde_node* h, const float* u_bar_dev, const float* saveval_bar_host,
                               float* x_bar_dev, float* p_bar_dev, float* tspan_bar_host,
                               void* stream);

/* The same reverse pass WITHOUT the final synchronisation: outputs are valid in stream order (x_bar_dev, p_bar_dev, and
 * tspan_bar_dev[2] when not NULL -- a DEVICE pointer here), the call returns as soon as the work is enqueued, so the caller
 * can queue the optimiser update and the next forward underneath the tail of this one (a training loop that never reads the
 * loss on the host has no reason to stop the GPU once per step).  A failure that only the GPU can report (a persistent
 * kernel abandoning a hand-off) surfaces as RNDE_ERR_HIP from the NEXT call on the handle. */
rnde_status rnde_node_backward_async(rnde_node* h, const float* u_bar_dev, const float* saveval_bar_host,
                                     float* x_bar_dev, float* p_bar_dev, float* tspan_bar_dev, void* stream);

rnde_status rnde_node_release_tape(rnde_node* h);

/* Host-pointer convenience variants (H2D/D2H copies inside; PCIe-inclusive). */
rnde_status rnde_node_forward_host(rnde_node* h, const float* x, const float* p, int32_t B, float t0,
                                   float t1, float* u_out, int64_t* nfe_out, float* saveval,
                                   int32_t* n_saveval_out, int32_t keep_tape);
rnde_status rnde_node_backward_host(rnde_node* h, const float* u_bar, const float* saveval_bar,
                                    float* x_bar, float* p_bar, float* tspan_bar);

/* Per-attempt log of the last forward: 4 floats per attempt (t, dt, EEst, accepted). */
rnde_status rnde_node_steps(rnde_node* h, float* steps_host, int32_t capacity, int32_t* n_attempts_out);
/* The same log with the controller's side of it: 6 floats per attempt (t, dt, dtp_in, EEst, accepted, q) -- dtp_in the step the controller
 * proposed (dt = min(dtp_in, t1 - t)), q its step-size factor.  Every engine.  out_host NULL: the count only; capacity below the attempt
 * count: RNDE_ERR_BAD_ARG.  (dtp_in, accepted) replays the solve through rnde_node_forward_replay with the same clamp to t1.) */
rnde_status rnde_node_attempts_ext(rnde_node* h, float* out_host, int32_t capacity, int32_t* n_attempts_out);

/* Kernel-level entry points used by the parity tests and by bench.py's roofline leg.
 * rnde_debug_attempt: ONE Tsit5 attempt (6 f evaluations + error estimate) from a given
 * (uprev, k1, t, dt); k_out_dev receives k2..k7 (6 x D x B), unew_out_dev D x B.
 * rnde_debug_feval: out = f(u, p, t).
 * rnde_bench_attempt: runs `iters` back-to-back launches of the step kernel on the handle's
 * workspace and returns the mean kernel time in microseconds measured with HIP events on
 * `stream` (the same kernel rocprofv3 reports as rnde_step_kernel). */
rnde_status rnde_debug_feval(rnde_node* h, const float* u_dev, const float* p_dev, int32_t B, float t,
                             float* out_dev, void* stream);
rnde_status rnde_debug_attempt(rnde_node* h, const float* uprev_dev, const float* k1_dev,
                               const float* p_dev, int32_t B, float t, float dt, float* k_out_dev,
                               float* unew_out_dev, float* eest_out, void* stream);
/* The element-wise device functions every kernel goes through, one at a time: out[i] = fn(in[i]) for i < n, by the functions in the kernels'
 * own headers (no copies), so that a test can take each of them to its thresholds, to saturation, and to +-0, subnormals, +-Inf and NaN.
 *   TANH_FAST        tanh_fast(in)                                   TANH_F / SIGMOID_F   the latent-ODE encoder's tanh and sigmoid
 *   TANH_FAST2_X/_Y  that lane of tanh_fast2, the other lane = in2   FF_SOFTPLUS          the ConcatSquash dynamics' softplus
 *   PRE_FWD / PRE_BWD   the map in front of a chain and its derivative times the cotangent in2; code = rnde_pre_act
 *   ACT_FWD / ACT_DY / ACT_D2Y   a Dense activation, and its first and second derivative FROM THE OUTPUT in; code = rnde_act
 * in2_dev is read by TANH_FAST2_* and PRE_BWD only (NULL otherwise); code is 0 where it selects nothing.  No handle: rnde_last_error(NULL)
 * explains a refusal.  An unknown selector, a code outside its enum, a negative n or a NULL operand is RNDE_ERR_BAD_ARG; n = 0 is RNDE_OK and
 * touches nothing.  Returns after the kernel has finished. */
typedef enum { RNDE_EW_TANH_FAST = 0, RNDE_EW_TANH_FAST2_X = 1, RNDE_EW_TANH_FAST2_Y = 2, RNDE_EW_PRE_FWD = 3, RNDE_EW_PRE_BWD = 4,
               RNDE_EW_ACT_FWD = 5, RNDE_EW_ACT_DY = 6, RNDE_EW_ACT_D2Y = 7, RNDE_EW_TANH_F = 8, RNDE_EW_SIGMOID_F = 9,
               RNDE_EW_FF_SOFTPLUS = 10 } rnde_elementwise_fn;
rnde_status rnde_debug_elementwise(int32_t fn, int32_t code, const float* in_dev, const float* in2_dev, int64_t n, float* out_dev,
                                   void* stream);
rnde_status rnde_bench_attempt(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B,
                               int32_t iters, float* mean_us_out, void* stream);
/* The same with the tape stores a training step's forward performs (keep_tape != 0): the kernel variant that dominates a
 * training step, which is what bench.py's roofline object is computed from. */
rnde_status rnde_bench_attempt_taped(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B,
                                     int32_t iters, float* mean_us_out, void* stream);
/* The same with a COLD tape: attempt i writes record i mod `records` of the arena (records >= 2), as the attempts of a solve do (31 records
 * of 21.7 MB at B = 512 per solve: the tape does not stay on the chip), where rnde_bench_attempt_taped rewrites record 0 for ever (it then
 * lives in the Infinity Cache).  Stage engine; this is the figure that agrees with the per-attempt time inside a training step. */
rnde_status rnde_bench_attempt_cold_tape(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, int32_t iters,
                                         int32_t records, float* mean_us_out, void* stream);
/* Measurement aid: with timing on, every forward / reverse records HIP events on the caller's stream around (a) the attempted
 * steps of the forward solve, (b) the reverse sweep, (c) the rest of the reverse pass (parameter-gradient GEMMs after the
 * sweep + reductions); rnde_node_timing waits for them and returns the three durations in ms (-1 = not recorded). */
rnde_status rnde_node_set_timing(rnde_node* h, int32_t on);
rnde_status rnde_node_timing(rnde_node* h, float* fwd_attempts_ms, float* rev_sweep_ms, float* rev_rest_ms);
int32_t     rnde_node_last_attempts(const rnde_node* h);   /* attempted steps of the last forward */
/* How often the one-launch attempt kernels gave up a hand-off (co-tenant on the CUs for > 1 s) and the handle went to the
 * 7-launch kernels; it returns to the one-launch kernels after 8, 16, 32, ... clean solves (not sticky). */
int32_t     rnde_node_fallback_count(const rnde_node* h);
/* How the handle currently runs one attempted step: number of kernel launches (1: rnde_stage_attempt_kernel /
 * rnde_step_kernel / rnde_chain_kernel; 7: rnde_stage_kernel START, 5 x STAGE, LAST) -- bench.py's roofline bookkeeping. */
int32_t     rnde_node_launches_per_attempt(const rnde_node* h);
/* How many forward solves of this handle ran as ONE kernel launch (attempt loop, PI controller and error-norm meeting inside the kernel:
 * rnde_stage_solve_kernel for the MNIST form at <= 512 columns, MW_SOLVE for the Dense-chain and SDE engines) -- the launch that replaces
 * the body of `solve(prob, Tsit5(); ...)`, reference src/models/neural_ode.jl:131-137.  bench.py's roofline bookkeeping and the tests. */
int32_t     rnde_node_one_launch_solves(const rnde_node* h);
/* How many launches of this handle took one of the folded forms around the two sweeps, in the order of their switches: counts[0]
 * RNDE_REDUCE_FOLD (the weight-gradient reduction's two passes as one launch), [1] RNDE_WGRAD_PAIR (both layers' weight-gradient launches behind the
 * sweep as one), [2] RNDE_X3_PACK_FOLD (the x3 weight split inside the pack launch), [3] RNDE_BINIT_PAIR (launches of rnde_binit_pair_kernel: two per
 * reverse pass).  For the tests, which must know that the form they compare actually ran. */
void        rnde_node_tail_folds(const rnde_node* h, int64_t counts[4]);
/* Which arithmetic unit forms the Dense-layer products of the stage engine -- the f(u, p, t) evaluations inside `solve(prob, Tsit5(); ...)`, reference
 * src/models/neural_ode.jl:131-137 with the dynamics of experiments/mnist_node.jl:41-54, their transposes in the reverse pass and the parameter-gradient GEMMs:
 *   RNDE_MATRIX_F32   (0) the fp32-input MFMA v_mfma_f32_16x16x4_f32 -- on gfx950 an instruction of the VECTOR ALUs (64 FLOP/clk/SIMD, no overlap with
 *                         other vector work: tools/micro/coexec.hip); bit-identical to the launch-per-attempt kernels and mirrored by the oracle's
 *                         device-order mode;
 *   RNDE_MATRIX_BF16X3 (1, default where it applies: the MNIST form D = 784, H = 100 on the persistent kernels, any batch) both operands split EXACTLY into three bf16 numbers, the six
 *                         leading cross products on the matrix cores (v_mfma_f32_16x16x32_bf16), fp32 accumulation: csrc/rnde_x3.h.  Closer to the fp64
 *                         restatement than mode 0 (fewer roundings per dot product), hence FEWER attempted steps at the reference tolerance, where
 *                         the step size is set by rounding noise; not bit-identical to mode 0.
 * The environment variable RNDE_X3 (0 / 1) sets the default of new handles.  Returns BAD_ARG for an unknown mode; a handle whose geometry the
 * bf16x3 kernels do not serve keeps mode 0 and says so through rnde_node_matrix_mode. */
#define RNDE_MATRIX_F32 0
#define RNDE_MATRIX_BF16X3 1
rnde_status rnde_node_set_matrix_mode(rnde_node* h, int32_t mode);
int32_t     rnde_node_matrix_mode(const rnde_node* h);

/* ======================================================================================================================
 * Several taped forwards alive at once behind one handle (the `tape_id` form of SURVEY.md 8b).  An rnde_node holds ONE tape; the
 * reference's loop sometimes needs more -- the NFE probe between a forward and its reverse (experiments/mnist_node.jl:245), two
 * batches in flight.  A tape pool is a set of solver instances of one configuration, created on demand (each taped one owns an
 * arena of max_attempts records): rnde_tapes_forward(keep_tape = 1) takes a free one and returns its index as the tape id,
 * rnde_tapes_backward(tape_id) or rnde_tapes_release(tape_id) frees it; keep_tape = 0 runs on an extra instance that never tapes
 * (tape id -1).  Arguments and results are those of rnde_node_forward / rnde_node_backward.
 * ====================================================================================================================== */
typedef struct rnde_tapes rnde_tapes;
rnde_status rnde_tapes_create(const rnde_node_config* cfg, int32_t max_tapes, rnde_tapes** out);
void        rnde_tapes_destroy(rnde_tapes* t);
const char* rnde_tapes_last_error(const rnde_tapes* t);     /* t may be NULL: last create error of this thread */
int32_t     rnde_tapes_in_use(const rnde_tapes* t);
rnde_node*  rnde_tapes_node(rnde_tapes* t, int32_t tape_id);  /* the instance behind a tape id (-1: the untaped one), for the rnde_node_* statistics / tuning calls */
rnde_status rnde_tapes_forward(rnde_tapes* t, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1, float* u_out_dev,
                               int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape, void* stream,
                               int32_t* tape_id_out);
rnde_status rnde_tapes_backward(rnde_tapes* t, int32_t tape_id, const float* u_bar_dev, const float* saveval_bar_host, float* x_bar_dev,
                                float* p_bar_dev, float* tspan_bar_host, void* stream);
rnde_status rnde_tapes_release(rnde_tapes* t, int32_t tape_id);

/* Fused caller of the hot path: postode Dense(D, C) + Flux.Losses.logitcrossentropy and their
 * reverse in one call -- replaces reference src/models/supervised_classification.jl:44-45 + experiments/mnist_node.jl:135
 * and the Tracker reverse of both.  p3 = Flux.destructure(Dense(D, C)) = [vec(W) (C x D col-major); b (C)];
 * y: one-hot C x B.  Outputs: logits (C x B, may be NULL), u_bar = d ce / d u (D x B), p3_bar (C*D + C),
 * ce (device scalar: mean cross entropy).  Asynchronous on `stream`. */
rnde_status rnde_classifier_head(rnde_node* h, const float* u_dev, const float* p3_dev, const float* y_dev,
                                 int32_t B, int32_t n_classes, float* logits_out_dev, float* u_bar_dev,
                                 float* p3_bar_dev, float* ce_out_dev, void* stream);

/* One training-step gradient of the reference's classifier loss in ONE call (experiments/mnist_node.jl:132-137 and :229-233:
 * `loss_function` + `Tracker.gradient` with ClassifierNODE, preode = identity):
 *     u = TrackedNeuralODE(x, p2)  ->  ce = logitcrossentropy(Dense_p3(u), y)  ->  loss = ce + lambda * mean(sv.saveval)
 * = rnde_node_forward (taped) + rnde_classifier_head + rnde_node_backward_async, with the head and the weight packs of the reverse
 * sweep queued BEFORE the forward's host wait, so the GPU does not idle while the host reads the step log and launches the sweep
 * (the three separate calls leave ~80 us of a 2.4 ms step idle at B = 512).  Stage engine only (two-layer dynamics, col_tile 0).
 * Outputs: p2_bar_dev (P), p3_bar_dev (C*D + C), x_bar_dev (D x B, may be NULL), ce_out_dev (device scalar), *reg_out_host =
 * lambda * mean(saveval) and *nfe_out (host, valid on return: the step log has been read); lambda = 0: no regulariser cotangent.
 * comm != NULL: both gradients are sum-all-reduced in place behind the reverse pass (rnde_comm_allreduce, mean = 0) -- in ONE call when
 * p3_bar_dev == p2_bar_dev + P (one flat buffer [p2-bar | p3-bar]), else in two.  Asynchronous from the reverse pass on, like
 * rnde_node_backward_async. */
rnde_status rnde_node_classifier_grad(rnde_node* h, const float* x_dev, const float* p2_dev, const float* p3_dev,
                                      const float* y_dev, int32_t B, int32_t n_classes, float t0, float t1, float lambda,
                                      float* p2_bar_dev, float* p3_bar_dev, float* x_bar_dev, float* ce_out_dev,
                                      float* reg_out_host, int64_t* nfe_out, rnde_comm* comm, void* stream);

/* The evaluation call of ClassifierNODE (reference src/metrics.jl:2-18 around src/models/supervised_classification.jl:40-46;
 * experiments/mnist_node.jl:185-186, :250-251 run it over both loaders at the end of every epoch): the UNTAPED solve (rnde_node_forward with
 * keep_tape = 0, into a workspace the handle owns; like every untaped forward it drops a tape the handle holds), postode Dense(D, C) on the
 * end state -> logits_out_dev (C x B, required) and, when y_dev (C x B) is given, the number of inputs whose predicted class -- the FIRST
 * index of the largest logit, Julia's argmax -- equals the first index of the largest entry of y's column, ADDED to the device int64
 * *correct_dev (the caller zeroes it once per data set and reads it once).  y_dev may be NULL; correct_dev may be NULL and must be NULL
 * when y_dev is (RNDE_ERR_BAD_ARG).  The logits are the bits rnde_classifier_head computes from the same end state.
 * ONE head launch does logits, both argmaxes and the count.  Without labels it is queued in front of the solve's host wait (a solve that is
 * redone queues it again and only overwrites logits_out_dev); WITH labels the fused count is kept and the counting variant is queued exactly
 * once, behind the solve's final status, so a redone solve never counts twice.
 * Served on every engine rnde_node_forward(keep_tape = 0) serves: the stage engine in both matrix modes, the chain engine, the tiled engine.
 * Limits, checked before anything is launched: 1 <= B <= cfg.max_batch, 2 <= n_classes <= 16, D <= 1024, t1 > t0.
 * Nothing is read back except what the solve itself reads (its step log): *nfe_out is valid on return, the logits and the counter in
 * stream order. */
rnde_status rnde_node_classifier_predict(rnde_node* h, const float* x_dev, const float* p2_dev, const float* p3_dev,
                                         const float* y_dev, int32_t B, int32_t n_classes, float t0, float t1,
                                         float* logits_out_dev, int64_t* correct_dev, int64_t* nfe_out, void* stream);

/* Optimiser update of the reference's training step, one launch per parameter group:
 * Flux.Optimise.Optimiser(InvDecay(gamma), Momentum(eta, rho)) applied by update_parameters! -- replaces reference
 * experiments/mnist_node.jl:130 + src/utils.jl:149-156 for one flat group:
 *     g' = g / (1 + gamma * n);   v = rho * v - eta * g';   p = p + v          (n = the group's InvDecay counter, >= 1)
 * p, g, v: device vectors of `len` floats; in place on p and v.  No handle: pure function of its arguments, asynchronous. */
rnde_status rnde_momentum_step(float* p_dev, const float* g_dev, float* v_dev, int64_t len, int64_t n, float gamma,
                               float eta, float rho, void* stream);

/* The same update with the gradient scaled first: g' = gscale * g / (1 + gamma * n).  gscale = 1 / world folds the averaging of a
 * sum-all-reduced gradient (rnde_comm_allreduce with mean = 0) into the optimiser launch. */
rnde_status rnde_momentum_step_scaled(float* p_dev, const float* g_dev, float* v_dev, int64_t len, int64_t n, float gamma,
                                      float eta, float rho, float gscale, void* stream);
/* Flux.Optimise.ADAM(eta, (beta1, beta2)) (the optimiser of reference experiments/mnist_nsde.jl) on one flat parameter group, one launch:
 * m = beta1 m + (1 - beta1) g ; v = beta2 v + (1 - beta2) g^2 ; p -= eta (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps), with g
 * scaled by gscale first (1 / world after a sum-all-reduce).  t = 1, 2, ... is the step being taken; m, v start at zero. */
rnde_status rnde_adam_step(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t len, int64_t t, float eta, float beta1,
                           float beta2, float eps, float gscale, void* stream);
/* Flux.Optimise.Optimiser(WeightDecay(wd), ADAM(eta, (beta1, beta2))) (the optimiser of reference experiments/ffjord_gaussian.jl:132 and
 * ffjord_tabular.jl:133) on one flat group, one launch: g' = gscale * g + wd * p, then the recurrence of rnde_adam_step on g'.  With wd = 0
 * and finite p it produces the bits of rnde_adam_step. */
rnde_status rnde_adam_wd_step(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t len, int64_t t, float eta, float beta1,
                              float beta2, float eps, float gscale, float wd, void* stream);
/* Flux.Optimise.AdaBelief(eta, (beta1, beta2)) (the optimiser of reference experiments/sde_toy_problem.jl:65, Flux 0.11.6 as pinned by the
 * reference's Manifest) on one flat parameter group, one launch, g scaled by gscale first:
 *     m = beta1 m + (1 - beta1) g ;  s = beta2 s + (1 - beta2) (g - m)^2 ;  p -= eta m / (sqrt(s) + eps)
 * with the m of this step inside (g - m), no bias correction, eps = 1e-8 there.  [RECALL] Flux 0.11.6's apply! for AdaBelief, as recalled:
 * its source is not available offline to check against.  m, s start at zero.  No handle, asynchronous. */
rnde_status rnde_adabelief_step(float* p_dev, const float* g_dev, float* m_dev, float* s_dev, int64_t len, float eta, float beta1, float beta2,
                                float eps, float gscale, void* stream);

/* ======================================================================================================================
 * Data parallelism: the one collective of a training step.  The reference is single-process; with the
 * minibatch sharded by columns over the GPUs of a node (one process per GPU, each integrating its shard with its own
 * controller), the only exchange is a sum of the flat gradient between Tracker.gradient and update_parameters!
 * (reference experiments/mnist_node.jl:229-233, src/utils.jl:149-156).  rnde_comm_* gives a non-Python caller that
 * collective from this library: RCCL over xGMI on the caller's stream.  RCCL is bound at run time (dlopen): no link-time
 * dependency, never loaded by single-GPU users.
 *   rank 0: rnde_comm_unique_id(id) -> ship the 128 bytes to the other ranks by any means (Julia: Distributed / MPI; Python:
 *   the torch.distributed store) -> every rank: rnde_comm_create(id, rank, world, device, &c) (collective: blocks until all
 *   ranks arrive) -> per step: rnde_comm_allreduce(c, grad_dev, n, mean, stream) -> rnde_comm_destroy(c).
 * ====================================================================================================================== */
#define RNDE_COMM_ID_BYTES 128
rnde_status rnde_comm_unique_id(uint8_t id_out[RNDE_COMM_ID_BYTES]);
rnde_status rnde_comm_create(const uint8_t id[RNDE_COMM_ID_BYTES], int32_t rank, int32_t world, int32_t device, rnde_comm** out);
void        rnde_comm_destroy(rnde_comm* c);
int32_t     rnde_comm_world(const rnde_comm* c);
const char* rnde_comm_last_error(const rnde_comm* c);   /* c may be NULL: last create / id error of this thread */
/* The file the collective library was bound from (an RCCL already loaded in the process -- e.g. the copy PyTorch bundles -- is reused
 * rather than a second instance loaded beside it), or the load error. */
const char* rnde_comm_library(void);
/* In-place sum of n floats over the ranks (mean != 0: followed by a scale by 1 / world), asynchronous on `stream`.
 * MNIST-NODE payload: 166,418 floats = 665,672 B in ONE call (latency bound: one contiguous buffer). */
rnde_status rnde_comm_allreduce(rnde_comm* c, float* buf_dev, int64_t n, int32_t mean, void* stream);
/* `world` ranks that live in ONE process on ONE device (out[world]): same interface, the all-reduce is a one-workgroup kernel
 * per rank meeting the others through device memory (n <= 8192 floats).  What the coupled controller below is tested with on a
 * single GPU (two host threads, two handles), and what several shards per device would use. */
rnde_status rnde_comm_create_local_group(int32_t world, int32_t device, rnde_comm** out);
/* RNDE_OK unless an all-reduce of this communicator gave up waiting for a rank (in-process groups and the one-shot path; blocking:
 * call after the stream has been synchronised).  The coupled solves below check it themselves at their synchronisation points.
 * One-shot path: a time-out is STICKY -- the kernel that gave up and every later one fill their buffer with NaN instead of a partial sum,
 * and every rnde_comm_allreduce enqueued after the time-out became visible to the host returns RNDE_ERR_HIP (rnde_comm_last_error names the
 * limit in force: 20 s, RNDE_ONESHOT_TIMEOUT_MS overrides it).  Its all-reduces may be enqueued on different streams: a call on another
 * stream than the previous one is ordered behind it with an event (RCCL has no such constraint). */
rnde_status rnde_comm_health(rnde_comm* c);
/* One-shot all-reduce over peer-mapped windows (the 0.67 MB gradient message is latency bound, so each rank reads
 * the N - 1 peers' copies directly over its xGMI links in ONE kernel and sums them in rank order -- the same bits on every rank --
 * instead of walking a ring).  Every rank owns a window in its HBM, exported with hipIpcGetMemHandle and mapped by all peers
 * (world <= 16, one process per rank, all on one node).  OPT-IN until it has been measured on N > 1 GPUs; two ways in:
 *   RNDE_ONESHOT=1 in the environment of rnde_comm_create: the handles travel through the RCCL communicator that call builds (one
 *     64-byte all-gather); all-reduces of n <= 262,144 floats then take the one-shot kernel, larger ones ncclAllReduce;
 *   rnde_comm_window_create(device, &win, handle) on every rank -> ship the 64 bytes to all ranks by any means ->
 *     rnde_comm_create_peers(win, handles_in_rank_order, rank, world, &c) (takes ownership of win on success): no RCCL at all; larger buffers go
 *     in pieces of 262,144 floats.
 * rnde_comm_path says which path a communicator's all-reduces take. */
#define RNDE_COMM_WINDOW_BYTES 64
typedef struct rnde_comm_window rnde_comm_window;
rnde_status rnde_comm_window_create(int32_t device, rnde_comm_window** win_out, uint8_t handle_out[RNDE_COMM_WINDOW_BYTES]);
void        rnde_comm_window_destroy(rnde_comm_window* w);   /* only for a window that was NOT handed to rnde_comm_create_peers */
rnde_status rnde_comm_create_peers(rnde_comm_window* win, const uint8_t* handles, int32_t rank, int32_t world, rnde_comm** out);
const char* rnde_comm_path(const rnde_comm* c);

/* SURVEY.md 8e mode 2 -- ONE controller for all shards: with the minibatch split by columns over `world` handles, the error norm
 * that drives the step size is the RMS over ALL D x B_global entries (what a single-device run at B_global computes), so every
 * shard takes the same (dt, accept) sequence and the sharded run reproduces the single-device one up to the order of the sums.
 * After rnde_node_set_coupling(h, c, global_batch) every launch that produces per-workgroup partial sums of a batch-wide norm --
 * the two of the initial-step rule, each attempted step, each reversed attempt, the reverse of the initial-step rule -- is
 * followed by rnde_comm_allreduce(c, partials) on the solve's stream, the norms are means over D x global_batch, and the cotangents
 * of the saved values are multiplied by world (each rank passes the cotangent of ITS loss, whose data term is a mean over its own
 * columns: with this the usual average of the ranks' gradients is the gradient of the single-device loss).  One small collective
 * per attempted step: the parity option, not the fast path (default: independent controllers, rnde_node_set_coupling(h, NULL, 0)).
 * Every rank must make the same calls in the same order and hold the same number of columns (equal shards: the partial arrays are
 * summed element-wise).  Engines: the stage engine (MNIST-form networks) and the chain engine's multi-wave kernels (Dense chains of
 * width <= 64, one launch per attempt -- the one-launch solve keeps its controller in the kernel and is not used when coupled). */
rnde_status rnde_node_set_coupling(rnde_node* h, rnde_comm* c, int32_t global_batch);

/* ======================================================================================================================
 * TrackedNeuralDSDE: the stochastic layer (reference src/models/neural_sde.jl:1-146; caller ClassifierNSDE,
 * src/models/supervised_classification.jl:82-103; experiment experiments/mnist_nsde.jl:70-100).
 *   rnde_nsde_create    TrackedNeuralDSDE(model1, model2, tspan, regularize, solver; kw...)   neural_sde.jl:13-41
 *   rnde_nsde_forward / rnde_nsde_forward_saveat   (n::TrackedNeuralDSDE{R,false / true})(x, p; func): the `solve(SDEProblem{false}(...), SOSRI(); callback, ...)`
 *                       between :98 and :108 (and :54-56 for the unregularised method), returning what :109-113 unpack:
 *                       u (D x B), nfe1, nfe2 (the closures' counters, :46,:50) and the saved EEst*dt values
 *   rnde_nsde_backward  the reverse sweep Tracker performs over that solve (sensealg = SensitivityADPassThrough, :104)
 * p = vcat(destructure(model1), destructure(model2)) (:15-17): the drift chain's parameters, then the diffusion chain's.
 * Diagonal noise: the diffusion chain maps D -> D and multiplies the increments element-wise (:49-52).
 * Noise: a pool of standard normals, n_pool draws of 2*D*B floats each (xi_W block then xi_Z block, both D x B column-major),
 * consumed in order -- draw 0 makes the first increments, every later accepted step that needs fresh or bridged noise and
 * every rejected step takes the next one (at most 1 + attempts draws).  noise_dev = NULL: the library fills its own pool
 * from `seed` (Philox4x32-10 + Box-Muller); a caller that wants its own random stream (Julia: randn!) passes the pool.
 * ====================================================================================================================== */
typedef enum { RNDE_SDE_SOSRI = 0, RNDE_SDE_SRIW1 = 1, RNDE_SDE_SOSRI2 = 2 } rnde_sde_solver;

typedef struct {
    int32_t drift_layers;                       /* Dense chain of the drift, time independent (neural_sde.jl:45-47) */
    int32_t drift_dims[RNDE_MAX_LAYERS + 1];    /* drift_dims[0] = drift_dims[drift_layers] = D; every width <= 64 */
    int32_t drift_act[RNDE_MAX_LAYERS];         /* rnde_act per layer */
    int32_t diff_layers;                        /* Dense chain of the diffusion (neural_sde.jl:49-52) */
    int32_t diff_dims[RNDE_MAX_LAYERS + 1];
    int32_t diff_act[RNDE_MAX_LAYERS];
    int32_t max_batch;                          /* largest B (= batch x trajectories) any call will pass */
    int32_t solver;                             /* rnde_sde_solver: the tableau */
    float   reltol, abstol;                     /* experiments/mnist_nsde.jl:79-80 */
    int32_t regularize;                         /* what the saving callback records per accepted step: RNDE_REG_NONE, RNDE_REG_ERR (func = EEst*dt,
                                                 * neural_sde.jl:87, experiments/mnist_nsde.jl:48) or RNDE_REG_STIFF (|eigen_est| / stability_size,
                                                 * mnist_nsde.jl:51-61 -- what the shipped configs/mnist_nsde.yml:6 selects; SOSRI2 only:
                                                 * eigen_est = rms(k4 - k3) / rms(H0_4 - H0_3), the estimate AutoSOSRI2(SOSRI2()) fills) */
    int32_t cb_save_start;                      /* 1: the saving callback also fires at initialisation (pushes 0) */
    int32_t max_attempts;
    int32_t device;
    /* controller constants, 0 = the StochasticDiffEq defaults as recalled: beta2 = 2/(5 order),
     * beta1 = 7/(10 order), order = 3/2, gamma = 0.9, qmin = 0.2, qmax = 1.125, qoldinit = 1e-4, delta = 1 (SRIW1: 1/6) */
    float   beta1, beta2, gamma, qmin, qmax, qoldinit, delta;
    int32_t generic;                            /* 1 = never use the instantiations with the reference's shape (32 -> 64 -> 32, 32 -> 32)
                                                 * as compile-time constants (A/B runs, parity tests of the generic kernels) */
    float   stability_size;                     /* RNDE_REG_STIFF: the constant the estimate is divided by; 0 = StochasticDiffEq.alg_stability_size(SOSRI2())
                                                 * = 10.6 (mnist_nsde.jl:54-55) */
} rnde_nsde_config;

typedef struct rnde_nsde rnde_nsde;

int32_t     rnde_nsde_param_count(const rnde_nsde_config* cfg, int32_t* len_drift_out);
rnde_status rnde_nsde_create(const rnde_nsde_config* cfg, rnde_nsde** out);
void        rnde_nsde_destroy(rnde_nsde* h);
const char* rnde_nsde_last_error(const rnde_nsde* h);   /* h may be NULL: last create error of this thread */

/* Forward solve on [t0, t1].  x_dev, u_out_dev: D x B.  saveval_host: room for max_attempts + 1 floats (may be NULL when
 * regularize == 0).  nfe1_out = drift evaluations, nfe2_out = diffusion evaluations (2 + 4 per attempted step each).
 * keep_tape != 0 records what rnde_nsde_backward needs.  Synchronises `stream` before returning. */
rnde_status rnde_nsde_forward(rnde_nsde* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1,
                              const float* noise_dev, int32_t n_pool, uint64_t seed, float* u_out_dev,
                              int64_t* nfe1_out, int64_t* nfe2_out, float* saveval_host, int32_t* n_saveval_out,
                              int32_t keep_tape, void* stream);
/* The {R,true} call methods (neural_sde.jl:44-61, :84-113; experiments/sde_toy_problem.jl:50-60): the same solve, returning the
 * state at every time of `saveat` (increasing, inside [t0, t1]) as the D x n_saveat x B array diffeqsol_to_3dtrackedarray builds
 * (src/utils.jl:17-19).  Points inside a step come from the SDE solution's linear interpolant (StochasticDiffEq has no
 * higher-order dense output), a save time equal to t0 is x.  rnde_nsde_backward then takes u_bar_dev of that D x n_saveat x B shape. */
rnde_status rnde_nsde_forward_saveat(rnde_nsde* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1,
                                     const float* noise_dev, int32_t n_pool, uint64_t seed, const float* saveat_host,
                                     int32_t n_saveat, float* u_saved_dev, int64_t* nfe1_out, int64_t* nfe2_out,
                                     float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape, void* stream);

/* save_everystep = true of the SDE layer (reference src/models/neural_sde.jl:14): as rnde_node_forward_everystep -- the state after every accepted
 * step (t0 first when save_start != 0), D x n x B with n <= capacity in *n_out and the times in t_host_out (may be NULL); two solves on the same
 * noise inside.  rnde_nsde_backward afterwards takes the D x n x B cotangent. */
rnde_status rnde_nsde_forward_everystep(rnde_nsde* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1,
                                        const float* noise_dev, int32_t n_pool, uint64_t seed, int32_t save_start, float* sol_out_dev,
                                        int32_t capacity, float* t_host_out, int32_t* n_out, int64_t* nfe1_out, int64_t* nfe2_out,
                                        float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape, void* stream);
/* Parity instrument (as rnde_node_forward_replay): the solve along n_steps given (dt, accepted != 0) pairs. */
rnde_status rnde_nsde_forward_replay(rnde_nsde* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1,
                                     const float* noise_dev, int32_t n_pool, const float* steps_host, int32_t n_steps,
                                     float* u_out_dev, int64_t* nfe1_out, int64_t* nfe2_out, float* saveval_host,
                                     int32_t* n_saveval_out, int32_t keep_tape, void* stream);
/* Reverse pass of the last recorded forward: u_bar_dev (D x B), saveval_bar_host (one per saveval element, NULL = zeros)
 * -> x_bar_dev (D x B), p_bar_dev (P, overwritten).  Step sizes and noise increments are constants of the reverse pass
 * (the SDE step-size controller strips tracking: DESIGN.md 3.2).  Synchronises `stream` before returning. */
rnde_status rnde_nsde_backward(rnde_nsde* h, const float* u_bar_dev, const float* saveval_bar_host, float* x_bar_dev,
                               float* p_bar_dev, void* stream);
/* The same without the trailing synchronisation (nothing is read back on the host): the optimiser update and the next step can be
 * queued behind it on `stream`; u_bar / x_bar / p_bar must stay alive until the stream has passed them. */
rnde_status rnde_nsde_backward_async(rnde_nsde* h, const float* u_bar_dev, const float* saveval_bar_host, float* x_bar_dev,
                               float* p_bar_dev, void* stream);
/* postsde Dense(D, C) + Flux.Losses.logitcrossentropy and their reverse for ClassifierNSDE with ONE trajectory per input (reference
 * src/models/supervised_classification.jl:96-97, experiments/mnist_nsde.jl): same contract as rnde_classifier_head, D = the SDE's state
 * dimension.  (With several trajectories the logits are averaged first: rnde_nsde_classifier_head_traj below.) */
rnde_status rnde_nsde_classifier_head(rnde_nsde* h, const float* u_dev, const float* p3_dev, const float* y_dev, int32_t B, int32_t n_classes,
                                      float* logits_out_dev, float* u_bar_dev, float* p3_bar_dev, float* ce_out_dev, void* stream);

/* The SDE counterpart of rnde_node_classifier_grad: one training-step gradient of ClassifierNSDE's loss around the solve, ONE trajectory
 * per input (reference src/models/supervised_classification.jl:82-103 with experiments/mnist_nsde.jl's loss_function and Tracker.gradient):
 *     u = TrackedNeuralDSDE(x, p2)  ->  ce = logitcrossentropy(Dense_p3(u), y)  ->  loss = ce + lambda * mean(sv.saveval)
 * = rnde_nsde_forward (taped; noise as there: the caller's pool, or NULL + seed for the library's stream) + rnde_nsde_classifier_head +
 * rnde_nsde_backward_async, the head queued before the forward's host wait.  x is the SDE's initial state (the presde layer's output), x_bar_dev
 * its cotangent (D x B, required: the presde layer's gradient needs it).  *reg_out_host, *nfe1_out, *nfe2_out are valid on return; the gradients and
 * ce_out_dev in stream order. */
rnde_status rnde_nsde_classifier_grad(rnde_nsde* h, const float* x_dev, const float* p2_dev, const float* p3_dev, const float* y_dev,
                                      int32_t B, int32_t n_classes, float t0, float t1, const float* noise_dev, int32_t n_pool,
                                      uint64_t seed, float lambda, float* p2_bar_dev, float* p3_bar_dev, float* x_bar_dev,
                                      float* ce_out_dev, float* reg_out_host, int64_t* nfe1_out, int64_t* nfe2_out, void* stream);
/* ---- ClassifierNSDE with several trajectories per input (reference src/models/supervised_classification.jl:82-100, `trajectories`) ----
 * Layout of the three calls: column j = t * B + b of the expanded batch is trajectory t of input b (Julia's repeat(x, 1, T), :92, :102-103);
 * T trajectories, B inputs.  Limits, checked before anything is launched (RNDE_ERR_BAD_ARG, rnde_nsde_last_error names the limit):
 * T >= 1, B >= 1, B * T <= cfg.max_batch, 2 <= n_classes <= 16.
 *
 * postsde Dense(D, C) on every trajectory, the mean of the logits over the trajectories (:96-98), Flux.Losses.logitcrossentropy (experiments/
 * mnist_nsde.jl) and the Tracker reverse of all three:
 *     z_tb = W3 u_tb + b3,  z_b = (1/T) sum_t z_tb,  ce = (1/B) sum_b -sum_i y_ib logsoftmax(z_b)_i
 *     delta_b = (softmax(z_b) sum_i y_ib - y_b) / B      (y need not be one-hot)
 *     u_bar_tb = W3^T delta_b / T,  W3_bar = (1/T) sum_{t,b} delta_b u_tb^T,  b3_bar = sum_b delta_b
 * u_dev, u_bar_dev: D x (B T); y_dev: C x B; logits_out_dev: C x B, the averaged logits (may be NULL); p3 / p3_bar in the
 * Flux.destructure(Dense(D, C)) layout of rnde_classifier_head; ce_out_dev: one float.  Every sum runs in a fixed order (csrc/rnde_head_traj.h
 * states it), no float atomics: the same bits run to run.  At T = 1 it agrees with rnde_nsde_classifier_head to rounding.  Asynchronous on `stream`. */
rnde_status rnde_nsde_classifier_head_traj(rnde_nsde* h, const float* u_dev, const float* p3_dev, const float* y_dev, int32_t B, int32_t T,
                                           int32_t n_classes, float* logits_out_dev, float* u_bar_dev, float* p3_bar_dev, float* ce_out_dev,
                                           void* stream);
/* rnde_nsde_classifier_grad with T trajectories per input (reference src/models/supervised_classification.jl:92-98 around the solve, with
 * experiments/mnist_nsde.jl's loss_function and Tracker.gradient): x_dev is the presde layer's output for the B inputs, D x B, NOT repeated.
 *     xe = repeat(x, 1, T)  ->  u = TrackedNeuralDSDE(xe, p2)  ->  rnde_nsde_classifier_head_traj  ->  loss = ce + lambda * mean(sv.saveval)
 * = the repeat, rnde_nsde_forward at B T columns (taped; bit for bit the solve of an explicitly repeated input on the same noise),
 * rnde_nsde_classifier_head_traj queued before the forward's host wait, rnde_nsde_backward_async, and the fold
 * x_bar_b = sum_t xe_bar_{tB+b} (added in the order t = 0 .. T-1).  Noise as in rnde_nsde_forward at B T columns: the caller's pool of
 * 2 * D * B * T floats per draw, or NULL + seed.  x_bar_dev: D x B, folded (required).  *reg_out_host, *nfe1_out, *nfe2_out are valid on
 * return; the gradients and ce_out_dev in stream order. */
rnde_status rnde_nsde_classifier_grad_traj(rnde_nsde* h, const float* x_dev, const float* p2_dev, const float* p3_dev, const float* y_dev,
                                           int32_t B, int32_t T, int32_t n_classes, float t0, float t1, const float* noise_dev, int32_t n_pool,
                                           uint64_t seed, float lambda, float* p2_bar_dev, float* p3_bar_dev, float* x_bar_dev,
                                           float* ce_out_dev, float* reg_out_host, int64_t* nfe1_out, int64_t* nfe2_out, void* stream);
/* The evaluation call (reference src/models/supervised_classification.jl:82-100 behind the presde layer; src/metrics.jl:2-9 for the count;
 * experiments/mnist_nsde.jl:154-155 calls it with 10 trajectories over the whole data set every epoch): the repeat of x_dev (D x B, NOT
 * repeated), the UNTAPED solve at B T columns (noise as above), the averaged logits -> logits_out_dev (C x B, required) and, when y_dev
 * (C x B) is given, the number of inputs whose predicted class -- the FIRST index of the largest averaged logit, Julia's argmax -- equals
 * the first index of the largest entry of y's column, ADDED to the device int64 *correct_dev (the caller zeroes it once per data set and
 * reads it once).  y_dev may be NULL; correct_dev may be NULL and must be NULL when y_dev is.  Nothing is read back except the NFE
 * counters the solve returns; logits and the counter in stream order. */
rnde_status rnde_nsde_classifier_predict(rnde_nsde* h, const float* x_dev, const float* p2_dev, const float* p3_dev, const float* y_dev,
                                         int32_t B, int32_t T, int32_t n_classes, float t0, float t1, const float* noise_dev, int32_t n_pool,
                                         uint64_t seed, float* logits_out_dev, int64_t* correct_dev, int64_t* nfe1_out, int64_t* nfe2_out,
                                         void* stream);
/* The moment-matching loss of reference experiments/sde_toy_problem.jl:27-40 on a D x T x B array of saved states (B trajectories):
 *     mu = mean over b of u[:, :, b],  var = sum over b of (u[:, :, b] - mu)^2 / (B - 1)   (Julia's var(...; dims = 3, mean = means): unbiased)
 *     loss_out_dev[0] = l2_means = mean((data_mean - mu)^2),  loss_out_dev[1] = l2_vars = mean((data_var - var)^2)   (means over D x T)
 * data_mean, data_var: D x T.  u_bar_dev (may be NULL): D x T x B, the cotangent of l2_means + l2_vars with respect to u_saved.  B >= 2.
 * Every sum runs in a fixed order (results are the same bits run to run).  ONE launch of one workgroup, asynchronous on `stream`; no handle.
 * That workgroup walks the D x T pairs serially (512 at a time): right for the toy's 2 x 30 x 100, slow for large arrays. */
rnde_status rnde_moment_loss(const float* u_saved_dev, const float* data_mean_dev, const float* data_var_dev, int32_t D, int32_t T, int32_t B,
                             float* loss_out_dev, float* u_bar_dev, void* stream);
/* The training step of reference experiments/sde_toy_problem.jl (loss_function :27-40 and Tracker.gradient) in one call:
 *     u = TrackedNeuralDSDE(x, p) at the n_saveat times of saveat_host  ->  rnde_moment_loss  ->  loss = l2_means + l2_vars + c * sum(sv.saveval)
 * = rnde_nsde_forward_saveat (taped; noise as there) + rnde_moment_loss + rnde_nsde_backward_async (every saved value's cotangent is c when
 * c != 0 and the handle records a callback).  Outputs: p_bar_dev (P), x_bar_dev (D x B, may be NULL), loss_out_dev[2] = (l2_means, l2_vars)
 * (device, stream order), *reg_out_host = c * sum(saveval), *nfe1_out, *nfe2_out (host, valid on return). */
rnde_status rnde_nsde_moment_grad(rnde_nsde* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1, const float* noise_dev,
                                  int32_t n_pool, uint64_t seed, const float* saveat_host, int32_t n_saveat, const float* data_mean_dev,
                                  const float* data_var_dev, float c, float* p_bar_dev, float* x_bar_dev, float* loss_out_dev, float* reg_out_host,
                                  int64_t* nfe1_out, int64_t* nfe2_out, void* stream);
/* The pre-activation (rnde_pre_act) of the drift and of the diffusion chain; new handles have none.  Allowed only while the handle holds no
 * tape (RNDE_ERR_BAD_ARG otherwise: the tape's reverse pass must see the map its forward ran).  Applies to every later solve and to
 * rnde_nsde_debug_attempt.  A nonzero selector takes the handle off the kernels with the reference's shape as compile-time constants. */
rnde_status rnde_nsde_set_pre_act(rnde_nsde* h, int32_t drift_pre, int32_t diff_pre);
/* Per-attempt log of the last forward: 4 floats per attempt (t, dt, EEst, accepted); draws_out = noise draws consumed. */
rnde_status rnde_nsde_steps(rnde_nsde* h, float* steps_host, int32_t capacity, int32_t* n_attempts_out, int32_t* draws_out);
/* Kernel-level parity entry: ONE attempted step from (uprev, dt, dW, dZ), all D x B device arrays: kg_out_dev receives
 * k1..k4, g1..g4 (8 x D x B), unew_out_dev the proposed state, eest_out the error estimate. */
rnde_status rnde_nsde_debug_attempt(rnde_nsde* h, const float* uprev_dev, const float* p_dev, int32_t B, float dt,
                                    const float* dW_dev, const float* dZ_dev, float* kg_out_dev, float* unew_out_dev,
                                    float* eest_out, void* stream);
/* Measurement aid: HIP-event durations (ms, on the caller's stream) of the last forward's solve kernel (ONE launch = the
 * whole adaptive solve) and of the last reverse sweep kernel, with the attempt counts of that forward; -1 = not recorded. */
rnde_status rnde_nsde_timing(rnde_nsde* h, float* solve_ms, float* rev_sweep_ms, int32_t* attempts, int32_t* accepted);
/* Fill `n` floats with standard normals from (seed, stream_id): the library's own generator, exposed for its statistical test. */
rnde_status rnde_normal_fill(float* out_dev, int64_t n, uint64_t seed, uint64_t stream_id, void* stream);

/* ======================================================================================================================
 * The latent-ODE caller of the hot path: recognition GRU, rec_to_gen + sampling, gen_to_data + masked likelihood
 * + KL, and their reverse passes -- what surrounds the layer call in LatentTimeSeriesModel (reference src/models/time_series.jl:40-70)
 * and loss_function (experiments/latent_ode.jl:206-236), at the reference's sizes: LatentGRU(37, 40, 50) (latent_ode.jl:39-106, :111),
 * rec_to_gen = Chain(Dense(100, 50, tanh), Dense(50, 40)) (:112), gen_to_data = Dense(20, 37) (:148).  One training step is
 *   rnde_latent_encode          x -> GRU over the time axis backwards (:99-106) -> rec_to_gen -> mu0, logvar, z0 = eps * exp(logvar / 2) + mu0
 *   rnde_node_forward_saveat    the layer call on z0 (the hot path, above)                                  (time_series.jl:61)
 *   rnde_latent_decode_loss     gen_to_data on every saved state, -mean(log_likelihood), mean(kl_divergence), and the reverse of the
 *                               likelihood term: res-bar (the u_bar of rnde_node_backward) and p4-bar          (latent_ode.jl:192-204, :226-233)
 *   rnde_node_backward          -> z0-bar
 *   rnde_latent_encode_backward z0-bar and lambda_k * mean(KL) -> p1-bar (GRU), p2-bar (rec_to_gen)
 * Layouts are Julia's: x is (2 * 37 + 1) x T x B = vcat(data, mask, dt) (latent_ode.jl:225), res is 20 x T x B, the parameter vectors are
 * Flux.destructure's (time_series.jl:11-14).  eps is the caller's standard-normal sample, 20 x B (CUDA.randn, time_series.jl:58).
 * All calls are asynchronous on `stream`; the handle keeps the tapes of ONE encode at a time.
 * ====================================================================================================================== */
typedef struct { int32_t max_batch, max_T, device; } rnde_latent_config;   /* max_T <= 64 save times */
typedef struct rnde_latent rnde_latent;
rnde_status rnde_latent_create(const rnde_latent_config* cfg, rnde_latent** out);
void        rnde_latent_destroy(rnde_latent* h);
const char* rnde_latent_last_error(const rnde_latent* h);      /* h may be NULL: last create error of this thread */
void        rnde_latent_param_counts(int32_t* n_p1, int32_t* n_p2, int32_t* n_p4);      /* 29,320 / 7,090 / 777 */
rnde_status rnde_latent_encode(rnde_latent* h, const float* x_dev, const float* p1_dev, const float* p2_dev, const float* eps_dev, int32_t B,
                               int32_t T, float* z0_out_dev, float* mu0_out_dev, float* logvar_out_dev, void* stream);
/* loss2_out_dev[0] = -mean_b(ll_b), [1] = mean_b(KL_b); res_bar_out_dev (20 x T x B) and p4_bar_out_dev (777) are the cotangents of term [0]. */
rnde_status rnde_latent_decode_loss(rnde_latent* h, const float* res_dev, const float* p4_dev, const float* x_dev, int32_t B, int32_t T,
                                    float* loss2_out_dev, float* res_bar_out_dev, float* p4_bar_out_dev, void* stream);
/* The evaluation pass, total_loss_on_dataset (experiments/latent_ode.jl:271-292) for one batch: gen_to_data on every saved state (the same
 * product, in the same order, as rnde_latent_decode_loss), then per sample
 *     mse_b = sum_{f,t} (pred * mask - data * mask)^2 / sum_{f,t} mask                                          (latent_ode.jl:281-286)
 * -> mse_out_dev (B floats, required); sum_b mse_b, added in increasing b in fp64, is ADDED to *sum_dev and B to *count_dev (both may be
 * NULL, and one is NULL exactly when the other is: RNDE_ERR_BAD_ARG otherwise); the data set's loss is sum / count, read once.  Layouts as
 * above; B <= max_batch, T <= max_T.  Needs no rnde_latent_encode of the same batch.  A sample with no observed entry gives what the
 * reference gives, a division by zero (NaN, or Inf); it is not special-cased.  Every sum has a fixed order: the same bits run to run. */
rnde_status rnde_latent_decode_mse(rnde_latent* h, const float* res_dev, const float* p4_dev, const float* x_dev, int32_t B, int32_t T,
                                   float* mse_out_dev, double* sum_dev, int64_t* count_dev, void* stream);
/* z0_bar_dev: 20 x B from the layer's reverse pass; the KL term enters with weight lambda_k (latent_ode.jl:178, :232). */
/* Flux.Optimise.Optimiser(InvDecay(gamma), AdaMax(eta, (beta1, beta2))) on one flat parameter group, in place (experiments/latent_ode.jl:108).
 * m, u: the caller's state arrays (zeros at the first step); n: the InvDecay counter (1 at the first step); beta1_pow: Flux's running
 * beta1^t (beta1 at the first step) -- the caller advances n and beta1_pow.  Asynchronous on `stream`. */
rnde_status rnde_adamax_step(float* p_dev, const float* g_dev, float* m_dev, float* u_dev, int64_t len, int64_t n, float gamma, float eta, float beta1,
                             float beta2, float eps, float beta1_pow, void* stream);
rnde_status rnde_latent_encode_backward(rnde_latent* h, const float* z0_bar_dev, float lambda_k, const float* p1_dev, const float* p2_dev,
                                        const float* x_dev, float* p1_bar_out_dev, float* p2_bar_out_dev, void* stream);

/* ======================================================================================================================
 * TrackedFFJORD (reference src/models/ffjord.jl:1-167, exported at src/RegNeuralDE.jl:88) with the ConcatSquash MLPDynamics of
 * experiments/ffjord_gaussian.jl:48-107: three ConcatSquashLinear layers in -> hidden -> hidden -> in, softplus between them, per layer
 * h = (W x + b) .* sig(gw t) + (bw t + bb).  State [z; l], dl/dt = -e . eJ (Hutchinson probe e, D x B, drawn once per call), Tsit5 with
 * the chain engine's controller over the D + 1 augmented rows.  logpx = sum -(log 2 pi + z^2) / 2 - l.
 *   regularize = 0: TrackedFFJORD{false} with regularize = false (:68-112)
 *   regularize = 1: TrackedFFJORD{true} (:114-135): SavingCallback EEst * dt per accepted step (and 0 at init with cb_save_start)
 * Parameters in Flux.destructure order: per layer layer_W (out x in, column-major), layer_B, bias_W, bias_B, gate_W (each out).
 * Refused at create with a message naming the limit: dynamics other than ConcatSquash (the default forw_n_back through Tracker.forward
 * is not described by this config: rnde_ffjord_create_chain below serves it),
 * in_dims + 1 > 64 or hidden > 64 (rnde_ffjord_create; rnde_ffjord_create_tiled below serves wider models), kinetic_reg != 0 (the
 * {false} method's regularize = true rows at create: the keyword is a call-time one, served by the *_kinetic entries below on handles
 * created with kinetic_reg = 0), solvers other than Tsit5.
 * ====================================================================================================================== */
typedef enum { RNDE_FFJORD_CONCAT_SQUASH = 0, RNDE_FFJORD_TRACKER_FORWARD = 1 } rnde_ffjord_dynamics;
typedef struct {
    int32_t in_dims, hidden;       /* MLPDynamics(in_dims, hidden) */
    int32_t dynamics;              /* rnde_ffjord_dynamics */
    int32_t time_dep;              /* the layer's time_dep flag (the ConcatSquash layers always read t) */
    int32_t regularize;            /* 0: {false}, 1: {true} */
    int32_t kinetic_reg;           /* must be 0: refused at create (regularize = true is a call-time keyword: the *_kinetic entries) */
    int32_t max_batch, solver;     /* solver: RNDE_SOLVER_TSIT5 */
    float reltol, abstol;
    int32_t cb_save_start;         /* 1: the saving callback also fires at init (value 0) */
    int32_t max_attempts, device;
} rnde_ffjord_config;
typedef struct rnde_ffjord rnde_ffjord;
int32_t     rnde_ffjord_param_count(const rnde_ffjord_config* cfg);     /* 456 for (2, 16); any widths (counted, not checked) */
rnde_status rnde_ffjord_create(const rnde_ffjord_config* cfg, rnde_ffjord** out);
void        rnde_ffjord_destroy(rnde_ffjord* h);
const char* rnde_ffjord_last_error(const rnde_ffjord* h);      /* h may be NULL: last create error of this thread */
/* Forward solve on [t0, t1].  x_dev, e_dev: D x B (e_dev NULL: standard normals from (seed) by the library's generator).  logpx_dev: B.
 * z_out_dev: the end state's data rows, D x B (may be NULL).  saveval_host: room for max_attempts + 1 floats.  keep_tape != 0 records what
 * rnde_ffjord_backward needs; x, p and e must then stay valid until the backward call. */
rnde_status rnde_ffjord_forward(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t0, float t1,
                                uint64_t seed, float* logpx_dev, float* z_out_dev, int64_t* nfe_out, float* saveval_host,
                                int32_t* n_saveval_out, int32_t keep_tape, void* stream);
/* Parity instrument (as rnde_node_forward_replay): the solve along n_steps given (dt, accepted != 0) pairs. */
rnde_status rnde_ffjord_forward_replay(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t0, float t1,
                                       uint64_t seed, const float* steps_host, int32_t n_steps, float* logpx_dev, float* z_out_dev,
                                       int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape, void* stream);
/* (dt, accepted) of every attempt of the last solve, as rnde_node_steps. */
rnde_status rnde_ffjord_steps(rnde_ffjord* h, float* steps_host, int32_t capacity, int32_t* n_attempts_out);
/* Reverse pass of the last taped forward (discretise-then-optimise; step sizes are constants): logpx_bar_dev (B) and saveval_bar_host
 * (one per saved value, NULL = zeros) -> p_bar_dev (P, overwritten), x_bar_dev (D x B, may be NULL).  Deterministic. */
rnde_status rnde_ffjord_backward(rnde_ffjord* h, const float* logpx_bar_dev, const float* saveval_bar_host, float* p_bar_dev, float* x_bar_dev,
                                 void* stream);
/* sample (ffjord.jl:137-167): z ~ N(0, I) (z_dev, D x n, or NULL: the library's normals from seed), solved from t1 back to t0 with the exact
 * trace (D VJPs with unit probes), i.e. tau in [0, t1 - t0] on -F(u, t1 - tau).  x_out_dev: D x n.  Forward only; drops a held tape. */
rnde_status rnde_ffjord_sample(rnde_ffjord* h, const float* p_dev, const float* z_dev, int32_t n, float t0, float t1, uint64_t seed,
                               float* x_out_dev, void* stream);
/* One evaluation of the augmented right-hand side: out_dev (D + 1) x B = [f(x, t); -e . eJ] (exact != 0: the exact trace, e unused). */
rnde_status rnde_ffjord_debug_feval(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t, int32_t exact,
                                    float* out_dev, void* stream);
/* HIP-event durations (ms) of the last solve launch and the last reverse sweep (+ reduction), with that solve's attempt counts. */
rnde_status rnde_ffjord_timing(rnde_ffjord* h, float* solve_ms, float* reverse_ms, int32_t* attempts, int32_t* accepted);
/* The tiled engine (opt-in; the same config struct, every other rnde_ffjord_* entry dispatches on the handle): one workgroup per 16 batch
 * columns, the layer products on the matrix cores (v_mfma_f32_16x16x4_f32, exact fp32 products), the padded parameters resident in LDS, the
 * workgroups meeting once per attempt for the error norm (bounded; a meeting that times out fails the call with a message naming it).
 * Serves what rnde_ffjord_create serves, at widths up to its LDS limit:
 *   in_dims <= 64 and hidden <= 112 (weights and activations of a tile within 160 KB of LDS; (43, 100) fits),
 *   max_batch <= 4096 (256 tiles: one meeting holds only resident workgroups), max_attempts <= 8000.
 * sample() and the exact trace of rnde_ffjord_debug_feval use the closed form tr J = a2' (W2 .* M') a1, M(t) = W1 diag(g3(t)) W3, with
 * a_l = sig(h_l) .* g_l: the same value as the D unit-probe VJPs, rounded differently. */
rnde_status rnde_ffjord_create_tiled(const rnde_ffjord_config* cfg, rnde_ffjord** out);
int32_t     rnde_ffjord_engine(const rnde_ffjord* h);          /* 0: one workgroup (rnde_ffjord_create), 1: tiled, 2: chain dynamics; -1 for NULL */
/* TrackedFFJORD{false} called with regularize = true (ffjord.jl:53-66): the state grows to [z; l; lambda1; lambda2] (D + 3 rows, the last
 * three starting at zero) with d lambda1 / dt = sum f^2 (the kinetic energy) and d lambda2 / dt = sum eJ^2 (the Hutchinson estimate of the
 * Jacobian's Frobenius norm), eJ as the trace row builds it.  The controller (initial step, error norm, PI step) runs over all D + 3 rows;
 * NFE is 3 + 6 per attempt as before.  reg_out_dev: 2 x B, the lambda1 row then the lambda2 row.  The other arguments are those of
 * rnde_ffjord_forward / _replay without the saved values.  On handles created with regularize = 0 and kinetic_reg = 0, either engine; a
 * handle's state, tape and reverse workspace grow to D + 3 rows at its first kinetic call, and plain calls on it are unaffected.
 * Limits: one workgroup in_dims + 3 <= 64 and hidden <= 64; tiled in_dims <= 64 and hidden <= 112 (no LDS beyond the plain kernels').  A
 * kinetic call outside them, or on a regularize = 1 handle, is RNDE_ERR_BAD_ARG with a message that names the limit. */
rnde_status rnde_ffjord_forward_kinetic(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t0, float t1,
                                        uint64_t seed, float* logpx_dev, float* reg_out_dev, float* z_out_dev, int64_t* nfe_out,
                                        int32_t keep_tape, void* stream);
rnde_status rnde_ffjord_forward_kinetic_replay(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t0,
                                               float t1, uint64_t seed, const float* steps_host, int32_t n_steps, float* logpx_dev,
                                               float* reg_out_dev, float* z_out_dev, int64_t* nfe_out, int32_t keep_tape, void* stream);
/* Reverse pass of a taped kinetic forward: end-state cotangents (-z logpx_bar, -logpx_bar, reg_bar row 0, reg_bar row 1); reg_bar_dev is
 * 2 x B (NULL = zeros).  rnde_ffjord_backward on a kinetic tape behaves as reg_bar_dev = NULL.  Deterministic. */
rnde_status rnde_ffjord_backward_kinetic(rnde_ffjord* h, const float* logpx_bar_dev, const float* reg_bar_dev, float* p_bar_dev, float* x_bar_dev,
                                         void* stream);
/* One evaluation of the kinetic right-hand side: out_dev (D + 3) x B = [f(x, t); -e . eJ; sum f^2; sum eJ^2]. */
rnde_status rnde_ffjord_debug_feval_kinetic(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t,
                                            float* out_dev, void* stream);
/* (t, dt, EEst, accepted) of every attempt of the last solve, plain or kinetic, as rnde_node_steps (log_host NULL: the count only). */
rnde_status rnde_ffjord_step_log(rnde_ffjord* h, float* log_host, int32_t capacity, int32_t* n_attempts_out);
/* The default dynamics of TrackedFFJORD (dynamics = nothing, ffjord.jl:21-27: Tracker.forward(z -> m(z, t), z), then back(e)) for a chain of
 * Dense layers, time dependent (TDChain: t appended to every layer's input) or plain: engine 2, on the tiled layout (one workgroup per 16
 * columns, the padded weights resident in LDS, layer products on the matrix cores, one bounded meeting per attempt).  With y_0 = z,
 *   a_l = W_l y_{l-1} + wt_l t + b_l,  y_l = phi_l(a_l),  f = y_n;   v_n = phi_n' .* e,  v_l = phi_l' .* (W_{l+1}' v_{l+1}),  eJ = W_1' v_1
 * and the state rows are those of the ConcatSquash engines: [f; -e . eJ] and, through the *_kinetic entries, [f; -e . eJ; sum f^2; sum eJ^2].
 * sample() and the exact trace are D unit-probe passes of the same VJP (the reference's jacobian_fn).  Parameters in Flux.destructure
 * order: per layer W (out x (in [+ 1]), column-major, the t column last), then b -- the layout of rnde_node_config.  rnde_ffjord_config
 * cannot describe a chain; every other rnde_ffjord_* entry dispatches on the handle and rnde_ffjord_engine returns 2.
 * Refused at create (before a device is needed) with a message naming the limit: n_layers outside 1..RNDE_MAX_LAYERS; a layer output or a
 * layer input above 64 (the time row is an epilogue vector and does not count: TD [48, 64, 64, 48] is served), or dims[0] + 1 > 64 (kinetic
 * calls: dims[0] + 3 <= 64, on regularize = 0 handles);
 * dims[0] != dims[n_layers]; an activation outside rnde_act; a solver other than Tsit5; max_batch > 4096 or max_attempts > 8000; weights plus
 * the solve's activations above 160 KB of LDS (the message gives the need and the limit).  No leading element-wise map. */
typedef struct {
    int32_t n_layers;
    int32_t dims[RNDE_MAX_LAYERS + 1]; /* dims[0] = dims[n_layers] = D */
    int32_t act[RNDE_MAX_LAYERS];      /* rnde_act per layer */
    int32_t time_dep;                  /* 1: TDChain, 0: Chain */
    int32_t regularize;                /* 0: {false}, 1: {true} */
    int32_t max_batch, solver;         /* solver: RNDE_SOLVER_TSIT5 */
    float reltol, abstol;
    int32_t cb_save_start;
    int32_t max_attempts, device;
} rnde_ffjord_chain_config;
int32_t     rnde_ffjord_chain_param_count(const rnde_ffjord_chain_config* cfg);   /* 64 for TD [2, 10, 2]; -1 for a bad shape */
rnde_status rnde_ffjord_create_chain(const rnde_ffjord_chain_config* cfg, rnde_ffjord** out);
/* The exact-trace forward: the state [z; l] with dl / dt = -tr J(z, t), no probe and no variance in logpx.  The function evaluated is the
 * reference's _deterministic_ffjord over jacobian_fn (ffjord.jl:137-158: D VJPs with unit probes), which the reference runs only inside
 * sample(), from t1 back to t0; it has no forward exact call, so these two entries are an extension and have no counterpart there.  The
 * arguments are those of rnde_ffjord_forward / _replay without e_dev and seed; the controller, the saved values (regularize = 1 handles),
 * rnde_ffjord_steps / _step_log / _timing and NFE (3 + 6 per attempt: right-hand-side calls, as the reference counts them) are unchanged.
 * keep_tape != 0 marks the tape as exact: rnde_ffjord_backward then runs the exact variant of the tile driver's reverse sweep, which
 * recomputes the stages with the exact trace and differentiates the trace row through -tr J = -sum_i e_i . (e_i J) -- D + 1 stage VJPs
 * where the Hutchinson sweep runs one, so the reverse costs about (D + 1) times the Hutchinson one.  Deterministic, and Hutchinson calls
 * on the same handle are unaffected.  ConcatSquash handles evaluate the trace in the closed form of rnde_ffjord_create_tiled and
 * differentiate its unit-probe form: the same function, rounded differently.
 * Engines 1 (rnde_ffjord_create_tiled) and 2 (rnde_ffjord_create_chain), regularize 0 or 1.  RNDE_ERR_BAD_ARG before any launch, with a
 * message that names the reason: a handle of rnde_ffjord_create (engine 0; the message points at the tiled engine), and
 * rnde_ffjord_backward_kinetic on an exact tape (the kinetic rows are not served with the exact trace: the Jacobian norm row is defined on
 * the probe). */
rnde_status rnde_ffjord_forward_exact(rnde_ffjord* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1, float* logpx_dev,
                                      float* z_out_dev, int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape,
                                      void* stream);
rnde_status rnde_ffjord_forward_exact_replay(rnde_ffjord* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1,
                                             const float* steps_host, int32_t n_steps, float* logpx_dev, float* z_out_dev, int64_t* nfe_out,
                                             float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape, void* stream);
/* The tracked-controller reverse sweep (opt-in; the default, 0, is the constant-step sweep above, bit for bit).  The reference's Tracker tape
 * runs through the solver's scalar arithmetic, so the saved value EEst * dt of TrackedFFJORD{true} depends on the parameters through dt as
 * well as through EEst; with on = 1, rnde_ffjord_backward differentiates the PI controller too (track_ctrl = 1, track_initdt = 0 in
 * rnde_node_config's terms: the initial step stays a constant, and no tspan cotangent is returned).  The sweep then walks every attempt,
 * rejected ones included, and the tiles meet once per attempt for the three sums of the dt cotangent (bounded, placed as the solve's
 * meetings; a meeting that times out fails the backward call with RNDE_ERR_HIP and a message naming it, nothing falls back).
 * Deterministic.  The tape remembers the setting of its forward, Hutchinson and exact-trace tapes alike; a tracked replay tape is
 * differentiated as if the controller had produced the sequence (the convention of rnde_node_forward_replay).
 * RNDE_ERR_BAD_ARG with a message that names the reason: a handle of rnde_ffjord_create (engine 0; the message points at the tiled engine);
 * a regularize = 0 handle (without a saved value the two sweeps agree to O(tol): 2e-10 to 2e-6 relative against the fp64 oracle; this keeps
 * the kinetic tapes out as well); a handle that holds a tape; max_batch above what the device keeps resident on the tracked kernel's
 * footprint (checked when tracking is first switched on). */
rnde_status rnde_ffjord_set_track_ctrl(rnde_ffjord* h, int32_t on);
int32_t     rnde_ffjord_track_ctrl(const rnde_ffjord* h);      /* the setting; -1 for NULL */
/* Several batches per launch (opt-in; the likelihood pass of src/metrics.jl:20-33, whose batches do not depend on each other).  A tile is one
 * workgroup on 16 columns and a 1024-column batch of the tabular widths is 64 of them, a quarter of the device; a group call places the
 * tiles of several independent batches ("groups") in one launch.  Each group keeps the semantics of a call of its own: its own initial
 * step, its own error norm over its own columns, its own controller and step log, and logpx, NFE and the (dt, accepted) log are bit for
 * bit those of rnde_ffjord_forward (or _forward_exact) on that batch alone with the same p, e and span.  It is NOT a larger batch: no
 * norm and no step is shared between groups, a group meets only with itself and leaves the launch when it is done.
 * The capacity is the switch (as rnde_node_tiled_reserve_saveat): rnde_ffjord_reserve_groups(h, max_groups, max_columns) allocates the
 * groups' workspace, control blocks, step logs and meeting granules for calls of up to max_groups groups and ceil(max_columns / 16)
 * tiles in all (every group takes ceil(B_g / 16) tiles of its own); 0, 0 releases it, and a handle that never reserved runs the kernels it
 * ran before.  Engines 1 and 2.  RNDE_ERR_BAD_ARG with a message that names the reason: a handle of rnde_ffjord_create (engine 0; the
 * message points at the tiled engine), a handle that holds a tape, max_groups outside 1..16, max_columns outside max_groups..4096, and
 * more tiles than the device keeps resident on the group kernel's footprint (the launch is at agent scope whatever the count).
 * rnde_ffjord_group_capacity reads the reservation back (0, 0 without one). */
rnde_status rnde_ffjord_reserve_groups(rnde_ffjord* h, int32_t max_groups, int32_t max_columns);
rnde_status rnde_ffjord_group_capacity(const rnde_ffjord* h, int32_t* max_groups_out, int32_t* max_columns_out);
/* The group call.  x_dev, e_dev, logpx_dev cover the groups' columns back to back in the caller layout (D x sum B, sum B); B_host: the
 * n_groups column counts.  exact != 0: the exact trace of rnde_ffjord_forward_exact, and e_dev must be NULL; otherwise e_dev is required
 * (the call draws no probes).  nfe_out_host, status_out_host: n_groups entries each (either may be NULL); status_out_host carries every
 * group's own rnde_status, the call returns the first failing group's with a message that gives the group index.  sum_dev (a double) and
 * count_dev (an int64), both or neither: when every group ended with RNDE_OK, sum_dev += the sum of logpx over all columns of the call (in
 * double, one workgroup, a fixed order, no atomics: the same bits run to run) and count_dev += sum B, queued on the stream behind the
 * solve and not waited for; a failed call adds nothing.  One launch and one stream synchronisation.  Forward only and untaped, as an
 * untaped rnde_ffjord_forward: a tape the handle holds, its step log and its operands stay as they were, and so does what rnde_ffjord_steps
 * / _step_log report; rnde_ffjord_timing's solve_ms becomes the group launch's.  Checked before any launch, each with a message naming
 * the limit (RNDE_ERR_BAD_ARG): no capacity, n_groups outside 1..max_groups, a B_g outside 1..max_batch, more tiles than reserved,
 * t1 <= t0, e_dev missing or (exact) given, only one of sum_dev / count_dev.  A meeting that times out ends every group: RNDE_ERR_HIP. */
rnde_status rnde_ffjord_forward_groups(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t n_groups,
                                       const int32_t* B_host, float t0, float t1, int32_t exact, float* logpx_dev, int64_t* nfe_out_host,
                                       int32_t* status_out_host, double* sum_dev, int64_t* count_dev, void* stream);
/* (dt, accepted) of every attempt of group g of the last group call, as rnde_ffjord_steps (steps_host NULL: the count only). */
rnde_status rnde_ffjord_group_steps(rnde_ffjord* h, int32_t g, float* steps_host, int32_t capacity, int32_t* n_attempts_out);
/* The gradient of the experiments' loss_function (reference experiments/ffjord_tabular.jl:143-147, ffjord_gaussian.jl:142-146) in one call:
 *     loss = -mean(logpx) + lambda_r * mean(sv.saveval) + lambda_k * mean(lambda1) + lambda_j * mean(lambda2)
 * the second term on regularize = 1 handles (the {true} method), the last two in mode 2 (the {false} method called with regularize = true).
 * It is the taped forward (mode 0: rnde_ffjord_forward, 1: _forward_exact, 2: _forward_kinetic), then the loss-and-seed kernel, then the
 * reverse sweep (rnde_ffjord_backward; mode 2: _backward_kinetic) -- the same launches, so p_bar, x_bar, logpx, NFE and the step log are
 * bit for bit those of the two calls, on every engine, with track_ctrl, with the library's probe draw (e_dev NULL, from seed), and
 * rnde_ffjord_timing / _steps / _step_log report the solve as after a forward.  No host round trip remains between solve and sweep.
 * The loss-and-seed kernel (one workgroup of 256 threads, queued directly behind the solve launch, in front of the forward's host wait):
 * thread i adds elements i, i + 256, ... in double, in rising index; the 256 partials are combined in a fixed tree; the result depends on
 * the values and on B only.  It writes
 *     terms_dev[0] = (float)(-sum(logpx) / B)
 *     terms_dev[1..2] = (float)(sum(lambda1) / B), (float)(sum(lambda2) / B), which are 0 outside mode 2
 *     logpx_bar[b] = -1.0f / (float)B
 *     in mode 2, reg_bar[0][b] = lambda_k / (float)B and reg_bar[1][b] = lambda_j / (float)B
 * The two seed arrays are fp32, with one fp32 division each; they go into buffers the handle owns.  A NaN in logpx stays a NaN in the term.
 * On the host, after the step log has been read (n = the number of saved values, including the 0 at init when cb_save_start is set):
 *     *reg_out_host = (float)((double)lambda_r * sum(saveval) / n), summed in double in log order; 0 on regularize = 0 handles
 *     saveval_bar[i] = lambda_r / (float)n, one fp32 division
 * p_bar_dev: P (overwritten).  x_bar_dev: D x B, may be NULL.  logpx_dev: B, may be NULL (a buffer of the handle then).  terms_dev: 3 floats
 * on the device, not read back.  The handle's buffers (logpx, logpx_bar, reg, reg_bar) are allocated at the first fused call.
 * After the call the handle holds no valid tape: the call consumes its own, x, p and e need not outlive it, and a later
 * rnde_ffjord_backward returns RNDE_ERR_NO_TAPE.  It synchronises where the two calls it replaces do.  A solve that ends with a non-zero
 * status returns that status and launches no sweep.
 * RNDE_ERR_BAD_ARG before any launch, each with a message naming the reason: mode outside 0..2; mode 1 on engine 0 (the message points at
 * the tiled engine) or with e_dev given; mode 2 on a regularize = 1 handle or outside the kinetic limits; lambda_k or lambda_j non-zero
 * outside mode 2; lambda_r non-zero on a regularize = 0 handle; p_bar_dev, terms_dev, reg_out_host or nfe_out NULL; B outside
 * 1..max_batch; t1 <= t0. */
rnde_status rnde_ffjord_nll_grad(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t0, float t1,
                                 uint64_t seed, int32_t mode, float lambda_r, float lambda_k, float lambda_j, float* p_bar_dev, float* x_bar_dev,
                                 float* logpx_dev, float* terms_dev, float* reg_out_host, int64_t* nfe_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
