"""The gradient collective behind the C ABI (rnde_comm_*, RCCL bound at run time) on the one GPU of the test box: world = 1
exercises id creation, communicator set-up, the all-reduce launch on the caller's stream and the folded averaging; the
world-2 arithmetic of the same classes is covered on CPU by tests/test_dist_gloo.py."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_comm_world1_through_the_abi():
    import torch
    from regneuralde_jl_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(128)
    assert L.rnde_comm_unique_id(buf) == 0, L.rnde_comm_last_error(None)
    comm = C.c_void_p()
    assert L.rnde_comm_create(bytes(buf.raw), 0, 1, 0, C.byref(comm)) == 0, L.rnde_comm_last_error(None)
    assert L.rnde_comm_world(comm) == 1
    g = torch.arange(166418, dtype=torch.float32, device="cuda") / 1000.0
    ref = g.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert L.rnde_comm_allreduce(comm, g.data_ptr(), g.numel(), 1, C.c_void_p(s.cuda_stream)) == 0
    s.synchronize()
    assert torch.equal(g, ref)
    assert L.rnde_comm_create(bytes(buf.raw), 3, 2, 0, C.byref(C.c_void_p())) == _lib.BAD_ARG     # rank >= world
    L.rnde_comm_destroy(comm)


def test_training_step_with_flat_gradients_and_early_allreduce():
    """fused_loss_and_grad(flat=, reducer=): the reverse pass writes into ONE buffer, the head's gradient is all-reduced before the
    sweep, the solve's behind it, 1/world rides in the optimiser launch -- same update as the single-process step."""
    import torch
    import torch.distributed as dist
    import regneuralde_jl_amd as rn
    store = tempfile.NamedTemporaryFile(delete=False)
    dist.init_process_group("gloo", init_method=f"file://{store.name}", rank=0, world_size=1)
    try:
        def make():
            g = torch.Generator().manual_seed(4)
            dyn = rn.MLPDynamics(784, 100, generator=g)
            node = rn.TrackedNeuralODE(dyn, [0.0, 1.0], True, True, "Tsit5", reltol=1e-3, abstol=1e-3, max_batch=32, max_attempts=64)
            return rn.ClassifierNODE(node, rn.Dense(784, 10, generator=g), device=torch.device("cuda", 0)), g
        m1, g1 = make()
        m2, _ = make()
        x = torch.rand(32, 1, 28, 28, generator=g1).cuda()
        y = torch.eye(10)[torch.randint(0, 10, (32,), generator=g1)].cuda()
        fg = rn.FlatGrads(m2.trainable())
        red = rn.GradientAllReducer(m2.trainable(), flat=fg)
        assert red.comm is not None and fg.flat.numel() == 158568 + 7850
        o1, o2 = rn.FluxOptimiser(m1.trainable()), rn.FluxOptimiser(m2.trainable())
        for _ in range(3):
            rn.fused_loss_and_grad(m1, x, y, sync=True)
            o1.step()
            rn.fused_loss_and_grad(m2, x, y, sync=False, flat=fg, reducer=red)
            assert m2.p2.grad.data_ptr() == fg.flat.data_ptr()
            o2.step(grad_scale=red.grad_scale)
        torch.cuda.synchronize()
        assert torch.equal(m1.p2, m2.p2) and torch.equal(m1.p3, m2.p3)
        # a reducer WITHOUT `flat` (the three-call path, sync=True): the gradients must still land in the buffer the collective reduces
        # (round-2 advisor finding: they went to fresh tensors and an unwritten buffer was all-reduced), and a foreign `flat` is refused
        fg.flat.fill_(float("nan"))
        rn.fused_loss_and_grad(m2, x, y, sync=True, reducer=red)
        assert m2.p2.grad.data_ptr() == red.fg.flat.data_ptr() and torch.isfinite(red.fg.flat).all()
        rn.fused_loss_and_grad(m1, x, y, sync=True)
        assert torch.equal(m1.p2.grad, m2.p2.grad) and torch.equal(m1.p3.grad, m2.p3.grad)
        with pytest.raises(ValueError):
            rn.fused_loss_and_grad(m2, x, y, sync=True, flat=rn.FlatGrads(m2.trainable()), reducer=red)
    finally:
        dist.destroy_process_group()
        if os.path.exists(store.name):
            os.unlink(store.name)


@pytest.mark.parametrize("world", [2, 3])
def test_in_process_group_allreduce(world):
    """rnde_comm_create_local_group: `world` ranks in this process, one host thread and one stream each; 40 consecutive all-reduces of
    different vectors (the two slot sets alternate) must give every rank the sum over the ranks, in rank order, bit for bit."""
    import threading
    import torch
    from regneuralde_jl_amd import _lib
    L = _lib.lib()
    comms = (C.c_void_p * world)()
    assert L.rnde_comm_create_local_group(world, 0, comms) == 0, L.rnde_comm_last_error(None)
    n = 3 * 224
    base = [torch.randn(40, n, generator=torch.Generator().manual_seed(100 + r)).cuda() for r in range(world)]
    out = [None] * world

    def work(r):
        st = torch.cuda.Stream()
        res = []
        with torch.cuda.stream(st):
            for k in range(40):
                buf = base[r][k].clone()
                assert L.rnde_comm_allreduce(C.c_void_p(comms[r]), buf.data_ptr(), n, 0, C.c_void_p(st.cuda_stream)) == 0, L.rnde_comm_last_error(C.c_void_p(comms[r]))
                res.append(buf)
        st.synchronize()
        out[r] = torch.stack(res).cpu()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(60) for t in th]
    assert all(o is not None for o in out)
    ref = base[0].cpu().clone()
    for r in range(1, world):
        ref = ref + base[r].cpu()            # rank order, as the sum kernel adds
    for r in range(world):
        assert torch.equal(out[r], ref)
        assert L.rnde_comm_health(C.c_void_p(comms[r])) == 0
    for c in comms:
        L.rnde_comm_destroy(C.c_void_p(c))


def _need_gpus_for_ranks(world):
    """Up to 4 ranks share device 0 (with this process: at most 5 processes on one GPU).  A world of more ranks runs one rank per device,
    as on config 3's 8-GPU node: the test looks at the device count before it starts anything and skips without enough devices.
    Returns True when the ranks are to get a device each."""
    import torch
    n = torch.cuda.device_count()
    if world > 4 and n < world:
        pytest.skip(f"needs {world} GPUs (one per rank), found {n}")
    return world > 4


@pytest.mark.parametrize("world,mean", [(2, 0), (4, 1), (8, 1)])      # (8: config 3's world size -- 7 peer windows per rank, 8-way flags -- one rank per device, on 8 GPUs)
def test_one_shot_allreduce_between_processes(world, mean, tmp_path):
    """rnde_comm_window_create / rnde_comm_create_peers: `world` PROCESSES (tools/oneshot_worker.py), each with its own window, mapped
    into every peer through hipIpc -- up to 4 ranks sit on device 0 of the test box (the mapping and the kernel are the ones a multi-GPU
    node runs); world 8 puts rank r on device r and needs 8 GPUs.  Every rank checks every all-reduce bit for bit against the rank-order fp32 sum: sizes 1 .. 300,001 floats
    (above one window slot: pieces), aligned and unaligned buffers, both slot sets, with and without the 1 / world scale."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    own_gpu = _need_gpus_for_ranks(world)          # world 8: rank r on device r, as on a multi-GPU node
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tools", "oneshot_worker.py"), "--rank", str(r), "--world", str(world),
                               "--dir", str(tmp_path), "--mean", str(mean), "--device", str(r if own_gpu else 0)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=400)
            assert p.returncode == 0, e[-2000:]
            outs.append(json.loads(o.strip().splitlines()[-1]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    print(outs)
    for o in outs:
        assert o["mismatches"] == 0 and o["checked"] == 42 and o["health"] == 0
        assert "one-shot" in o["path"]


@pytest.mark.parametrize("coupled,strong", [(False, False), (True, False), (False, True)])
def test_bench_runs_two_ranks_on_one_gpu_through_the_one_shot_collective(coupled, strong):
    """The driver's N > 1 command line (torchrun, one process per rank, barrier + max-over-ranks timing, one gradient all-reduce per step)
    with `--share-gpu`: both ranks on device 0, torch.distributed on gloo, the gradient collective = the one-shot kernel over peer-mapped
    windows.  Checks the contract line and the `dist` diagnostics; the data-parallel numerics are the next test's."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "64", "--share-gpu", "--full", "--no-cpu-baseline"] + ([] if strong else ["--no-extras"]) + (["--coupled"] if coupled else []) + (["--global-batch", "96"] if strong else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    o = json.loads(line)
    assert o["n_gpus"] == 2 and o["steps"] == 3 and o["value"] > 0
    # --global-batch G: strong scaling, the global batch is fixed and split over the ranks (48 per rank here); default: weak, --batch per rank
    assert o["scaling"] == ("strong" if strong else "weak") and o["config"]["global_batch"] == (96 if strong else 128)
    d = o["dist"]
    assert "one-shot" in d["collective_path"] and d["allreduce_floats"] == 166418 and len(d["nfe_per_rank"]) == 2
    if coupled:     # one controller for both ranks (SURVEY 8e mode 2): the same accept / reject sequence, hence the same NFE, on every rank
        assert o["controller"].startswith("coupled") and d["nfe_per_rank"][0] == d["nfe_per_rank"][1]
    assert d["persist_fallback_count_per_rank"] == [0, 0]      # (two ranks of 28 / 21 workgroups each share the 256 CUs: every persistent launch is resident)
    print(o["value"], d)
    if strong:
        # both ends of a strong-scaling ratio must share one NFE: the N-rank line carries a fixed-weights leg (same --steps / --warmup), and the N = 1
        # anchor (bench.global_batch_anchor: the global batch on ONE GPU, same two legs) must report the same step count for it -- the training legs
        # drift apart with the weights, which is exactly why the ratio is formed from `value_fixed_weights` (round-4 review, weak #7)
        import sys as _sys
        _sys.path.insert(0, root)
        import torch
        import bench
        a = bench.global_batch_anchor(96, torch.device("cuda", 0), 3, 1)
        assert o["value_fixed_weights"] and o["fixed_weights"]["mean_nfe"] > 0 and a["value_fixed_weights"] > 0
        assert a["steps"] == o["steps"] and a["warmup"] == o["warmup"]
        print("fixed-weights NFE: 2 ranks x 48 columns", o["fixed_weights"]["mean_nfe"], "| one GPU x 96 columns", a["fixed_weights"]["mean_nfe"])
        assert abs(o["fixed_weights"]["mean_nfe"] - a["fixed_weights"]["mean_nfe"]) <= 6


def _dp_worker(rank, world, store, q):
    """One data-parallel rank (all on device 0): gloo process group, peers collective, three fused training steps on its column shard."""
    import sys
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import regneuralde_jl_amd as rn
    import bench
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    B = 32
    torch.manual_seed(7)
    model = bench.build_model(rn, dev, B)
    g = torch.Generator().manual_seed(5)
    X = torch.rand(world * B, 1, 28, 28, generator=g)
    Y = torch.eye(10)[torch.randint(0, 10, (world * B,), generator=g)]
    start = [p.detach().clone() for p in model.trainable()]

    def run(shards, reducer, fg):
        with torch.no_grad():
            for p, s0 in zip(model.trainable(), start):
                p.copy_(s0)
        opt = rn.FluxOptimiser(model.trainable())
        for _ in range(3):
            if reducer is not None:
                (r,) = shards
                rn.fused_loss_and_grad(model, X[r * B:(r + 1) * B].to(dev), Y[r * B:(r + 1) * B].to(dev), lam=1.0e2, sync=False, flat=fg, reducer=reducer)
            else:   # what the collective must reproduce: the shards' gradients summed in rank order
                tot = None
                for r in shards:
                    rn.fused_loss_and_grad(model, X[r * B:(r + 1) * B].to(dev), Y[r * B:(r + 1) * B].to(dev), lam=1.0e2, sync=True, flat=fg)
                    tot = fg.flat.clone() if tot is None else tot + fg.flat
                fg.flat.copy_(tot)
            opt.step(grad_scale=1.0 / world)
        torch.cuda.synchronize()
        return torch.cat([p.detach().reshape(-1) for p in model.trainable()]).cpu()

    fg = rn.FlatGrads(model.trainable())
    red = rn.GradientAllReducer(model.trainable(), flat=fg, collective="peers")
    got = run([rank], red, fg)
    want = run(list(range(world)), None, fg)
    q.put((rank, got.numpy(), want.numpy()))      # (numpy: a tensor would travel as a file descriptor of a process that may be gone)
    dist.barrier()
    dist.destroy_process_group()


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_data_parallel_steps_between_two_processes_equal_the_rank_order_sum():
    """Two processes, each integrating ITS 32 columns of a 64-column minibatch with its own controller (SURVEY 8e mode 1), one gradient
    all-reduce per step through the peer windows, InvDecay/Momentum with 1 / world folded in: after three steps every rank's parameters
    equal -- bit for bit -- what one process gets by running both shards itself and adding their gradients in rank order."""
    import tempfile
    import torch
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    fd, store = tempfile.mkstemp(prefix="rnde_dp_")
    os.close(fd)
    os.unlink(store)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, store, q)) for r in range(2)]
    try:
        for p in procs:
            p.start()
        res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
        if os.path.exists(store):
            os.unlink(store)
    (_, g0, w0), (_, g1, w1) = res
    assert np.array_equal(g0, g1)                      # replicas stay identical
    assert np.array_equal(w0, w1)
    print("max |distributed - rank-order reference| =", np.abs(g0 - w0).max(), "over", g0.size, "parameters")
    assert np.array_equal(g0, w0)


def test_one_shot_allreduce_reports_an_absent_rank(tmp_path):
    """A rank that never reaches the all-reduce: the waiting rank's kernel gives up (RNDE_ONESHOT_TIMEOUT_MS=300 here, 20 s by default),
    the stream drains, and rnde_comm_health says what happened -- no hang, no silent garbage (NaN in the buffer, a sticky error at the next enqueue)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RNDE_ONESHOT_TIMEOUT_MS="300")
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tools", "oneshot_worker.py"), "--rank", str(r), "--world", "2", "--dir", str(tmp_path),
                               "--absent", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for r in range(2)]
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=120)
            assert p.returncode == 0, e[-2000:]
            outs.append(json.loads(o.strip().splitlines()[-1]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    r0 = [o for o in outs if o["rank"] == 0][0]
    assert r0["enqueue"] == 0 and r0["health"] != 0 and "gave up" in r0["error"]
    # (round-3 advisor finding) the failure must reach a training loop that never calls rnde_comm_health: the reduced buffer is NaN, not a
    # partial sum, and the NEXT all-reduce of the communicator is refused -- on another stream too -- with the limit in force in the message
    assert r0["nan_frac"] == 1.0 and r0["next_enqueue"] != 0 and "gave up after 0.3 s" in r0["next_error"] and "failed for good" in r0["next_error"]


def test_bench_runs_eight_ranks_of_512_on_one_gpu_config3_rehearsal(share_gpu=False):
    """Config 3 as the driver launches it (`torchrun --nproc-per-node 8 bench.py --gpus 8 --global-batch 4096 ...`, 8 x 512 = global batch 4096, one
    gradient all-reduce per step): eight ranks, rank r on device r (RCCL, persistent kernels on every rank); it needs the 8 GPUs of config 3 and skips
    before it starts anything without them.  What it covers: the command line, rank / shard arithmetic, eight B = 512 solves and reverse sweeps, the
    8-way all-reduce of the 166,418-float buffer, the barrier + max-over-ranks timing, the `dist` diagnostics.  Not: any throughput figure.
    share_gpu=True is the one-device rig of the same run (`--share-gpu`: all eight ranks on device 0, gloo + the one-shot collective over eight
    peer-mapped windows, RCCL refusing two ranks on one device) -- nine processes on one GPU, so the suite does not run it; its assertions are kept
    for a hand run on a device that may hold them."""
    import json
    import socket
    import subprocess
    import sys
    if not share_gpu:
        _need_gpus_for_ranks(8)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "3", "--warmup", "1", "--global-batch", "4096", "--full", "--no-cpu-baseline", "--no-extras"]
    cmd += ["--share-gpu"] if share_gpu else []
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    o = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    d = o["dist"]
    print(json.dumps({k: o[k] for k in ("value", "ms_per_step", "mean_nfe", "n_gpus", "scaling")}), d)
    assert o["n_gpus"] == 8 and o["scaling"] == "strong" and o["config"]["global_batch"] == 4096 and o["value"] > 0
    assert d["allreduce_floats"] == 166418 and len(d["nfe_per_rank"]) == 8
    assert all(n > 0 for n in d["nfe_per_rank"])
    if share_gpu:
        # eight persistent 224-workgroup kernels cannot be co-resident on the 256 CUs of ONE device: the rig runs these ranks launch by launch (7 launches per
        # attempted step, stated in the line); persist_fallback_count is then 0 by construction
        assert "one-shot" in d["collective_path"]
        assert "persistent kernels OFF" in o["rig"] and d["launches_per_attempt_per_rank"] == [7] * 8 and d["persist_fallback_count_per_rank"] == [0] * 8
    else:
        # a rank that owns its GPU: RCCL, no rig, and the one-launch persistent kernels on every rank with no fallback
        assert o["rig"] is None and d["collective_library"] and d["collective_fallback"] is None
        assert not o["persist_fallback"] and d["launches_per_attempt_per_rank"] == [1] * 8 and d["persist_fallback_count_per_rank"] == [0] * 8
    assert np.isfinite(o["final_loss"])


def test_rccl_init_with_an_absent_rank_fails_loudly_in_bounded_time():
    """rnde_comm_create at world 2 with NO second rank: ncclCommInitRank would block for ever; the library waits RNDE_COMM_INIT_TIMEOUT_S for it and then
    returns an error that names the limit (round-5 review: fail loudly, not hang).  In a child process: the helper thread stuck inside RCCL dies with it."""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import ctypes as C, sys; sys.path.insert(0, %r)\n"
            "from regneuralde_jl_amd import _lib\n"
            "L = _lib.lib(); buf = C.create_string_buffer(128)\n"
            "assert L.rnde_comm_unique_id(buf) == 0\n"
            "comm = C.c_void_p()\n"
            "st = L.rnde_comm_create(bytes(buf.raw), 0, 2, 0, C.byref(comm))\n"
            "print('STATUS', st, L.rnde_comm_last_error(None).decode(), flush=True)\n"
            "import os; os._exit(0)\n") % root
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, RNDE_COMM_INIT_TIMEOUT_S="4"))
    el = time.time() - t0
    line = [l for l in r.stdout.splitlines() if l.startswith("STATUS")]
    assert line, (r.stdout[-500:], r.stderr[-1500:])
    print(line[0], "in %.1f s" % el)
    st = int(line[0].split()[1])
    assert st != 0 and ("did not return within 4 s" in line[0] or "ncclCommInitRank" in line[0])
