"""Time of TrackedFFJORD's likelihood pass (regneuralde_jl_amd.loglikelihood, reference src/metrics.jl:20-33), one solve per batch against several
batches per launch (groups=k: rnde_ffjord_forward_groups), at the two experiments' geometries with synthetic data from the training tools'
own generators:

  tabular    MLPDynamics(43, 100) on engine="tiled", tol 1.4e-8, 32 batches of 1024 (tools/train_ffjord_tabular.py: synthetic), groups 1, 2, 4
  gaussian   MLPDynamics(2, 16) on engine="tiled", tol 1.4e-8, batches of 1024 of the gaussian mixture (load_gaussian_mixture), groups 1, 4

groups=1 is the loop as it was: one untaped solve and one float(logpx.sum()) read-back per batch -- the baseline.  A sample is the host time
of one whole pass between two device synchronisations; the legs of a geometry alternate inside every round of one process, after `--warmup`
untimed rounds.  The layer's seed is set back in front of every pass, so every leg solves with the same probes: the NFE of every batch is
recorded per leg and asserted equal; the likelihoods agree to fp32's rounding of groups=1's per-batch sums (asserted to 1e-6 relative).  Beside the passes:
the HIP-event time of one launch per leg over its attempts (rnde_ffjord_timing; a group launch lasts as long as its longest group), which
shows what agent-scope meetings and a shared L2 cost per attempt.  --bench-before / --bench-after: files holding one `python bench.py` result
line each (the parent's library and this one), copied into the record.  Writes profiles/ffjord_groups.json.

    python tools/time_ffjord_groups.py [--rounds 7] [--warmup 3] [--batches 32] [--gaussian-batches 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEED = 0x5EED


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(variants, warmup, rounds):
    ms = {k: [] for k in variants}
    for r in range(warmup + rounds):
        for k, fn in variants.items():                # alternated: every leg sees the same clocks and the same neighbours
            v = timed(fn)
            if r >= warmup:
                ms[k].append(v)
    return {k: dict(min=float(np.min(v)), median=float(np.median(v)), max=float(np.max(v)), samples_ms=v) for k, v in ms.items()}


def overlap(a, b):
    return not (a["max"] < b["min"] or b["max"] < a["min"])


def leg(rn, ff, batches, ks, warmup, rounds):
    """The passes of one geometry: groups in ks (1 first), alternated."""
    dev = torch.device("cuda", ff.device)
    got = {}

    def run(k):
        def fn():
            ff._seed = SEED
            got[k] = rn.loglikelihood(ff, batches, groups=k)
        return fn
    res = alternate({f"groups={k}": run(k) for k in ks}, warmup, rounds)
    # equal work: the NFE of every batch, per leg, on the passes' own probes
    nfe = {}
    ff._seed = SEED
    nfe[1] = []
    with torch.no_grad():
        for x in batches:
            nfe[1].append(int(ff(torch.from_numpy(x).to(dev))[3]))
    attempt_us = {}
    s, _, n, _ = ff.timing()
    attempt_us["groups=1"] = dict(launch_ms=s, attempts=n, us_per_attempt=1e3 * s / n, batch="the last")
    for k in ks[1:]:
        ff._seed = SEED
        nfe[k] = []
        for i in range(0, len(batches), k):
            nfe[k] += ff.logpx_batches([torch.from_numpy(x).to(dev) for x in batches[i:i + k]])[1]
        assert nfe[k] == nfe[1], (k, nfe[k], nfe[1])
        # (groups=1 adds each batch's logpx in fp32, float(logpx.sum()); the grouped legs add every column in double: they agree to fp32's
        # rounding of a 1024-term sum, and the grouped legs agree with each other to double's)
        assert abs(got[k] - got[1]) <= 1e-6 * abs(got[1]), (k, got[k], got[1])
        assert abs(got[k] - got[ks[1]]) <= 1e-12 * abs(got[k]), (k, got[k], got[ks[1]])
        s = ff.timing()[0]                            # the last call: the last <= k batches
        last = nfe[k][-(len(batches) % k or k):]
        att = max((v - 3) // 6 for v in last)
        attempt_us[f"groups={k}"] = dict(launch_ms=s, groups_in_launch=len(last), attempts_of_the_longest_group=att, us_per_attempt=1e3 * s / att)
    base = res["groups=1"]
    pairs = {}
    for k in ks[1:]:
        r = res[f"groups={k}"]
        pairs[f"groups={k}"] = dict(median_ratio_groups1_over_this=base["median"] / r["median"], ranges_overlap=overlap(base, r))
    return dict(batches=len(batches), batch=int(batches[0].shape[0]), ms_per_pass=res, against_groups_1=pairs, nfe_per_batch=nfe[1],
                nfe_equal_in_every_leg=True, loglikelihood={f"groups={k}": got[k] for k in ks}, launch=attempt_us,
                group_capacity=list(ff.group_capacity()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--gaussian-batches", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bench-before", default=None, help="a file with one `python bench.py` result line of the parent's library")
    ap.add_argument("--bench-after", default=None, help="the same of this library")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffjord_groups.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert a.rounds >= 5
    import regneuralde_jl_amd as rn
    from train_ffjord_tabular import synthetic

    B = a.batch
    tr, _ = synthetic(B, 43, 0, n=int(round(a.batches * B / 0.8)), split=0.8)
    tab = [tr.X[i * B:(i + 1) * B] for i in range(a.batches)]
    assert all(x.shape == (B, 43) for x in tab)
    ff_t = rn.TrackedFFJORD(rn.ffjord.MLPDynamics(43, 100, generator=torch.Generator().manual_seed(0)), [0.0, 1.0], True, False, "Tsit5",
                            reltol=1.4e-8, abstol=1.4e-8, max_batch=B, engine="tiled")
    gtr, _ = rn.load_gaussian_mixture(B, nsamples=int(round(a.gaussian_batches * B / 0.75)) + 12, ngaussians=6, seed=0)
    gau = [gtr.X[i * B:(i + 1) * B] for i in range(a.gaussian_batches)]
    assert all(x.shape == (B, 2) for x in gau)
    ff_g = rn.TrackedFFJORD(rn.ffjord.MLPDynamics(2, 16, generator=torch.Generator().manual_seed(0)), [0.0, 1.0], True, False, "Tsit5",
                            reltol=1.4e-8, abstol=1.4e-8, max_batch=B, engine="tiled")
    out = dict(method=f"host clock around one whole likelihood pass between two device synchronisations; {a.rounds} rounds after {a.warmup} warm-up rounds, the "
                      "legs of a geometry alternated inside every round of one process; groups=1 is the one-solve-per-batch loop (the baseline); the same "
                      "probes in every leg, NFE of every batch asserted equal between the legs; launch: HIP events around one solve launch",
               tabular=leg(rn, ff_t, tab, [1, 2, 4], a.warmup, a.rounds),
               gaussian=leg(rn, ff_g, gau, [1, 4], a.warmup, a.rounds))
    for key, path in (("bench_before", a.bench_before), ("bench_after", a.bench_after)):
        if path:
            lines = [l for l in open(path).read().splitlines() if l.startswith("{")]
            out[key] = json.loads(lines[-1])
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
