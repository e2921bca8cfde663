#!/usr/bin/env python3
"""Times one tree of the native booster without row sampling, under query bagging 0.5 and under GOSS 0.2 / 0.1, with both growth policies,
and the sampler's own entry points against their byte bounds.

    python profiles/prof_gbdt_sample.py profiles/mi355x_gbdt_sample.json

The method and the shapes of prof_gbdt.py and prof_gbdt_level.py: "mslr" = 2.28 M documents x 136 features, "wide" = 0.5 M documents x 700
features; max_bin 255, num_leaves 400, min_data_in_leaf 50.  Each shape runs in a fresh child process under a time limit of its own, and
the first failure ends the run; the parent never opens the GPU.  Every figure is the median of ROUNDS rounds; the six configurations
(sampling x policy) alternate inside a round on the SAME booster, bins and gradients.  A host clock around a device synchronise for whole
trees, device events around every C-ABI call for the entry points.  Every tree is grown as tree number WARM (past GOSS's warm-up of
floor(1 / learning_rate) trees) and draws its bag afresh.  The baseline of every ratio is the unsampled tree of the same process; it is
compared with mi355x_gbdt.json's one_tree.wall_ms and that file's round-to-round spread.  All rounds are kept.

Byte models (per row of the n, over peaks.HBM_PEAK_GBPS): bag mask 1 written (+ 4 of qid by query); GOSS 3 counting passes x 8 read + the
apply pass 8 read, 8 + 1 written = 41; the mask partition 2 x 1 read (count, scatter) + 4 written = 6; the out-of-bag walk per TAIL row 4
(row index) + 8 (score read and written) + 64 (one line of the row's bins at the least).
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

ROUNDS = 7
SHAPE_SECONDS = 420
SAMPLING = {"none": {"data_sample_strategy": "bagging", "bagging_freq": 0, "bagging_fraction": 1.0, "bagging_by_query": False},
            "query_bagging_0.5": {"data_sample_strategy": "bagging", "bagging_freq": 1, "bagging_fraction": 0.5, "bagging_by_query": True},
            "goss_0.2_0.1": {"data_sample_strategy": "goss", "bagging_freq": 0, "bagging_fraction": 1.0, "bagging_by_query": False,
                             "top_rate": 0.2, "other_rate": 0.1}}
POLICIES = ("leafwise", "depthwise")
SAMPLER_ENTRIES = ("ptr_gbdt_bag_mask", "ptr_gbdt_goss", "ptr_gbdt_partition_mask", "ptr_gbdt_add_tree_binned")


def measure(shape):
    import numpy as np
    import torch
    import prof_gbdt
    import prof_tree
    import ptranking_amd as pa
    from bench import MSLR_P
    from ptranking_amd import _lib, tree
    from ptranking_amd.peaks import HBM_PEAK_GBPS

    assert torch.cuda.is_available(), "prof_gbdt_sample.py measures on the GPU only"
    dev = torch.device("cuda:0")
    nf = prof_gbdt.SHAPES[shape]["features"]
    _, _, group = prof_tree.draw()
    if prof_gbdt.SHAPES[shape]["documents"]:
        group = group[:int(np.searchsorted(np.cumsum(group), prof_gbdt.SHAPES[shape]["documents"]))]
    n = int(group.sum())
    gen = torch.Generator(device=dev).manual_seed(137)
    X = torch.randn((n, nf), device=dev, generator=gen)
    w = torch.randn(nf, device=dev, generator=gen) / nf ** 0.5
    s = X @ w + 0.8 * X[:, 0] * X[:, 1] + 0.5 * torch.randn(n, device=dev, generator=gen)
    cuts = torch.quantile(s[:1_000_000], torch.tensor(np.cumsum(MSLR_P)[:-1] / np.sum(MSLR_P), device=dev, dtype=torch.float32))
    y = torch.bucketize(s, cuts).float().cpu().numpy()
    # one booster, one set of bins, the sampler's buffers allocated (GOSS needs them all): the configuration is switched between trees
    booster = pa.GBDT(dict(prof_gbdt.PARAMS, **SAMPLING["goss_0.2_0.1"])).fit_bins(X, group=group)
    warm = int(np.floor(1.0 / booster.params["learning_rate"]))
    print(f"{shape}: {n} documents x {nf} features binned", file=sys.stderr, flush=True)
    lm = pa.LambdaMART(prof_gbdt.PARAMS)
    res = tree._Resident(y, group, dev)
    g0, h0 = (t.clone() for t in lm.grad_hess(booster.scores, res))

    def grow(sampling, policy, timing):
        booster.params.update(SAMPLING[sampling], grow_policy=policy)
        booster.scores.zero_()
        booster.trees[:] = [None] * warm                               # tree number `warm`: past GOSS's warm-up
        booster._bag_draw = None                                       # the bag is drawn, not reused
        reads = booster.host_reads
        _lib.TIMING = {} if timing else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = booster.update(g0, h0)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        stamps, _lib.TIMING = _lib.TIMING, None
        info = dict(ms=ms, leaves=int(t["value"].size), host_reads=booster.host_reads - reads,
                    bag=int(booster._mask.sum()) if sampling != "none" else n)
        if timing:
            info["per_call_ms"] = {k: [a.elapsed_time(b) for a, b in v] for k, v in stamps.items()}
        return info

    configs = [(s_, p) for s_ in SAMPLING for p in POLICIES]
    for c in configs:
        grow(*c, False), grow(*c, True)
    trees, timed = {c: [] for c in configs}, {c: [] for c in configs}
    for i in range(ROUNDS):
        print(f"{shape}: round {i + 1} of {ROUNDS}", file=sys.stderr, flush=True)
        for c in configs if i % 2 == 0 else configs[::-1]:
            trees[c].append(grow(*c, False))
            timed[c].append(grow(*c, True))
    med = statistics.median
    stride = booster.bins.shape[1]
    out = dict(shape=shape, documents=n, queries=int(group.size), features=nf, params=prof_gbdt.PARAMS, tree_number=warm, hbm_peak_gbps=HBM_PEAK_GBPS)
    for s_ in SAMPLING:
        out[s_] = {}
        for p in POLICIES:
            c = (s_, p)
            bag = trees[c][0]["bag"]
            r = dict(tree_wall_ms=med(t["ms"] for t in trees[c]), all_rounds_tree_wall_ms=[t["ms"] for t in trees[c]], leaves=trees[c][0]["leaves"],
                     host_reads=trees[c][0]["host_reads"], bag_rows=bag, bag_share=bag / n,
                     entry_points_total_ms=med(sum(sum(v) for v in t["per_call_ms"].values()) for t in timed[c]),
                     entry_point_ms={k: med(sum(t["per_call_ms"][k]) for t in timed[c]) for k in timed[c][0]["per_call_ms"]})
            bytes_ = {"ptr_gbdt_bag_mask": n * (1 + (4 if SAMPLING[s_]["bagging_by_query"] else 0)), "ptr_gbdt_goss": n * 41, "ptr_gbdt_partition_mask": n * 6,
                      "ptr_gbdt_add_tree_binned": (n - bag) * (12 + min(stride, 64))}
            r["sampler"] = {k: dict(ms=r["entry_point_ms"][k], byte_bound_ms=bytes_[k] / (HBM_PEAK_GBPS * 1e9) * 1e3,
                                    share_of_byte_bound=bytes_[k] / (HBM_PEAK_GBPS * 1e9) * 1e3 / r["entry_point_ms"][k])
                            for k in SAMPLER_ENTRIES if k in r["entry_point_ms"]}
            out[s_][p] = r
    for p in POLICIES:
        base = out["none"][p]["tree_wall_ms"]
        out[f"{p}_over_unsampled"] = {s_: out[s_][p]["tree_wall_ms"] / base for s_ in SAMPLING if s_ != "none"}
    with open(os.path.join(ROOT, "profiles", "mi355x_gbdt.json")) as f:
        parent = json.load(f)
    one = parent.get("shapes", parent)[shape]["one_tree"]
    lo, hi = min(one["all_rounds_wall_ms"]), max(one["all_rounds_wall_ms"])
    mine = out["none"]["leafwise"]["tree_wall_ms"]
    out["baseline"] = dict(unsampled_leafwise_tree_wall_ms=mine, mi355x_gbdt_one_tree_wall_ms=one["wall_ms"], mi355x_gbdt_rounds_min_max_ms=[lo, hi],
                           within_that_spread=abs(mine - one["wall_ms"]) <= hi - lo)
    print(json.dumps(out))


def main(out_path):
    results = {}
    for shape in ("mslr", "wide"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", shape], stdout=subprocess.PIPE, text=True, cwd=ROOT, timeout=SHAPE_SECONDS)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"shape {shape} ran past {SHAPE_SECONDS} s: nothing more is started")
        if r.returncode != 0:
            raise SystemExit(f"shape {shape} failed with status {r.returncode}: nothing more is started")
        results[shape] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps({"shape": shape, "baseline": results[shape]["baseline"]}
                         | {s_: {p: {k: results[shape][s_][p][k] for k in ("tree_wall_ms", "leaves", "host_reads", "bag_share")} for p in POLICIES} for s_ in SAMPLING}),
              flush=True)
    with open(out_path, "w") as f:
        json.dump(dict(rounds=ROUNDS, shapes=results), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--shape":
        measure(sys.argv[2])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_gbdt_sample.json"))
