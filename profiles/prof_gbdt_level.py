#!/usr/bin/env python3
"""Times one tree of the native booster under both growth policies (grow_policy 'leafwise' and 'depthwise' of ptranking_amd/gbdt.py).

    python profiles/prof_gbdt_level.py profiles/mi355x_gbdt_level.json

The method and the shapes of prof_gbdt.py: "mslr" = 2.28 M documents x 136 features, "wide" = 0.5 M documents x 700 features; max_bin 255,
num_leaves 400, min_data_in_leaf 50.  Each shape runs in a fresh child process under a time limit of its own, and the first failure ends
the run; the parent never opens the GPU.  Every figure is the median of ROUNDS rounds, the two policies alternating inside a round on the
SAME booster and the same gradients: a host clock around a device synchronise for whole trees and LambdaMART rounds, device events around
every C-ABI call for the entry points (so the four batched entry points are timed once per level).  All rounds are kept.
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
LEVEL_ENTRIES = ("ptr_gbdt_partition_segments", "ptr_gbdt_histogram_segments", "ptr_gbdt_hist_sub_segments", "ptr_gbdt_best_split_slots")
# kernel launches behind one call (include/ptranking_amd.h): the batched histogram makes at most two, one per form
LAUNCHES = {"ptr_gbdt_quantize": 2, "ptr_gbdt_histogram": 1, "ptr_gbdt_hist_sub": 1, "ptr_gbdt_best_split": 2, "ptr_gbdt_partition": 3,
            "ptr_gbdt_add_leaf_values": 1, "ptr_gbdt_histogram_segments": 2, "ptr_gbdt_hist_sub_segments": 1, "ptr_gbdt_best_split_slots": 2,
            "ptr_gbdt_partition_segments": 3}


def measure(shape):
    import numpy as np
    import torch
    import prof_gbdt
    import prof_tree
    import ptranking_amd as pa
    from bench import MSLR_P
    from ptranking_amd import _lib, tree

    assert torch.cuda.is_available(), "prof_gbdt_level.py measures on the GPU only"
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
    booster = pa.GBDT(prof_gbdt.PARAMS, X)                          # one booster, one set of bins: the policy is switched between trees
    print(f"{shape}: {n} documents x {nf} features binned", file=sys.stderr, flush=True)
    lm = pa.LambdaMART(prof_gbdt.PARAMS)
    res = tree._Resident(y, group, dev)
    g, h = lm.grad_hess(booster.scores, res)
    g0, h0 = g.clone(), h.clone()

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def grow(policy, timing):
        booster.params["grow_policy"] = policy
        booster.scores.zero_()
        booster.trees.clear()
        reads = booster.host_reads
        _lib.TIMING = {} if timing else None
        ms, t = wall(lambda: booster.update(g0, h0))
        stamps, _lib.TIMING = _lib.TIMING, None
        info = dict(ms=ms, leaves=int(t["value"].size), host_reads=booster.host_reads - reads)
        if timing:
            info["per_call_ms"] = {k: [a.elapsed_time(b) for a, b in v] for k, v in stamps.items()}
        return info

    def round_(policy):
        booster.params["grow_policy"] = policy
        booster.scores.zero_()
        booster.trees.clear()

        def go():
            lm.grad_hess(booster.scores, res, (g, h))
            booster.update(g, h)
        return wall(go)[0]

    policies = ("leafwise", "depthwise")
    for p in policies:
        grow(p, False), grow(p, True), round_(p)
    trees, timed, rounds = {p: [] for p in policies}, {p: [] for p in policies}, {p: [] for p in policies}
    for i in range(ROUNDS):
        print(f"{shape}: round {i + 1} of {ROUNDS}", file=sys.stderr, flush=True)
        for p in policies if i % 2 == 0 else policies[::-1]:
            trees[p].append(grow(p, False))
            timed[p].append(grow(p, True))
            rounds[p].append(round_(p))
    out = dict(shape=shape, documents=n, features=nf, params=prof_gbdt.PARAMS)
    for p in policies:
        calls = {k: len(v) for k, v in timed[p][0]["per_call_ms"].items()}
        total = {k: statistics.median(sum(t["per_call_ms"][k]) for t in timed[p]) for k in calls}
        out[p] = dict(tree_wall_ms=statistics.median(t["ms"] for t in trees[p]), all_rounds_tree_wall_ms=[t["ms"] for t in trees[p]],
                      leaves=trees[p][0]["leaves"], host_reads=trees[p][0]["host_reads"], entry_point_calls=calls,
                      kernel_launches_at_most=sum(LAUNCHES.get(k, 1) * c for k, c in calls.items()), entry_point_ms=total,
                      entry_points_total_ms=statistics.median(sum(sum(v) for v in t["per_call_ms"].values()) for t in timed[p]),
                      lambdamart_round_wall_ms=statistics.median(rounds[p]), all_rounds_round_wall_ms=rounds[p])
    levels = calls.get("ptr_gbdt_partition_segments", 0)
    out["depthwise"]["levels"] = levels
    out["depthwise"]["per_level_ms"] = {k: [statistics.median(t["per_call_ms"][k][i] for t in timed["depthwise"]) for i in range(len(timed["depthwise"][0]["per_call_ms"].get(k, [])))]
                                        for k in LEVEL_ENTRIES}
    out["depthwise_faster"] = out["depthwise"]["tree_wall_ms"] < out["leafwise"]["tree_wall_ms"]
    out["leafwise_over_depthwise"] = out["leafwise"]["tree_wall_ms"] / out["depthwise"]["tree_wall_ms"]
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
        print(json.dumps({k: results[shape][k] for k in ("shape", "depthwise_faster", "leafwise_over_depthwise")}
                         | {p: {k: results[shape][p][k] for k in ("tree_wall_ms", "leaves", "host_reads", "kernel_launches_at_most", "lambdamart_round_wall_ms")}
                            for p in ("leafwise", "depthwise")}), flush=True)
    with open(out_path, "w") as f:
        json.dump(dict(rounds=ROUNDS, shapes=results), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--shape":
        measure(sys.argv[2])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_gbdt_level.json"))
