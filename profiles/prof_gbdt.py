#!/usr/bin/env python3
"""Times the gradient-boosted tree kernels (csrc/gbdt.hip) and one LambdaMART round of ptranking_amd/gbdt.py on MSLR-shaped data.

    python profiles/prof_gbdt.py profiles/mi355x_gbdt.json

Shapes: "mslr" = the dataset of prof_tree.py (19 000 queries, 2.28 M documents) with F = 136, and "wide" = F = 700 at 0.5 M documents;
max_bin 255, num_leaves 400, min_data_in_leaf 50.  Features are N(0, 1), the relevance is planted (linear + one interaction) and graded with
bench.MSLR_P.  Each shape is measured in a fresh child process; the parent never opens the GPU.  Every figure is the median of ROUNDS rounds
with the items alternating inside a round, timed with device events (kernels) or a host clock around a device synchronise (whole trees and
rounds); all rounds are kept.  A histogram's byte bound is (16 bytes of bins + 8 bytes of qg, qh per row and feature tile + 4 bytes of row
index when a row list is given + 24 bytes per (feature, bin) of flush) over the HBM figure of ptranking_amd/peaks.py.
No LightGBM figure stands beside these: the library is not installed on these machines.
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
SHAPES = {"mslr": dict(features=136, documents=None), "wide": dict(features=700, documents=500_000)}
PARAMS = {"num_leaves": 400, "max_bin": 255, "min_data_in_leaf": 50, "learning_rate": 0.05, "min_sum_hessian_in_leaf": 1e-3}
OBJECTIVE_CALL_MS = 4.5            # profiles/mi355x_tree_objectives.json: one TreeObjective call, wall (2.0 ms of it in kernels)


def measure(shape):
    import numpy as np
    import torch
    import prof_tree
    import ptranking_amd as pa
    import ptranking_amd.functional as F
    from bench import MSLR_P
    from ptranking_amd import _lib, tree
    from ptranking_amd.peaks import HBM_PEAK_GBPS

    assert torch.cuda.is_available(), "prof_gbdt.py measures on the GPU only"
    dev = torch.device("cuda:0")
    nf = SHAPES[shape]["features"]
    _, _, group = prof_tree.draw()
    if SHAPES[shape]["documents"]:
        group = group[:int(np.searchsorted(np.cumsum(group), SHAPES[shape]["documents"]))]
    n = int(group.sum())
    gen = torch.Generator(device=dev).manual_seed(137)
    X = torch.randn((n, nf), device=dev, generator=gen)
    w = torch.randn(nf, device=dev, generator=gen) / nf ** 0.5
    s = X @ w + 0.8 * X[:, 0] * X[:, 1] + 0.5 * torch.randn(n, device=dev, generator=gen)
    cuts = torch.quantile(s[:1_000_000], torch.tensor(np.cumsum(MSLR_P)[:-1] / np.sum(MSLR_P), device=dev, dtype=torch.float32))
    y = torch.bucketize(s, cuts).float().cpu().numpy()
    t0 = time.perf_counter()
    booster = pa.GBDT(PARAMS, X)
    fit_bins_s = time.perf_counter() - t0
    print(f"{shape}: {n} documents x {nf} features binned in {fit_bins_s:.1f} s", file=sys.stderr, flush=True)
    lm = pa.LambdaMART(PARAMS)
    res = tree._Resident(y, group, dev)
    mb, stride = PARAMS["max_bin"], booster.bins.shape[1]
    tiles = stride // 16

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    g, h = lm.grad_hess(booster.scores, res)
    qg, qh, expo, _ = F.gbdt_quantize(g, h)
    perm = torch.randperm(n, device=dev, generator=gen).to(torch.int32)
    lists = {"root": None, "mid": torch.sort(perm[:n // 16])[0].contiguous(), "small": perm[:256].contiguous(), "small_lds": perm[:257].contiguous()}
    const_bins = torch.zeros_like(booster.bins)
    hist = torch.zeros((nf, mb, 3), device=dev, dtype=torch.int64)
    pool = torch.zeros((400, nf, mb, 3), device=dev, dtype=torch.int64)
    pool[:] = F.gbdt_histogram(booster.bins, qg, qh, None, nf, mb)
    all_rows = torch.arange(n, device=dev, dtype=torch.int32)
    first = booster.update(g, h)                                   # one tree of 400 leaves: also the model predict walks
    feature0, bin0 = int(first["feature"][0]), int(np.searchsorted(booster.edges[first["feature"][0]], first["threshold"][0]))

    def grow(timing):
        booster.scores.zero_()
        booster.trees.clear()
        _lib.TIMING = {} if timing else None
        ms, _ = wall(lambda: booster.update(g, h))
        stamps, _lib.TIMING = _lib.TIMING, None
        if not timing:
            return ms
        per = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in stamps.items()}
        return ms, per, {k: len(v) for k, v in stamps.items()}

    def round_():
        booster.scores.zero_()
        booster.trees.clear()

        def go():
            lm.grad_hess(booster.scores, res, (g, h))
            booster.update(g, h)
        return wall(go)[0]

    items = {f"hist_{k}": (lambda r=r: F.gbdt_histogram(booster.bins, qg, qh, r, nf, mb, hist=hist)) for k, r in lists.items()}
    items.update({f"hist_const_{k}": (lambda r=lists[k]: F.gbdt_histogram(const_bins, qg, qh, r, nf, mb, hist=hist)) for k in ("root", "mid")})
    items.update({"split_1": lambda: F.gbdt_best_split(pool[:1], booster._nbins_d, expo, 0.0, 50, 1e-3, 0.0),
                  "split_400": lambda: F.gbdt_best_split(pool, booster._nbins_d, expo, 0.0, 50, 1e-3, 0.0),
                  "hist_sub": lambda: F.gbdt_hist_sub(pool[0], pool[1], out=pool[2]),
                  "partition_all_rows": lambda: F.gbdt_partition(booster.bins, all_rows, feature0, bin0, nf),
                  "quantize": lambda: F.gbdt_quantize(g, h),
                  "predict_one_tree_400_leaves": lambda: booster.predict(X)})
    for fn in items.values():
        fn()
    grow(False), grow(True), round_()
    rounds = {k: [] for k in items}
    tree_wall, tree_timed, round_wall = [], [], []
    for i in range(ROUNDS):
        print(f"{shape}: round {i + 1} of {ROUNDS}", file=sys.stderr, flush=True)
        for k, fn in items.items():
            rounds[k].append(events(fn)[0])
        tree_wall.append(grow(False))
        tree_timed.append(grow(True))
        round_wall.append(round_())
    med = {k: statistics.median(v) for k, v in rounds.items()}
    bounds = {}
    for k, r in lists.items():
        m = n if r is None else r.numel()
        nbytes = m * tiles * (16 + 8) + (0 if r is None else 4 * m) + nf * mb * 24
        bound_ms = nbytes / (HBM_PEAK_GBPS * 1e9) * 1e3
        bounds[f"hist_{k}"] = dict(rows=m, bytes=nbytes, bound_ms=bound_ms, share_of_bound=bound_ms / med[f"hist_{k}"],
                                   form=list(_form(m, nf, mb)))
    kernel_ms = [sum(per.values()) for _, per, _ in tree_timed]
    breakdown = {k: statistics.median(per.get(k, 0.0) for _, per, _ in tree_timed) for k in tree_timed[0][1]}
    tree_ms = statistics.median(tree_wall)
    out = dict(shape=shape, documents=n, queries=int(group.size), features=nf, params=PARAMS, fit_bins_seconds=fit_bins_s, median_ms=med,
               all_rounds_ms=rounds, histogram_byte_bounds=bounds,
               constant_feature_vs_random=dict(root=med["hist_const_root"] / med["hist_root"], mid=med["hist_const_mid"] / med["hist_mid"]),
               one_tree=dict(splits=int(first["feature"].size), wall_ms=tree_ms, all_rounds_wall_ms=tree_wall,
                             wall_ms_with_event_brackets=statistics.median(t for t, _, _ in tree_timed),
                             entry_point_ms=breakdown, entry_point_calls=tree_timed[0][2], entry_points_total_ms=statistics.median(kernel_ms),
                             host_and_sync_ms=tree_ms - statistics.median(kernel_ms),
                             note="entry_point_ms: device events around every C-ABI call of one update(); host_and_sync_ms = wall of an "
                                  "unbracketed update() minus their sum: the per-split record read-back, torch's own small kernels and Python"),
               lambdamart_round=dict(wall_ms=statistics.median(round_wall), all_rounds_wall_ms=round_wall, objective_call_ms_existing_path=OBJECTIVE_CALL_MS,
                                     note="one round = gradients on the device + quantize + one tree of 400 leaves; the existing path's figure is the "
                                          "objective call ALONE (preds up, grad / hess down), with the boosting left to a CPU library that is not here"))
    print(json.dumps(out))


def _form(m, nf, mb):
    import ctypes
    from ptranking_amd import _lib
    a, o = (ctypes.c_int64 * 3)(m, nf, mb), (ctypes.c_int32 * 8)()
    assert _lib.load().ptr_launch_form(b"ptr_gbdt_histogram", a, 3, o, 8) == 0
    return tuple(o)[:5]


def main(out_path):
    results = {}
    for shape in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", shape], stdout=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:
            raise SystemExit(f"shape {shape} failed")
        results[shape] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps({"shape": shape, "median_ms": results[shape]["median_ms"], "one_tree_ms": results[shape]["one_tree"]["wall_ms"],
                          "round_ms": results[shape]["lambdamart_round"]["wall_ms"]}), flush=True)
    with open(out_path, "w") as f:
        json.dump(dict(rounds=ROUNDS, note="no LightGBM comparison exists: the library is not installed on these machines", shapes=results), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--shape":
        measure(sys.argv[2])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_gbdt.json"))
