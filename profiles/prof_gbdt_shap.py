#!/usr/bin/env python3
"""What TreeSHAP contributions (GBDT.predict(pred_contrib=True), ptr_gbdt_shap of csrc/gbdt.hip) cost.

    python profiles/prof_gbdt_shap.py --run > R.json                     one fresh process
    python profiles/prof_gbdt_shap.py profiles/mi355x_gbdt_shap.json      PROCESSES fresh processes of --run, one after the other, and the summary

The workload: 100 trees of 400 leaves on 136 features, fitted leaf-wise on 100 000 MSLR-shaped synthetic documents under squared error
(fitted, not hand-built: the lengths of the paths and the number of distinct features on them decide the cost); the training matrix is
the background; 4096 of its rows are explained.  Inside a process the calls alternate contributions, plain predict, contributions, ...
for ROUNDS rounds after a warm-up, HIP events around each call; a process reports its medians and the summary the median over the
processes with their spread.  The figure is rows x trees per second.  The parent commit has no such call: the number is recorded, nobody
gates on it.  set_background (one counting launch, then the host builds the path tables) is timed once per process by the wall clock."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DOCUMENTS, FEATURES, TREES, LEAVES, ROWS = 100_000, 136, 100, 400, 4096
ROUNDS, PROCESSES = 7, 3
PARAMS = {"num_leaves": LEAVES, "max_bin": 255, "min_data_in_leaf": 50, "learning_rate": 0.1}


def run():
    import numpy as np
    import torch
    import ptranking_amd as pa

    assert torch.cuda.is_available(), "prof_gbdt_shap.py measures on the GPU only"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(137)
    X = torch.randn((DOCUMENTS, FEATURES), device=dev, generator=gen)
    w = torch.randn(FEATURES, device=dev, generator=gen) / FEATURES ** 0.5
    y = X @ w + 0.8 * X[:, 0] * X[:, 1] + 0.5 * torch.randn(DOCUMENTS, device=dev, generator=gen)
    booster = pa.GBDT(PARAMS, X)
    ones = torch.ones(DOCUMENTS, device=dev)
    for _ in range(TREES):
        booster.update(booster.scores - y, ones)
    torch.cuda.synchronize()
    t = time.perf_counter()
    booster.set_background(X)
    torch.cuda.synchronize()
    background_s = time.perf_counter() - t
    tables = booster._shap["tables"]
    per_leaf = np.diff(tables["elem_offsets"].cpu().numpy())
    nodes_per_leaf = np.diff(tables["path_offsets"].cpu().numpy())
    Xe = X[:ROWS].contiguous()
    calls = {"contrib": lambda: booster.predict(Xe, check_finite=False, pred_contrib=True), "predict": lambda: booster.predict(Xe, check_finite=False)}
    for fn in calls.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    phi = booster.predict(Xe, check_finite=False, pred_contrib=True)
    gap = float((phi.sum(dim=1) - booster.predict(Xe, check_finite=False).double()).abs().max())
    print(json.dumps(dict(trees=len(booster.trees), leaves=int(per_leaf.size), elements_per_leaf_mean=float(per_leaf.mean()),
                          elements_per_leaf_max=int(per_leaf.max()), nodes_per_leaf_mean=float(nodes_per_leaf.mean()), nodes_per_leaf_max=int(nodes_per_leaf.max()),
                          set_background_wall_s=background_s, median_ms={k: statistics.median(v) for k, v in ms.items()}, all_ms=ms,
                          rows_x_trees_per_s=ROWS * len(booster.trees) / (statistics.median(ms["contrib"]) * 1e-3), local_accuracy_gap=gap)))


def main(out_path):
    runs = []
    for _ in range(PROCESSES):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--run"], stdout=subprocess.PIPE, text=True, check=True, timeout=900)
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(runs[-1]["median_ms"]), flush=True)
    rate = [r["rows_x_trees_per_s"] for r in runs]
    result = dict(note=f"{PROCESSES} fresh processes one after the other; inside each the calls alternate contributions / plain predict for {ROUNDS} rounds "
                       "after a warm-up, HIP events around each call, the process's median; the figures below are medians over the processes",
                  documents=DOCUMENTS, features=FEATURES, rows=ROWS, params=PARAMS,
                  rows_x_trees_per_s=dict(median=statistics.median(rate), processes=rate, spread=max(rate) - min(rate)),
                  contrib_ms=statistics.median([r["median_ms"]["contrib"] for r in runs]),
                  predict_ms=statistics.median([r["median_ms"]["predict"] for r in runs]),
                  set_background_wall_s=statistics.median([r["set_background_wall_s"] for r in runs]), processes=runs)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--run":
        run()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_gbdt_shap.json"))
