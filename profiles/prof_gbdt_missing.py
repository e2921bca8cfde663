#!/usr/bin/env python3
"""What missing-value handling (use_missing=True of ptranking_amd/gbdt.py) costs, and that it costs nothing where it is off.

    python profiles/prof_gbdt_missing.py profiles/mi355x_gbdt_missing.json [--parent P1.json P2.json ... --head H1.json H2.json ...]
                                                                           [--measured M.json]

(--measured: the output of `python profiles/prof_gbdt_missing.py --measure > M.json` from an earlier process, in place of measuring now.)

1. A fit with NaNs against the same data imputed.  MSLR-shaped data of prof_gbdt.py (its "mslr" shape cut to 500 000 documents, F = 136,
   max_bin 255, num_leaves 400, min_data_in_leaf 50); a quarter of the features hold NaNs at a rate of 0.25.  One tree under
   use_missing=True on that matrix against one tree under use_missing=False on the matrix with every NaN replaced by its feature's mean,
   both policies, the two boosters alternating inside a round, ROUNDS rounds, wall clock around a device synchronise, all rounds kept.  The
   trees differ (the imputed matrix is another dataset), so the splits and the host reads of each stand beside its time.
2. Without the switch.  --parent / --head take the outputs of `python profiles/prof_gbdt.py --shape S > file`, run unchanged on the parent
   commit and on this one in alternating fresh processes; their one-tree and one-round wall times are folded into the output, with the
   parent's own spread between repeats beside the difference of the medians.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

ROUNDS = 5
DOCUMENTS, FEATURES, NAN_RATE = 500_000, 136, 0.25
PARAMS = {"num_leaves": 400, "max_bin": 255, "min_data_in_leaf": 50, "learning_rate": 0.05, "min_sum_hessian_in_leaf": 1e-3}


def measure():
    import numpy as np
    import torch
    import prof_tree
    import ptranking_amd as pa
    from bench import MSLR_P
    from ptranking_amd import tree

    assert torch.cuda.is_available(), "prof_gbdt_missing.py measures on the GPU only"
    dev = torch.device("cuda:0")
    _, _, group = prof_tree.draw()
    group = group[:int(np.searchsorted(np.cumsum(group), DOCUMENTS))]
    n = int(group.sum())
    gen = torch.Generator(device=dev).manual_seed(137)
    X = torch.randn((n, FEATURES), device=dev, generator=gen)
    w = torch.randn(FEATURES, device=dev, generator=gen) / FEATURES ** 0.5
    s = X @ w + 0.8 * X[:, 0] * X[:, 1] + 0.5 * torch.randn(n, device=dev, generator=gen)
    cuts = torch.quantile(s, torch.tensor(np.cumsum(MSLR_P)[:-1] / np.sum(MSLR_P), device=dev, dtype=torch.float32))
    y = torch.bucketize(s, cuts).float().cpu().numpy()
    holes = torch.rand((n, FEATURES // 4), device=dev, generator=gen) < NAN_RATE
    Xn = X.clone()
    Xn[:, ::4][holes] = float("nan")
    Xi = torch.where(torch.isnan(Xn), torch.nanmean(Xn, dim=0, keepdim=True), Xn)
    res = tree._Resident(y, group, dev)
    out = {}
    for policy in ("leafwise", "depthwise"):
        p = dict(PARAMS, grow_policy=policy)
        boosters = {"missing": pa.GBDT(dict(p, use_missing=True), Xn), "imputed": pa.GBDT(p, Xi)}
        lm = pa.LambdaMART(p)
        g, h = lm.grad_hess(boosters["imputed"].scores, res)

        def grow(b):
            b.scores.zero_()
            b.trees.clear()
            reads = b.host_reads
            torch.cuda.synchronize()
            t = time.perf_counter()
            first = b.update(g, h)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3, int(first["feature"].size), b.host_reads - reads

        for b in boosters.values():
            grow(b)
        walls = {k: [] for k in boosters}
        for i in range(ROUNDS):
            print(f"{policy}: round {i + 1} of {ROUNDS}", file=sys.stderr, flush=True)
            for k, b in boosters.items():
                ms, splits, reads = grow(b)
                walls[k].append(ms)
                out.setdefault(policy, {})[k] = dict(splits=splits, host_reads=reads)
        for k in boosters:
            out[policy][k].update(one_tree_wall_ms=statistics.median(walls[k]), all_rounds_wall_ms=walls[k])
        left = int(sum(int(t["default_left"].sum()) for t in boosters["missing"].trees))
        out[policy]["missing_over_imputed"] = out[policy]["missing"]["one_tree_wall_ms"] / out[policy]["imputed"]["one_tree_wall_ms"]
        out[policy]["missing"]["nodes_with_default_left"] = left
    print(json.dumps(dict(documents=n, features=FEATURES, features_with_nans=FEATURES // 4, nan_rate=NAN_RATE, params=PARAMS, rounds=ROUNDS,
                          policies=out)))


def fold(paths):
    """One-tree and one-round wall times of prof_gbdt.py outputs, by shape."""
    by_shape = {}
    for path in paths:
        with open(path) as f:
            r = json.loads(f.read().strip().splitlines()[-1])
        d = by_shape.setdefault(r["shape"], dict(one_tree_wall_ms=[], round_wall_ms=[], split_400_ms=[], partition_all_rows_ms=[], predict_ms=[]))
        d["one_tree_wall_ms"].append(r["one_tree"]["wall_ms"])
        d["round_wall_ms"].append(r["lambdamart_round"]["wall_ms"])
        d["split_400_ms"].append(r["median_ms"]["split_400"])
        d["partition_all_rows_ms"].append(r["median_ms"]["partition_all_rows"])
        d["predict_ms"].append(r["median_ms"]["predict_one_tree_400_leaves"])
    return by_shape


def main(argv):
    import subprocess
    out_path = argv[0] if argv and not argv[0].startswith("--") else os.path.join(ROOT, "profiles", "mi355x_gbdt_missing.json")
    lists, key = {"--parent": [], "--head": [], "--measured": []}, None
    for a in argv[1:]:
        if a in lists:
            key = a
        elif key:
            lists[key].append(a)
    if lists["--measured"]:
        with open(lists["--measured"][0]) as f:
            text = f.read()
    else:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure"], stdout=subprocess.PIPE, text=True, cwd=ROOT)
        if r.returncode != 0:
            raise SystemExit("the measurement failed")
        text = r.stdout
    result = dict(with_nans_against_imputed=json.loads(text.strip().splitlines()[-1]))
    if lists["--parent"] and lists["--head"]:
        parent, head = fold(lists["--parent"]), fold(lists["--head"])
        ab = {}
        for shape in parent:
            ab[shape] = {}
            for k, pv in parent[shape].items():
                hv = head[shape][k]
                ab[shape][k] = dict(parent=pv, head=hv, parent_median=statistics.median(pv), head_median=statistics.median(hv),
                                    head_minus_parent=statistics.median(hv) - statistics.median(pv), parent_spread=max(pv) - min(pv))
        result["without_the_switch"] = dict(note="profiles/prof_gbdt.py, unchanged, on the parent commit and on this one in alternating fresh "
                                                 "processes (parent, head, parent, head per shape); each figure is that script's median of 7",
                                            shapes=ab)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--measure":
        measure()
    else:
        main(sys.argv[1:])
