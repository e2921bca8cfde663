#!/usr/bin/env python3
"""Measures ONE ptr_gbdt_dart_walk launch over k trees against k launches of ptr_gbdt_add_tree_binned on the same trees.

    python profiles/prof_gbdt_dart.py profiles/mi355x_gbdt_dart.json

Rows: ROWS x 136 features of uniform random bins (0 .. 254).  Trees: random leaf-wise growth (a random leaf is split on a random feature at
a random bin) to 31 and to 400 leaves, 50 of each.  k in {1, 4, 16, 50}: the first k trees.  Both forms of the walk are measured on the
same bins: the tile form on the matrix at its stride of 144, the direct form on a copy padded to a stride of 160, which the launcher
sends to the direct form (ptr_gbdt.h).  The per-tree kernel as it stands is the baseline; its trees are uploaded before the clock starts.

Every (leaves, form) pair is measured in a fresh process.  Device events around the whole set of launches; the baseline and the walk
alternate inside each of ROUNDS rounds behind one dropped warm-up round; medians and all rounds are kept.  The two results are compared:
they agree up to fp32 rounding, not bit for bit (the baseline adds tree after tree into the score, the walk sums the trees first).
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, FEATURES, TREES, ROUNDS, KS, LEAVES = 1_000_000, 136, 50, 9, (1, 4, 16, 50), (31, 400)
STRIDES = {"tile": 144, "direct": 160}


def random_tree(leaves, rng):
    import numpy as np
    feature, bin, left, right, slot = [], [], [], [], [None]            # slot[l]: (node, side) that points at leaf l
    while len(slot) < leaves:
        l, node = int(rng.integers(len(slot))), len(feature)
        feature.append(int(rng.integers(FEATURES))); bin.append(int(rng.integers(255))); left.append(~l); right.append(~len(slot))
        if slot[l] is not None:
            (left if slot[l][1] == 0 else right)[slot[l][0]] = node
        slot[l] = (node, 0)
        slot.append((node, 1))
    return [np.array(a, np.int32) for a in (feature, bin, left, right)] + [rng.standard_normal(leaves).astype(np.float32) * 0.1]


def child(leaves, form):
    import numpy as np
    import torch
    import ptranking_amd.functional as F

    assert torch.cuda.is_available(), "prof_gbdt_dart.py measures on the GPU only"
    dev, rng = torch.device("cuda:0"), np.random.default_rng(leaves)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    bins = torch.zeros((ROWS, STRIDES[form]), device=dev, dtype=torch.uint8)
    bins[:, :FEATURES] = torch.randint(0, 255, (ROWS, FEATURES), device=dev, generator=torch.Generator(device=dev).manual_seed(137), dtype=torch.uint8)
    trees = [random_tree(leaves, rng) for _ in range(TREES)]
    per_tree = [[up(a) for a in t] for t in trees]
    nodes = up(np.concatenate([F.gbdt_dart_pack(*t[:4]) for t in trees]))
    values = up(np.concatenate([t[4] for t in trees]))
    offsets = up(np.concatenate([[0], np.cumsum([t[0].size for t in trees])]).astype(np.int32))
    scores = torch.zeros(ROWS, device=dev)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def baseline(k, out):
        for t in per_tree[:k]:
            F.gbdt_add_tree_binned(out, bins, FEATURES, None, *t)

    out = {}
    for k in KS:
        lst = torch.arange(k, device=dev, dtype=torch.int32)
        a, b = torch.zeros_like(scores), torch.zeros_like(scores)
        baseline(k, a)
        F.gbdt_dart_walk(b, bins, FEATURES, nodes, values, offsets, lst, 1)
        ms = {"per_tree": [], "walk": []}
        for _ in range(ROUNDS + 1):
            ms["per_tree"].append(events(lambda: baseline(k, scores)))
            ms["walk"].append(events(lambda: F.gbdt_dart_walk(scores, bins, FEATURES, nodes, values, offsets, lst, 1)))
        med = {name: statistics.median(v[1:]) for name, v in ms.items()}
        out[str(k)] = dict(median_ms=med, all_rounds_ms={name: v[1:] for name, v in ms.items()}, walk_over_per_tree=med["walk"] / med["per_tree"],
                           max_abs_difference=float((a - b).abs().max()), finite=bool(torch.isfinite(b).all()))
    print(json.dumps(out))


def main(out_path):
    results = {}
    for leaves in LEAVES:
        for form in STRIDES:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(leaves), form], stdout=subprocess.PIPE, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"the measurement of {leaves} leaves, {form} form ended with status {r.returncode}")
            results[f"leaves{leaves}_{form}"] = json.loads(r.stdout.strip().splitlines()[-1])
            print(leaves, form, {k: v["median_ms"] for k, v in results[f"leaves{leaves}_{form}"].items()}, file=sys.stderr, flush=True)
    out = dict(rows=ROWS, features=FEATURES, strides=STRIDES, trees=TREES, rounds=ROUNDS, results=results,
               note="device events around all launches of a set; the per-tree kernel (k launches of ptr_gbdt_add_tree_binned) and one "
                    "ptr_gbdt_dart_walk launch alternate inside each round, one warm-up round dropped; one fresh process per (leaves, form)")
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({name: {k: round(v["walk_over_per_tree"], 3) for k, v in r.items()} for name, r in results.items()}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), sys.argv[3])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_gbdt_dart.json"))
