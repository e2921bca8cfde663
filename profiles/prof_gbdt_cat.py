#!/usr/bin/env python3
"""What categorical features (categorical_feature of ptranking_amd/gbdt.py) cost, and that they cost nothing where they are off.

    python profiles/prof_gbdt_cat.py --scan [LIB] > S.json        one fresh process: the split scan alone, on the library LIB
    python profiles/prof_gbdt_cat.py --fit > F.json               one fresh process: time per tree of a whole fit
    python profiles/prof_gbdt_cat.py profiles/mi355x_gbdt_cat.json --parent P1.json P2.json ... --head H1.json H2.json ... --fit F.json

1. The split scan alone.  F = 136, 255 bins, 31 leaves, histograms of 2 000 000 synthetic rows: ptr_gbdt_best_split (the numeric scan, the
   symbol both libraries export) and, where the library has it, ptr_gbdt_best_split_cat with 0, 8 and 136 categorical features.  HIP events
   around REPEATS calls, the median of ROUNDS such figures.  --parent takes the outputs of --scan on the parent commit's library, --head
   those of this one, run in alternating fresh processes; the parent's spread between its processes stands beside the difference.
2. Time per tree of a whole fit.  MSLR-shaped data (200 000 documents, F = 136, max_bin 255, num_leaves 255, min_data_in_leaf 50); 8 columns
   hold one of 64 codes, with relevance planted on a scattered set of each.  One tree with those columns categorical against one tree with
   them as numbers, both policies, the two boosters alternating inside a round, all rounds kept.  The trees differ (a set split is another
   split), so the splits and the host reads of each stand beside its time.
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

LEAVES, FEATURES, MAX_BIN, ROWS = 31, 136, 255, 2_000_000
REPEATS, ROUNDS = 20, 7
DOCUMENTS, CODES, CAT_COLUMNS = 200_000, 64, tuple(range(3, 136, 17))
PARAMS = {"num_leaves": 255, "max_bin": 255, "min_data_in_leaf": 50, "learning_rate": 0.05, "min_sum_hessian_in_leaf": 1e-3}


def scan(lib_path):
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "prof_gbdt_cat.py measures on the GPU only"
    lib = C.CDLL(lib_path)
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    lib.ptr_gbdt_best_split.argtypes = [vp, i, i, i, vp, vp, d, C.c_int64, d, d, vp, vp, vp]
    has_cat = hasattr(lib, "ptr_gbdt_best_split_cat")
    if has_cat:
        lib.ptr_gbdt_best_split_cat.argtypes = [vp, i, i, i, vp, vp, vp, vp, d, C.c_int64, d, d, d, vp, vp, vp, vp]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    # every leaf a share of the rows; per feature the rows spread over its bins: every feature of a leaf holds the leaf's totals
    hist = np.zeros((LEAVES, FEATURES, MAX_BIN, 3), np.int64)
    share = rng.multinomial(ROWS, rng.dirichlet(np.ones(LEAVES)))
    for leaf in range(LEAVES):
        for f in range(FEATURES):
            c = rng.multinomial(share[leaf], rng.dirichlet(np.ones(MAX_BIN)))
            hist[leaf, f, :, 2] = c
            hist[leaf, f, :, 1] = c << 10
            hist[leaf, f, :, 0] = (rng.standard_normal(MAX_BIN) * np.sqrt(c) * 512).astype(np.int64)
        hist[leaf, :, 0, 0] -= hist[leaf, :, :, 0].sum(axis=1) - hist[leaf, 0, :, 0].sum()
    hist_d = torch.from_numpy(hist).to(dev)
    nbins = torch.full((FEATURES,), MAX_BIN, device=dev, dtype=torch.int32)
    expo = torch.tensor([10, 10], device=dev, dtype=torch.int32)
    ws = torch.empty((LEAVES * FEATURES, 13), device=dev, dtype=torch.int64)
    rec = torch.empty((LEAVES, 9), device=dev, dtype=torch.int64)
    sets = torch.empty((LEAVES, 4), device=dev, dtype=torch.int64)
    masks = {}
    for k in (0, 8, 136):
        m = np.zeros(FEATURES, np.uint8)
        m[np.linspace(0, FEATURES - 1, k).astype(int) if k else []] = 1
        masks[k] = torch.from_numpy(m).to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    tail = (d(0.0), C.c_int64(20), d(1e-3), d(0.0))

    def numeric():
        assert lib.ptr_gbdt_best_split(p(hist_d), LEAVES, FEATURES, MAX_BIN, p(nbins), p(expo), *tail, p(ws), p(rec), None) == 0

    def cat(k):
        assert lib.ptr_gbdt_best_split_cat(p(hist_d), LEAVES, FEATURES, MAX_BIN, p(nbins), None, p(masks[k]), p(expo), *tail, d(10.0), p(ws), p(rec), p(sets),
                                           None) == 0

    calls = {"numeric": numeric}
    if has_cat:
        calls.update({f"cat_{k}_of_136": (lambda k=k: cat(k)) for k in masks})
    out = {k: [] for k in calls}
    for name, fn in calls.items():
        fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPEATS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / REPEATS)
    print(json.dumps(dict(library=os.path.basename(lib_path), leaves=LEAVES, features=FEATURES, max_bin=MAX_BIN, repeats=REPEATS,
                          median_us={k: statistics.median(v) for k, v in out.items()}, all_us=out)))


def fit():
    import numpy as np
    import torch
    import prof_tree
    import ptranking_amd as pa
    from bench import MSLR_P
    from ptranking_amd import tree

    assert torch.cuda.is_available(), "prof_gbdt_cat.py measures on the GPU only"
    dev = torch.device("cuda:0")
    _, _, group = prof_tree.draw()
    group = group[:int(np.searchsorted(np.cumsum(group), DOCUMENTS))]
    n = int(group.sum())
    gen = torch.Generator(device=dev).manual_seed(137)
    X = torch.randn((n, FEATURES), device=dev, generator=gen)
    w = torch.randn(FEATURES, device=dev, generator=gen) / FEATURES ** 0.5
    w[list(CAT_COLUMNS)] = 0.0
    s = X @ w + 0.8 * X[:, 0] * X[:, 1] + 0.5 * torch.randn(n, device=dev, generator=gen)
    for f in CAT_COLUMNS:
        X[:, f] = torch.randint(0, CODES, (n,), device=dev, generator=gen).float()
        planted = torch.randperm(CODES, device=dev, generator=gen)[:CODES // 4].float()
        s = s + 0.4 * torch.isin(X[:, f], planted).float()
    cuts = torch.quantile(s, torch.tensor(np.cumsum(MSLR_P)[:-1] / np.sum(MSLR_P), device=dev, dtype=torch.float32))
    y = torch.bucketize(s, cuts).float().cpu().numpy()
    res = tree._Resident(y, group, dev)
    out = {}
    for policy in ("leafwise", "depthwise"):
        p = dict(PARAMS, grow_policy=policy)
        boosters = {"categorical": pa.GBDT(dict(p, categorical_feature=list(CAT_COLUMNS)), X), "numeric": pa.GBDT(p, X)}
        lm = pa.LambdaMART(p)
        g, h = lm.grad_hess(boosters["numeric"].scores, res)

        def grow(b):
            b.scores.zero_()
            b.trees.clear()
            reads = b.host_reads
            torch.cuda.synchronize()
            t = time.perf_counter()
            first = b.update(g, h)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3, first, b.host_reads - reads

        for b in boosters.values():
            grow(b)
        walls = {k: [] for k in boosters}
        for r in range(ROUNDS):
            for k, b in boosters.items():
                ms, first, reads = grow(b)
                walls[k].append(ms)
                out.setdefault(policy, {})[k] = dict(splits=int(first["feature"].size), host_reads=reads)
                if k == "categorical":
                    out[policy][k]["set_splits"] = int((first["cat_index"] >= 0).sum())
        for k in boosters:
            out[policy][k].update(one_tree_wall_ms=statistics.median(walls[k]), all_rounds_wall_ms=walls[k])
        out[policy]["categorical_over_numeric"] = out[policy]["categorical"]["one_tree_wall_ms"] / out[policy]["numeric"]["one_tree_wall_ms"]
    print(json.dumps(dict(documents=n, features=FEATURES, categorical_columns=list(CAT_COLUMNS), codes=CODES, params=PARAMS, rounds=ROUNDS, policies=out)))


def load(path):
    with open(path) as f:
        return json.loads(f.read().strip().splitlines()[-1])


def main(argv):
    out_path = argv[0]
    lists, key = {"--parent": [], "--head": [], "--fit": []}, None
    for a in argv[1:]:
        if a in lists:
            key = a
        elif key:
            lists[key].append(a)
    parent, head = [load(p) for p in lists["--parent"]], [load(p) for p in lists["--head"]]
    pn, hn = [r["median_us"]["numeric"] for r in parent], [r["median_us"]["numeric"] for r in head]
    scan_out = dict(note="fresh processes alternating parent, head, parent, head, ...; each figure is one process's median of "
                         f"{ROUNDS} timings of {REPEATS} calls, in microseconds per call", leaves=LEAVES, features=FEATURES, max_bin=MAX_BIN,
                    numeric_scan=dict(parent=pn, head=hn, parent_median=statistics.median(pn), head_median=statistics.median(hn),
                                      head_minus_parent=statistics.median(hn) - statistics.median(pn), parent_spread=max(pn) - min(pn)),
                    head={k: dict(processes=[r["median_us"][k] for r in head], median=statistics.median([r["median_us"][k] for r in head]))
                          for k in head[0]["median_us"] if k != "numeric"})
    result = dict(split_scan=scan_out, whole_fit=load(lists["--fit"][0]))
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--scan":
        scan(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "ptranking_amd", "libptranking_amd.so"))
    elif len(sys.argv) > 1 and sys.argv[1] == "--fit":
        fit()
    else:
        main(sys.argv[1:])
