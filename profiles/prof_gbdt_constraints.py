#!/usr/bin/env python3
"""What monotone and interaction constraints (monotone_constraints, interaction_constraints of ptranking_amd/gbdt.py) cost, and that they
cost nothing where they are off.  The protocol of prof_gbdt_cat.py: fresh processes alternating parent and head, each figure one
process's median of ROUNDS timings of REPEATS calls.

    python profiles/prof_gbdt_constraints.py --scan [LIB] > S.json      one fresh process: the split scan alone, on the library LIB
    python profiles/prof_gbdt_constraints.py --fit [ROOT] > F.json      one fresh process: time per tree, with the package under ROOT
    python profiles/prof_gbdt_constraints.py profiles/mi355x_gbdt_constraints.json --parent-scan P.json ... --head-scan H.json ...
                                                                           --parent-fit P.json ... --head-fit H.json ...

1. The split scan alone.  F = 136, 255 bins, 31 leaves: ptr_gbdt_best_split (the unconstrained scan, the symbol both libraries export) and,
   where the library has it, ptr_gbdt_best_split_cst with monotone constraints on 8 of the 136 features (finite bounds on every second
   leaf), with two interaction groups (the halves of the features, the leaves alternating between them), and with both.
2. Time per tree of a whole fit.  MSLR-shaped data (200 000 documents, F = 136, max_bin 255, num_leaves 255, min_data_in_leaf 50), both
   policies: the unconstrained fit (parent and head) and, on the head, the fit with 8 constrained columns and two interaction groups.  The
   trees differ, so the splits and the host reads of each stand beside its time.
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

LEAVES, FEATURES, MAX_BIN = 31, 136, 255
REPEATS, ROUNDS = 20, 7
DOCUMENTS, MONO_COLUMNS = 200_000, tuple(range(3, 136, 17))
GROUPS = (tuple(range(0, 68)), tuple(range(68, 136)))
PARAMS = {"num_leaves": 255, "max_bin": 255, "min_data_in_leaf": 50, "learning_rate": 0.05, "min_sum_hessian_in_leaf": 1e-3}


def scan(lib_path):
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "prof_gbdt_constraints.py measures on the GPU only"
    lib = C.CDLL(lib_path)
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    lib.ptr_gbdt_best_split.argtypes = [vp, i, i, i, vp, vp, d, C.c_int64, d, d, vp, vp, vp]
    has_cst = hasattr(lib, "ptr_gbdt_best_split_cst")
    if has_cst:
        lib.ptr_gbdt_best_split_cst.argtypes = [vp, i, i, i, vp, vp, vp, vp, d, C.c_int64, d, d, d, vp, vp, vp, vp, vp, vp, vp]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    count = rng.integers(20, 600, (LEAVES, MAX_BIN)).astype(np.int64)
    one = np.stack([(rng.standard_normal(count.shape) * np.sqrt(count) * 512).astype(np.int64), count << 10, count], axis=2)
    # every feature of a leaf holds the leaf's totals: the same bins in another order
    hist = np.stack([one[:, rng.permutation(MAX_BIN)] for _ in range(FEATURES)], axis=1)
    hist_d = torch.from_numpy(hist).to(dev)
    nbins = torch.full((FEATURES,), MAX_BIN, device=dev, dtype=torch.int32)
    expo = torch.tensor([10, 10], device=dev, dtype=torch.int32)
    ws = torch.empty((LEAVES * FEATURES, 13), device=dev, dtype=torch.int64)
    rec = torch.empty((LEAVES, 9), device=dev, dtype=torch.int64)
    mono = np.zeros(FEATURES, np.int8)
    mono[list(MONO_COLUMNS)] = [1, -1] * (len(MONO_COLUMNS) // 2)
    v = -hist[:, 0, :, 0].sum(axis=1) / hist[:, 0, :, 1].sum(axis=1)
    cst = np.stack([np.where(np.arange(LEAVES) % 2, v - 0.01, -np.inf), np.where(np.arange(LEAVES) % 2, v + 0.01, np.inf), v], axis=1)
    allowed = np.zeros((LEAVES, FEATURES), np.uint8)
    for leaf in range(LEAVES):
        allowed[leaf, list(GROUPS[leaf % 2])] = 1
    mono_d, cst_d, allowed_d = torch.from_numpy(mono).to(dev), torch.from_numpy(cst).to(dev), torch.from_numpy(allowed).to(dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    tail = (d(0.0), C.c_int64(20), d(1e-3), d(0.0))

    def unconstrained():
        assert lib.ptr_gbdt_best_split(p(hist_d), LEAVES, FEATURES, MAX_BIN, p(nbins), p(expo), *tail, p(ws), p(rec), None) == 0

    def constrained(c, a):
        assert lib.ptr_gbdt_best_split_cst(p(hist_d), LEAVES, FEATURES, MAX_BIN, p(nbins), None, None, p(expo), *tail, d(10.0), p(ws), p(rec), None,
                                           p(mono_d), p(c), p(a), None) == 0

    calls = {"unconstrained": unconstrained}
    if has_cst:
        calls.update(monotone_8_of_136=lambda: constrained(cst_d, None), interaction_2_groups=lambda: constrained(None, allowed_d),
                     both=lambda: constrained(cst_d, allowed_d))
    out = {k: [] for k in calls}
    for fn in calls.values():
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
    print(json.dumps(dict(library=lib_path, leaves=LEAVES, features=FEATURES, max_bin=MAX_BIN, repeats=REPEATS,
                          median_us={k: statistics.median(v) for k, v in out.items()}, all_us=out)))


def fit(root):
    sys.path.insert(0, root)
    sys.path.insert(1, os.path.join(root, "profiles"))
    import numpy as np
    import torch
    import prof_tree
    import ptranking_amd as pa
    from bench import MSLR_P
    from ptranking_amd import tree

    assert torch.cuda.is_available(), "prof_gbdt_constraints.py measures on the GPU only"
    assert os.path.abspath(os.path.dirname(os.path.dirname(pa.__file__))) == os.path.abspath(root)
    dev = torch.device("cuda:0")
    _, _, group = prof_tree.draw()
    group = group[:int(np.searchsorted(np.cumsum(group), DOCUMENTS))]
    n = int(group.sum())
    gen = torch.Generator(device=dev).manual_seed(137)
    X = torch.randn((n, FEATURES), device=dev, generator=gen)
    w = torch.randn(FEATURES, device=dev, generator=gen) / FEATURES ** 0.5
    s = X @ w + 0.8 * X[:, 0] * X[:, 1] + 0.6 * torch.sin(3.0 * X[:, list(MONO_COLUMNS)]).sum(dim=1) + 0.5 * torch.randn(n, device=dev, generator=gen)
    cuts = torch.quantile(s, torch.tensor(np.cumsum(MSLR_P)[:-1] / np.sum(MSLR_P), device=dev, dtype=torch.float32))
    y = torch.bucketize(s, cuts).float().cpu().numpy()
    res = tree._Resident(y, group, dev)
    has_cst = "monotone_constraints" in pa.gbdt.DEFAULT_PARAMS
    mono = [0] * FEATURES
    for k, c in enumerate(MONO_COLUMNS):
        mono[c] = 1 if float(w[c]) >= 0 else -1
    out = {}
    for policy in ("leafwise", "depthwise"):
        p = dict(PARAMS, grow_policy=policy)
        boosters = {"unconstrained": pa.GBDT(p, X)}
        if has_cst:
            boosters["constrained"] = pa.GBDT(dict(p, monotone_constraints=mono, interaction_constraints=[list(g) for g in GROUPS]), X)
        lm = pa.LambdaMART(p)
        g, h = lm.grad_hess(boosters["unconstrained"].scores, res)

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
        for k in boosters:
            out[policy][k].update(one_tree_wall_ms=statistics.median(walls[k]), all_rounds_wall_ms=walls[k])
        if has_cst:
            out[policy]["constrained_over_unconstrained"] = out[policy]["constrained"]["one_tree_wall_ms"] / out[policy]["unconstrained"]["one_tree_wall_ms"]
    print(json.dumps(dict(package=root, documents=n, features=FEATURES, monotone_columns=list(MONO_COLUMNS), groups=[[g[0], g[-1]] for g in GROUPS],
                          params=PARAMS, rounds=ROUNDS, policies=out)))


def load(path):
    with open(path) as f:
        return json.loads(f.read().strip().splitlines()[-1])


def compare(parent, head):
    return dict(parent=parent, head=head, parent_median=statistics.median(parent), head_median=statistics.median(head),
                head_minus_parent=statistics.median(head) - statistics.median(parent), parent_spread=max(parent) - min(parent),
                head_inside_parent_spread=min(parent) <= statistics.median(head) <= max(parent))


def main(argv):
    out_path = argv[0]
    lists, key = {"--parent-scan": [], "--head-scan": [], "--parent-fit": [], "--head-fit": []}, None
    for a in argv[1:]:
        if a in lists:
            key = a
        elif key:
            lists[key].append(a)
    ps, hs, pf, hf = ([load(p) for p in lists[k]] for k in ("--parent-scan", "--head-scan", "--parent-fit", "--head-fit"))
    med = lambda runs, k: [r["median_us"][k] for r in runs]
    base = statistics.median(med(hs, "unconstrained"))
    scan_out = dict(note="fresh processes alternating parent, head, parent, head, ...; each figure is one process's median of "
                         f"{ROUNDS} timings of {REPEATS} calls, in microseconds per call", leaves=LEAVES, features=FEATURES, max_bin=MAX_BIN,
                    unconstrained_scan=compare(med(ps, "unconstrained"), med(hs, "unconstrained")),
                    head={k: dict(processes=med(hs, k), median=statistics.median(med(hs, k)), over_unconstrained=statistics.median(med(hs, k)) / base)
                          for k in hs[0]["median_us"] if k != "unconstrained"})
    fit_out = dict(note="one tree of the whole fit, wall milliseconds; each figure is one process's median of its rounds", documents=hf[0]["documents"],
                   params=PARAMS, monotone_columns=list(MONO_COLUMNS), groups=hf[0]["groups"])
    for policy in ("leafwise", "depthwise"):
        tree_ms = lambda runs, k: [r["policies"][policy][k]["one_tree_wall_ms"] for r in runs]
        fit_out[policy] = dict(unconstrained=compare(tree_ms(pf, "unconstrained"), tree_ms(hf, "unconstrained")),
                               constrained=dict(processes=tree_ms(hf, "constrained"), median=statistics.median(tree_ms(hf, "constrained")),
                                                over_unconstrained=[r["policies"][policy]["constrained_over_unconstrained"] for r in hf]),
                               shapes={k: {q: hf[0]["policies"][policy][k][q] for q in ("splits", "host_reads")} for k in ("unconstrained", "constrained")})
    with open(out_path, "w") as f:
        json.dump(dict(split_scan=scan_out, whole_fit=fit_out), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--scan":
        scan(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "ptranking_amd", "libptranking_amd.so"))
    elif len(sys.argv) > 1 and sys.argv[1] == "--fit":
        fit(os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ROOT)
    else:
        main(sys.argv[1:])
