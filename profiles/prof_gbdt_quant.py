#!/usr/bin/env python3
"""Measures quantized-gradient training (use_quantized_grad of ptranking_amd/gbdt.py) on MSLR-shaped data.

    python profiles/prof_gbdt_quant.py profiles/mi355x_gbdt_quant.json

Data: the generator of prof_gbdt.py (prof_tree.draw()'s queries, N(0, 1) features, a planted relevance graded with bench.MSLR_P) at F = 136,
max_bin = 255, cut to DOCUMENTS documents so that a run fits a short GPU visit; the last fifth of the queries is held out.

  histogram   ptr_gbdt_histogram_packed against ptr_gbdt_histogram on the SAME low-bit (qg, qh), B in {4, 256}, over the root (every training
              row, no list) and a mid-sized sorted list (1 / 16 of them): device events, the two kernels alternating inside each of ROUNDS
              rounds, medians and all rounds kept; the outputs are compared bit for bit first
  fit         TREES trees of LambdaMART(objective='lambdarank_ndcg') under use_quantized_grad off / on / on with quant_train_renew_leaf: the
              three boosters take their rounds in turn, each update() timed with a host clock around a device synchronise; the median
              per tree, and nDCG@5 of the held-out queries after the last tree
No LightGBM figure stands beside these: the library is not installed on these machines.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

ROUNDS, TREES, DOCUMENTS, FEATURES = 7, 20, 1_000_000, 136
PARAMS = {"num_leaves": 255, "max_bin": 255, "min_data_in_leaf": 50, "learning_rate": 0.1, "min_sum_hessian_in_leaf": 1e-3}
SETTINGS = {"off": {}, "on": {"use_quantized_grad": True}, "on_renew": {"use_quantized_grad": True, "quant_train_renew_leaf": True}}


def main(out_path):
    import numpy as np
    import torch
    import prof_tree
    import ptranking_amd as pa
    import ptranking_amd.functional as F
    from bench import MSLR_P
    from ptranking_amd import tree

    assert torch.cuda.is_available(), "prof_gbdt_quant.py measures on the GPU only"
    dev = torch.device("cuda:0")
    _, _, group = prof_tree.draw()
    group = group[:int(np.searchsorted(np.cumsum(group), DOCUMENTS))]
    n, nf, mb = int(group.sum()), FEATURES, PARAMS["max_bin"]
    gen = torch.Generator(device=dev).manual_seed(137)
    X = torch.randn((n, nf), device=dev, generator=gen)
    w = torch.randn(nf, device=dev, generator=gen) / nf ** 0.5
    s = X @ w + 0.8 * X[:, 0] * X[:, 1] + 0.5 * torch.randn(n, device=dev, generator=gen)
    cuts = torch.quantile(s[:1_000_000], torch.tensor(np.cumsum(MSLR_P)[:-1] / np.sum(MSLR_P), device=dev, dtype=torch.float32))
    y = torch.bucketize(s, cuts).float()
    q_train = int(group.size * 0.8)
    n_train = int(group[:q_train].sum())
    Xt, yt, gt, Xh, yh, gh_ = X[:n_train], y[:n_train].cpu().numpy(), group[:q_train], X[n_train:], y[n_train:], group[q_train:]
    t0 = time.perf_counter()
    boosters = {k: pa.GBDT(dict(PARAMS, **extra)).fit_bins(Xt, group=gt) for k, extra in SETTINGS.items()}
    print(f"{n_train} training documents x {nf} features binned three times in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    lm = pa.LambdaMART(PARAMS, objective="lambdarank_ndcg")
    res = tree._Resident(yt, gt, dev)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # ---- the histogram kernels on the same low-bit arrays
    bins = boosters["off"].bins
    g, h = lm.grad_hess(boosters["off"].scores, res)
    perm = torch.randperm(n_train, device=dev, generator=gen).to(torch.int32)
    lists = {"root": None, "mid": torch.sort(perm[:n_train // 16])[0].contiguous()}
    hist = torch.zeros((nf, mb, 3), device=dev, dtype=torch.int64)
    kernels = {}
    for B in (4, 256):
        qg, qh, _, _ = F.gbdt_quantize_low(g, h, B, True, 0, 0)
        for name, rows in lists.items():
            forms = {"int64": {}, "packed": {"bounds": (B // 2, B)}}
            same = torch.equal(*(F.gbdt_histogram(bins, qg, qh, rows, nf, mb, **kw) for kw in forms.values()))
            ms = {k: [] for k in forms}
            for _ in range(ROUNDS + 1):                                # the first round warms both up and is dropped
                for k, kw in forms.items():
                    ms[k].append(events(lambda: F.gbdt_histogram(bins, qg, qh, rows, nf, mb, hist=hist, **kw)))
            med = {k: statistics.median(v[1:]) for k, v in ms.items()}
            kernels[f"B{B}_{name}"] = dict(rows=n_train if rows is None else rows.numel(), bit_equal=same, median_ms=med, all_rounds_ms={k: v[1:] for k, v in ms.items()},
                                           packed_over_int64=med["packed"] / med["int64"])
            print(f"B={B} {name}: {med} bit-equal {same}", file=sys.stderr, flush=True)

    # ---- whole fits, the three settings taking their rounds in turn
    gh = (torch.empty(n_train, device=dev), torch.empty(n_train, device=dev))
    tree_ms = {k: [] for k in SETTINGS}
    for t in range(TREES):
        for k, b in boosters.items():
            lm.grad_hess(b.scores, res, gh, draw=t)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.update(*gh)
            torch.cuda.synchronize()
            tree_ms[k].append((time.perf_counter() - t0) * 1e3)
    index = pa.LambdaMART.padded_index(gh_, dev)
    fits = {k: dict(median_tree_ms=statistics.median(v[1:]), all_trees_ms=v, host_reads=boosters[k].host_reads,
                    splits=int(sum(t["feature"].size for t in boosters[k].trees)),
                    heldout_ndcg5=pa.LambdaMART.ndcg_at(boosters[k].predict(Xh), yh, None, 5, index=index)) for k, v in tree_ms.items()}
    out = dict(documents=n_train, heldout_documents=n - n_train, features=nf, params=PARAMS, objective="lambdarank_ndcg", trees=TREES, rounds=ROUNDS,
               histogram_kernels=kernels, fits=fits,
               note="histogram: device events, the int64 and the packed kernel alternating on the same low-bit arrays; fits: wall per update() around a "
                    "device synchronise, the first tree dropped from the median; no LightGBM comparison exists")
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"histogram": {k: v["median_ms"] for k, v in kernels.items()}, "fits": {k: (v["median_tree_ms"], v["heldout_ndcg5"]) for k, v in fits.items()}}))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_gbdt_quant.json"))
