#!/usr/bin/env python3
"""Times the truncated, normalised lambdarank (csrc/tree.hip tree_lambdarank_ndcg_kernel) on the MSLR-shaped ragged batch of
profiles/prof_tree.py (its draw(): 19 000 queries, four lists of 1 251 documents planted) against the all-pairs Delta-nDCG kernel that was
the booster's only lambdarank before it ('lambdarank' / 'DeltaNDCG' / 'sum': the lambdamart_sum row of profiles/mi355x_tree_objectives.json).

    python profiles/prof_lambdarank_ndcg.py profiles/mi355x_lambdarank_ndcg.json

Kernel time alone, from device events around the launches of one objective call (one launch per length class, as TreeObjective and
LambdaMART issue them; scores, labels and offsets resident): medians of ROUNDS rounds, the variants alternating inside a round, every round
kept.  Per variant the pairs it evaluates on this draw are counted on the host from the rule: `walked` is the ordered partner visits of
the kernel's loops (the thread of a document ranked in the first T walks its whole list, any other the first min(T, n) ranks; the all-pairs
kernel walks n per document), `counted` the unordered pairs that pass the rule (labels differ, and for the new objective the better-ranked
document is in the first T).  pairs/s is `walked` per kernel second.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from prof_tree import draw  # noqa: E402

ROUNDS = 7
VARIANTS = {"lambdarank_ndcg_T30": dict(objective="lambdarank_ndcg", truncation_level=30, norm=True),
            "lambdarank_ndcg_T1251": dict(objective="lambdarank_ndcg", truncation_level=1251, norm=True),
            "lambdamart_sum": dict(objective="lambdarank", weighting="DeltaNDCG", hessian="sum")}


def pair_counts(preds, labels, group, T):
    """(walked, counted) for truncation level T (None: the all-pairs kernel), summed over the draw."""
    import numpy as np
    walked = counted = 0
    a = 0
    for n in group.astype(np.int64):
        s, y = preds[a:a + n], labels[a:a + n]
        a += n
        differ = lambda v: (v.size * v.size - int((np.bincount(v.astype(np.int64), minlength=5) ** 2).sum())) // 2
        if T is None:
            walked += int(n * n)
            counted += differ(y)
            continue
        order = np.lexsort((np.arange(n), -s.astype(np.float64)))
        tn = min(T, int(n))
        walked += int(tn * n + (n - tn) * tn)
        counted += differ(y) - differ(y[order[tn:]])
    return walked, counted


def main(out_path):
    import numpy as np
    import torch
    import ptranking_amd as pa
    import ptranking_amd.functional as F

    assert torch.cuda.is_available(), "prof_lambdarank_ndcg.py measures on the GPU only"
    dev = torch.device("cuda:0")
    preds, labels, group = draw()
    objs = {k: pa.TreeObjective(labels, group, **kw) for k, kw in VARIANTS.items()}
    p = torch.from_numpy(preds).to(dev)
    out = (torch.empty_like(p), torch.empty_like(p))

    def launches(obj):
        res = obj._own
        for max_len, queries in res.buckets:
            if obj.kind == "pair":
                F.tree_pair_grad_hess(p, res.labels, res.offsets, obj.pair_type, obj.weighting, obj.epsilon, obj.hessian, queries, max_len, out)
            else:
                F.tree_lambdarank_ndcg_grad_hess(p, res.labels, res.offsets, obj.truncation_level, obj.sigmoid, obj.norm, queries, max_len, out)

    def kernel_ms(obj):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launches(obj)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # same results first: at T >= the longest list, without norm, the new kernel is the all-pairs Delta-nDCG kernel up to fp32 rounding
    full = pa.TreeObjective(labels, group, "lambdarank_ndcg", truncation_level=1251, norm=False)
    launches(full)
    mine = torch.stack(out).clone()
    launches(objs["lambdamart_sum"])
    theirs = torch.stack(out)
    agree = float(((mine - theirs).abs().amax(1) / theirs.abs().amax(1)).max())
    assert agree <= 1e-4, agree

    for obj in objs.values():                                   # warm up every shape of the timed window
        kernel_ms(obj); kernel_ms(obj)
    rounds = {k: [] for k in objs}
    for _ in range(ROUNDS):
        for k, obj in objs.items():
            rounds[k].append(kernel_ms(obj))
    rows = {}
    for k, r in rounds.items():
        T = VARIANTS[k].get("truncation_level")
        walked, counted = pair_counts(preds, labels, group, T)
        med = statistics.median(r)
        rows[k] = dict(config=VARIANTS[k], median_kernel_ms=med, all_rounds_kernel_ms=r, walked_ordered_pairs=walked, counted_unordered_pairs=counted,
                       walked_pairs_per_s=walked / (med * 1e-3))
        print(json.dumps({"variant": k, "median_kernel_ms": med, "walked": walked, "counted": counted, "pairs_per_s": rows[k]["walked_pairs_per_s"]}), flush=True)
    base = rows["lambdamart_sum"]["median_kernel_ms"]
    scenario = dict(queries=int(group.size), documents=int(group.sum()), longest=int(group.max()), mean_len=float(group.mean()),
                    lengths="profiles/prof_tree.py draw(): Gamma(2.2), mean 120, clipped to [1, 1251], four lists of 1251 planted", labels="bench.MSLR_P",
                    length_classes=[(m, len(i)) for m, i in objs["lambdamart_sum"]._own.buckets_host], rounds=ROUNDS,
                    timing="device events around the launches of one objective call; inputs resident; variants alternate inside a round")
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, scenario=scenario, variants=rows,
                       speedup_vs_all_pairs={k: base / v["median_kernel_ms"] for k, v in rows.items()},
                       max_rel_diff_full_truncation_vs_all_pairs=agree), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_lambdarank_ndcg.json"))
