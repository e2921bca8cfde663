#!/usr/bin/env python3
"""Times the position-debiased lambdarank (csrc/tree.hip tree_lambdarank_ndcg_kernel<G, true> + tree_position_bias_update_kernel) against
the plain lambdarank_ndcg kernel of the same build, on the draw of profiles/prof_lambdarank_ndcg.py (prof_tree.draw(): 19 000 queries,
2.28 M documents), T = 30 with norm.

    python profiles/prof_lambdarank_unbiased.py profiles/mi355x_lambdarank_unbiased.json

Kernel time alone, from device events around the launches of one objective call (one launch per length class as TreeObjective and
LambdaMART issue them, and for the unbiased variant the update launch; inputs, biases and accumulator resident): medians of ROUNDS rounds,
the two variants alternating inside a round, every round kept.  The unbiased variant runs at the biases its own updates leave (they move
every round, as in a fit), positions = the index within the query, P = 30.
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
T, P, P_NORM = 30, 30, 0.5


def main(out_path):
    import torch
    import ptranking_amd as pa
    import ptranking_amd.functional as F
    from ptranking_amd.tree import PositionBias

    assert torch.cuda.is_available(), "prof_lambdarank_unbiased.py measures on the GPU only"
    dev = torch.device("cuda:0")
    preds, labels, group = draw()
    res = pa.TreeObjective(labels, group, "lambdarank_ndcg", truncation_level=T)._own
    p = torch.from_numpy(preds).to(dev)
    out = (torch.empty_like(p), torch.empty_like(p))
    bias = PositionBias(P, P_NORM, dev)

    def plain():
        for max_len, queries in res.buckets:
            F.tree_lambdarank_ndcg_grad_hess(p, res.labels, res.offsets, T, 1.0, True, queries, max_len, out)

    def unbiased():
        for max_len, queries in res.buckets:
            F.tree_lambdarank_unbiased_grad_hess(p, res.labels, res.offsets, bias.cost_acc, bias.biases, None, T, 1.0, True, queries, max_len, out)
        bias.update()

    def kernel_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # same results first: the first unbiased call runs at unit biases and must give the plain kernel's bits
    plain()
    want = torch.stack(out).clone()
    unbiased()
    assert torch.equal(torch.stack(out).view(torch.int32), want.view(torch.int32)), "unit biases must reproduce lambdarank_ndcg bit for bit"
    variants = {"lambdarank_ndcg": plain, "lambdarank_unbiased_with_update": unbiased}
    for fn in variants.values():                                # warm up every shape of the timed window
        kernel_ms(fn); kernel_ms(fn)
    rounds = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            rounds[k].append(kernel_ms(fn))
    rows = {k: dict(median_kernel_ms=statistics.median(r), all_rounds_kernel_ms=r) for k, r in rounds.items()}
    ratio = rows["lambdarank_unbiased_with_update"]["median_kernel_ms"] / rows["lambdarank_ndcg"]["median_kernel_ms"]
    for k, v in rows.items():
        print(json.dumps({"variant": k, "median_kernel_ms": v["median_kernel_ms"]}), flush=True)
    scenario = dict(queries=int(group.size), documents=int(group.sum()), longest=int(group.max()), truncation_level=T, norm=True, bias_positions=P,
                    bias_p_norm=P_NORM, length_classes=[(m, len(i)) for m, i in res.buckets_host], rounds=ROUNDS, library=os.environ.get("PTR_LIB", "the product build"),
                    timing="device events around the launches of one objective call; inputs resident; variants alternate inside a round")
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, scenario=scenario, variants=rows, unbiased_over_plain=ratio,
                       learned_t_plus=bias.biases[0].cpu().tolist()), f, indent=1)
        f.write("\n")
    print(f"unbiased / plain = {ratio:.3f}; wrote {out_path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_lambdarank_unbiased.json"))
