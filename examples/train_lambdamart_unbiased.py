"""Unbiased LambdaMART on synthetic click logs: LambdaMART(objective='lambdarank_ndcg') with lambdarank_unbiased against the same objective
without it, both trained on CLICKS and measured on the true grades.

The data: graded relevance from a noisy linear model; every query's documents are SHOWN in a noisy order (a production ranker of middling
quality); a click is drawn from the position-based model P(click) = examination[position] * attraction[grade], with a known examination
propensity 1 / (1 + position)^eta.  Training sees the clicks and the shown positions alone.

The script prints the learned t+[p] beside the true propensity ratios examination[p] / examination[0], and nDCG@5 on the true grades for
both models.  Whether debiasing wins on a draw is not measured anywhere in this project: the script prints, and asserts nothing about it.

    python examples/train_lambdamart_unbiased.py --queries 2000 --rounds 50
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def click_log(n_queries, eta, seed, features=10, lo=8, hi=30):
    rng = np.random.default_rng(seed)
    group = rng.integers(lo, hi + 1, n_queries)
    n = int(group.sum())
    X = rng.standard_normal((n, features)).astype(np.float32)
    z = X @ rng.standard_normal(features) / np.sqrt(features) + 0.4 * rng.standard_normal(n)
    grade = np.digitize(z, np.quantile(z, [0.55, 0.8, 0.92, 0.98])).astype(np.float32)
    attraction = 0.05 + 0.9 * (2.0 ** grade - 1.0) / 15.0                       # P(click | examined)
    position = np.empty(n, np.int64)
    for a, e in zip(np.cumsum(group) - group, np.cumsum(group)):                  # shown by a noisy view of the relevance
        order = np.argsort(-(z[a:e] + 1.0 * rng.standard_normal(e - a)))
        position[a + order] = np.arange(e - a)
    examination = 1.0 / (1.0 + position) ** eta
    clicks = (rng.random(n) < examination * attraction).astype(np.float32)
    return X, grade, clicks, position, group


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--eta", type=float, default=1.0, help="the examination propensity falls as 1 / (1 + position)^eta")
    ap.add_argument("--positions", type=int, default=10, help="lambdarank_bias_positions: position classes with a bias of their own")
    ap.add_argument("--p-norm", type=float, default=0.5, help="lambdarank_bias_p_norm")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    import ptranking_amd as pa

    X, grade, clicks, position, group = click_log(args.queries, args.eta, args.seed)
    Xt, grade_t, _, _, group_t = click_log(max(args.queries // 4, 50), args.eta, args.seed + 1)
    print(f"{args.queries} queries, {len(grade)} documents, {int(clicks.sum())} clicks; test: {len(group_t)} queries")
    params = {"num_trees": args.rounds, "num_leaves": 15, "min_data_in_leaf": 10, "learning_rate": 0.1, "lambdarank_truncation_level": 30}
    labels_t = torch.from_numpy(grade_t).cuda()
    for name, extra in (("plain   ", {}), ("unbiased", {"lambdarank_unbiased": True, "lambdarank_bias_positions": args.positions,
                                                        "lambdarank_bias_p_norm": args.p_norm})):
        lm = pa.LambdaMART(dict(params, **extra), objective="lambdarank_ndcg").fit(X, clicks, group, position=position)
        ndcg = pa.LambdaMART.ndcg_at(lm.predict(Xt), labels_t, group_t, 5)
        print(f"{name}: nDCG@5 on the true grades {ndcg:.4f}")
        if extra:
            t = lm.position_biases
            truth = 1.0 / (1.0 + np.arange(args.positions)) ** args.eta
            print("position   t+[p]    t-[p]    examination[p] / examination[0]")
            for p in range(args.positions):
                print(f"{p:8d}   {t[0, p]:.4f}   {t[1, p]:.4f}   {truth[p]:.4f}")


if __name__ == "__main__":
    main()
