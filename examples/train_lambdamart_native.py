"""LambdaMART trained end to end on the GPU: the tree frame's objectives (csrc/tree.hip) under the native histogram booster (csrc/gbdt.hip).

    python examples/train_lambdamart_native.py                                   # synthetic data
    python examples/train_lambdamart_native.py train.txt [vali.txt] [test.txt]   # LETOR text files
    python examples/train_lambdamart_native.py --grow-policy depthwise           # level by level, in batched passes
    python examples/train_lambdamart_native.py --bagging-fraction 0.5 --bagging-freq 1 --by-query   # every tree on a fresh half of the queries
    python examples/train_lambdamart_native.py --goss                            # gradient-based one-side sampling (top 0.2, other 0.1)
    python examples/train_lambdamart_native.py --objective lambdarank_ndcg       # the truncated, normalised lambdarank (level 30)
    python examples/train_lambdamart_native.py --objective rank_xendcg           # cross-entropy nDCG: O(n) per query
    python examples/train_lambdamart_native.py --categorical 3,7                 # the columns 3 and 7 hold codes: set splits
    python examples/train_lambdamart_native.py --monotone 0:1,5:-1               # scores non-decreasing in column 0, non-increasing in 5
    python examples/train_lambdamart_native.py --interaction "0,1;2,3"           # a path uses the columns of one group only (the rest: one more group)

The synthetic relevance is planted: a linear part plus a feature interaction a linear scorer cannot express, graded with MSLR-WEB30K's label
mix; a column named by --categorical holds one of 23 codes, and membership in a scattered set of 5 of them lifts the relevance, which a
node that cuts codes into "low" and "high" needs many splits to isolate.  Prints the validation nDCG@5 every 10 rounds.  No LightGBM comparison: the library is not installed where this project is tested.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptranking_amd as pa   # noqa: E402
from ptranking_amd import letor   # noqa: E402

MSLR_P = (0.5147, 0.3250, 0.1339, 0.0183, 0.0081)      # MSLR-WEB30K's grade frequencies, 0 .. 4


CODES, PLANTED = 23, (1, 4, 7, 13, 20)


def synthetic(queries, features, seed, categorical=()):
    rng = np.random.default_rng(seed)
    group = rng.integers(20, 120, queries)
    n = int(group.sum())
    X = rng.standard_normal((n, features)).astype(np.float32)
    w = np.random.default_rng(1).standard_normal(features) / np.sqrt(features)
    w[list(categorical)] = 0.0
    s = X @ w + 0.8 * X[:, 0] * X[:, 1] + 0.5 * rng.standard_normal(n)
    for f in categorical:
        X[:, f] = rng.integers(0, CODES, n)
        s = s + 0.9 * np.isin(X[:, f], PLANTED)
    y = np.digitize(s, np.quantile(s, np.cumsum(MSLR_P)[:-1])).astype(np.float32)
    return X, y, group


def from_file(path):
    qs = letor.load_letor_queries(path)
    return np.concatenate([x for _, x, _ in qs]), np.concatenate([lab for _, _, lab in qs]), np.array([lab.size for _, _, lab in qs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*", help="train.txt [vali.txt] [test.txt]")
    ap.add_argument("--objective", default="lambdarank", choices=list(pa.tree.OBJECTIVES),
                    help="lambdarank_ndcg: the truncated, normalised lambdarank; rank_xendcg: cross-entropy nDCG (this project's rules, modelled "
                         "on LightGBM's two built-in ranking objectives)")
    ap.add_argument("--truncation-level", type=int, default=30, help="lambdarank_truncation_level (lambdarank_ndcg only)")
    ap.add_argument("--no-norm", action="store_true", help="lambdarank_norm=False (lambdarank_ndcg only)")
    ap.add_argument("--sigmoid", type=float, default=1.0, help="the sigmoid's steepness (lambdarank_ndcg only)")
    ap.add_argument("--objective-seed", type=int, default=5, help="the seed of the uniforms rank_xendcg draws every round (rank_xendcg only)")
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--num-leaves", type=int, default=31)
    ap.add_argument("--learning-rate", type=float, default=0.1)
    ap.add_argument("--min-data-in-leaf", type=int, default=20)
    ap.add_argument("--grow-policy", default="leafwise", choices=["leafwise", "depthwise"],
                    help="depthwise: all leaves of a level are split in one batched pass (one host read per level, not per split)")
    ap.add_argument("--bagging-fraction", type=float, default=1.0, help="the share of rows (of queries with --by-query) a tree is grown on")
    ap.add_argument("--bagging-freq", type=int, default=0, help="redraw the bag every k trees; 0: no bagging")
    ap.add_argument("--by-query", action="store_true", help="bagging samples whole queries")
    ap.add_argument("--goss", action="store_true", help="data_sample_strategy='goss' in place of bagging")
    ap.add_argument("--categorical", default="", help="0-based columns that hold integer codes, as in 3,7 (categorical_feature)")
    ap.add_argument("--monotone", default="", help="column:sign pairs, as in 0:1,5:-1 (monotone_constraints; the other columns get 0)")
    ap.add_argument("--interaction", default="", help="groups of columns, as in 0,1;2,3 (interaction_constraints)")
    ap.add_argument("--queries", type=int, default=600)
    ap.add_argument("--features", type=int, default=40)
    args = ap.parse_args()
    cats = tuple(int(c) for c in args.categorical.split(",") if c.strip())
    if args.files:
        train = from_file(args.files[0])
        valid = from_file(args.files[1]) if len(args.files) > 1 else train
        test = from_file(args.files[2]) if len(args.files) > 2 else valid
    else:
        train, valid, test = (synthetic(q, args.features, seed, cats) for q, seed in ((args.queries, 7), (args.queries // 4, 8), (args.queries // 4, 9)))
    params = {"num_leaves": args.num_leaves, "learning_rate": args.learning_rate, "min_data_in_leaf": args.min_data_in_leaf, "num_trees": args.rounds,
              "grow_policy": args.grow_policy, "bagging_fraction": args.bagging_fraction, "bagging_freq": args.bagging_freq,
              "bagging_by_query": args.by_query, "data_sample_strategy": "goss" if args.goss else "bagging",
              "lambdarank_truncation_level": args.truncation_level, "lambdarank_norm": not args.no_norm, "sigmoid": args.sigmoid,
              "objective_seed": args.objective_seed,
              "categorical_feature": cats}
    if args.monotone:
        mono = [0] * train[0].shape[1]
        for pair in args.monotone.split(","):
            col, sign = pair.split(":")
            mono[int(col)] = int(sign)
        params["monotone_constraints"] = mono
    if args.interaction:
        params["interaction_constraints"] = [[int(c) for c in g.split(",") if c.strip()] for g in args.interaction.split(";") if g.strip()]
    lm = pa.LambdaMART(params, objective=args.objective)
    if pa.gbdt.constraints(lm.params):
        print(f"constraints: {', '.join(pa.gbdt.constraints(lm.params))} (monotone on the columns "
              f"{[c for c, m in enumerate(lm.params['monotone_constraints']) if m]}, groups {[list(g) for g in lm.params['interaction_constraints']]})")
    how = {None: "none", "goss": f"goss (top_rate {lm.params['top_rate']}, other_rate {lm.params['other_rate']})",
           "bagging": f"bagging {args.bagging_fraction} {'by query' if args.by_query else 'by row'}, redrawn every {args.bagging_freq} trees"}
    print(f"sampling: {how[pa.gbdt.sampling(lm.params)]}")
    yv = torch.from_numpy(valid[1]).cuda()
    constant = pa.LambdaMART.ndcg_at(torch.zeros(valid[0].shape[0], device="cuda"), yv, valid[2], 5)
    print(f"{train[0].shape[0]} training documents in {train[2].size} queries, {train[0].shape[1]} features; constant scores: valid nDCG@5 {constant:.4f}")
    lm.fit(*train, eval_set=valid[:2], eval_group=valid[2], eval_at=5)
    for it, score in enumerate(lm.evals_result, 1):
        if it % 10 == 0:
            print(f"round {it}: valid nDCG@5 {score:.4f}")
    yt = torch.from_numpy(test[1]).cuda()
    if cats:
        nodes = sum(int((t["cat_index"] >= 0).sum()) for t in lm.booster.trees)
        print(f"categorical columns {list(cats)}: {nodes} of {sum(t['feature'].size for t in lm.booster.trees)} nodes split on a set of codes")
    print(f"test nDCG@5 {pa.LambdaMART.ndcg_at(lm.predict(test[0]), yt, test[2], 5):.4f} with {len(lm.booster.trees)} trees")


if __name__ == "__main__":
    main()
