"""LambdaMART with DART boosting: every round drops a set of earlier trees, fits the new tree on what is left and puts them back rescaled.

    python examples/train_lambdamart_dart.py                                     # synthetic data, drop_rate 0.1, skip_drop 0.5
    python examples/train_lambdamart_dart.py --drop-rate 0.3 --skip-drop 0       # drop more, in every round
    python examples/train_lambdamart_dart.py --uniform-drop --xgboost-dart-mode
    python examples/train_lambdamart_dart.py train.txt [vali.txt] [test.txt]     # LETOR text files

Trains the same model twice, with boosting='gbdt' and boosting='dart', and prints both validation curves side by side.  The dropped trees
leave and re-enter the resident training and validation scores in one kernel launch per direction (ptr_gbdt_dart_walk).  The names are
LightGBM's; the rule is this project's own (ptranking_amd/gbdt.py).  There is no early stopping under 'dart': later rounds rewrite earlier
trees.  No LightGBM comparison: the library is not installed where this project is tested.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptranking_amd as pa   # noqa: E402
from train_lambdamart_native import from_file, synthetic   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*", help="train.txt [vali.txt] [test.txt]")
    ap.add_argument("--objective", default="lambdarank_ndcg", choices=list(pa.tree.OBJECTIVES))
    ap.add_argument("--drop-rate", type=float, default=0.1)
    ap.add_argument("--max-drop", type=int, default=50)
    ap.add_argument("--skip-drop", type=float, default=0.5)
    ap.add_argument("--uniform-drop", action="store_true")
    ap.add_argument("--xgboost-dart-mode", action="store_true")
    ap.add_argument("--drop-seed", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--num-leaves", type=int, default=31)
    ap.add_argument("--learning-rate", type=float, default=0.1)
    ap.add_argument("--queries", type=int, default=600)
    ap.add_argument("--features", type=int, default=40)
    args = ap.parse_args()
    if args.files:
        train = from_file(args.files[0])
        valid = from_file(args.files[1]) if len(args.files) > 1 else train
        test = from_file(args.files[2]) if len(args.files) > 2 else valid
    else:
        train, valid, test = (synthetic(q, args.features, seed) for q, seed in ((args.queries, 7), (args.queries // 4, 8), (args.queries // 4, 9)))
    base = {"num_leaves": args.num_leaves, "learning_rate": args.learning_rate, "num_trees": args.rounds}
    dart = {"drop_rate": args.drop_rate, "max_drop": args.max_drop, "skip_drop": args.skip_drop,
            "uniform_drop": args.uniform_drop, "xgboost_dart_mode": args.xgboost_dart_mode, "drop_seed": args.drop_seed}
    print(f"{train[0].shape[0]} training documents in {train[2].size} queries, {train[0].shape[1]} features; objective {args.objective}")
    models = {name: pa.LambdaMART(dict(base, **extra), objective=args.objective, boosting=name).fit(*train, eval_set=valid[:2], eval_group=valid[2], eval_at=5)
              for name, extra in (("gbdt", {}), ("dart", dart))}
    for it in range(10, args.rounds + 1, 10):
        print(f"round {it}: valid nDCG@5 " + ", ".join(f"{name} {m.evals_result[it - 1]:.4f}" for name, m in models.items()))
    yt = torch.from_numpy(test[1]).cuda()
    for name, m in models.items():
        print(f"{name}: test nDCG@5 {pa.LambdaMART.ndcg_at(m.predict(test[0]), yt, test[2], 5):.4f} with {len(m.booster.trees)} trees, "
              f"{m.booster.host_reads} host reads; the last round dropped {len(m.booster.last_drop)} trees")


if __name__ == "__main__":
    main()
