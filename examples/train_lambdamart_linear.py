"""LambdaMART with linear trees: every leaf carries a linear model over the features on its path.

    python examples/train_lambdamart_linear.py                                   # synthetic data
    python examples/train_lambdamart_linear.py --linear-lambda 1.0 --num-leaves 8
    python examples/train_lambdamart_linear.py train.txt [vali.txt] [test.txt]   # LETOR text files

Trains the same model twice, with linear_tree off and on, and prints both validation curves side by side.  The leaf fits run on the fp64
matrix instruction (ptr_gbdt_linear_moments, ptr_gbdt_linear_solve) and cost one more host read per tree.  The names are LightGBM's; the
rule is this project's own (ptranking_amd/gbdt.py).  No LightGBM comparison: the library is not installed where this project is tested.
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
    ap.add_argument("--linear-lambda", type=float, default=0.0)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--num-leaves", type=int, default=15)
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
    print(f"{train[0].shape[0]} training documents in {train[2].size} queries, {train[0].shape[1]} features; objective {args.objective}")
    models = {name: pa.LambdaMART(dict(base, **extra), objective=args.objective).fit(*train, eval_set=valid[:2], eval_group=valid[2], eval_at=5)
              for name, extra in (("constant", {}), ("linear", {"linear_tree": True, "linear_lambda": args.linear_lambda}))}
    for it in range(10, args.rounds + 1, 10):
        print(f"round {it}: valid nDCG@5 " + ", ".join(f"{name} {m.evals_result[it - 1]:.4f}" for name, m in models.items()))
    yt = torch.from_numpy(test[1]).cuda()
    for name, m in models.items():
        fitted = sum(int((t["leaf_features"][:, 0] >= 0).sum()) for t in m.booster.trees) if name == "linear" else 0
        print(f"{name}: test nDCG@5 {pa.LambdaMART.ndcg_at(m.predict(test[0]), yt, test[2], 5):.4f} with {len(m.booster.trees)} trees, "
              f"{m.booster.host_reads} host reads, {fitted} linear leaves")


if __name__ == "__main__":
    main()
