"""LambdaMART with quantized gradients: low-bit integer gradients, the packed histogram kernel, leaves renewed from the full-precision sums.

    python examples/train_lambdamart_quantized.py                                # synthetic data, 4 levels, leaves renewed
    python examples/train_lambdamart_quantized.py --bins 16 --no-renew           # 16 levels, leaf values from the low-bit sums
    python examples/train_lambdamart_quantized.py --deterministic                # rint in place of stochastic rounding
    python examples/train_lambdamart_quantized.py train.txt [vali.txt] [test.txt]   # LETOR text files

Trains the same model twice, with use_quantized_grad off and on, and prints both validation curves side by side: the quantized fit rounds
every gradient to num_grad_quant_bins integer levels (stochastically, so that the expectation is kept), builds its histograms in one 64-bit
LDS word per (feature, bin), and, under quant_train_renew_leaf, takes the leaf values from the 30-bit sums.  The names are LightGBM's; the
rules are this project's own (ptranking_amd/gbdt.py).  No LightGBM comparison: the library is not installed where this project is tested.
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
    ap.add_argument("--bins", type=int, default=4, help="num_grad_quant_bins: a power of two in 2 .. 256")
    ap.add_argument("--deterministic", action="store_true", help="stochastic_rounding=False")
    ap.add_argument("--no-renew", action="store_true", help="quant_train_renew_leaf=False")
    ap.add_argument("--quant-seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--num-leaves", type=int, default=31)
    ap.add_argument("--learning-rate", type=float, default=0.1)
    ap.add_argument("--grow-policy", default="leafwise", choices=["leafwise", "depthwise"])
    ap.add_argument("--queries", type=int, default=600)
    ap.add_argument("--features", type=int, default=40)
    args = ap.parse_args()
    if args.files:
        train = from_file(args.files[0])
        valid = from_file(args.files[1]) if len(args.files) > 1 else train
        test = from_file(args.files[2]) if len(args.files) > 2 else valid
    else:
        train, valid, test = (synthetic(q, args.features, seed) for q, seed in ((args.queries, 7), (args.queries // 4, 8), (args.queries // 4, 9)))
    base = {"num_leaves": args.num_leaves, "learning_rate": args.learning_rate, "num_trees": args.rounds, "grow_policy": args.grow_policy}
    quant = {"use_quantized_grad": True, "num_grad_quant_bins": args.bins, "stochastic_rounding": not args.deterministic,
             "quant_train_renew_leaf": not args.no_renew, "quant_seed": args.quant_seed}
    print(f"{train[0].shape[0]} training documents in {train[2].size} queries, {train[0].shape[1]} features; objective {args.objective}")
    print(f"quantized: {args.bins} levels, {'rint' if args.deterministic else 'stochastic rounding'}, leaves {'from the low-bit sums' if args.no_renew else 'renewed'}")
    models = {name: pa.LambdaMART(dict(base, **extra), objective=args.objective).fit(*train, eval_set=valid[:2], eval_group=valid[2], eval_at=5)
              for name, extra in (("full precision", {}), ("quantized", quant))}
    for it in range(10, args.rounds + 1, 10):
        print(f"round {it}: valid nDCG@5 " + ", ".join(f"{name} {m.evals_result[it - 1]:.4f}" for name, m in models.items()))
    yt = torch.from_numpy(test[1]).cuda()
    for name, m in models.items():
        print(f"{name}: test nDCG@5 {pa.LambdaMART.ndcg_at(m.predict(test[0]), yt, test[2], 5):.4f} with {len(m.booster.trees)} trees, "
              f"{m.booster.host_reads} host reads")


if __name__ == "__main__":
    main()
