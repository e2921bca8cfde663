"""Why a document was scored as it was: TreeSHAP feature contributions of a native LambdaMART (csrc/gbdt.hip, ptr_gbdt_shap).

    python examples/explain_lambdamart_native.py                      # synthetic data
    python examples/explain_lambdamart_native.py --rounds 50 --top 8

The synthetic relevance is planted on the columns 0, 1 and 2 (a linear part on 2, an interaction of 0 and 1) out of --features columns of
noise.  The ranker is fitted, the training matrix becomes the background (the trees keep no row counts: set_background walks the matrix
through every tree once and counts the rows per leaf), and predict(pred_contrib=True) returns one contribution per feature and document
plus the expected value: each row sums to the document's score.  Prints the features by mean |contribution| beside their split counts,
and one document explained.  No LightGBM or shap comparison: neither is installed where this project is tested.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptranking_amd as pa   # noqa: E402

MSLR_P = (0.5147, 0.3250, 0.1339, 0.0183, 0.0081)      # MSLR-WEB30K's grade frequencies, 0 .. 4


def synthetic(queries, features, seed):
    rng = np.random.default_rng(seed)
    group = rng.integers(20, 120, queries)
    n = int(group.sum())
    X = rng.standard_normal((n, features)).astype(np.float32)
    s = 1.2 * X[:, 2] + 1.0 * X[:, 0] * X[:, 1] + 0.4 * rng.standard_normal(n)
    y = np.digitize(s, np.quantile(s, np.cumsum(MSLR_P)[:-1])).astype(np.float32)
    return X, y, group


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--num-leaves", type=int, default=15)
    ap.add_argument("--queries", type=int, default=300)
    ap.add_argument("--features", type=int, default=20)
    ap.add_argument("--top", type=int, default=5, help="how many features to print")
    args = ap.parse_args()
    X, y, group = synthetic(args.queries, args.features, 7)
    lm = pa.LambdaMART({"num_leaves": args.num_leaves, "num_trees": args.rounds, "min_data_in_leaf": 20, "learning_rate": 0.1})
    lm.fit(X, y, group)
    lm.set_background(X)                                                  # the covers: the training matrix gives the counts the trees were grown on
    phi = lm.predict(X, pred_contrib=True)                                # device float64 [n, F + 1]
    scores = lm.predict(X)
    gap = float((phi.sum(dim=1) - scores.double()).abs().max())
    print(f"{X.shape[0]} documents, {X.shape[1]} features, {len(lm.booster.trees)} trees; the contributions of a document sum to its score "
          f"(largest gap {gap:.2e}, the fp32 rounding of the score)")
    mean_abs = phi[:, :-1].abs().mean(dim=0).cpu().numpy()
    splits = lm.booster.feature_importance("split")
    print(f"expected value {float(phi[0, -1]):+.4f}; features by mean |contribution|:")
    for f in np.argsort(-mean_abs)[:args.top]:
        print(f"  feature {int(f):3d}: mean |phi| {mean_abs[f]:.4f}, {int(splits[f])} splits")
    doc = int(scores.argmax())
    row = phi[doc].cpu().numpy()
    order = np.argsort(-np.abs(row[:-1]))[:args.top]
    print(f"document {doc} (score {float(scores[doc]):+.4f}, label {int(y[doc])}): " +
          ", ".join(f"f{int(f)}={X[doc, f]:+.2f} -> {row[f]:+.4f}" for f in order))


if __name__ == "__main__":
    main()
