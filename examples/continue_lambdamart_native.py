"""Yesterday's model on today's data: continue, refit and embed a native LambdaMART (csrc/gbdt.hip; GBDT.fit_bins(init_model=...),
GBDT.refit, predict(pred_leaf=True)).

    python examples/continue_lambdamart_native.py                      # synthetic data
    python examples/continue_lambdamart_native.py --rounds 40 --more 20 --decay 0.8

Trains a ranker on one set of synthetic queries, saves it, loads the file and
  1. continues it on the same queries (init_model): the result is, bit for bit, the model trained in one go;
  2. continues it on FRESH queries, whose relevance has drifted: more trees on new data under the old bins;
  3. refits it on the fresh queries: the same tree structures, every leaf value re-estimated and blended with the old one by --decay;
  4. reads the leaf every tree puts a document in (pred_leaf): the usual GBDT-to-embedding features of a neural ranker.
Prints nDCG@5 on held-out fresh queries for each.  No LightGBM comparison: the library is not installed where this project is tested.
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptranking_amd as pa   # noqa: E402

MSLR_P = (0.5147, 0.3250, 0.1339, 0.0183, 0.0081)      # MSLR-WEB30K's grade frequencies, 0 .. 4


def synthetic(queries, features, seed, drift=0.0):
    """Relevance planted on the columns 0, 1 and 2; `drift` moves weight from column 2 to column 3."""
    rng = np.random.default_rng(seed)
    group = rng.integers(20, 120, queries)
    n = int(group.sum())
    X = rng.standard_normal((n, features)).astype(np.float32)
    s = 1.2 * (1.0 - drift) * X[:, 2] + 1.2 * drift * X[:, 3] + 1.0 * X[:, 0] * X[:, 1] + 0.4 * rng.standard_normal(n)
    y = np.digitize(s, np.quantile(s, np.cumsum(MSLR_P)[:-1])).astype(np.float32)
    return X, y, group


def ndcg(ranker, X, y, group):
    labels = torch.from_numpy(y).to(ranker.device)
    return pa.LambdaMART.ndcg_at(ranker.predict(X), labels, group, k=5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20, help="trees of the first model")
    ap.add_argument("--more", type=int, default=10, help="trees added by the continuation")
    ap.add_argument("--decay", type=float, default=0.9, help="refit: the weight of the old leaf value")
    ap.add_argument("--num-leaves", type=int, default=15)
    ap.add_argument("--queries", type=int, default=300)
    ap.add_argument("--features", type=int, default=20)
    args = ap.parse_args()
    params = {"num_leaves": args.num_leaves, "min_data_in_leaf": 20, "learning_rate": 0.1}
    X, y, group = synthetic(args.queries, args.features, 7)
    Xn, yn, gn = synthetic(args.queries, args.features, 8, drift=0.6)      # today's queries
    Xt, yt, gt = synthetic(args.queries // 2, args.features, 9, drift=0.6)  # held out, drifted as well

    first = pa.LambdaMART(params).fit(X, y, group, num_boost_round=args.rounds)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "yesterday.npz")
        first.booster.save_model(path)
        same = pa.LambdaMART(params).fit(X, y, group, num_boost_round=args.more, init_model=path)
        whole = pa.LambdaMART(params).fit(X, y, group, num_boost_round=args.rounds + args.more)
        identical = all(np.array_equal(a[k], b[k]) for a, b in zip(same.booster.trees, whole.booster.trees) for k in a)
        print(f"{args.rounds} trees, saved, loaded, {args.more} more on the same queries: {len(same.booster.trees)} trees, "
              f"{'identical to' if identical else 'DIFFERENT from'} {args.rounds + args.more} trees trained in one go")
        continued = pa.LambdaMART(params).fit(Xn, yn, gn, num_boost_round=args.more, init_model=path)
    refitted = first.refit(Xn, yn, gn, decay_rate=args.decay)
    print(f"nDCG@5 on held-out drifted queries: yesterday's model {ndcg(first, Xt, yt, gt):.4f}, "
          f"+{args.more} trees on today's queries {ndcg(continued, Xt, yt, gt):.4f}, "
          f"refit on today's queries (decay {args.decay}) {ndcg(refitted, Xt, yt, gt):.4f}")
    moved = sum(int((a["value"] != b["value"]).sum()) for a, b in zip(refitted.booster.trees, first.booster.trees))
    print(f"refit kept {len(refitted.booster.trees)} tree structures and moved {moved} leaf values in {refitted.booster.host_reads - first.booster.host_reads} host reads")
    leaves = continued.predict(Xt[:5], pred_leaf=True)                    # device int32 [5, trees]
    print(f"pred_leaf: {tuple(leaves.shape)} leaf indices; document 0 lands in the leaves {leaves[0, :8].tolist()} ... of the first trees")


if __name__ == "__main__":
    main()
