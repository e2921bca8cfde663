#!/usr/bin/env python3
"""The tree frame's custom objective on one MI355X: LETOR text file -> TreeObjective (gradient + Hessian per document, one fused kernel per
length class) -> a few Newton rounds of a trivial additive model -> nDCG@10 from the device evaluator.

    python examples/train_lambdamart_objective.py path/to/train.txt [--rounds 8] [--objective lambdarank] [--weighting DeltaNDCG]

What the reference does for the same job (ptranking/ltr_tree/util/lightgbm_util.py:120-302): a Python `for` loop over the document pairs
of every query, every boosting round.  LightGBM is not installed where this package is developed, so this example does NOT train trees
and nothing here has been run end to end with LightGBM.  The "model" is one free score per document, moved by
-learning_rate * grad / (hess + lambda) each round (a boosting round whose weak learner fits every document exactly), under
hessian='sum' — the Hessian LightGBM and XGBoost use, never negative; the reference's rank-signed one is not a curvature.  It shows the
objective's contract and that its gradients rank the training lists.  With LightGBM the same object plugs in as:

    obj = pa.TreeObjective(labels, group, "lambdarank", weighting="DeltaNDCG", hessian="sum")
    booster = lightgbm.train(params, lightgbm.Dataset(X, labels, group=group), fobj=obj.fobj)    # LightGBM >= 4: params["objective"] = obj.fobj
    ranker = lightgbm.LGBMRanker(objective=obj.sklearn).fit(X, labels, group=group)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout
import ptranking_amd as pa  # noqa: E402
from ptranking_amd.letor import parse_letor_file  # noqa: E402


class ScoreTable(pa.DeviceEvaluator):
    """One score per document behind the evaluator's ranker surface: a batch's "features" are the documents' flat indices."""

    def __init__(self, n_docs, device):
        self.device = device
        self.scores = torch.zeros(n_docs, device=device)

    def eval_mode(self):
        pass

    def predict(self, batch_q_doc_vectors):
        return self.scores[batch_q_doc_vectors[..., 0].long()]


def padded_batch(labels, group, device):
    """(ids, X, Y, lens) of batching.unpack_batch for the whole collection: X [B, L, 1] holds flat document indices."""
    B, L = len(group), int(group.max())
    off = np.concatenate([[0], np.cumsum(group)])
    X, Y = np.zeros((B, L, 1), np.float32), np.zeros((B, L), np.float32)
    for q in range(B):
        X[q, :group[q], 0] = np.arange(off[q], off[q + 1])
        Y[q, :group[q]] = labels[off[q]:off[q + 1]]
    to = lambda a: torch.from_numpy(a).to(device)
    return [(list(range(B)), to(X), to(Y), to(group.astype(np.int32)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("train")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--objective", default="lambdarank", choices=list(pa.tree.OBJECTIVES))
    ap.add_argument("--weighting", default="DeltaNDCG", choices=["none", "DeltaNDCG", "DeltaGain"])
    ap.add_argument("--learning-rate", type=float, default=0.5)
    ap.add_argument("--reg-lambda", type=float, default=1e-3, help="added to the Hessian, as LightGBM's lambda_l2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: ptranking_amd has no CPU fallback")
    dev = "cuda:0"

    _, labels, _, qoff = parse_letor_file(args.train)
    group = np.diff(qoff)
    assert len(labels) < 2 ** 24, "the score table is indexed through a float32 feature"
    if args.objective in ("lambdarank_ndcg", "rank_xendcg"):      # the weight and the Hessian are part of the rule: --weighting does not apply
        obj = pa.TreeObjective(labels, group, args.objective)
    else:
        obj = pa.TreeObjective(labels, group, args.objective, weighting=None if args.weighting == "none" else args.weighting, hessian="sum")
    table = ScoreTable(len(labels), dev)
    data = padded_batch(labels, group, dev)
    ndcg = lambda: float(table.ndcg_at_k(test_data=data, k=10, label_type=pa.LABEL_TYPE.MultiLabel)[0])
    print(f"{len(group)} queries, {len(labels)} documents, lists of {group.min()} .. {group.max()}; {len(obj._own.buckets)} length classes")
    print(f"round 0: nDCG@10 {ndcg():.4f}")
    scores = np.zeros(len(labels))
    for r in range(1, args.rounds + 1):
        t0 = time.perf_counter()
        grad, hess = obj(scores)                                  # float64 numpy arrays, as LightGBM expects them
        dt = time.perf_counter() - t0
        scores -= args.learning_rate * grad / (hess + args.reg_lambda)
        table.scores = torch.from_numpy(scores.astype(np.float32)).to(dev)
        print(f"round {r}: nDCG@10 {ndcg():.4f}  objective call {1e3 * dt:.2f} ms  |grad| {np.abs(grad).mean():.4f}  min hess {hess.min():.3e}")


if __name__ == "__main__":
    main()
