#!/usr/bin/env python3
"""Train a pointwise scorer on FastSoftRank — soft nDCG (or Spearman) on soft ranks that are the projection of the scores onto the
permutahedron — on synthetic graded data, and print the hard metrics.

    python examples/train_fastsoftrank_synthetic.py [--eps 0.02] [--objective nDCG] [--queries 512] [--steps 30] [--device cuda:0]

One step is one scorer forward, ONE fused launch for the loss and its exact gradient (ptr_fastsoftrank_fwd_bwd: one sort, one isotonic
regression and one block-mean pass per query, O(L) state, lists of up to 4096 documents), the scorer backward and the optimiser step.
A useful eps is of the order of (score range) / (list length): far above it every document gets the mean rank and the gradient vanishes,
far below it the ranks are hard and the gradient vanishes as well.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ptranking_amd as pa  # noqa: E402
import ptranking_amd.functional as F  # noqa: E402
from train_neuralndcg_synthetic import synthetic_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eps", type=float, default=0.02)
    ap.add_argument("--objective", default="nDCG", choices=sorted(F.FASTSOFTRANK_OBJECTIVES))
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    torch.manual_seed(137)
    X, Y, lens = (t.to(args.device) for t in synthetic_batch(args.queries))
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 2e-3,
          "pointsf": dict(num_features=16, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False,
                          dropout=0.0)}
    ranker = pa.FastSoftRank(sf_para_dict=sf, model_para_dict=dict(eps=args.eps, objective=args.objective), gpu=True, device=args.device)
    ranker.init()
    ks = [1, 5, 10]

    def report(tag):
        ranker.eval_mode()
        with torch.no_grad():
            out = F.metrics_at_ks(ranker.predict(X), Y, ks, presort=True, max_label=4.0, lens=lens)
        ranker.train_mode()
        print(tag + "   " + f"ndcg@{ks} {out['ndcg'].mean(0).cpu().numpy().round(4)}")

    report("before")
    for step in range(1, args.steps + 1):
        loss, stop = ranker.train_op(X, Y, epoch_k=step, presort=True, label_type=pa.LABEL_TYPE.MultiLabel, lens=lens)
        if stop:
            break
        if step % 10 == 0 or step == args.steps:
            print(f"step {step:3d}  {args.objective} objective per query {loss.item() / args.queries:.4f}")
    report("after ")


if __name__ == "__main__":
    main()
