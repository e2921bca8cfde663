#!/usr/bin/env python3
"""Train a variance-aware pointwise scorer directly on a ranking metric — AP@10 by default — through Gaussian expected ranks, on synthetic
graded data, and print the hard metrics.

    python examples/train_prob_smooth_metric.py [--metric P|AP|nERR|nDCG] [--top-k 10] [--resort] [--head sigmoid|exp|const]
                                                [--sort-id ExpRele|RiskAware|RERAR] [--queries 512] [--steps 30] [--device cuda:0]

Each query has 20..120 documents with graded labels 0..4 and features that carry the label with noise; the documents are presorted by label
(the reference's `presort`).  The scorer predicts a mean and a variance per document (--head sigmoid: variance = sigmoid * limit_delta;
exp; const: a mean alone and the standard deviation 0.5 for every document, SoftRank's rank model).  One step is one scorer forward, ONE
fused launch for the loss and both gradients (ptr_gaussmetric_fwd_bwd: the expected ranks 1 + sum_j erfc(x_ij) / 2, then minus the metric
on them), the scorer backward and the optimiser step — where prob_utils.get_expected_rank and metric_as_opt_objective.py build [B, L, L]
tensors, sort, gather and scan per step.  --resort weighs the documents by their current expected rank instead of their ideal position
(opt_ideal=False); --sort-id chooses the scores predict() ranks by.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ptranking_amd as pa  # noqa: E402
import ptranking_amd.functional as F  # noqa: E402


def synthetic_batch(nq, L=128, nf=16, seed=137):
    """(X [nq, L, nf], labels [nq, L] presorted, lens int32 [nq]) on the CPU."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, L - 7, size=nq).astype(np.int32)
    Y = rng.choice(5, size=(nq, L), p=[0.5, 0.3, 0.13, 0.05, 0.02]).astype(np.float32)
    for q in range(nq):
        Y[q, lens[q]:] = -1.0
        Y[q, 0] = max(Y[q, 0], 1.0)
    Y = -np.sort(-Y, axis=1)
    Y[Y < 0] = 0.0
    X = rng.standard_normal((nq, L, nf)).astype(np.float32)
    X[:, :, :4] += 0.5 * Y[:, :, None]
    for q in range(nq):
        X[q, lens[q]:] = 0.0
    return torch.from_numpy(X), torch.from_numpy(Y), torch.from_numpy(lens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--metric", default="AP", choices=["P", "AP", "nERR", "nDCG"])
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--resort", action="store_true")
    ap.add_argument("--head", default="sigmoid", choices=["sigmoid", "exp", "const"])
    ap.add_argument("--sort-id", default="ExpRele", choices=["ExpRele", "RiskAware", "RERAR"])
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    torch.manual_seed(137)
    X, Y, lens = (t.to(args.device) for t in synthetic_batch(args.queries))
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 2e-3,
          "pointsf": dict(num_features=16, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False,
                          dropout=0.0)}
    head = {"sigmoid": dict(limit_delta=0.01), "exp": dict(limit_delta=None), "const": dict(const_std=0.5)}[args.head]
    paras = dict(pa.DEFAULT_PARAS["ProbSmoothMetric"], metric=args.metric, top_k=args.top_k or None, opt_ideal=not args.resort, max_label=4.0,
                 sort_id=args.sort_id, **head)
    ranker = pa.ProbSmoothMetric(sf_para_dict=sf, model_para_dict=paras, gpu=True, device=args.device)
    ranker.init()
    ks = [1, 5, 10]

    def report(tag):
        ranker.eval_mode()
        with torch.no_grad():
            out = F.metrics_at_ks(ranker.predict(X, lens=lens).contiguous(), Y, ks, presort=True, max_label=4.0, lens=lens)
        ranker.train_mode()
        print(tag + "   " + "   ".join(f"{m}@{ks} {out[m].mean(0).cpu().numpy().round(4)}" for m in ("p", "ap", "nerr", "ndcg")))

    report("before")
    ranker.train_mode()
    for step in range(1, args.steps + 1):
        loss, stop = ranker.train_op(X, Y, epoch_k=step, presort=True, label_type=pa.LABEL_TYPE.MultiLabel, lens=lens)
        if stop:
            break
        if step % 10 == 0 or step == args.steps:
            print(f"step {step:3d}  expected-rank {args.metric}@{args.top_k or 'all'} per query {-loss.item() / args.queries:.4f}")
    report("after ")


if __name__ == "__main__":
    main()
