#!/usr/bin/env python3
"""Train a pointwise scorer with PL-Rank — the policy gradient of a Plackett-Luce ranking policy's expected nDCG@k — on synthetic graded data,
and print the hard metrics.

    python examples/train_plrank_synthetic.py [--samples 32] [--top-k 10] [--queries 512] [--steps 30] [--device cuda:0]

One step is one scorer forward, ONE fused launch that draws `samples` rankings per query and returns the sampled reward and the PL-Rank
gradient estimate (ptr_plrank_fwd_bwd: nothing of size [B, S, L] reaches HBM), the scorer backward and the optimiser step.
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
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    torch.manual_seed(137)
    X, Y, lens = (t.to(args.device) for t in synthetic_batch(args.queries))
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 2e-3,
          "pointsf": dict(num_features=16, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False,
                          dropout=0.0)}
    ranker = pa.PLRank(sf_para_dict=sf, model_para_dict=dict(samples=args.samples, top_k=args.top_k or None), gpu=True, device=args.device)
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
            print(f"step {step:3d}  sampled nDCG@{args.top_k or 'all'} per query {-loss.item() / args.queries:.4f}")
    report("after ")


if __name__ == "__main__":
    main()
