#!/usr/bin/env python3
"""Train a pointwise scorer with MDPRank whose rankings are sampled on the device, four per query and step, on synthetic graded data.

    python examples/train_mdprank_device.py [--distribution PL|STPL] [--samples 4] [--temperature 1.0] [--queries 512] [--steps 30] [--device cuda:0]

Each query has 20..120 documents with graded labels 0..4 and features that carry the label with noise; the documents are presorted by label
(the reference's `presort`).  One step is one scorer forward, ONE fused launch that draws the rankings from the Plackett-Luce model of the
scores and evaluates the return-weighted ListMLE of each (ptr_mdprank_sample_fwd_bwd), the scorer backward and the optimiser step — where
ptranking/ltr_adhoc/listwise/mdprank.py draws one ranking per query with torch.multinomial (or torch.rand and torch.sort), one query per step.
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
    ap.add_argument("--distribution", default="PL", choices=["PL", "STPL"])
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    torch.manual_seed(137)
    X, Y, lens = (t.to(args.device) for t in synthetic_batch(args.queries))
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 2e-3,
          "pointsf": dict(num_features=16, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False,
                          dropout=0.0)}
    paras = dict(pa.DEFAULT_PARAS["MDPRank"], distribution=args.distribution, temperature=args.temperature, sampler="device",
                 samples_per_query=args.samples)
    ranker = pa.MDPRank(sf_para_dict=sf, model_para_dict=paras, gpu=True, device=args.device)
    ranker.init()
    ks = [1, 5, 10]

    def report(tag):
        ranker.eval_mode()
        with torch.no_grad():
            out = F.metrics_at_ks(ranker.predict(X), Y, ks, presort=True, max_label=4.0, lens=lens, which=("ndcg",))
        ranker.train_mode()
        print(f"{tag}   ndcg@{ks} {out['ndcg'].mean(0).cpu().numpy().round(4)}")

    report("before")
    ranker.train_mode()
    for step in range(1, args.steps + 1):
        loss, stop = ranker.train_op(X, Y, epoch_k=step, presort=True, label_type=pa.LABEL_TYPE.MultiLabel, lens=lens)
        if stop:
            break
        if step % 10 == 0 or step == args.steps:
            print(f"step {step:3d}  MDPRank loss per query {loss.item() / args.queries:.4f}  ({args.samples} sampled rankings each)")
    report("after ")


if __name__ == "__main__":
    main()
