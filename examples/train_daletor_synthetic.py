#!/usr/bin/env python3
"""Train DALETOR (search-result diversification) on synthetic subtopic data and print alpha-nDCG@{5,10,20}.

    python examples/train_daletor_synthetic.py [--queries 400] [--epochs 20] [--device cuda:0]

The TREC Web-track diversity data the reference's DIVDataset parses is not needed: every query here is generated — a query vector, 10..80
documents whose first features carry noisy subtopic relevance, and a subtopic-by-document relevance matrix presorted so that the documents
covering most subtopics come first (the reference's `presort`).  The queries are packed once into padded device batches (DivQueryBatches);
every train step is one scorer forward, ONE fused alpha-DCG loss launch for the whole batch, the scorer backward and the optimiser step, and
every evaluation pass is one metric launch per batch — where the reference runs one query per step and sorts every prediction on the CPU.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ptranking_amd as pa  # noqa: E402


def synthetic_queries(n_queries, n_features=16, seed=137):
    rng = np.random.default_rng(seed)
    out = []
    for qid in range(n_queries):
        n, T = int(rng.integers(10, 81)), int(rng.integers(2, 9))
        rele = (rng.random((T, n)) < 0.15).astype(np.float32)
        rele = np.ascontiguousarray(rele[:, np.argsort(-rele.sum(axis=0), kind="stable")])
        docs = (0.5 * rng.standard_normal((n, n_features))).astype(np.float32)
        docs[:, :T] += rele.T
        q_repr = rng.standard_normal((1, n_features)).astype(np.float32)
        out.append((q_repr, docs, rele))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=400)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    torch.manual_seed(137)
    data = synthetic_queries(args.queries)
    split = int(0.8 * len(data))
    train = pa.DivQueryBatches(data[:split], args.device, rough_batch_size=2048, shuffle=True)
    test = pa.DivQueryBatches(data[split:], args.device)
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 2e-3,
          "pointsf": dict(num_features=16, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False,
                          dropout=0.1)}
    ranker = pa.DALETOR(sf_para_dict=sf, model_para_dict={"rt": 10.0, "top_k": 10}, gpu=True, device=args.device)
    ranker.init()
    ks = [5, 10, 20]
    print("before training: alpha-nDCG@%s = %s" % (ks, ranker.alpha_ndcg_at_ks(test, ks=ks).numpy().round(4)))
    for epoch in range(1, args.epochs + 1):
        loss, stop = ranker.div_train(train, epoch_k=epoch)
        if stop:
            break
        if epoch % 5 == 0 or epoch == args.epochs:
            print(f"epoch {epoch:3d}  loss {loss.item():+.4f}  vali alpha-nDCG@10 {ranker.div_validation(test, 'aNDCG', k=10).item():.4f}")
    andcg, err_ia, nerr_ia = ranker.srd_performance_at_ks(test, ks=ks, max_label=1.0)
    for k, a, e, n in zip(ks, andcg.tolist(), err_ia.tolist(), nerr_ia.tolist()):
        print(f"alpha-nDCG@{k} {a:.4f}   ERR-IA@{k} {e:.4f}   nERR-IA@{k} {n:.4f}")


if __name__ == "__main__":
    main()
