#!/usr/bin/env python3
"""Train DivProbRanker (search-result diversification with a mean and a variance per document) on synthetic subtopic data and print
alpha-nDCG@{5,10,20}.

    python examples/train_divprob_synthetic.py [--opt-id SuperSoft|PairCLS|LambdaPairCLS] [--metric aNDCG|nERR-IA] [--K 1]
                                               [--sort-id ExpRele|RiskAware|RERAR] [--queries 400] [--epochs 20] [--device cuda:0]

The data is generated as in examples/train_daletor_synthetic.py: a query vector, 10..80 documents whose first features carry noisy subtopic
relevance, and a subtopic-by-document relevance matrix presorted so that the documents covering most subtopics come first (the reference's
`presort`).  The queries are packed once into padded device batches (DivQueryBatches); every train step is one scorer forward (two outputs
per document, or 3 K for a mixture), ONE fused launch for the loss and both gradients of the whole batch (ptr_divprob_fwd_bwd), the scorer
backward and the optimiser step — where the reference runs one query per step and builds [1, L, L] and [T, L, L] tensors for each.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ptranking_amd as pa  # noqa: E402
from train_daletor_synthetic import synthetic_queries  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--opt-id", default="SuperSoft", choices=["SuperSoft", "PairCLS", "LambdaPairCLS"])
    ap.add_argument("--metric", default="aNDCG", choices=["aNDCG", "nERR-IA"])
    ap.add_argument("--K", type=int, default=1)
    ap.add_argument("--sort-id", default="ExpRele", choices=["ExpRele", "RiskAware", "RERAR"])
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
    paras = dict(pa.diversity.DEFAULT_DIV_PARAS["DivProbRanker"], opt_id=args.opt_id, metric=args.metric, K=args.K, sort_id=args.sort_id,
                 top_k=10, limit_delta=0.1)        # the reference's grid: top_k = 10, limit_delta in {None, 0.1} (div_prob_ranker.py:448-456)
    ranker = pa.DivProbRanker(sf_para_dict=sf, model_para_dict=paras, gpu=True, device=args.device)
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
