"""IRGAN's point and pair machines on synthetic presorted queries with a planted linear signal: a few mini-max rounds each, nDCG@5 of the
generator and of the discriminator per round.

    python examples/train_irgan_synthetic.py [--queries 256] [--epochs 10] [--machine both|point|pair] [--loss-type svm|log]

Every query's documents are sorted by label (train_presort), which IRGAN needs: the relevant documents sit at the front of a list.  The
players are the fused point scorers; sampling and both players' losses run in the kernels of csrc/irgan.hip, one launch per batch.
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptranking_amd as pa                                   # noqa: E402
from ptranking_amd.adversarial import DEFAULT_AD_PARAS, ndcg_at_5   # noqa: E402


def synthetic_queries(num_queries, num_features, seed, min_docs=12, max_docs=60):
    """(qid, features [n, F], labels [n]) with labels 0..4 cut from a noisy linear score."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(num_features)
    for q in range(num_queries):
        n = int(rng.integers(min_docs, max_docs + 1))
        X = rng.standard_normal((n, num_features)).astype(np.float32)
        s = X @ w + 0.3 * rng.standard_normal(n)
        y = np.clip(np.floor((s - s.mean()) / (s.std() + 1e-9) + 0.5), 0, 4).astype(np.float32)
        yield q, X, y


def build_machine(name, num_features, device, loss_type="svm", lr=1e-2, **ad_paras):
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": lr,
          "pointsf": dict(num_features=num_features, num_layers=3, AF="R", TL_AF="S", apply_tl_af=True, BN=False, bn_type=None, bn_affine=False)}
    ad = dict(copy.deepcopy(DEFAULT_AD_PARAS[name]), **ad_paras)
    if name == "IRGAN_Pair":
        ad["loss_type"] = loss_type
    machine = getattr(pa, name)(eval_dict=None, data_dict=dict(train_presort=True), sf_para_dict=sf, ad_para_dict=ad, gpu=True, device=device)
    machine.reset_generator_discriminator()
    return machine


def run(machine, data, epochs, log=print, name=""):
    buffer = {}
    machine.fill_global_buffer(data, dict_buffer=buffer)
    g, d = machine.get_generator(), machine.get_discriminator()
    history = [(ndcg_at_5(g, data), ndcg_at_5(d, data))]
    log(f"{name} epoch 0: G nDCG@5 {history[0][0]:.4f}  D nDCG@5 {history[0][1]:.4f}")
    for epoch in range(1, epochs + 1):
        stop = machine.mini_max_train(train_data=data, generator=g, discriminator=d, global_buffer=buffer)
        history.append((ndcg_at_5(g, data), ndcg_at_5(d, data)))
        log(f"{name} epoch {epoch}: G nDCG@5 {history[-1][0]:.4f}  D nDCG@5 {history[-1][1]:.4f}")
        if stop:
            log(f"{name}: training stopped (NaN)")
            break
    return history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--features", type=int, default=24)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--machine", choices=("both", "point", "pair"), default="both")
    ap.add_argument("--loss-type", choices=("svm", "log"), default="svm")
    ap.add_argument("--rough-batch-size", type=int, default=1024)
    args = ap.parse_args()
    device = "cuda:0"
    torch.manual_seed(137)
    data = pa.PaddedQueryBatches(synthetic_queries(args.queries, args.features, seed=7), device, rough_batch_size=args.rough_batch_size, presort=True)
    for key, name in (("point", "IRGAN_Point"), ("pair", "IRGAN_Pair")):
        if args.machine in ("both", key):
            run(build_machine(name, args.features, device, loss_type=args.loss_type), data, args.epochs, name=name)


if __name__ == "__main__":
    main()
