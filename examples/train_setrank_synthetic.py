#!/usr/bin/env python3
"""Train the SetRank ranker — a listwise scorer whose encoder layers are induced multi-head self-attention blocks — on synthetic graded data,
and print the hard metrics.

    python examples/train_setrank_synthetic.py [--n-induce 32] [--layers 2] [--heads 2] [--queries 256] [--steps 30] [--device cuda:0]

Each query has 20..120 documents (padded to 128) with graded labels 0..4 and features that carry the label with noise.  Every encoder layer
is two rectangular attentions through `n_induce` learned inducing points (ptr_xattn_forward / ptr_xattn_backward: O(L n_induce) per query
and head, nothing of size [L, L] or [L, n_induce] reaches HBM); the loss is ListNet's softmax cross-entropy.  The rule is this project's own,
modelled on SetRank (Pang et al. 2020) and the Set Transformer (Lee et al. 2019); no parity with the authors' code is claimed.
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
    ap.add_argument("--n-induce", type=int, default=32)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    torch.manual_seed(137)
    X, Y, lens = (t.to(args.device) for t in synthetic_batch(args.queries))
    sf = {"sf_id": "listsf", "opt": "Adam", "lr": 2e-3,
          "listsf": dict(num_features=16, ff_dims=[32, 32], n_heads=args.heads, n_induce=args.n_induce, encoder_layers=args.layers, dropout=0.0,
                         AF="R", TL_AF="GE", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False)}
    ranker = pa.SetRank(sf_para_dict=sf, gpu=True, device=args.device)
    ranker.init()
    ks = [1, 5, 10]

    def report(tag):
        ranker.eval_mode()
        ranker._batch_lens = lens
        with torch.no_grad():
            out = F.metrics_at_ks(ranker.predict(X), Y, ks, presort=True, max_label=4.0, lens=lens)
        ranker._batch_lens = None
        ranker.train_mode()
        print(tag + "   " + "   ".join(f"{m}@{ks} {out[m].mean(0).cpu().numpy().round(4)}" for m in ("p", "ap", "nerr", "ndcg")))

    report("before")
    ranker.train_mode()
    for step in range(1, args.steps + 1):
        loss, stop = ranker.train_op(X, Y, epoch_k=step, presort=True, label_type=pa.LABEL_TYPE.MultiLabel, lens=lens)
        if stop:
            break
        if step % 10 == 0 or step == args.steps:
            print(f"step {step:3d}  softmax cross-entropy per query {loss.item() / args.queries:.4f}")
    report("after ")


if __name__ == "__main__":
    main()
