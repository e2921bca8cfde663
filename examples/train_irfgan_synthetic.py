"""IRFGAN's point and pair machines on synthetic presorted queries with a planted linear signal: a few mini-max rounds each under one
f-divergence, nDCG@5 of the generator and of the discriminator per round.

    python examples/train_irfgan_synthetic.py [--queries 256] [--epochs 10] [--machine both|point|pair] [--f-div KL]

The data and the round loop are those of train_irgan_synthetic.py.  A round is one pass of train_discriminator_generator_single_step: per
batch one sampling launch (csrc/irfgan.hip: the pair machine's n x n Bernoulli mask is recomputed there and never stored), one step of the
discriminator, one of the generator.
"""
import argparse
import copy
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ptranking_amd as pa                                   # noqa: E402
from ptranking_amd.adversarial import DEFAULT_AD_PARAS       # noqa: E402
from ptranking_amd.functional import F_DIVERGENCES           # noqa: E402
from train_irgan_synthetic import run, synthetic_queries     # noqa: E402


def build_machine(name, num_features, device, f_div="KL", lr=1e-2, **ad_paras):
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": lr,
          "pointsf": dict(num_features=num_features, num_layers=3, AF="R", TL_AF="S", apply_tl_af=True, BN=False, bn_type=None, bn_affine=False)}
    ad = dict(copy.deepcopy(DEFAULT_AD_PARAS[name]), f_div_id=f_div, **ad_paras)
    machine = getattr(pa, name)(eval_dict=None, data_dict=dict(train_presort=True), sf_para_dict=sf, ad_para_dict=ad, gpu=True, device=device)
    machine.reset_generator_discriminator()
    return machine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--features", type=int, default=24)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--machine", choices=("both", "point", "pair"), default="both")
    ap.add_argument("--f-div", choices=tuple(F_DIVERGENCES), default="KL")
    ap.add_argument("--rough-batch-size", type=int, default=1024)
    args = ap.parse_args()
    device = "cuda:0"
    torch.manual_seed(137)
    data = pa.PaddedQueryBatches(synthetic_queries(args.queries, args.features, seed=7), device, rough_batch_size=args.rough_batch_size, presort=True)
    for key, name in (("point", "IRFGAN_Point"), ("pair", "IRFGAN_Pair")):
        if args.machine in ("both", key):
            run(build_machine(name, args.features, device, f_div=args.f_div), data, args.epochs, name=f"{name} {args.f_div}")


if __name__ == "__main__":
    main()
