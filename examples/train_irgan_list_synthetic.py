"""IRGAN's and IRFGAN's list machines on synthetic presorted queries with a planted linear signal: a few mini-max rounds each, nDCG@5 of the
generator and of the discriminator per round.

    python examples/train_irgan_list_synthetic.py [--queries 256] [--epochs 10] [--machine both|irgan|irfgan] [--top-k 5] [--bt] [--f-div KL]

The data and the round loop are those of train_irgan_synthetic.py.  A round is one pass of mini_max_train: per batch one sampling launch
(csrc/adlist.hip: the standard rankings by label with shuffled ties, the generator's Gumbel-softmax rankings), one step of the
discriminator on the ranking probabilities of its own scores, and one fused launch that draws, sorts and differentiates the generator's
step.  --top-k 0 plays on whole lists; --bt takes the Bradley-Terry ranking probability for the discriminator (PL_D False).
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
from train_irgan_synthetic import run, synthetic_queries     # noqa: E402, F401


def build_machine(name, num_features, device, lr=1e-2, **ad_paras):
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": lr,
          "pointsf": dict(num_features=num_features, num_layers=3, AF="R", TL_AF="S", apply_tl_af=True, BN=False, bn_type=None, bn_affine=False)}
    ad = dict(copy.deepcopy(DEFAULT_AD_PARAS[name]), **ad_paras)
    machine = getattr(pa, name)(eval_dict=None, data_dict=dict(train_presort=True), sf_para_dict=sf, ad_para_dict=ad, gpu=True, device=device)
    machine.reset_generator()
    machine.reset_discriminator()
    return machine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--features", type=int, default=24)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--machine", choices=("both", "irgan", "irfgan"), default="both")
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--bt", action="store_true")
    ap.add_argument("--f-div", choices=tuple(F_DIVERGENCES), default="KL")
    ap.add_argument("--rough-batch-size", type=int, default=1024)
    args = ap.parse_args()
    device = "cuda:0"
    torch.manual_seed(137)
    data = pa.PaddedQueryBatches(synthetic_queries(args.queries, args.features, seed=7), device, rough_batch_size=args.rough_batch_size, presort=True)
    for key, name in (("irgan", "IRGAN_List"), ("irfgan", "IRFGAN_List")):
        if args.machine in ("both", key):
            paras = dict(top_k=args.top_k or None, PL_D=not args.bt, **(dict(f_div_id=args.f_div) if name == "IRFGAN_List" else {}))
            run(build_machine(name, args.features, device, **paras), data, args.epochs, name=name)


if __name__ == "__main__":
    main()
