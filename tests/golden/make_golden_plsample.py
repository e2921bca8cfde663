#!/usr/bin/env python3
"""Generate tests/golden/plsample.npz by RUNNING THE REFERENCE ITSELF: the Gumbel samplers of ptranking/ltr_adhoc/util/sampling_utils.py:60-81
and ptranking/ltr_adversarial/util/list_sampling.py:38-67, and MDPRank.custom_loss_function (ptranking/ltr_adhoc/listwise/mdprank.py:24-80) with
distribution='STPL', with the torch.rand draws captured (the spy of make_golden.py gen_siblings).

Run on the build machine, never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_plsample.py

It imports wildltr/ptranking read-only from $PTRANKING_REF, default /root/reference.  Layout (<family>/<case>/<field>):

  sampler/<fn>_n<n>_t<T>_i<only_indices>   fn = adhoc (sampling_utils), adv1 / adv5 (list_sampling with num_sample_ranking 1 / 5);
      preds fp32 [1, n], unif fp32 [S, n] (S = 1 or 5), temperature, only_indices, inds int64 [S, n], and with only_indices = 0
      logits fp32 [S, n] (the sorted (preds + gumbel) / T).  T in {1, 0.5, 2}, n in {1, 2, 3, 17, 64, 65, 130, 300}.
  mdprank/n<n>_k<top_k>_g<gamma>_t<T>      preds / labels fp32 [1, n] (labels presorted), unif fp32 [1, n], top_k (0 = None), gamma, temperature,
      perm int64 [1, n] (the sampled ranking), loss fp32, grad fp32 [1, n].  n in {12, 40, 150}, (top_k, gamma) in {(10, 1), (None, 0.9),
      (3, 0.5)}, T in {1, 2}.
  seed int64 per case: the torch seed of its draws.

A fixture pins a ranking exactly only when no two adjacent sorted keys are closer than rounding: every case redraws its seed (seed + 1000,
...) until each adjacent gap of the float64 keys preds + gumbel exceeds 2^-16 max|key|, and that is asserted.  The archive is written with
fixed zip timestamps so that a rerun reproduces it byte for byte.
"""
import io
import os
import sys
import zipfile

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = os.environ.get("PTRANKING_REF") or "/root/reference"
if not os.path.isdir(REF):
    raise SystemExit(f"no wildltr/ptranking checkout at {REF} (set PTRANKING_REF)")
sys.path.insert(0, REF)

import numpy as np
import torch

import ptranking.ltr_adhoc.listwise.mdprank as ref_mdprank
from ptranking.data.data_utils import LABEL_TYPE
from ptranking.ltr_adhoc.util import sampling_utils
from ptranking.ltr_adversarial.util import list_sampling

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 137
MSLR_P = [0.5147, 0.3250, 0.1339, 0.0183, 0.0081]   # testing/data/testing_data_utils.py:326, as make_golden.py
GAP = 2.0 ** -16
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False)}


class _StubOptimizer:
    def zero_grad(self):
        pass

    def step(self):
        pass


def with_rand_spy(fn):
    """Run fn() with torch.rand wrapped -> (result, the one captured draw as fp32)."""
    captured = []
    orig = torch.rand

    def spy(*a, **k):
        out = orig(*a, **k)
        captured.append(out.numpy().astype(np.float32).copy())
        return out

    torch.rand = spy
    try:
        res = fn()
    finally:
        torch.rand = orig
    assert len(captured) == 1
    return res, captured[0]


def gaps_ok(preds, unif):
    """Every adjacent gap of the float64 keys preds + gumbel(unif), row by row, above 2^-16 max|key|."""
    u = (unif.astype(np.float32) + np.float32(1e-20)).astype(np.float64)
    key = preds.astype(np.float64) + -np.log(-np.log(u) + 1e-20)
    for row in np.atleast_2d(key):
        if row.size > 1:
            srt = -np.sort(-row)
            if not np.min(srt[:-1] - srt[1:]) > GAP * np.max(np.abs(row)):
                return False
    return True


def redrawn(seed, preds, shape, run):
    """run() under torch.manual_seed(seed), seed + 1000, ... until the captured uniforms separate the keys.  A seed is screened with the
    draw the reference is about to make (its first torch.rand of `shape` after seeding) before the reference runs under it: five rankings
    of 300 documents pass once in some 10^4 seeds."""
    for _ in range(4000000):
        torch.manual_seed(seed)
        if gaps_ok(preds, torch.rand(shape).numpy()):
            torch.manual_seed(seed)
            res, unif = with_rand_spy(run)
            assert gaps_ok(preds, unif)
            return seed, res, unif
        seed += 1000
    raise AssertionError("no seed separates the keys")


def main():
    torch.set_num_threads(1)
    rng = np.random.default_rng(SEED)
    store = {}
    count = redraws = 0
    case_seed = SEED * 7
    for n in (1, 2, 3, 17, 64, 65, 130, 300):
        preds = rng.standard_normal((1, n)).astype(np.float32)
        for T in (1.0, 0.5, 2.0):
            for fn, S in (("adhoc", 1), ("adv1", 1), ("adv5", 5)):
                for only in (1, 0):
                    tp = torch.from_numpy(preds)

                    def run():
                        if fn == "adhoc":
                            return sampling_utils.sample_ranking_PL_gumbel_softmax(batch_preds=tp, only_indices=bool(only), temperature=T, device="cpu")
                        return list_sampling.sample_ranking_PL_gumbel_softmax(batch_preds=tp, num_sample_ranking=S, only_indices=bool(only), temperature=T)

                    case_seed += 1
                    seed, res, unif = redrawn(case_seed, preds, (S, n), run)
                    redraws += (seed - case_seed) // 1000
                    assert unif.shape == (S, n) and gaps_ok(preds, unif)
                    name = f"sampler/{fn}_n{n}_t{T:g}_i{only}"
                    inds = (res if only else res[0]).numpy().astype(np.int64)
                    store[f"{name}/preds"], store[f"{name}/unif"], store[f"{name}/inds"] = preds, unif, inds
                    store[f"{name}/temperature"], store[f"{name}/only_indices"] = np.float32(T), np.int32(only)
                    store[f"{name}/seed"] = np.int64(seed)
                    if not only:
                        store[f"{name}/logits"] = res[1].numpy().astype(np.float32)
                    count += 1
    for n in (12, 40, 150):
        preds = rng.standard_normal((1, n)).astype(np.float32)
        labels = -np.sort(-rng.choice(5, size=(1, n), p=np.asarray(MSLR_P) / np.sum(MSLR_P)).astype(np.float32), axis=1)
        labels[0, 0] = max(labels[0, 0], 1.0)
        for top_k, gamma in ((10, 1.0), (None, 0.9), (3, 0.5)):
            for T in (1.0, 2.0):
                out = {}

                def run():
                    ranker = ref_mdprank.MDPRank(sf_para_dict=SF, model_para_dict=dict(gamma=gamma, top_k=top_k, temperature=T, distribution='STPL'),
                                                 device="cpu")
                    ranker.optimizer = _StubOptimizer()
                    p = torch.from_numpy(preds).clone().requires_grad_(True)
                    orig = ref_mdprank.sample_ranking_PL_gumbel_softmax

                    def spy(*a, **k):
                        r = orig(*a, **k)
                        out["perm"] = r[0].numpy().astype(np.int64).copy()
                        return r

                    ref_mdprank.sample_ranking_PL_gumbel_softmax = spy
                    try:
                        loss = ranker.custom_loss_function(p, torch.from_numpy(labels).clone(), presort=True, label_type=LABEL_TYPE.MultiLabel)
                    finally:
                        ref_mdprank.sample_ranking_PL_gumbel_softmax = orig
                    return np.float32(loss.detach().item()), p.grad.detach().numpy().astype(np.float32)

                case_seed += 1
                seed, (loss, grad), unif = redrawn(case_seed, preds, (1, n), run)
                redraws += (seed - case_seed) // 1000
                assert unif.shape == (1, n) and gaps_ok(preds, unif)
                name = f"mdprank/n{n}_k{top_k or 0}_g{gamma:g}_t{T:g}"
                for k, v in dict(preds=preds, labels=labels, unif=unif, top_k=np.int32(top_k or 0), gamma=np.float32(gamma), temperature=np.float32(T),
                                 perm=out["perm"], loss=loss, grad=grad, seed=np.int64(seed)).items():
                    store[f"{name}/{k}"] = v
                count += 1

    out_path = os.path.join(HERE, "plsample.npz")
    with zipfile.ZipFile(out_path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.array(store[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"wrote {out_path}: {count} cases, {redraws} seeds redrawn for the gap condition, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
