#!/usr/bin/env python3
"""Generate tests/golden/wassrank.npz by RUNNING THE REFERENCE ITSELF (WassRank, mode 'SinkhornOT', smooth_type 'ST', norm_type 'BothST').

Run here (the build container), never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wassrank.py

It imports wildltr/ptranking read-only from $PTRANKING_REF, default /root/reference.  Every case is one query (B = 1: the only batch size
the reference runs — it squeezes the [B,L,L] cost to 2-D, wassRank.py:73) and stores, under 'wassrank/<case>/<field>':

  preds, labels (fp32 [1, L]) and the parameters (cost_type index into COST_TYPES, lam, sh_itr, gain_base, non_rele_gap, var_penalty,
  scale = 1 for the TL_AF 'S' branch of get_normalized_histograms);
  loss32, grad32, ref32_finite — the reference in fp32: its own WassRank.custom_loss_function (wassRank.py:43-88) with a stub optimiser
  and stdout redirected (it prints batch_preds), or, for the TL_AF 'S' cases, its component functions called with TL_AF='S'.  Stored
  even when NaN (the reference's one-shift-per-query stabilisation, pytorch_wasserstein.py:343-350, underflows to log(0));
  loss64, grad64 — the reference's component functions get_explicit_cost_mat, get_normalized_histograms and OldSinkhornOT run on float64
  tensors (asserted finite).

The archive is written with fixed zip timestamps so that a rerun reproduces it bit for bit.
"""
import contextlib
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

from ptranking.ltr_adhoc.listwise.wassrank.wassRank import WassRank, WassRankParameter
from ptranking.ltr_adhoc.listwise.wassrank.pytorch_wasserstein import OldSinkhornOT
from ptranking.ltr_adhoc.listwise.wassrank.wasserstein_cost_mat import get_explicit_cost_mat, get_normalized_histograms

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 137
MSLR_P = [0.5147, 0.3250, 0.1339, 0.0183, 0.0081]
COST_TYPES = ("p1", "p2", "eg", "dg", "ddg")
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False)}


class _StubOptimizer:
    def zero_grad(self):
        pass

    def step(self):
        pass


def para(cost_type, lam, sh_itr, gain_base, non_rele_gap, var_penalty):
    d = WassRankParameter().default_para_dict()
    d.update(cost_type=cost_type, lam=lam, sh_itr=sh_itr, gain_base=gain_base, non_rele_gap=non_rele_gap, var_penalty=var_penalty)
    return d


def ref32_own(preds, labels, wd, qid):
    """The reference's own custom_loss_function (fp32, CPU)."""
    r = WassRank(sf_para_dict=SF, wass_para_dict=wd, dict_cost_mats={}, dict_std_dists={}, gpu=False)
    r.optimizer = _StubOptimizer()
    p = torch.from_numpy(preds).clone().requires_grad_(True)
    with contextlib.redirect_stdout(io.StringIO()):
        loss = r.custom_loss_function(p, torch.from_numpy(labels).clone(), batch_ids=[qid])
    return np.float32(loss.detach().item()), p.grad.detach().numpy().astype(np.float32)


def ref_components(preds, labels, wd, dtype, tl_af):
    """get_explicit_cost_mat -> get_normalized_histograms -> OldSinkhornOT in `dtype` (wassRank.py:61-73 with TL_AF passed explicitly)."""
    p = torch.from_numpy(preds).to(dtype).requires_grad_(True)
    y = torch.from_numpy(labels).to(dtype)
    C = get_explicit_cost_mat(y, wass_para_dict=wd, gpu=False).to(dtype)     # p1 / p2 build an fp32 position matrix whatever the labels' dtype
    std_h, pred_h = get_normalized_histograms(batch_std_labels=y, batch_preds=p, wass_dict_std_dists=None, qid=None, wass_para_dict=wd,
                                              TL_AF=tl_af)
    loss = OldSinkhornOT.apply(pred_h, std_h, torch.squeeze(C, dim=0), wd['lam'], wd['sh_itr'])
    loss.backward()
    return loss.detach().item(), p.grad.detach().numpy().astype(np.float64)


def labels_mslr(rng, L):
    y = rng.choice(5, size=L, p=np.asarray(MSLR_P) / np.sum(MSLR_P)).astype(np.float32)
    if y.max() < 1:
        y[rng.integers(L)] = 1.0
    return -np.sort(-y)


def main():
    rng = np.random.default_rng(SEED)
    torch.manual_seed(SEED)
    e = float(np.e)
    cases = []     # (name, L, sigma, labels or None, cost, lam, sh_itr, gain_base, non_rele_gap, var_penalty, scale)
    for cost in COST_TYPES:
        for L in (7, 64, 256) + ((512,) if cost == "eg" else ()):
            cases.append((f"{cost}_L{L}_s1", L, 1.0, None, cost, 0.1, 20, 4.0, 100.0, e, 0))
        for L in (128, 512):
            cases.append((f"{cost}_L{L}_s3", L, 3.0, None, cost, 0.1, 20, 4.0, 100.0, e, 0))
    cases += [
        ("eg_L1", 1, 1.0, None, "eg", 0.1, 20, 4.0, 100.0, e, 0),
        ("eg_L2", 2, 1.0, np.array([2.0, 0.0], np.float32), "eg", 0.1, 20, 4.0, 100.0, e, 0),
        ("p1_L2", 2, 3.0, None, "p1", 0.1, 20, 4.0, 100.0, e, 0),
        ("eg_lam001_L64", 64, 1.0, None, "eg", 0.01, 20, 4.0, 100.0, e, 0),
        ("eg_lam1_L128", 128, 3.0, None, "eg", 1.0, 20, 4.0, 100.0, e, 0),
        ("p1_lam001_L64", 64, 1.0, None, "p1", 0.01, 20, 4.0, 100.0, e, 0),
        ("ddg_lam1_L64", 64, 3.0, None, "ddg", 1.0, 20, 4.0, 100.0, e, 0),
        ("eg_itr0_L64", 64, 1.0, None, "eg", 0.1, 0, 4.0, 100.0, e, 0),
        ("p2_itr0_L64", 64, 3.0, None, "p2", 0.1, 0, 4.0, 100.0, e, 0),
        ("eg_itr1_L128", 128, 1.0, None, "eg", 0.1, 1, 4.0, 100.0, e, 0),
        ("dg_itr1_L64", 64, 3.0, None, "dg", 0.1, 1, 4.0, 100.0, e, 0),
        ("eg_itr50_L128", 128, 1.0, None, "eg", 0.1, 50, 4.0, 100.0, e, 0),
        ("p1_itr50_L64", 64, 1.0, None, "p1", 0.1, 50, 4.0, 100.0, e, 0),
        ("eg_params_L64", 64, 1.0, None, "eg", 0.1, 20, 3.0, 10.0, 0.5, 0),
        ("eg_params_L256", 256, 3.0, None, "eg", 0.1, 20, 2.0, 25.0, 2.0, 0),
        ("eg_zero_L64", 64, 1.0, np.zeros(64, np.float32), "eg", 0.1, 20, 4.0, 100.0, e, 0),
        ("dg_zero_L64", 64, 1.0, np.zeros(64, np.float32), "dg", 0.1, 20, 4.0, 100.0, e, 0),
        ("eg_equal_L64", 64, 1.0, np.full(64, 2.0, np.float32), "eg", 0.1, 20, 4.0, 100.0, e, 0),
        ("ddg_equal_L64", 64, 3.0, np.full(64, 3.0, np.float32), "ddg", 0.1, 20, 4.0, 100.0, e, 0),
        # fractional labels: 4^y - 1 for y in {0.3, 0.6, 0.8, 1.05, 1.1, ...} — gains < 1 become -non_rele_gap, and pairs of gains closer
        # than 1 (not equal) take var_penalty (wasserstein_cost_mat.py:100-104)
        ("eg_frac_L64", 64, 1.0, "frac", "eg", 0.1, 20, 4.0, 100.0, e, 0),
        ("eg_frac_L256", 256, 3.0, "frac", "eg", 0.1, 20, 4.0, 100.0, e, 0),
        # TL_AF 'S': predictions scaled by the maximum label (get_normalized_histograms, wasserstein_cost_mat.py:196-198)
        ("eg_tlafS_L64", 64, 1.0, None, "eg", 0.1, 20, 4.0, 100.0, e, 1),
        ("p2_tlafS_L128", 128, 1.0, None, "p2", 0.1, 20, 4.0, 100.0, e, 1),
        ("dg_tlafS_zero_L64", 64, 1.0, np.zeros(64, np.float32), "dg", 0.1, 20, 4.0, 100.0, e, 1),
    ]
    store = {}
    n_nan = 0
    for name, L, sigma, lab, cost, lam, sh_itr, gb, gap, vp, scale in cases:
        preds = (sigma * rng.standard_normal((1, L))).astype(np.float32)
        if lab is None:
            labels = labels_mslr(rng, L)[None, :]
        elif isinstance(lab, str):
            labels = -np.sort(-rng.choice(np.array([0.0, 0.3, 0.6, 0.8, 1.05, 1.1, 1.3, 2.0, 2.1], np.float32), size=L))[None, :]
        else:
            labels = lab[None, :].astype(np.float32)
        labels = np.ascontiguousarray(labels, dtype=np.float32)
        wd = para(cost, lam, sh_itr, gb, gap, vp)
        if scale:
            l32, g32 = ref_components(preds, labels, wd, torch.float32, "S")
            l32, g32 = np.float32(l32), g32.astype(np.float32)
            l64, g64 = ref_components(preds, labels, wd, torch.float64, "S")
        else:
            l32, g32 = ref32_own(preds, labels, wd, name)
            l64, g64 = ref_components(preds, labels, wd, torch.float64, None)
        assert np.isfinite(l64) and np.all(np.isfinite(g64)), name
        finite = bool(np.isfinite(l32) and np.all(np.isfinite(g32)))
        n_nan += not finite
        fields = dict(preds=preds, labels=labels, cost_type=np.int32(COST_TYPES.index(cost)), lam=np.float32(lam), sh_itr=np.int32(sh_itr),
                      gain_base=np.float32(gb), non_rele_gap=np.float32(gap), var_penalty=np.float32(vp), scale=np.int32(scale),
                      loss32=np.float32(l32), grad32=g32, ref32_finite=np.bool_(finite), loss64=np.float64(l64), grad64=g64)
        for k, v in fields.items():
            store[f"wassrank/{name}/{k}"] = np.asarray(v)
        print(f"{name:22s} loss64 {l64:.6g}  ref32 {'finite' if finite else 'NaN'}", flush=True)
    assert n_nan >= 3, f"only {n_nan} cases where the reference's fp32 run is not finite"
    out = os.path.join(HERE, "wassrank.npz")
    with zipfile.ZipFile(out, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.array(store[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"wrote {out}: {len(cases)} cases, {n_nan} with a non-finite fp32 reference, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
