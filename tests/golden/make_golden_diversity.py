#!/usr/bin/env python3
"""Generate tests/golden/diversity.npz by RUNNING THE REFERENCE ITSELF (the ltr_diversification frame: DALETOR's loss and the diversity metrics).

Run on the build machine, never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_diversity.py

It imports wildltr/ptranking read-only from $PTRANKING_REF, default /root/reference.  Every case is ONE query (the only batch size the reference
runs, ptranking/base/ranker.py:636-669).

  daletor/<case>/...   preds fp32 [1, L], rele uint8 [T, L] (q_doc_rele_mat; expand to float on load), rt, top_k (0 = None);
                       loss32 / grad32 = the reference's own alphaDCG_as_a_loss (daletor.py:23-38, alpha = 0.5 as DALETOR calls it) + autograd on
                       fp32 tensors, loss64 / grad64 = the same functions on float64 tensors, need32 = how many times the element-wise gate of
                       tests/golden_util.assert_close (1e-5 |b| + 1e-6 max(1, max|b|)) the fp32 gradient needs against the float64 one.
                       Cases named steep_* (rt = 100) are kept apart: there the reference's own fp32 gradient misses that gate; every other
                       case is ASSERTED here to have need32 <= 0.5, so the GPU test's gate asks nothing the reference does not deliver with room.
  metrics/<case>/...   preds fp32 [L] (tie-free), rele uint8 [T, L], ks, max_label, k1; andcg / err_ia / nerr_ia [nk] = the reference's
                       torch_alpha_ndcg_at_ks / torch_err_ia_at_ks / torch_nerr_ia_at_ks on its own CPU torch.sort of preds (ideal = the input
                       order, ranker.py:296), andcg_k1 / err_ia_k1 / nerr_ia_k1 = the single-cut-off functions at k1 <= L, valid = the
                       evaluator's skip rule (ranker.py:282).

tests/golden/diversity_edge.npz (a second archive, so that diversity.npz keeps its bytes) holds what the reference returns for NON-FINITE scores:

  nonfinite/<case>/... preds fp32 [1, L] with one NaN, two +inf and one -inf score (and each kind alone), rele uint8 [T, L], rt, top_k;
                       loss32 / grad32 and loss64 / grad64 as above.  Robust_Sigmoid's two torch.where take a NaN difference (a NaN score,
                       inf - inf) as 0.5, so loss and gradient stay finite: asserted here.

Both archives are written with fixed zip timestamps so that a rerun reproduces them bit for bit.
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

from ptranking.ltr_diversification.score_and_sort.daletor import alphaDCG_as_a_loss
from ptranking.metric.srd.diversity_metric import (torch_alpha_ndcg_at_k, torch_alpha_ndcg_at_ks, torch_err_ia_at_k, torch_err_ia_at_ks,
                                                   torch_nerr_ia_at_k, torch_nerr_ia_at_ks)

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 137


def need(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / (1e-5 * np.abs(b) + 1e-6 * max(1.0, float(np.max(np.abs(b)))))))


def ref_loss(preds, rele, rt, top_k, dtype):
    p = torch.from_numpy(preds).to(dtype).requires_grad_(True)
    R = torch.from_numpy(rele.astype(np.float64)).to(dtype)
    loss = alphaDCG_as_a_loss(batch_preds=p, q_doc_rele_mat=R, rt=rt, device='cpu', top_k=top_k)
    loss.backward()
    return loss.detach().item(), p.grad.detach().numpy()


def presorted_rele(rng, T, L, density, graded=False):
    """A relevance matrix whose documents are in a plausible ideal order: relevant documents first (the reference's presort)."""
    R = (rng.random((T, L)) < density).astype(np.uint8)
    if graded:
        R = R * rng.integers(1, 4, size=(T, L)).astype(np.uint8)
    order = np.argsort(-R.sum(axis=0, dtype=np.int64), kind="stable")
    return np.ascontiguousarray(R[:, order])


def main():
    rng = np.random.default_rng(SEED)
    torch.manual_seed(SEED)
    store = {}
    # ---------------------------------------------------------------- DALETOR loss
    # (name, T, L, sigma, density, rt, top_k, special)
    cases = [
        ("T1_L20", 1, 20, 1.0, 0.3, 10.0, 10, None),
        ("T3_L5_k10", 3, 5, 1.0, 0.5, 10.0, 10, None),               # L < top_k and T < top_k
        ("T5_L40_k10", 5, 40, 1.0, 0.2, 10.0, 10, None),             # T < top_k
        ("T12_L64_k4", 12, 64, 2.0, 0.15, 10.0, 4, None),            # T > top_k
        ("T30_L50_k20", 30, 50, 0.3, 0.1, 10.0, 20, None),
        ("T8_L128_full", 8, 128, 1.0, 0.1, 10.0, None, None),
        ("T6_L100_rt1", 6, 100, 5.0, 0.25, 1.0, 10, None),
        ("T6_L200_rt50", 6, 200, 0.3, 0.1, 50.0, 10, None),
        ("T9_L300_k2", 9, 300, 1.0, 0.05, 10.0, 2, None),
        ("T4_L512", 4, 512, 1.0, 0.05, 10.0, 10, None),
        ("T5_L1000", 5, 1000, 1.0, 0.05, 10.0, 10, None),
        ("T16_L129", 16, 129, 1.0, 0.1, 10.0, None, None),
        ("T7_L64_ties", 7, 64, 0.5, 0.2, 10.0, 10, "ties"),           # score differences of exactly 0
        ("T5_L32_zeroR", 5, 32, 1.0, 0.0, 10.0, 10, None),            # all-zero R
        ("T6_L48_emptytopic", 6, 48, 1.0, 0.2, 10.0, 10, "empty"),    # a subtopic without a relevant document
        ("T5_L60_graded", 5, 60, 1.0, 0.2, 10.0, 10, "graded"),
        ("steep_T7_L64_a", 7, 64, 1.0, 0.2, 100.0, None, None),
        ("steep_T7_L64_b", 7, 64, 1.0, 0.2, 100.0, None, None),
    ]
    for name, T, L, sigma, dens, rt, top_k, special in cases:
        preds = (sigma * rng.standard_normal((1, L))).astype(np.float32)
        rele = presorted_rele(rng, T, L, dens, graded=special == "graded")
        if special == "ties":
            preds[0, 5] = preds[0, 17]
            preds[0, 40:42] = preds[0, 3]
        if special == "empty":
            rele[2, :] = 0
        l32, g32 = ref_loss(preds, rele, rt, top_k, torch.float32)
        l64, g64 = ref_loss(preds, rele, rt, top_k, torch.float64)
        n32 = need(g32, g64)
        assert np.all(np.isfinite(g64)) and np.isfinite(l64), name
        if name.startswith("steep_"):
            assert np.max(np.abs(g32 - g64)) <= 1e-5 + 1e-5 * np.max(np.abs(g64)), name
        else:
            assert n32 <= 0.5, f"{name}: the reference's own fp32 gradient needs {n32:.3f} of the gate"
        fields = dict(preds=preds, rele=rele, rt=np.float32(rt), top_k=np.int32(top_k or 0), loss32=np.float32(l32),
                      grad32=g32.astype(np.float32), loss64=np.float64(l64), grad64=g64.astype(np.float64), need32=np.float64(n32))
        for k, v in fields.items():
            store[f"daletor/{name}/{k}"] = np.asarray(v)
        print(f"daletor {name:22s} loss64 {l64:+.6g}  need32 {n32:.3f}", flush=True)

    # ---------------------------------------------------------------- metrics
    # (name, T, L, density, ks, max_label, k1, special)
    mcases = [
        ("T5_L40", 5, 40, 0.2, [1, 3, 5, 10, 20], 1.0, 5, None),
        ("T1_L12", 1, 12, 0.4, [1, 5, 10], 1.0, 10, None),
        ("T8_L100", 8, 100, 0.1, [1, 5, 10, 20, 50, 100], 1.0, 20, None),
        ("T6_L7_klarge", 6, 7, 0.4, [1, 5, 10, 20], 1.0, 5, None),             # k > L: the reference pads with 0
        ("T4_L30_ideal0", 4, 30, 0.2, [1, 2, 5, 10], 1.0, 1, "ideal0"),        # the first input document is irrelevant: ideal@1 = 0
        ("T5_L25_zeroR", 5, 25, 0.0, [1, 5, 10], 1.0, 5, None),                # valid = 0
        ("T6_L50_graded", 6, 50, 0.2, [1, 5, 10, 20], 3.0, 10, "graded"),      # max_label > 1
        ("T20_L300", 20, 300, 0.05, [5, 10, 20, 100, 300], 2.0, 100, "graded"),
        ("T3_L1000", 3, 1000, 0.02, [1, 10, 100, 1000], 1.0, 10, None),
        ("T6_L40_emptytopic", 6, 40, 0.2, [1, 5, 10], 1.0, 5, "empty"),
    ]
    for name, T, L, dens, ks, max_label, k1, special in mcases:
        preds = rng.standard_normal(L).astype(np.float32)
        assert len(np.unique(preds)) == L, name                                  # tie-free: the two sorts may order ties differently
        rele = presorted_rele(rng, T, L, dens, graded=special == "graded")
        if special == "ideal0":
            rele = np.ascontiguousarray(np.roll(rele, 1, axis=1))
            rele[:, 0] = 0
        if special == "empty":
            rele[1, :] = 0
        R = torch.from_numpy(rele.astype(np.float32))
        _, inds = torch.sort(torch.from_numpy(preds).view(1, -1), dim=1, descending=True)
        sys_R = torch.gather(R, dim=1, index=inds.expand(T, -1))
        a = torch_alpha_ndcg_at_ks(sys_q_doc_rele_mat=sys_R, ideal_q_doc_rele_mat=R, ks=ks, alpha=0.5, device='cpu').numpy()
        a = np.asarray(a, np.float64).reshape(-1, len(ks))[0]                    # the padded form is [T, nk] with equal rows
        e = np.asarray(torch_err_ia_at_ks(sorted_q_doc_rele_mat=sys_R, max_label=max_label, ks=ks, device='cpu').numpy(), np.float64).reshape(-1)
        ne = np.asarray(torch_nerr_ia_at_ks(sys_q_doc_rele_mat=sys_R, ideal_q_doc_rele_mat=R, max_label=max_label, ks=ks, device='cpu').numpy(),
                        np.float64).reshape(-1)
        if ne.shape[0] != len(ks):                                               # zero_metric_value: the reference returns zeros(1)
            assert ne.shape[0] == 1 and ne[0] == 0.0
            ne = np.zeros(len(ks))
        assert a.shape == e.shape == ne.shape == (len(ks),), name
        assert k1 <= L
        a1 = float(np.asarray(torch_alpha_ndcg_at_k(sys_q_doc_rele_mat=sys_R, ideal_q_doc_rele_mat=R, k=k1, alpha=0.5, device='cpu')).reshape(-1)[0])
        e1 = float(np.asarray(torch_err_ia_at_k(sorted_q_doc_rele_mat=sys_R, max_label=max_label, k=k1, device='cpu')).reshape(-1)[0])
        n1 = float(np.asarray(torch_nerr_ia_at_k(sys_q_doc_rele_mat=sys_R, ideal_q_doc_rele_mat=R, max_label=max_label, k=k1, device='cpu')).reshape(-1)[0])
        fields = dict(preds=preds, rele=rele, ks=np.asarray(ks, np.int32), max_label=np.float32(max_label), k1=np.int32(k1), andcg=a, err_ia=e,
                      nerr_ia=ne, andcg_k1=np.float64(a1), err_ia_k1=np.float64(e1), nerr_ia_k1=np.float64(n1),
                      valid=np.int32(int(rele.sum() >= 1)))
        for k, v in fields.items():
            store[f"metrics/{name}/{k}"] = np.asarray(v)
        print(f"metrics {name:22s} andcg {np.round(a, 4)}", flush=True)

    out = write_archive("diversity.npz", store)
    print(f"wrote {out}: {len(cases)} loss cases, {len(mcases)} metric cases, {os.path.getsize(out)} bytes")

    # ---------------------------------------------------------------- non-finite scores (a generator of their own: diversity.npz keeps its bytes)
    rng = np.random.default_rng(SEED + 1)
    edge = {}
    # (name, T, L, rt, top_k, {index: value})
    ecases = [
        ("mixed_T5_L40", 5, 40, 10.0, 10, {3: np.nan, 7: np.inf, 21: np.inf, 30: -np.inf}),
        ("mixed_T7_L130_full", 7, 130, 10.0, None, {0: np.inf, 64: np.nan, 100: np.inf, 129: -np.inf}),
        ("nan_T3_L20", 3, 20, 10.0, 10, {11: np.nan}),
        ("two_nan_T3_L20", 3, 20, 10.0, 2, {0: np.nan, 19: np.nan}),
        ("pinf_T4_L33", 4, 33, 100.0, None, {5: np.inf, 6: np.inf}),
        ("ninf_T4_L33", 4, 33, 10.0, 3, {32: -np.inf}),
    ]
    for name, T, L, rt, top_k, planted in ecases:
        preds = rng.standard_normal((1, L)).astype(np.float32)
        for i, v in planted.items():
            preds[0, i] = v
        rele = presorted_rele(rng, T, L, 0.3, graded=True)
        l32, g32 = ref_loss(preds, rele, rt, top_k, torch.float32)
        l64, g64 = ref_loss(preds, rele, rt, top_k, torch.float64)
        assert np.isfinite(l64) and np.all(np.isfinite(g64)) and np.isfinite(l32) and np.all(np.isfinite(g32)), name
        fields = dict(preds=preds, rele=rele, rt=np.float32(rt), top_k=np.int32(top_k or 0), loss32=np.float32(l32), grad32=g32.astype(np.float32),
                      loss64=np.float64(l64), grad64=g64.astype(np.float64))
        for k, v in fields.items():
            edge[f"nonfinite/{name}/{k}"] = np.asarray(v)
        print(f"nonfinite {name:22s} loss64 {l64:+.6g}  max|grad64| {np.max(np.abs(g64)):.4g}", flush=True)
    out = write_archive("diversity_edge.npz", edge)
    print(f"wrote {out}: {len(ecases)} non-finite cases, {os.path.getsize(out)} bytes")


def write_archive(fname, store):
    out = os.path.join(HERE, fname)
    with zipfile.ZipFile(out, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.array(store[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    return out


if __name__ == "__main__":
    main()
