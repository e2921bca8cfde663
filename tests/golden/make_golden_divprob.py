#!/usr/bin/env python3
"""Generate tests/golden/divprob.npz by RUNNING THE REFERENCE ITSELF: DivProbRanker's three module-level loss functions and get_expected_rank.

Run on the build machine, never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_divprob.py

It imports wildltr/ptranking read-only from $PTRANKING_REF, default /root/reference.  Every case is ONE query (the only batch size the reference
runs, ptranking/ltr_diversification/base/div_mdn_ranker.py:251), opt_ideal=True, presort=True, beta = 0.5.

  a|b|c/<shape>/...    mus fp32 [L], vars fp32 [L], rele uint8 [T, L] (q_doc_rele_mat; expand to float on load), max_label, max_abs_x (the
                       largest |x| = |mu_i - mu_j| / sqrt(2 (var_i + var_j)) over the pairs), ranks64 = get_expected_rank in float64;
                       combos int32 [n, 3] = (objective, top_k, norm) per row, objective 0 aNDCG = alpha_dcg_as_a_loss, 1 nERR-IA =
                       err_ia_as_a_loss, 2 PairCLS, 3 LambdaPairCLS = prob_lambda_loss, top_k 0 = None;
                       res32 fp32 [n, 1 + 2 L] = (loss, grad_mu, grad_var) of the reference on fp32 leaf tensors + autograd per row,
                       res64 float64 [n, 1 + 2 L] = the same functions on float64 tensors (few large arrays: a zip entry costs ~270 bytes)
  family a             the four objectives x top_k in {None, 3, 10} (the two SuperSoft objectives) x norm in {True, False} (LambdaPairCLS) over
                       lists of 1 .. 130 documents and 1 .. 20 subtopics, binary and graded, a query without a relevant document, a subtopic
                       without a document.  err_ia_as_a_loss with top_k > L > 1 does not run (its `[:, 1:top_k] = [:, 0:top_k - 1]` assignment
                       does not fit); that is asserted and the combination left out.
  family b             "well-conditioned" pairwise cases: variances U(0.5, 2), means N(0, 1) redrawn until max|x| <= 3 (asserted): there the
                       reference's own fp32 is a faithful evaluation, and its float64 is a parity target.
  family c             "saturated" pairwise cases: variances U(0.005, 0.01), U(0.02, 0.05), U(0.1, 0.3).  `1 - erfc(x) / 2` rounds to 1 in fp32
                       from |x| = 3.8 on (in float64 from 5.9 on) and the result is an artefact of F.binary_cross_entropy's 1e-12 floor; both
                       precisions are stored as a RECORD of what the reference returns, not as a target.

The archive is written with fixed zip timestamps so that a rerun reproduces it bit for bit.
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

from ptranking.ltr_diversification.score_and_sort.div_prob_ranker import alpha_dcg_as_a_loss, err_ia_as_a_loss, prob_lambda_loss
from ptranking.ltr_diversification.util.prob_utils import get_expected_rank

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 137
OBJ = {"aNDCG": 0, "nERR-IA": 1, "PairCLS": 2, "LambdaPairCLS": 3}


def run_reference(objective, mus, vars_, rele, top_k, norm, max_label, dtype):
    m = torch.from_numpy(mus).to(dtype).view(1, -1).requires_grad_(True)
    v = torch.from_numpy(vars_).to(dtype).view(1, -1).requires_grad_(True)
    R = torch.from_numpy(rele.astype(np.float64)).to(dtype)
    if objective == "aNDCG":
        loss = alpha_dcg_as_a_loss(top_k=top_k, batch_mus=m, batch_vars=v, q_doc_rele_mat=R, opt_ideal=True, presort=True, beta=0.5)
    elif objective == "nERR-IA":
        loss = err_ia_as_a_loss(top_k=top_k, batch_mus=m, batch_vars=v, q_doc_rele_mat=R, opt_ideal=True, presort=True, max_label=max_label,
                                device="cpu")
    else:
        loss = prob_lambda_loss(opt_id=objective, batch_mus=m, batch_vars=v, q_doc_rele_mat=R, opt_ideal=True, presort=True, beta=0.5,
                                device="cpu", norm=norm)
    loss.backward()
    zero = lambda t: np.zeros(mus.shape[0]) if t.grad is None else t.grad.detach().numpy().reshape(-1)
    return float(loss.detach()), zero(m), zero(v)


def presorted_rele(rng, T, L, density, graded=False):
    """A relevance matrix whose documents are in a plausible ideal order: relevant documents first (the reference's presort)."""
    R = (rng.random((T, L)) < density).astype(np.uint8)
    if graded:
        R = R * rng.integers(1, 4, size=(T, L)).astype(np.uint8)
    order = np.argsort(-R.sum(axis=0, dtype=np.int64), kind="stable")
    return np.ascontiguousarray(R[:, order])


def max_abs_x(mus, vars_):
    m, v = mus.astype(np.float64), vars_.astype(np.float64)
    return float(np.max(np.abs((m[:, None] - m[None, :]) / np.sqrt(2.0 * (v[:, None] + v[None, :])))))


def main():
    torch.set_num_threads(1)
    rng = np.random.default_rng(SEED)
    torch.manual_seed(SEED)
    store = {}
    counts = {"a": 0, "b": 0, "c": 0}

    rows = {}

    def put_inputs(fam, shape, mus, vars_, rele, max_label):
        ranks = get_expected_rank(batch_mus=torch.from_numpy(mus).double().view(1, -1), batch_vars=torch.from_numpy(vars_).double().view(1, -1))
        fields = dict(mus=mus, vars=vars_, rele=rele, max_label=np.float32(max_label), max_abs_x=np.float64(max_abs_x(mus, vars_)),
                      ranks64=ranks.numpy().reshape(-1).astype(np.float64))
        for k, val in fields.items():
            store[f"{fam}/{shape}/{k}"] = np.asarray(val)

    def put_case(fam, shape, objective, top_k, norm, mus, vars_, rele, max_label):
        l32, gm32, gv32 = run_reference(objective, mus, vars_, rele, top_k, norm, max_label, torch.float32)
        l64, gm64, gv64 = run_reference(objective, mus, vars_, rele, top_k, norm, max_label, torch.float64)
        name = f"{shape}__{objective}_k{top_k or 0}_n{int(bool(norm))}"
        r = rows.setdefault((fam, shape), ([], [], []))
        r[0].append((OBJ[objective], top_k or 0, int(bool(norm))))
        r[1].append(np.concatenate([[l32], gm32, gv32]).astype(np.float32))
        r[2].append(np.concatenate([[l64], gm64, gv64]).astype(np.float64))
        counts[fam] += 1
        print(f"{fam} {name:44s} loss64 {l64:+.9g}  loss32 {l32:+.9g}", flush=True)

    # ---------------------------------------------------------------- family a
    # (shape, T, L, density, special); variances = 0.1 sigmoid(N(0, 1)), the limit_delta = 0.1 head of the reference's own grid
    shapes = [("T1_L1", 1, 1, 1.0, None), ("T3_L2", 3, 2, 0.6, None), ("T1_L7_graded", 1, 7, 0.5, "graded"), ("T8_L7", 8, 7, 0.4, None),
              ("T3_L40_graded", 3, 40, 0.3, "graded"), ("T20_L40", 20, 40, 0.15, None), ("T8_L130", 8, 130, 0.1, None),
              ("T20_L130_graded", 20, 130, 0.08, "graded"), ("T8_L40_norel", 8, 40, 0.0, None), ("T8_L40_emptytopic", 8, 40, 0.25, "empty")]
    for shape, T, L, dens, special in shapes:
        mus = rng.standard_normal(L).astype(np.float32)
        vars_ = (0.1 / (1.0 + np.exp(-rng.standard_normal(L)))).astype(np.float32)
        rele = presorted_rele(rng, T, L, dens, graded=special == "graded")
        if special == "empty":
            rele[3, :] = 0
        max_label = 3.0 if special == "graded" else 1.0
        put_inputs("a", shape, mus, vars_, rele, max_label)
        for top_k in (None, 3, 10):
            put_case("a", shape, "aNDCG", top_k, False, mus, vars_, rele, max_label)
            if top_k is not None and top_k > L > 1:         # (L = 1: the one-column source broadcasts into the empty slice, and it runs)
                try:
                    run_reference("nERR-IA", mus, vars_, rele, top_k, False, max_label, torch.float64)
                except RuntimeError:
                    continue
                raise AssertionError(f"{shape}: err_ia_as_a_loss ran with top_k={top_k} > L={L}")
            put_case("a", shape, "nERR-IA", top_k, False, mus, vars_, rele, max_label)
        put_case("a", shape, "PairCLS", None, False, mus, vars_, rele, max_label)
        for norm in (True, False):
            put_case("a", shape, "LambdaPairCLS", None, norm, mus, vars_, rele, max_label)

    # ---------------------------------------------------------------- family b
    for shape, T, L, graded in [("wc_T6_L40", 6, 40, False), ("wc_T7_L44_graded", 7, 44, True), ("wc_T6_L48", 6, 48, False)]:
        vars_ = rng.uniform(0.5, 2.0, L).astype(np.float32)
        for _ in range(1000):
            mus = rng.standard_normal(L).astype(np.float32)
            if max_abs_x(mus, vars_) <= 3.0:
                break
        assert max_abs_x(mus, vars_) <= 3.0, shape
        rele = presorted_rele(rng, T, L, 0.25, graded=graded)
        put_inputs("b", shape, mus, vars_, rele, 3.0 if graded else 1.0)
        put_case("b", shape, "PairCLS", None, False, mus, vars_, rele, 1.0)
        for norm in (True, False):
            put_case("b", shape, "LambdaPairCLS", None, norm, mus, vars_, rele, 1.0)

    # ---------------------------------------------------------------- family c
    for shape, lo, hi in [("sat_v0005", 0.005, 0.01), ("sat_v002", 0.02, 0.05), ("sat_v01", 0.1, 0.3)]:
        T, L = 6, 40
        mus, vars_ = rng.standard_normal(L).astype(np.float32), rng.uniform(lo, hi, L).astype(np.float32)
        rele = presorted_rele(rng, T, L, 0.25)
        put_inputs("c", shape, mus, vars_, rele, 1.0)
        assert max_abs_x(mus, vars_) > 3.8, shape
        put_case("c", shape, "PairCLS", None, False, mus, vars_, rele, 1.0)
        put_case("c", shape, "LambdaPairCLS", None, True, mus, vars_, rele, 1.0)

    for (fam, shape), (combos, r32, r64) in rows.items():
        store[f"{fam}/{shape}/combos"] = np.asarray(combos, np.int32)
        store[f"{fam}/{shape}/res32"] = np.stack(r32)
        store[f"{fam}/{shape}/res64"] = np.stack(r64)
    out = os.path.join(HERE, "divprob.npz")
    with zipfile.ZipFile(out, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.array(store[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"wrote {out}: {counts} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
