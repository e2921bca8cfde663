#!/usr/bin/env python3
"""Generate tests/golden/smooth_metric.npz by RUNNING THE REFERENCE ITSELF: get_approx_ranks (ptranking/ltr_adhoc/listwise/approxNDCG.py:19-27),
then precision_ / AP_ / nERR_ / nDCG_as_opt_objective (ptranking/metric/smooth_metric/metric_as_opt_objective.py), then autograd, in float64
AND in fp32.

Run on the build machine, never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_smooth.py

It imports wildltr/ptranking read-only from $PTRANKING_REF, default /root/reference.  Layout (<family>/<case>/<field>):

  preds fp32 [n] (batch case: [B, n]), labels fp32 (presorted, descending), alpha, max_label (what nERR's torch.max(batch_std_labels) is),
  combos int32 [R, 3] = (metric 0 P / 1 AP / 2 nERR / 3 nDCG, opt_ideal, top_k with 0 = None) per row,
  res64 float64 [R, 1 + B n] = (loss, gradient) of the reference on float64 tensors, res32 fp32 the same on fp32 tensors,
  valid fp32 [R, B]: 0 where the reference's pos_inds filter drops the query (its zero_metric_value for the query alone; loss and gradient
  are then recorded as 0), 1 elsewhere.

  main   one query each: n in {2, 3, 17, 64, 65, 130} x alpha in {1, 10}, the label mix of make_golden.py (MSLR), pairwise distinct scores;
         4 metrics x opt_ideal 0 / 1 x top_k in {None, 1, 5, n}.  The fp32 and float64 orders of the smooth ranks are asserted equal.
         nERR with top_k > n does not run in the reference (torch_rankwise_err asserts); that is asserted and the combination left out.
  edge   n = 1 (relevant / not), a list without a relevant document in every form, relevant documents only beyond position K, top_k > n for
         P, AP and nDCG, and a batch of 3 with one filtered query (valid matters).  nERR on that batch is recorded one query at a time and
         summed: the reference's batched nERR couples the queries through a [B] / [B, 1] broadcast (see put()).

The archive is written with fixed zip timestamps so that a rerun reproduces it byte for byte.
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

from ptranking.data.data_utils import LABEL_TYPE
from ptranking.ltr_adhoc.listwise.approxNDCG import get_approx_ranks
from ptranking.metric.smooth_metric.metric_as_opt_objective import (AP_as_opt_objective, nDCG_as_opt_objective, nERR_as_opt_objective,
                                                                    precision_as_opt_objective)

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 137
MSLR_P = [0.5147, 0.3250, 0.1339, 0.0183, 0.0081]   # testing/data/testing_data_utils.py:326, as make_golden.py
METRICS = ("P", "AP", "nERR", "nDCG")


def run_reference(metric, preds, labels, alpha, top_k, opt_ideal, dtype):
    """-> (loss, grad [B, n], filtered, rank order [B, n]) for a [B, n] batch."""
    p = torch.from_numpy(preds).to(dtype).requires_grad_(True)
    y = torch.from_numpy(labels).to(dtype)
    ranks = get_approx_ranks(p, alpha=alpha, device="cpu")
    kw = dict(top_k=top_k, batch_smooth_ranks=ranks, batch_std_labels=y, presort=True, opt_ideal=opt_ideal, device="cpu")
    if metric == "P":
        loss, zero = precision_as_opt_objective(**kw)
    elif metric == "AP":
        loss, zero = AP_as_opt_objective(**kw)
    elif metric == "nERR":
        loss, zero = nERR_as_opt_objective(**kw)
    else:
        loss, zero = nDCG_as_opt_objective(label_type=LABEL_TYPE.MultiLabel, **kw)
    order = torch.sort(ranks.detach(), dim=1)[1].numpy()
    if zero:
        return 0.0, np.zeros(preds.shape), True, order
    loss.backward()
    return float(loss.detach()), p.grad.detach().numpy().astype(np.float64), False, order


def labels_mslr(rng, n, relevant=True):
    y = rng.choice(len(MSLR_P), size=n, p=np.asarray(MSLR_P) / np.sum(MSLR_P)).astype(np.float32)
    if relevant and y.max() < 1:
        y[rng.integers(n)] = 1.0
    return -np.sort(-y)


def distinct_scores(rng, n, alpha):
    """N(0, 1) scores (alpha = 10) or N(0, 3) (alpha = 1), redrawn until pairwise distinct in fp32 by at least 1e-3 / alpha."""
    for _ in range(1000):
        s = (rng.standard_normal(n) * (1.0 if alpha >= 10 else 3.0)).astype(np.float32)
        v = np.sort(s.astype(np.float64))
        if n < 2 or np.min(np.diff(v)) >= 1e-3 / alpha:
            return s
    raise AssertionError("no distinct scores")


def main():
    torch.set_num_threads(1)
    rng = np.random.default_rng(SEED)
    torch.manual_seed(SEED)
    store = {}
    count = skipped = 0

    def put(fam, case, preds, labels, alpha, combos):
        nonlocal count, skipped
        P2, Y2 = np.atleast_2d(preds), np.atleast_2d(labels)
        B, n = P2.shape
        rows = []
        for metric, opt_ideal, top_k in combos:
            k = top_k or None
            if metric == "nERR" and k is not None and k > n:
                try:
                    run_reference(metric, P2, Y2, alpha, k, bool(opt_ideal), torch.float64)
                except AssertionError:
                    skipped += 1
                    continue
                raise AssertionError(f"{fam}/{case}: nERR ran with top_k={k} > n={n}")
            if metric == "nERR" and B > 1:
                # the reference's batched nERR divides batch_err [B] by batch_ideal_err [B, 1] (:184, :208): a [B, B] broadcast that couples
                # the queries, as ApproxNDCG's does.  The contract is the reference one query at a time: B runs, summed.  Every query of
                # the batch holds the batch's maximum label (asserted), so each run's torch.max(batch_std_labels) is the batch-wide value.
                assert (Y2.max(1) == Y2.max()).all()

                def per_query(dtype):
                    runs = [run_reference(metric, P2[q:q + 1], Y2[q:q + 1], alpha, k, bool(opt_ideal), dtype) for q in range(B)]
                    return sum(r[0] for r in runs), np.concatenate([r[1] for r in runs]), all(r[2] for r in runs), np.concatenate([r[3] for r in runs])
                l64, g64, z64, o64 = per_query(torch.float64)
                l32, g32, z32, o32 = per_query(torch.float32)
            else:
                l64, g64, z64, o64 = run_reference(metric, P2, Y2, alpha, k, bool(opt_ideal), torch.float64)
                l32, g32, z32, o32 = run_reference(metric, P2, Y2, alpha, k, bool(opt_ideal), torch.float32)
            assert z64 == z32, (fam, case, metric)
            if fam == "main":
                assert np.array_equal(o64, o32), f"{fam}/{case}: the fp32 and float64 rank orders differ"
            valid = np.ones(B, np.float32)
            if not opt_ideal and k is not None:
                for q in range(B):                               # the reference's own flag for the query alone
                    valid[q] = 0.0 if run_reference(metric, P2[q:q + 1], Y2[q:q + 1], alpha, k, False, torch.float64)[2] else 1.0
            rows.append(((METRICS.index(metric), int(opt_ideal), top_k or 0), np.concatenate([[l32], g32.reshape(-1)]).astype(np.float32),
                         np.concatenate([[l64], g64.reshape(-1)]).astype(np.float64), valid))
            count += 1
        for k_, v in dict(preds=preds, labels=labels, alpha=np.float32(alpha), max_label=np.float32(Y2.max()),
                          combos=np.asarray([r[0] for r in rows], np.int32), res32=np.stack([r[1] for r in rows]),
                          res64=np.stack([r[2] for r in rows]), valid=np.stack([r[3] for r in rows])).items():
            store[f"{fam}/{case}/{k_}"] = np.asarray(v)
        print(f"{fam}/{case}: {len(rows)} runs", flush=True)

    def forms(n, top_ks, metrics=METRICS):
        return [(m, oi, k) for m in metrics for oi in (1, 0) for k in top_ks]

    # ---------------------------------------------------------------- main
    for n in (2, 3, 17, 64, 65, 130):
        for alpha in (1.0, 10.0):
            put("main", f"n{n}_a{int(alpha)}", distinct_scores(rng, n, alpha), labels_mslr(rng, n), alpha, forms(n, (0, 1, 5, n)))

    # ---------------------------------------------------------------- edge
    one = np.asarray([0.3], np.float32)
    put("edge", "n1_rel", one, np.asarray([2.0], np.float32), 10.0, forms(1, (0, 1)))
    put("edge", "n1_norel", one, np.asarray([0.0], np.float32), 10.0, forms(1, (0, 1)))
    put("edge", "norel_n5", distinct_scores(rng, 5, 10.0), np.zeros(5, np.float32), 10.0, forms(5, (0, 1, 3, 5)))
    # relevant documents only beyond position K: presorted labels (3, 1, 0, ...), scores that rank those two last
    n = 8
    s = np.sort(distinct_scores(rng, n, 10.0)).astype(np.float32)            # ascending: document 0 scores lowest
    put("edge", "rel_beyond_k", s, np.asarray([3, 1, 0, 0, 0, 0, 0, 0], np.float32), 10.0, forms(n, (2, 5)))
    put("edge", "topk_gt_n", distinct_scores(rng, 4, 10.0), np.asarray([2, 1, 0, 0], np.float32), 10.0, forms(4, (10,), ("P", "AP", "nDCG")))
    # a batch of 3: query 1 is filtered at top_k = 2 (its relevant documents rank last), every query holds the maximum label (nERR: see put())
    n = 6
    sb = np.stack([distinct_scores(rng, n, 10.0), np.sort(distinct_scores(rng, n, 10.0)), distinct_scores(rng, n, 10.0)]).astype(np.float32)
    yb = np.asarray([[4, 2, 1, 0, 0, 0], [4, 1, 0, 0, 0, 0], [4, 1, 1, 0, 0, 0]], np.float32)
    sb[0] = -np.sort(-sb[0])                                                 # query 0 ranks its relevant documents first
    sb[2, 0] = sb[2].max() + 0.5                                             # query 2 ranks a relevant document first
    put("edge", "batch3", sb, yb, 10.0, [(m, 0, 2) for m in METRICS] + [(m, 1, 2) for m in METRICS])

    out = os.path.join(HERE, "smooth_metric.npz")
    with zipfile.ZipFile(out, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.array(store[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"wrote {out}: {count} runs ({skipped} nERR forms with top_k > n do not run), {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
