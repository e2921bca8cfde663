#!/usr/bin/env python3
"""Generate tests/golden/gauss_metric.npz by RUNNING THE REFERENCE ITSELF: get_expected_rank / get_expected_rank_const
(ptranking/ltr_diversification/util/prob_utils.py:62-101), then precision_ / AP_ / nERR_ / nDCG_as_opt_objective
(ptranking/metric/smooth_metric/metric_as_opt_objective.py), then autograd with respect to the means AND the variances, in float64 AND in fp32
— the composition every one of the four objectives carries as a commented-out line (`#batch_expt_ranks = get_expected_rank(...)`).

Run on the build machine, never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gauss_metric.py

It imports wildltr/ptranking read-only from $PTRANKING_REF, default /root/reference.  Layout (<family>/<case>/<field>):

  mus fp32 [n] (batch case: [B, n]), vars fp32 of the same shape (absent in the constant-variance family, which has const_std instead: the
  reference's `const_var`, a standard deviation), labels fp32 (presorted, descending), max_label,
  combos int32 [R, 3] = (metric 0 P / 1 AP / 2 nERR / 3 nDCG, opt_ideal, top_k with 0 = None) per row,
  res64 float64 [R, 1 + 2 B n] = (loss, d loss / d mus, d loss / d vars) of the reference on float64 tensors ([R, 1 + B n] in the
  constant-variance family), res32 fp32 the same on fp32 tensors,
  valid fp32 [R, B]: 0 where the reference's pos_inds filter drops the query (loss and gradients are then recorded as 0), 1 elsewhere,
  ranks64 float64 [B, n] the expected ranks and order int64 [B, n] = torch.sort(ranks64)[1], the order the re-sorted forms weigh by.

  main   one query each: n in {1, 2, 3, 17, 64, 65, 130} x three families — `wide` (variances in [0.05, 1.05], means 2 N(0, 1)), `head` (the
         range of a learned sigmoid * limit_delta head: variances in [1e-4, 1e-2], means 0.5 N(0, 1)), `const` (const_std = 0.5, means
         2 N(0, 1)); 4 metrics x opt_ideal 0 / 1 x top_k in {None, 1, 5, n}.  The draws are repeated until adjacent sorted float64 expected
         ranks are more than 1e-3 apart, and the fp32 and float64 orders are asserted equal.
         nERR with top_k > n does not run in the reference (torch_rankwise_err asserts); that is asserted and the combination left out.
  edge   n = 1 without a relevant document, a list without a relevant document in every form, relevant documents only beyond position K,
         top_k > n for P, AP and nDCG, and a batch of 3 with one filtered query (valid matters).  nERR on that batch is recorded one query at
         a time and summed, as make_golden_smooth.py does and for its reason.

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
from ptranking.ltr_diversification.util.prob_utils import get_expected_rank, get_expected_rank_const
from ptranking.metric.smooth_metric.metric_as_opt_objective import (AP_as_opt_objective, nDCG_as_opt_objective, nERR_as_opt_objective,
                                                                    precision_as_opt_objective)

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 211
MSLR_P = [0.5147, 0.3250, 0.1339, 0.0183, 0.0081]   # testing/data/testing_data_utils.py:326, as make_golden.py
METRICS = ("P", "AP", "nERR", "nDCG")
CONST_STD = 0.5
MIN_GAP = 1e-3


def expected_ranks(m, v, const_std):
    if v is None:
        return get_expected_rank_const(batch_mus=m, const_var=torch.tensor(const_std, dtype=m.dtype))
    return get_expected_rank(batch_mus=m, batch_vars=v)


def run_reference(metric, mus, vars_, const_std, labels, top_k, opt_ideal, dtype):
    """-> (loss, grad_mu [B, n], grad_var [B, n] or None, filtered, ranks [B, n], order [B, n]) for a [B, n] batch."""
    m = torch.from_numpy(mus).to(dtype).requires_grad_(True)
    v = None if vars_ is None else torch.from_numpy(vars_).to(dtype).requires_grad_(True)
    y = torch.from_numpy(labels).to(dtype)
    ranks = expected_ranks(m, v, const_std)
    kw = dict(top_k=top_k, batch_smooth_ranks=ranks, batch_std_labels=y, presort=True, opt_ideal=opt_ideal, device="cpu")
    if metric == "P":
        loss, zero = precision_as_opt_objective(**kw)
    elif metric == "AP":
        loss, zero = AP_as_opt_objective(**kw)
    elif metric == "nERR":
        loss, zero = nERR_as_opt_objective(**kw)
    else:
        loss, zero = nDCG_as_opt_objective(label_type=LABEL_TYPE.MultiLabel, **kw)
    rk = ranks.detach().numpy().astype(np.float64)
    order = torch.sort(ranks.detach(), dim=1)[1].numpy()
    zeros = np.zeros(mus.shape)
    if zero:
        return 0.0, zeros, None if v is None else zeros, True, rk, order
    loss.backward()
    g = lambda t: zeros if t.grad is None else t.grad.detach().numpy().astype(np.float64)
    return float(loss.detach()), g(m), None if v is None else g(v), False, rk, order


def labels_mslr(rng, n, relevant=True):
    y = rng.choice(len(MSLR_P), size=n, p=np.asarray(MSLR_P) / np.sum(MSLR_P)).astype(np.float32)
    if relevant and y.max() < 1:
        y[rng.integers(n)] = 1.0
    return -np.sort(-y)


def ranks64(mus, vars_, const_std):
    m = torch.from_numpy(np.atleast_2d(mus)).to(torch.float64)
    v = None if vars_ is None else torch.from_numpy(np.atleast_2d(vars_)).to(torch.float64)
    return expected_ranks(m, v, const_std).numpy()


def draw(rng, n, family, ascending=False):
    """(mus fp32 [n], vars fp32 [n] or None), redrawn until adjacent sorted float64 expected ranks are more than MIN_GAP apart."""
    for _ in range(1000):
        if family == "head":
            m, v = 0.5 * rng.standard_normal(n), rng.uniform(1e-4, 1e-2, n)
        else:
            m, v = 2.0 * rng.standard_normal(n), rng.uniform(0.05, 1.05, n)
        m = m.astype(np.float32)
        if ascending:
            m = np.sort(m)
        v = None if family == "const" else v.astype(np.float32)
        r = np.sort(ranks64(m, v, CONST_STD)[0])
        if n < 2 or np.min(np.diff(r)) > MIN_GAP:
            return m, v
    raise AssertionError("no separated expected ranks")


def main():
    torch.set_num_threads(1)
    rng = np.random.default_rng(SEED)
    torch.manual_seed(SEED)
    store = {}
    count = skipped = 0

    def put(fam, case, mus, vars_, labels, combos):
        nonlocal count, skipped
        M2, Y2 = np.atleast_2d(mus), np.atleast_2d(labels)
        V2 = None if vars_ is None else np.atleast_2d(vars_)
        B, n = M2.shape
        rows = []
        sl = lambda a, q: None if a is None else a[q:q + 1]

        def flat(l, gm, gv):
            return np.concatenate([[l], gm.reshape(-1)] + ([] if gv is None else [gv.reshape(-1)]))

        for metric, opt_ideal, top_k in combos:
            k = top_k or None
            if metric == "nERR" and k is not None and k > n:
                try:
                    run_reference(metric, M2, V2, CONST_STD, Y2, k, bool(opt_ideal), torch.float64)
                except AssertionError:
                    skipped += 1
                    continue
                raise AssertionError(f"{fam}/{case}: nERR ran with top_k={k} > n={n}")
            if metric == "nERR" and B > 1:
                assert (Y2.max(1) == Y2.max()).all()

                def per_query(dtype):
                    runs = [run_reference(metric, M2[q:q + 1], sl(V2, q), CONST_STD, Y2[q:q + 1], k, bool(opt_ideal), dtype) for q in range(B)]
                    return (sum(r[0] for r in runs), np.concatenate([r[1] for r in runs]),
                            None if V2 is None else np.concatenate([r[2] for r in runs]), all(r[3] for r in runs),
                            np.concatenate([r[4] for r in runs]), np.concatenate([r[5] for r in runs]))
                r64, r32 = per_query(torch.float64), per_query(torch.float32)
            else:
                r64 = run_reference(metric, M2, V2, CONST_STD, Y2, k, bool(opt_ideal), torch.float64)
                r32 = run_reference(metric, M2, V2, CONST_STD, Y2, k, bool(opt_ideal), torch.float32)
            assert r64[3] == r32[3], (fam, case, metric)
            assert np.array_equal(r64[5], r32[5]), f"{fam}/{case}: the fp32 and float64 rank orders differ"
            valid = np.ones(B, np.float32)
            if not opt_ideal and k is not None:
                for q in range(B):                               # the reference's own flag for the query alone
                    valid[q] = 0.0 if run_reference(metric, M2[q:q + 1], sl(V2, q), CONST_STD, Y2[q:q + 1], k, False, torch.float64)[3] else 1.0
            rows.append(((METRICS.index(metric), int(opt_ideal), top_k or 0), flat(*r32[:3]).astype(np.float32), flat(*r64[:3]).astype(np.float64),
                         valid))
            count += 1
        rk = ranks64(M2, V2, CONST_STD)
        fields = dict(mus=mus, labels=labels, max_label=np.float32(Y2.max()), combos=np.asarray([r[0] for r in rows], np.int32),
                      res32=np.stack([r[1] for r in rows]), res64=np.stack([r[2] for r in rows]), valid=np.stack([r[3] for r in rows]),
                      ranks64=rk, order=np.argsort(rk, axis=1, kind="stable").astype(np.int64))
        assert np.array_equal(fields["order"], torch.sort(torch.from_numpy(rk), dim=1)[1].numpy())
        if vars_ is None:
            fields["const_std"] = np.float32(CONST_STD)
        else:
            fields["vars"] = vars_
        for k_, v in fields.items():
            store[f"{fam}/{case}/{k_}"] = np.asarray(v)
        print(f"{fam}/{case}: {len(rows)} runs", flush=True)

    def forms(n, top_ks, metrics=METRICS):
        return [(m, oi, k) for m in metrics for oi in (1, 0) for k in top_ks]

    # ---------------------------------------------------------------- main
    for n in (1, 2, 3, 17, 64, 65, 130):
        for family in ("wide", "head", "const"):
            m, v = draw(rng, n, family)
            put("main", f"{family}_n{n}", m, v, labels_mslr(rng, n), forms(n, sorted({0, 1, 5, n})))

    # ---------------------------------------------------------------- edge
    one = np.asarray([0.3], np.float32)
    put("edge", "n1_norel", one, np.asarray([0.2], np.float32), np.asarray([0.0], np.float32), forms(1, (0, 1)))
    put("edge", "n1_norel_const", one, None, np.asarray([0.0], np.float32), forms(1, (0, 1)))
    m, v = draw(rng, 5, "wide")
    put("edge", "norel_n5", m, v, np.zeros(5, np.float32), forms(5, (0, 1, 3, 5)))
    # relevant documents only beyond position K: presorted labels (3, 1, 0, ...), means ascending so that those two rank last
    n = 8
    for _ in range(1000):
        m, v = draw(rng, n, "head", ascending=True)
        if np.all(np.argsort(ranks64(m, v, CONST_STD)[0])[-2:][::-1] == [0, 1]):
            break
    else:
        raise AssertionError("rel_beyond_k")
    put("edge", "rel_beyond_k", m, v, np.asarray([3, 1, 0, 0, 0, 0, 0, 0], np.float32), forms(n, (2, 5)))
    m, v = draw(rng, 4, "wide")
    put("edge", "topk_gt_n", m, v, np.asarray([2, 1, 0, 0], np.float32), forms(4, (10,), ("P", "AP", "nDCG")))
    # a batch of 3: query 1 is filtered at top_k = 2 (its relevant documents rank last), every query holds the maximum label (nERR: see put())
    n = 6
    rows = [draw(rng, n, "head", ascending=True) for _ in range(3)]
    mb, vb = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    mb[0], mb[2] = mb[0][::-1].copy(), mb[2][::-1].copy()                    # queries 0 and 2 rank their relevant documents first
    yb = np.asarray([[4, 2, 1, 0, 0, 0], [4, 1, 0, 0, 0, 0], [4, 1, 1, 0, 0, 0]], np.float32)
    rk = ranks64(mb, vb, CONST_STD)
    assert np.min(np.diff(np.sort(rk, axis=1), axis=1)) > MIN_GAP
    put("edge", "batch3", mb, vb, yb, [(m_, 0, 2) for m_ in METRICS] + [(m_, 1, 2) for m_ in METRICS])
    assert store["edge/batch3/valid"][0].tolist() == [1.0, 0.0, 1.0]
    assert (store["edge/rel_beyond_k/valid"][[c[1] == 0 for c in store["edge/rel_beyond_k/combos"]]] == 0.0).all()

    out = os.path.join(HERE, "gauss_metric.npz")
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
