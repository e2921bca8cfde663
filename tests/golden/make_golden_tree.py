#!/usr/bin/env python3
"""Generate tests/golden/tree.npz by RUNNING THE REFERENCE ITSELF: the custom LightGBM objectives of ptranking/ltr_tree/util/lightgbm_util.py.

Run on the build machine, never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tree.py

It imports wildltr/ptranking read-only from $PTRANKING_REF, default /root/reference.  The reference's wrappers call group.astype(np.int),
which numpy >= 1.24 no longer has: this process sets np.int = int before the import; the reference is not edited.

Every score is fp32-representable and PAIRWISE DISTINCT within its query (asserted): np.flip(np.argsort(preds)) breaks ties in an
implementation-defined way, so ties are never compared against the reference.  The reference runs in float64 on those values.

  pq/n<N>/...      preds fp32 [n], labels fp32 [n]; combos int32 [24, 3] = (pair type 0 All 1 NoTies 2 No00 3 00, weighting 0 none 1 DeltaNDCG
                   2 DeltaGain, epsilon) per row; res float64 [24, 2, n] = (grad, hess) of per_query_gradient_hessian_lambda; listnet float64
                   [2, 2, n] = (grad, hess) of per_query_gradient_hessian_listnet for gain_type 'Power', 'Label'.  n in 1, 2, 3, 17, 64, 65, 130.
  wr/ragged/...    preds, labels fp32 [98], group int32 = [12, 1, 18, 64, 3]; res float64 [6, 2, 98] = (grad, hess) of the six wrappers in the
                   order of `names` (the *_fobj forms through an object with get_label() / get_group()).
  edge/<name>/...  preds, labels, combos, res as pq: 'equal_labels' (NoTies under the three weightings: no pair, exactly 0), 'norel' (no
                   relevant document; All pairs under DeltaNDCG: NaN, as stored), 'nanscore' (one NaN score; All and NoTies pairs, unweighted:
                   what the reference returns, NaN included — under NoTies it keeps the documents that share the NaN document's label finite,
                   where the product gives the whole list NaN).
The archive is written with fixed zip timestamps so that a rerun reproduces it byte for byte.
"""
import io
import os
import sys
import warnings
import zipfile

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = os.environ.get("PTRANKING_REF") or "/root/reference"
if not os.path.isdir(REF):
    raise SystemExit(f"no wildltr/ptranking checkout at {REF} (set PTRANKING_REF)")
sys.path.insert(0, REF)

import numpy as np

if not hasattr(np, "int"):
    np.int = int                                   # lightgbm_util.py:199 etc.; this process only

from ptranking.ltr_tree.util import lightgbm_util as LU

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 211
PAIR_TYPES = ("All", "NoTies", "No00", "00")
WEIGHTINGS = (None, "DeltaNDCG", "DeltaGain")
SIZES = (1, 2, 3, 17, 64, 65, 130)
GROUP = (12, 1, 18, 64, 3)
NAMES = ("lightgbm_custom_obj_ranknet", "lightgbm_custom_obj_lambdarank", "lightgbm_custom_obj_listnet", "lightgbm_custom_obj_ranknet_fobj",
         "lightgbm_custom_obj_lambdarank_fobj", "lightgbm_custom_obj_listnet_fobj")


class Dataset:
    """What the *_fobj wrappers read of a lightgbm.Dataset."""

    def __init__(self, labels, group):
        self._labels, self._group = labels, group

    def get_label(self):
        return self._labels

    def get_group(self):
        return self._group


def draw(rng, n, relevant=True):
    y = rng.choice(5, size=n, p=[0.5, 0.3, 0.13, 0.05, 0.02]).astype(np.float32)
    if relevant and n >= 2:
        y[rng.integers(0, n)] = 2.0
        if len(np.unique(y)) == 1:
            y[(int(np.argmax(y)) + 1) % n] = 0.0
    for _ in range(100):
        s = (0.8 * y + 1.5 * rng.standard_normal(n)).astype(np.float32)
        if len(np.unique(s)) == n:
            return s, y
    raise AssertionError("could not draw distinct scores")


def distinct(s, group):
    head = 0
    for g in group:
        v = s[head:head + g]
        v = v[~np.isnan(v)]
        assert len(np.unique(v)) == len(v), "scores must be pairwise distinct within a query"
        head += g


def run_lambda(s, y, pt, w, eps):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        grad, hess = LU.per_query_gradient_hessian_lambda(preds=s.astype(np.float64), labels=y.astype(np.float64), first_order=False,
                                                          weighting=w if w else False, weighting_type=w if w else "DeltaNDCG",
                                                          pair_type=pt, epsilon=eps)
    return np.stack([grad, hess])


def main():
    assert LU.FIRST_ORDER is False
    rng = np.random.default_rng(SEED)
    store = {}
    grid = [(p, w, e) for p in range(4) for w in range(3) for e in (1.0, 2.0)]
    for n in SIZES:
        s, y = draw(rng, n)
        distinct(s, [n])
        key = f"pq/n{n}"
        store[f"{key}/preds"], store[f"{key}/labels"] = s, y
        store[f"{key}/combos"] = np.asarray([(p, w, int(e)) for p, w, e in grid], np.int32)
        store[f"{key}/res"] = np.stack([run_lambda(s, y, PAIR_TYPES[p], WEIGHTINGS[w], e) for p, w, e in grid])
        ln = [LU.per_query_gradient_hessian_listnet(preds=s.astype(np.float64), labels=y.astype(np.float64), gain_type=g, first_order=False)
              for g in ("Power", "Label")]
        store[f"{key}/listnet"] = np.stack([np.stack(r) for r in ln])
        print(f"{key}: {len(grid)} runs", flush=True)

    parts = [draw(rng, g) for g in GROUP]
    s, y = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    group = np.asarray(GROUP, np.int32)
    distinct(s, GROUP)
    s64, y64 = s.astype(np.float64), y.astype(np.float64)
    res = []
    for name in NAMES:
        fn = getattr(LU, name)
        out = fn(s64, Dataset(y64, group)) if name.endswith("_fobj") else fn(labels=y64, preds=s64, group=group)
        res.append(np.stack(out))
    store["wr/ragged/preds"], store["wr/ragged/labels"], store["wr/ragged/group"] = s, y, group
    store["wr/ragged/res"] = np.stack(res)
    store["wr/ragged/names"] = np.asarray(NAMES)

    def edge(name, s, y, combos):
        distinct(s, [len(s)])
        store[f"edge/{name}/preds"], store[f"edge/{name}/labels"] = s, y
        store[f"edge/{name}/combos"] = np.asarray([(p, w, int(e)) for p, w, e in combos], np.int32)
        store[f"edge/{name}/res"] = np.stack([run_lambda(s, y, PAIR_TYPES[p], WEIGHTINGS[w], e) for p, w, e in combos])

    s, _ = draw(rng, 9)
    edge("equal_labels", s, np.full(9, 2.0, np.float32), [(1, w, 1.0) for w in range(3)])
    s, _ = draw(rng, 7)
    edge("norel", s, np.zeros(7, np.float32), [(0, 1, 1.0), (3, 1, 1.0), (2, 1, 1.0)])
    s, y = draw(rng, 8)
    s[3] = np.nan
    edge("nanscore", s, y, [(0, 0, 1.0), (1, 0, 1.0)])
    assert np.isnan(store["edge/norel/res"][0]).all() and not store["edge/equal_labels/res"].any()

    out = os.path.join(HERE, "tree.npz")
    with zipfile.ZipFile(out, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.array(store[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"wrote {out}: {len(store)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
