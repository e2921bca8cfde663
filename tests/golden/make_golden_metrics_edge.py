#!/usr/bin/env python3
"""Generate tests/golden/metrics_edge.npz by RUNNING THE REFERENCE ITSELF: the Evaluator prologue (torch.sort, gather, the ideal sort,
ptranking/base/ranker.py:46-60) and ptranking/metric/adhoc/adhoc_metric.py's torch_*_at_ks / torch_*_at_k on the inputs the older
fixture (metrics.npz, make_golden.py gen_metrics) never holds.

Run on the build machine, never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics_edge.py

It imports wildltr/ptranking read-only from $PTRANKING_REF, default /root/reference (only inside generate(): load() and write_npz() work
without it).  Every case is a rectangular batch (the reference has no list lengths) of at most 300 documents:

  edge/<case>/xy      fp32 [2, B, L]: preds, labels
  edge/<case>/spec    float64 [4 + nk]: presort, permutation (LABEL_TYPE.Permutation: nDCG's gain is the label; no nERR), k1, max_label
                      (NaN = None, the batch maximum), then the cut-offs in the order given to the reference
  edge/<case>/out     fp32 [8, B, nk]: rows 0-3 torch_ndcg_at_ks, torch_nerr_at_ks, torch_ap_at_ks, torch_precision_at_ks; rows 4-7, column 0:
                      the single-cut-off functions torch_*_at_k at k1 (<= L: torch_ndcg_at_k does not clamp).  The nERR rows of a Permutation
                      case are NaN.
(three members per case keep the archive below metrics.npz: a zip member costs about 200 bytes.)  load() unpacks them into the fields
preds, labels, ks, presort, permutation, max_label, k1, ndcg, nerr, ap, p, ndcg_k, nerr_k, ap_k, p_k.

Cases: a list with no relevant document (`norel`), relevant documents only beyond the cut-offs (`beyond`), cut-offs larger than the list
mixed with fitting ones in sorted and unsorted order (`over_sorted`, `over_unsorted`), cut-offs 64 / 65 / 128 / 129 on 130 and 300
documents, Permutation labels, max_label None / 4 / 2 (below the labels) / 2.5, fractional labels, and NaN scores.  torch.sort is not
stable among NaNs on longer rows (NaNs come first, but not in index order from about 70 documents on), so in the NaN cases every
NaN-scored document of a list carries ONE and the same label: the reference's answer does not depend on their order.
The archive is written with fixed zip timestamps and sorted members so that a rerun reproduces it byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = "metrics_edge.npz"
SEED = 251
MSLR_P = [0.5, 0.3, 0.13, 0.05, 0.02]
YAHOO_P = [0.25, 0.35, 0.25, 0.1, 0.05]


def write_npz(path, store):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.array(store[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


NAMES = ("ndcg", "nerr", "ap", "p")


def load(path=None):
    """{case: {field: array}} with the fields of the module docstring."""
    z = np.load(path or os.path.join(HERE, FILE), allow_pickle=False)
    out = {}
    for case in sorted({key.split("/")[1] for key in z.files}):
        xy, spec, o = z[f"edge/{case}/xy"], z[f"edge/{case}/spec"], z[f"edge/{case}/out"]
        c = dict(preds=xy[0], labels=xy[1], presort=np.int32(spec[0]), permutation=np.int32(spec[1]), k1=np.int32(spec[2]),
                 max_label=np.float32(spec[3]), ks=spec[4:].astype(np.int32))
        for i, m in enumerate(NAMES):
            if m == "nerr" and int(spec[1]):
                continue
            c[m], c[m + "_k"] = o[i], o[4 + i][:, :1]
        out[case] = c
    return out


def inputs():
    """[(case, preds, labels, ks, presort, permutation, max_label or None, k1)] — seeded, reference-free."""
    rng = np.random.default_rng(SEED)
    out = []

    def draw(B, L, p=MSLR_P, relevant=True):
        s = rng.standard_normal((B, L)).astype(np.float32)
        y = rng.choice(5, size=(B, L), p=p).astype(np.float32)
        if relevant:
            y[:, 0] = np.maximum(y[:, 0], 1.0)
        return s, y

    def add(case, s, y, ks, presort=False, permutation=False, max_label=None, k1=5):
        if presort:
            y = -np.sort(-y, axis=1)
        out.append((case, s, y, [int(k) for k in ks], presort, permutation, max_label, int(k1)))

    s, y = draw(3, 12)
    y[1] = 0.0
    add("norel", s, y, [1, 3, 5, 10])
    s, y = draw(2, 5)
    y[:] = 0.0
    y[0, 2] = 3.0
    add("norel_presort", s, y, [1, 2, 5], presort=True, max_label=4.0, k1=2)
    s, y = draw(2, 40, YAHOO_P)
    for q in range(2):
        o = np.argsort(-s[q], kind="stable")
        y[q, o[:20]] = 0.0
        y[q, o[-1]] = 2.0
    add("beyond", s, y, [1, 5, 10, 20], k1=10)
    s, y = draw(3, 30, YAHOO_P)
    add("over_sorted", s, y, [1, 5, 10, 30, 31, 50], k1=30)
    add("over_unsorted", s, y, [50, 10, 1, 31, 30, 5], k1=30)
    add("over_presort", s, y, [31, 30, 29, 1], presort=True, k1=29)
    for L in (130, 300):
        s, y = draw(2 if L == 130 else 1, L)
        add(f"chunk_n{L}", s, y, [1, 10, 64, 65, 128, 129], k1=65)
        add(f"chunk_n{L}_presort", s, y, [129, 128, 65, 64], presort=True, k1=129)
    for L in (9, 130):
        s = rng.standard_normal((2, L)).astype(np.float32)
        y = np.stack([rng.permutation(L) + 1 for _ in range(2)]).astype(np.float32)
        add(f"perm_n{L}", s, y, [1, 5, 64, 65, 128, L], permutation=True, k1=5)
    s, y = draw(2, 50, YAHOO_P)
    y[0, 3] = 4.0
    for tag, ml in (("none", None), ("4", 4.0), ("2", 2.0), ("2p5", 2.5)):
        add(f"maxlabel_{tag}", s, y, [1, 3, 10, 50], max_label=ml, k1=10)
    s, _ = draw(2, 64)
    add("frac", s, (4.0 * rng.random((2, 64))).astype(np.float32), [1, 2, 5, 10, 63, 64], max_label=4.0)
    add("frac_maxlabel_none", s, (4.0 * rng.random((2, 64))).astype(np.float32), [1, 5, 64], k1=64)
    # NaN scores: every NaN-scored document of a list carries one and the same label
    for case, L, count, lab in (("nan_one_n8", 8, 1, 2.0), ("nan_several_n70", 70, 9, 1.0), ("nan_several_n200", 200, 40, 0.0),
                                ("nan_nm1_n130", 130, 129, 1.0), ("nan_all_n20", 20, 20, 2.0)):
        s, y = draw(2, L, YAHOO_P)
        for q in range(2):
            pos = rng.permutation(L)[:count]
            s[q, pos] = np.nan
            y[q, pos] = lab
        add(case, s, y, [k for k in (1, 5, 10, 64, 65, 129) if k <= L] + [L, L + 1], k1=5)
    s, y = draw(2, 16)
    s[0, 3], s[0, 9], s[1, 0], s[1, 15] = np.inf, -np.inf, -np.inf, np.inf
    add("inf_n16", s, y, [1, 2, 15, 16])
    return out


def generate():
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.dont_write_bytecode = True
    ref = os.environ.get("PTRANKING_REF") or "/root/reference"
    if not os.path.isdir(ref):
        raise SystemExit(f"no wildltr/ptranking checkout at {ref} (set PTRANKING_REF)")
    if ref not in sys.path:
        sys.path.insert(0, ref)
    import torch
    from ptranking.data.data_utils import LABEL_TYPE
    from ptranking.metric.adhoc.adhoc_metric import (
        torch_ndcg_at_k, torch_ndcg_at_ks, torch_ap_at_k, torch_ap_at_ks,
        torch_nerr_at_k, torch_nerr_at_ks, torch_precision_at_k, torch_precision_at_ks)

    store = {}
    for case, s, y, ks, presort, permutation, max_label, k1 in inputs():
        assert s.shape[1] <= 300
        nan = np.isnan(s)
        for q in range(s.shape[0]):
            assert len(np.unique(y[q][nan[q]])) <= 1, "NaN-scored documents of a list must share one label"
        tp, tl = torch.from_numpy(s), torch.from_numpy(y)
        _, idx = torch.sort(tp, dim=1, descending=True)                        # ranker.py:50
        sys_sorted = torch.gather(tl, dim=1, index=idx)                         # ranker.py:52
        ideal = tl if presort else torch.sort(tl, dim=1, descending=True)[0]    # ranker.py:53-56
        lt = LABEL_TYPE.Permutation if permutation else LABEL_TYPE.MultiLabel
        out = dict(ndcg=torch_ndcg_at_ks(sys_sorted, ideal, ks=ks, label_type=lt), ap=torch_ap_at_ks(sys_sorted, ideal, ks=ks),
                   p=torch_precision_at_ks(sys_sorted, ks=ks),
                   ndcg_k=torch_ndcg_at_k(sys_sorted, ideal, k=k1, label_type=lt), ap_k=torch_ap_at_k(sys_sorted, ideal, k=k1),
                   p_k=torch_precision_at_k(sys_sorted, k=k1))
        if not permutation:
            out["nerr"] = torch_nerr_at_ks(sys_sorted, ideal, ks=ks, label_type=lt, max_label=max_label)
            out["nerr_k"] = torch_nerr_at_k(sys_sorted, ideal, k=k1, label_type=lt, max_label=max_label, device="cpu")
        key = f"edge/{case}"
        B, nk = s.shape[0], len(ks)
        packed = np.zeros((8, B, nk), np.float32)
        for i, m in enumerate(NAMES):
            if m in out:
                packed[i], packed[4 + i][:, 0] = out[m].numpy(), out[m + "_k"].numpy()[:, 0]
            else:
                packed[i], packed[4 + i] = np.nan, np.nan
        store[f"{key}/xy"] = np.stack([s, y]).astype(np.float32)
        store[f"{key}/spec"] = np.asarray([presort, permutation, k1, np.nan if max_label is None else max_label] + list(ks), np.float64)
        store[f"{key}/out"] = packed
    return store


def main():
    store = generate()
    out = os.path.join(HERE, FILE)
    write_npz(out, store)
    print(f"wrote {out}: {len(store)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
