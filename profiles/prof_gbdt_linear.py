#!/usr/bin/env python3
"""Measures what linear trees add to a boosting round: the moments, the solve and the linear add beside the growth of the same tree.

    python profiles/prof_gbdt_linear.py profiles/mi355x_gbdt_linear.json

Rows: ROWS x 136 standard-normal fp32 features (the row count of profiles/mi355x_gbdt_quant.json), a piecewise-linear target, squared
error, 31 leaves, max_bin 255.  TREES rounds with linear_tree on; the first is dropped as warm-up.  Per tree: the wall time of update()
around a device synchronise, and the device-event time of every entry point it calls (the binding's timing hook), summed into the three
new ones and the rest, which is the growth.  The same fit with the switch off gives the wall time of a tree without the fits.  The
gather's bytes are counted from the tree: per entry of a leaf of k regressors 4 k bytes of features, 8 of (g, h) and 4 of the row index.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, FEATURES, TREES = 795_428, 136, 9
PARAMS = dict(num_leaves=31, max_bin=255, min_data_in_leaf=50, learning_rate=0.1)
NEW = ("ptr_gbdt_linear_moments", "ptr_gbdt_linear_solve", "ptr_gbdt_add_tree_linear")


def fit(linear, X, y):
    import numpy as np
    import torch
    from ptranking_amd import _lib, gbdt, peaks
    b = gbdt.GBDT(dict(PARAMS, linear_tree=linear)).fit_bins(X)
    rows = []
    for _ in range(TREES):
        g, h = b.scores - y, torch.ones_like(y)
        torch.cuda.synchronize()
        _lib.TIMING = {}
        t0 = time.perf_counter()
        t = b.update(g, h)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ev = {name: sum(e0.elapsed_time(e1) for e0, e1 in pairs) for name, pairs in _lib.TIMING.items()}
        _lib.TIMING = None
        row = dict(wall_ms=wall, growth_kernels_ms=sum(v for k, v in ev.items() if k not in NEW), **{k[9:] + "_ms": ev[k] for k in NEW if k in ev})
        if linear:
            k = (t["leaf_features"] >= 0).sum(1)
            count = np.bincount(b.predict(X, num_iteration=len(b.trees), first_tree=len(b.trees) - 1, pred_leaf=True).cpu().numpy().reshape(-1), minlength=k.size)
            bytes_ = int((count * (4 * k + 12))[k > 0].sum())
            row.update(gather_bytes=bytes_, fitted_leaves=int((k > 0).sum()), mean_regressors=float(k[k > 0].mean()) if (k > 0).any() else 0.0,
                       gather_GBps=bytes_ / (ev[NEW[0]] * 1e-3) / 1e9, frac_of_hbm_peak=bytes_ / (ev[NEW[0]] * 1e-3) / (peaks.HBM_PEAK_GBPS * 1e9))
        rows.append(row)
    med = {k: statistics.median(r[k] for r in rows[1:]) for k in rows[0]}
    return dict(median=med, trees=rows[1:], host_reads=b.host_reads, loss=float(((b.scores - y) ** 2).mean()))


def main(out_path):
    import torch
    assert torch.cuda.is_available(), "prof_gbdt_linear.py measures on the GPU only"
    gen = torch.Generator(device="cuda").manual_seed(137)
    X = torch.randn((ROWS, FEATURES), device="cuda", generator=gen)
    y = (torch.where(X[:, 0] > 0, 2.0 * X[:, 1] + 1.0, -1.5 * X[:, 2]) + torch.where(X[:, 3] > 0.5, X[:, 0], torch.zeros_like(X[:, 0]))).contiguous()
    out = dict(rows=ROWS, features=FEATURES, params=PARAMS, trees=TREES - 1, results={("linear" if lin else "constant"): fit(lin, X, y) for lin in (False, True)},
               note="wall: host clock per update() around a device synchronise; *_ms: device events around each entry point, summed per tree; the "
                    "event hook slows the host, so wall is an upper figure; gather bytes are algorithmic (4 k + 12 per entry of a fitted leaf), "
                    "not cache-line traffic; first tree dropped")
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {m: round(v, 4) for m, v in r["median"].items()} for k, r in out["results"].items()}))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_gbdt_linear.json"))
