#!/usr/bin/env python3
"""Times ptr_ndeval_measures (csrc/ndeval.hip: ndeval's diversity measures + the greedy ideal ranking, float64) per launch.

    python profiles/prof_ndeval.py profiles/mi355x_ndeval.json

Shapes: a TREC-like evaluation (B = 200 topics, about 250 documents each in L = 256, T = 8 subtopics), a training-sized batch of short
lists (B = 4096, L = 64, T = 8) and the longest list the entry point serves, which is also its LDS limit (L = 4096, T = 32, B = 256: one
workgroup per compute unit).  Judgment density 0.1, scores rounded to one decimal, ks = (5, 10, 20), alpha = beta = 0.5.

Each shape is timed in PROCS fresh processes (this script re-run with --child; the parent never opens the GPU): the child warms the launch
up, then times ROUNDS single launches with device events around the entry point alone (outputs allocated beforehand) and a second set with
the measures switched off (ideal_order only: what div_ideal_order costs).  The JSON keeps every sample and reports the median of the
per-process medians.  There is no earlier implementation on the device to compare with — the reference shells out to a C program per run
file — so the numbers are stated and nothing is gated on them.  Not measured: the share of the greedy rounds, of the rank counting and of
the serial float64 sums inside the launch.
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [dict(name="trec_like", B=200, L=256, T=8, min_len=200), dict(name="short_lists", B=4096, L=64, T=8, min_len=64),
          dict(name="lds_limit", B=256, L=4096, T=32, min_len=4096)]
PROCS, ROUNDS, WARMUP = 3, 15, 3
KS = (5, 10, 20)


def child(shape):
    import ctypes as C

    import torch

    from ptranking_amd import _lib
    assert torch.cuda.is_available(), "prof_ndeval.py measures on the GPU only"
    dev = torch.device("cuda:0")
    B, L, T = shape["B"], shape["L"], shape["T"]
    g = torch.Generator(device="cpu").manual_seed(4404 + L)
    preds = (torch.randn(B, L, generator=g) * 2.0).mul(10).round().div(10).to(dev)
    rele = (torch.rand(B, T, L, generator=g) < 0.1).float().to(dev)
    lens = torch.randint(shape["min_len"], L + 1, (B,), generator=g, dtype=torch.int32).to(dev)
    per_k = torch.empty((B, 6, len(KS)), dtype=torch.float64, device=dev)
    per_q = torch.empty((B, 3), dtype=torch.float64, device=dev)
    S = torch.empty(B, dtype=torch.int32, device=dev)
    ideal = torch.empty((B, L), dtype=torch.int32, device=dev)
    ks = (C.c_int32 * len(KS))(*KS)
    stream = _lib.current_stream(dev)

    def launch(measures):
        _lib.call("ptr_ndeval_measures", _lib.ptr(preds), _lib.ptr(rele), _lib.ptr(lens), None, B, T, L, ks, len(KS), C.c_double(0.5),
                  C.c_double(0.5), 0, _lib.ptr(per_k) if measures else None, _lib.ptr(per_q) if measures else None, _lib.ptr(S), _lib.ptr(ideal),
                  stream)

    def timed(measures):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(measures)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    out = {}
    for key, measures in (("measures_ms", True), ("ideal_order_only_ms", False)):
        for _ in range(WARMUP):
            launch(measures)
        torch.cuda.synchronize()
        out[key] = [timed(measures) for _ in range(ROUNDS)]
    out["device"] = torch.cuda.get_device_name(0)
    out["torch"] = torch.__version__
    out["mean_actual_subtopics"] = float(S.float().mean())
    print(json.dumps(out), flush=True)


def main(out_path):
    rows, device, tver = [], None, None
    for shape in SHAPES:
        samples = {"measures_ms": [], "ideal_order_only_ms": []}
        for _ in range(PROCS):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(shape)], check=True, stdout=subprocess.PIPE,
                               text=True, timeout=300)
            res = json.loads(r.stdout.strip().splitlines()[-1])
            device, tver = res["device"], res["torch"]
            for k in samples:
                samples[k].append(res[k])
        med = {k: statistics.median(statistics.median(p) for p in v) for k, v in samples.items()}
        row = dict(shape, ks=list(KS), alpha=0.5, beta=0.5, density=0.1, processes=PROCS, rounds_per_process=ROUNDS, median_ms=med,
                   per_query_us={k: v * 1e3 / shape["B"] for k, v in med.items()}, all_samples_ms=samples)
        print(json.dumps({k: row[k] for k in ("name", "B", "L", "T", "median_ms")}), flush=True)
        rows.append(row)
    with open(out_path, "w") as f:
        json.dump(dict(device=device, torch=tver, entry_point="ptr_ndeval_measures", gated=False,
                       not_measured=["share of the greedy rounds", "share of the rank counting", "share of the serial float64 sums",
                                     "hardware counters"], shapes=rows), f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(json.loads(sys.argv[2]))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mi355x_ndeval.json"))
