#!/usr/bin/env python3
"""Generate tests/golden/ndeval.npz by RUNNING THE REFERENCE'S OWN ndeval (ptranking/metric/srd/ndeval.c, TREC ndeval 4.4).

Run on the build machine, never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ndeval.py

It compiles $PTRANKING_REF/ptranking/metric/srd/ndeval.c (default /root/reference) with the system C compiler into a temporary directory
— the binary is never kept — writes qrels and run files for synthetic topics, runs the program and stores what it printed:

  topics/<id>/...   rele uint8 [T, n] (graded judgments 0..3, subtopic by document), preds fp32 [n] (rounded to one decimal: ties),
                    lens = n, ntopics = T, noline uint8 [T] (1: the subtopic has NO qrels line at all — a gap in the subtopic indices;
                    a never-relevant subtopic with lines has an all-zero row and noline 0).
  runs/<name>/...   alpha, beta, depth_m (0: no -M), topics int32 [N] (ids of topics/), names [21] (the CSV header's measure names),
                    field_str [N, 21] / field_f64 [N, 21] = the per-topic CSV fields as printed / parsed, amean_str / amean_f64 [21].

qrels: `topic subtopic docno judgment`, docno = d%05d of the document index; a document whose column is all zero is an unjudged
document: with an even index it has no qrels line (it is not in ndeval's pool), with an odd one a single judgment-0 line.  Run:
`topic Q0 docno rank score runid` with explicit ranks in ptr_sort_desc's order (score descending, index ascending); -traditional is not used.

The archive is written only if tests/ndeval_ref.py reproduces EVERY per-topic field string for string, and with fixed zip timestamps, so a
rerun reproduces it byte for byte.
"""
import io
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("PTRANKING_REF") or "/root/reference"
NDEVAL_C = os.path.join(REF, "ptranking", "metric", "srd", "ndeval.c")
if not os.path.isfile(NDEVAL_C):
    raise SystemExit(f"no ndeval.c at {NDEVAL_C} (set PTRANKING_REF)")

import numpy as np

import ndeval_ref as NR

SEED = 4404


def make_topic(rng, T, n, density, special=None):
    rele = (rng.random((T, n)) < density).astype(np.uint8) * rng.integers(1, 4, (T, n)).astype(np.uint8)      # graded 0..3
    noline = np.zeros(T, np.uint8)
    if special == "zero":
        rele[:] = 0
    if special == "never" and T >= 2:
        rele[T // 2] = 0                                   # judged, never relevant
    if special == "gap" and T >= 3:
        rele[1] = 0
        noline[1] = 1                                      # no qrels line at all
        rele[T - 1, 0] = 2                                 # ... and the indices above the gap are in use
    if special == "unjudged" and n >= 4:
        rele[:, ::3] = 0                                   # a third of the run is unjudged
    preds = np.round(rng.standard_normal(n) * 2.0, 1).astype(np.float32)
    return dict(rele=rele, preds=preds, lens=np.int32(n), ntopics=np.int32(T), noline=noline)


def build_topics():
    rng = np.random.default_rng(SEED)
    topics = []
    dens = (0.05, 0.2, 0.6)
    for i, n in enumerate((1, 4, 5, 9, 10, 19, 20, 21)):
        topics.append(make_topic(rng, int(rng.integers(1, 21)), n, dens[i % 3]))
    for i in range(24):
        topics.append(make_topic(rng, int(rng.integers(1, 21)), int(rng.integers(1, 301)), dens[i % 3]))
    topics.append(make_topic(rng, 1, 300, 0.2))
    topics.append(make_topic(rng, 20, 1, 0.6))
    topics.append(make_topic(rng, 7, 57, 0.2, "never"))
    topics.append(make_topic(rng, 6, 83, 0.2, "gap"))
    topics.append(make_topic(rng, 5, 40, 0.2, "zero"))
    topics.append(make_topic(rng, 1, 1, 0.2, "zero"))
    topics.append(make_topic(rng, 9, 120, 0.6, "unjudged"))
    topics.append(make_topic(rng, 12, 260, 0.05, "unjudged"))
    short = len(topics)
    for n in (1024, 1025, 4096):
        topics.append(make_topic(rng, 32, n, 0.1))
    return topics, short


def write_files(tmp, ids, topics):
    qrels, run = os.path.join(tmp, "qrels.txt"), os.path.join(tmp, "run.txt")
    with open(qrels, "w") as fq, open(run, "w") as fr:
        for tid in ids:
            t = topics[tid]
            rele, preds = t["rele"], t["preds"]
            T, n = rele.shape
            for i in range(n):
                col = rele[:, i]
                if not col.any():
                    # an unjudged document; the topic's first document always keeps a line so that the topic exists in the qrels
                    if i % 2 == 1 or i == 0:
                        fq.write(f"{tid + 1} 0 d{i:05d} 0\n")
                    continue
                for j in range(T):
                    if not t["noline"][j]:
                        fq.write(f"{tid + 1} {j} d{i:05d} {int(col[j])}\n")
            for r, i in enumerate(NR.run_order(preds, n)):
                fr.write(f"{tid + 1} Q0 d{int(i):05d} {r + 1} {float(preds[i]):.1f} golden\n")
    return qrels, run


def run_ndeval(exe, tmp, ids, topics, alpha, beta, depth_m):
    qrels, run = write_files(tmp, ids, topics)
    cmd = [exe]
    if (alpha, beta) != (0.5, 0.5):
        cmd += ["-alpha", repr(alpha), "-beta", repr(beta)]
    if depth_m:
        cmd += ["-M", str(depth_m)]
    out = subprocess.run(cmd + [qrels, run], check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()
    header = out[0].split(",")
    assert header[:2] == ["runid", "topic"] and tuple(header[2:]) == NR.FIELD_NAMES, header
    rows = [line.split(",") for line in out[1:]]
    assert [r[1] for r in rows] == [str(t + 1) for t in ids] + ["amean"], [r[1] for r in rows]
    return header[2:], [r[2:] for r in rows[:-1]], rows[-1][2:]


def to_f64(strs):
    return np.array([[float("nan") if "nan" in s else float(s) for s in row] for row in strs], np.float64)


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


def main():
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    if not cc:
        raise SystemExit("no C compiler")
    topics, short = build_topics()
    store = {}
    for tid, t in enumerate(topics):
        for k, v in t.items():
            store[f"topics/t{tid:03d}/{k}"] = np.asarray(v)
    a_ids, d_ids = list(range(short)), list(range(short, len(topics)))
    runs = [("a", a_ids, 0.5, 0.5, 0), ("b_a03_b08", a_ids, 0.3, 0.8, 0), ("b_a09_b05", a_ids, 0.9, 0.5, 0), ("c_M10", a_ids, 0.5, 0.5, 10),
            ("c_M100", a_ids, 0.5, 0.5, 100), ("d_long", d_ids, 0.5, 0.5, 0)]
    checked = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ndeval")
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-w", "-o", exe, NDEVAL_C, "-lm"], check=True)
        for name, ids, alpha, beta, depth_m in runs:
            names, rows, amean = run_ndeval(exe, tmp, ids, topics, alpha, beta, depth_m)
            for tid, row in zip(ids, rows):
                t = topics[tid]
                mine = NR.fields(NR.topic(t["preds"], t["rele"], alpha, beta, depth_m))
                for nm, a, b in zip(names, mine, row):
                    if not NR.same_field(a, b):
                        raise SystemExit(f"run {name}, topic {tid}, {nm}: the restatement gives {a}, ndeval prints {b}: NOT written")
                    checked += 1
            store[f"runs/{name}/alpha"] = np.float64(alpha)
            store[f"runs/{name}/beta"] = np.float64(beta)
            store[f"runs/{name}/depth_m"] = np.int32(depth_m)
            store[f"runs/{name}/topics"] = np.array(ids, np.int32)
            store[f"runs/{name}/names"] = np.array(names)
            store[f"runs/{name}/field_str"] = np.array(rows)
            store[f"runs/{name}/field_f64"] = to_f64(rows)
            store[f"runs/{name}/amean_str"] = np.array(amean)
            store[f"runs/{name}/amean_f64"] = to_f64([amean])[0]
            print(f"run {name:10s} {len(ids):3d} topics  amean alpha-nDCG@20 {amean[11]}  nNRBP {amean[13]}", flush=True)
    out = write_archive("ndeval.npz", store)
    print(f"wrote {out}: {len(topics)} topics, {len(runs)} runs, {checked} fields reproduced string for string, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
