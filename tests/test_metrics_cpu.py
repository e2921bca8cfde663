"""CPU: the float64 restatement and the error bounds of tests/metrics_ref.py, before the GPU sees them.

  * the restatement reproduces the reference's own fp32 outputs (metrics.npz, siblings.npz permndcg/*, metrics_edge.npz) to 1e-6, NaN
    placement exact;
  * metrics_edge.npz rewrites byte for byte, and regenerates byte for byte where the reference checkout is present;
  * C_METRIC comes from the fp32 REFERENCES (oracle/torch_ref.py and the C oracle) on every input of the GPU cases A - E, never from the
    kernel: the recorded needs are re-measured here;
  * planted faults fail the gate while the unmodified fp32 reference passes it;
  * the C oracle's and torch_ref's sorts order NaN first, index ascending, like the restatement.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import golden_util as G
import metrics_ref as MR
from oracle import c_oracle as CO
from oracle import torch_ref as T

REF = os.environ.get("PTRANKING_REF") or "/root/reference"


def _maker():
    spec = importlib.util.spec_from_file_location("make_golden_metrics_edge", os.path.join(G.GOLDEN_DIR, "make_golden_metrics_edge.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _close(got, ref, what):
    """|got - ref| <= 1e-6 max(1, |ref|) element by element, NaN exactly where the reference has NaN."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN placement differs"
    ok = ~np.isnan(ref)
    err = np.abs(got - ref)[ok]
    lim = 1e-6 * np.maximum(1.0, np.abs(ref[ok]))
    assert (err <= lim).all(), f"{what}: max excess {float((err - lim).max()):.3e}"


def _ml(c):
    ml = float(c["max_label"])
    return None if np.isnan(ml) else ml


# ---------------------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", G.case_ids("rand", "metrics"))
def test_restatement_reproduces_metrics_npz(name):
    c = G.metrics()["rand"][name]
    ks, k1, presort = [int(k) for k in c["ks"]], int(c["k1"]), bool(int(c["presort"]))
    r = MR.metrics(c["preds"], c["labels"], None, ks, presort=presort)
    r1 = MR.metrics(c["preds"], c["labels"], None, [k1], presort=presort)
    for m in MR.METRICS:
        _close(r[m], c[m], f"{name} {m}")
        _close(r1[m], c[m + "_k"], f"{name} {m}@{k1}")
    vals, idx = MR.sort_desc(c["preds"])
    assert np.array_equal(idx, c["sort_idx"]) and np.array_equal(vals, c["sorted_vals"])


@pytest.mark.parametrize("name", G.case_ids("kat", "metrics"))
def test_restatement_reproduces_the_known_answers(name):
    c = G.metrics()["kat"][name]
    ys, yi, ks = c["sys_sorted"][0].astype(np.float64), c["ideal_sorted"][0].astype(np.float64), [int(k) for k in c["ks"]]
    kind = str(c["kind"])
    rw = MR.query_metrics(ys, yi, max(ks), False, float(yi.max()), MR.C_METRIC, (kind,))
    _close(rw[kind][0][np.asarray(ks) - 1][None], c["expected"], name)


@pytest.mark.parametrize("name", G.case_ids("permndcg", "siblings"))
def test_restatement_reproduces_permutation_ndcg(name):
    c = G.siblings()["permndcg"][name]
    ks = [int(k) for k in c["ks"]]
    r = MR.metrics(c["preds"], c["labels"], None, ks, permutation_labels=True, which=("ndcg",))
    _close(r["ndcg"], c["ndcg"], name)
    k1 = min(5, c["preds"].shape[1])
    _close(MR.metrics(c["preds"], c["labels"], None, [k1], permutation_labels=True, which=("ndcg",))["ndcg"], c["ndcg_k"], name + " @k")


EDGE = _maker().load()


@pytest.mark.parametrize("name", sorted(EDGE))
def test_restatement_reproduces_metrics_edge_npz(name):
    c = EDGE[name]
    kw = dict(presort=bool(int(c["presort"])), permutation_labels=bool(int(c["permutation"])), max_label=_ml(c))
    r = MR.metrics(c["preds"], c["labels"], None, [int(k) for k in c["ks"]], **kw)
    r1 = MR.metrics(c["preds"], c["labels"], None, [int(c["k1"])], **kw)
    for m in MR.METRICS:
        if m in c:
            _close(r[m], c[m], f"{name} {m}")
            _close(r1[m], c[m + "_k"], f"{name} {m}@k1")
    if name.startswith("norel"):
        assert np.isnan(c["ndcg"]).any() and np.isnan(c["ap"]).any() and np.isnan(c["nerr"]).any()
        assert not np.isnan(c["p"]).any()


def test_edge_fixture_is_small_and_rewrites_byte_for_byte(tmp_path):
    M = _maker()
    path = os.path.join(G.GOLDEN_DIR, M.FILE)
    assert os.path.getsize(path) < os.path.getsize(os.path.join(G.GOLDEN_DIR, "metrics.npz"))
    assert 24 <= len(EDGE) <= 48 and max(c["preds"].shape[1] for c in EDGE.values()) <= 300
    assert [i[0] for i in M.inputs()] == list(dict.fromkeys(i[0] for i in M.inputs())) and sorted(i[0] for i in M.inputs()) == sorted(EDGE)
    for case, s, y, ks, presort, perm, ml, k1 in M.inputs():                  # the committed inputs are the seeded ones
        c = EDGE[case]
        assert np.array_equal(c["preds"], s, equal_nan=True) and np.array_equal(c["labels"], y) and list(c["ks"]) == ks
        nan = np.isnan(s)
        assert all(len(np.unique(y[q][nan[q]])) <= 1 for q in range(len(s))), "NaN-scored documents of a list share one label"
    z = np.load(path, allow_pickle=False)
    again = str(tmp_path / M.FILE)
    M.write_npz(again, {k: z[k] for k in z.files})
    assert open(again, "rb").read() == open(path, "rb").read()


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "ptranking", "metric")), reason="the reference checkout is not on this machine")
def test_edge_fixture_regenerates_byte_for_byte(tmp_path):
    M = _maker()
    again = str(tmp_path / M.FILE)
    M.write_npz(again, M.generate())
    assert open(again, "rb").read() == open(os.path.join(G.GOLDEN_DIR, M.FILE), "rb").read()


# ---------------------------------------------------------------------------------------------------------------------------- references
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def torch_ref_metrics(cs):
    """oracle/torch_ref.py (fp32 torch) on one case: whole batch without lens, per query with them; max_label=None: the batch maximum."""
    preds, labels, lens, ks = cs["preds"], cs["labels"], cs["lens"], cs["ks"]
    B, L = preds.shape
    perm, presort = cs["permutation_labels"], cs["presort"]
    ml = cs["max_label"]
    if ml is None and not perm:
        ml = MR.batch_max_label(labels, lens)
    out = {m: np.zeros((B, len(ks)), np.float32) for m in MR.METRICS if not (perm and m == "nerr")}

    def run(rows, n):
        tp, tl = _t(preds[rows, :n]), _t(labels[rows, :n])
        _, idx = T.sort_desc(tp)
        sys_sorted = torch.gather(tl, 1, idx)
        ideal = tl if presort else torch.sort(tl, dim=1, descending=True)[0]
        out["ndcg"][rows] = T.ndcg_at_ks(sys_sorted, ideal, ks, permutation_labels=perm).numpy()
        out["ap"][rows] = T.ap_at_ks(sys_sorted, ideal, ks).numpy()
        out["p"][rows] = T.precision_at_ks(sys_sorted, ks).numpy()
        if not perm:
            out["nerr"][rows] = T.nerr_at_ks(sys_sorted, ideal, ks, ml).numpy()
    if lens is None:
        run(slice(0, B), L)
    else:
        for q in range(B):
            n = MR._qlen(lens, q, L)
            if n:
                run(slice(q, q + 1), n)
    return out


def c_oracle_metrics(cs):
    out = CO.metrics_at_ks(cs["preds"], cs["labels"], cs["ks"], cs["presort"], max_label=cs["max_label"], lens=cs["lens"],
                           permutation_labels=cs["permutation_labels"])
    if cs["permutation_labels"]:
        out.pop("nerr")
    return out


@pytest.fixture(scope="module")
def reference_needs():
    """What each fp32 reference needs under the bounds at c = 1, over every input of the GPU cases A - E, the C oracle's also over the
    cases of at most 1024 and at most 2049 documents.  NaN placement and P (bit for bit: both divide in IEEE arithmetic) are asserted
    here for both; the bounds themselves are asserted by test_reference_needs_give_the_constant."""
    needs = {"torch_ref": (0.0, ""), "c_oracle": (0.0, ""), "c_oracle_1024": (0.0, ""), "c_oracle_2049": (0.0, "")}
    for name, cs in MR.all_gpu_cases():
        ref1 = MR.restate(cs, c=1.0)
        for who, fn in (("torch_ref", torch_ref_metrics), ("c_oracle", c_oracle_metrics)):
            got = fn(cs)
            w = MR.need(got, ref1)
            if w > needs[who][0]:
                needs[who] = (w, name)
            if who == "c_oracle":
                for lim in (1024, 2049):
                    if cs["preds"].shape[1] <= lim and w > needs[f"c_oracle_{lim}"][0]:
                        needs[f"c_oracle_{lim}"] = (w, name)
            for m in got:                                                  # NaN placement and the exact elements
                r = ref1[m]
                g = np.asarray(got[m], np.float64)
                assert np.array_equal(np.isnan(g), np.isnan(r)), f"{who} {name} {m}: NaN placement"
            ex = ref1["p_exact"]
            assert np.array_equal(np.asarray(got["p"], np.float32)[ex].view(np.uint32), MR.p_bits(ref1["p"])[ex].view(np.uint32)), f"{who} {name} p"
    return needs


def test_reference_needs_give_the_constant(reference_needs):
    """C_METRIC = 2 x the larger need of the two fp32 references, rounded up to the next half, capped at 4 — and the needs recorded beside
    the constant are the measured ones."""
    t, c = reference_needs["torch_ref"], reference_needs["c_oracle"]
    print(f"MEASURED reference needs at c = 1: torch_ref {t[0]:.3f} ({t[1]}), C oracle {c[0]:.3f} ({c[1]}); "
          f"C_METRIC {MR.C_METRIC} = ceil_half(2 x {max(t[0], c[0]):.3f})")
    assert MR.C_METRIC == MR.constant_from_needs(MR.NEED_TORCH_REF, MR.NEED_C_ORACLE) <= MR.C_CAP
    assert MR.constant_from_needs(t[0], c[0]) == MR.C_METRIC
    assert abs(t[0] - MR.NEED_TORCH_REF) <= 0.05 and abs(c[0] - MR.NEED_C_ORACLE) <= 0.05
    # fp32 torch passes the gate the kernel is held to everywhere; the C oracle (one in-order chain per sum) up to 1024 documents
    s, m = reference_needs["c_oracle_1024"], reference_needs["c_oracle_2049"]
    print(f"MEASURED C oracle up to 1024 documents: {s[0]:.3f} ({s[1]}); up to 2049: {m[0]:.3f} ({m[1]})")
    assert s[0] > 0.0 and m[0] >= s[0] and c[0] >= m[0]                       # the bands were measured
    assert abs(s[0] - MR.NEED_C_ORACLE_1024) <= 0.05 and abs(m[0] - MR.NEED_C_ORACLE_2049) <= 0.05
    assert t[0] <= MR.C_METRIC and s[0] <= MR.C_METRIC


def test_coverage_of_the_case_lists():
    names = [n for n, _ in MR.all_gpu_cases()]
    assert len(names) == len(set(names))
    a = [cs for n, cs in MR.all_gpu_cases() if n.startswith("A ")]
    assert {cs["preds"].shape[1] for cs in a} == set(MR.TILING_LENGTHS)
    for L in (2, 65, 4096):
        mine = [(n, cs) for n, cs in MR.cases_A(L)]
        assert {(cs["lens"] is None, cs["presort"]) for _, cs in mine} == {(a, b) for a in (False, True) for b in (False, True)}
        assert {n.split()[5] for n, _ in mine} == {"mslr", "binary"} and {n.split()[6] for n, _ in mine} == {"ks-ascending", "ks-shuffled"}
        for _, cs in mine:
            if cs["lens"] is not None:
                assert {0, 1, 2, L} <= set(int(v) for v in cs["lens"])
            assert len(cs["ks"]) <= MR.MAX_CUTOFFS and max(cs["ks"]) == 2 * L
    assert max(MR.cutoffs_for(4096)) == 8192 and {4095, 4096, 4097, 1023, 1024, 1025, 192, 193} <= set(MR.cutoffs_for(4096))
    for L in MR.NAN_LENGTHS:
        for n, cs in MR.cases_E(L):
            nan = np.isnan(cs["preds"])
            for q in range(len(nan)):
                k = int(nan[q, :int(cs["lens"][q])].sum()); m = int(cs["lens"][q])
                if m and "nan_all" in n:
                    assert k == m
                if m and "nan_nm1" in n:
                    assert k == max(1, m - 1)
                if m and "nan1" in n:
                    assert k == 1


# ---------------------------------------------------------------------------------------------------------------------------- planted faults
def fp32_walk(ys, yi, m, max_label, fault=None):
    """The metric walk in fp32 (in-order sums, IEEE division), rank-wise over 0 .. m-1, with one planted fault."""
    f = np.float32
    ys, yi = ys[:m].astype(f), yi[:m].astype(f)
    r = np.arange(m, dtype=f)
    d = (f(1.0) / np.log2(r + f(2.0))).astype(f)
    ds = d.copy()
    if fault == "discount":
        ds[0] = f(np.float64(ds[0]) * (1.0 + 1e-6))
    gs, gi = np.exp2(ys) - f(1.0), np.exp2(yi) - f(1.0)
    sd, idg = np.cumsum(gs * ds, dtype=f), np.cumsum(gi * d, dtype=f)
    if fault == "carry" and m > 64:
        sd[64:] -= sd[63]
    rel = np.clip(ys, 0, 1)
    prec = (np.cumsum(rel, dtype=f) / (r + f(1.0))).astype(f)
    p_out = np.nextafter(prec, f(-1.0)) if fault == "p_ulp" else prec
    ap = np.cumsum(prec * rel, dtype=f) / np.cumsum(yi, dtype=f)
    pw = f(2.0 ** (max_label - (1.0 if fault == "max_label" else 0.0)))

    def err(g):
        sat = (g / pw).astype(f)
        incl = np.cumprod(f(1.0) - sat, dtype=f)
        casc = incl if fault == "cascade" else np.concatenate(([f(1.0)], incl[:-1]))
        return np.cumsum(sat * casc / (r + f(1.0)), dtype=f)
    with np.errstate(all="ignore"):
        return dict(ndcg=sd / idg, nerr=err(gs) / err(gi), ap=ap, p=p_out)


def fp32_model(cs, fault=None):
    preds, labels, lens, ks = cs["preds"], cs["labels"], cs["lens"], cs["ks"]
    B, L = preds.shape
    ml = cs["max_label"] if cs["max_label"] is not None else MR.batch_max_label(labels, lens)
    out = {m: np.zeros((B, len(ks)), np.float32) for m in MR.METRICS}
    for q in range(B):
        n = MR._qlen(lens, q, L)
        used = [k for k in ks if 1 <= k <= n]
        if not used:
            continue
        y = labels[q, :n]
        o = MR.order_desc(preds[q, :n])
        rw = fp32_walk(y[o], y if cs["presort"] else -np.sort(-y), max(used), ml, fault)
        for m in MR.METRICS:
            out[m][q, :len(used)] = rw[m][np.asarray(used) - 1]
    return out


@pytest.fixture(scope="module")
def fault_case():
    """130 documents, scores that follow the labels loosely, a relevant document planted at rank 0 (nDCG@1 = 1), cut-offs on both sides of
    the chunk boundary at rank 64."""
    g = np.random.default_rng(5)
    labels = MR.make_labels("yahoo", 4, 130, g)
    labels[:, 0] = 4.0
    preds = (labels + 1.5 * g.standard_normal(labels.shape)).astype(np.float32)
    preds[:, 0] = 9.0
    cs = dict(preds=preds, labels=labels, lens=None, ks=[1, 2, 5, 10, 64, 65, 128, 130], presort=False, permutation_labels=False, max_label=None)
    return cs, MR.restate(cs)


def test_the_unmodified_fp32_walk_passes_the_gate(fault_case):
    cs, ref = fault_case
    MR.gate_metrics(fp32_model(cs), ref, "fp32 walk", MR.C_METRIC)


@pytest.mark.parametrize("fault,metric", [("discount", "ndcg"), ("carry", "ndcg"), ("cascade", "nerr"), ("max_label", "nerr"), ("p_ulp", "p")])
def test_planted_faults_fail_the_gate(fault_case, fault, metric):
    """One discount off by 1e-6 relative; one chunk carry dropped (the prefix restarts at rank 64); the cascade's exclusive product taken
    inclusive; a max_label too small by one; a P@k one ulp low."""
    cs, ref = fault_case
    got = fp32_model(cs, fault)
    with pytest.raises(AssertionError, match=metric):
        MR.gate_metrics({metric: got[metric]}, ref, f"planted {fault}", MR.C_METRIC)
    for m in MR.METRICS:                                                      # and nothing else moved
        if m != metric:
            MR.gate_metrics({m: got[m]}, ref, f"planted {fault}: untouched", MR.C_METRIC)


def test_the_old_rule_misses_the_discount_fault(fault_case):
    cs, _ = fault_case
    G.assert_close(fp32_model(cs, "discount")["ndcg"], fp32_model(cs)["ndcg"], "golden rule")


# ---------------------------------------------------------------------------------------------------------------------------- NaN order
@pytest.mark.parametrize("L", MR.NAN_LENGTHS)
def test_oracle_sorts_order_nan_first_like_the_restatement(L):
    for name, cs in MR.cases_E(L):
        vals, idx = MR.sort_desc(cs["preds"], cs["lens"])
        cv, ci = CO.sort_desc(cs["preds"], cs["lens"])
        assert np.array_equal(ci, idx), f"C oracle {name}"
        assert np.array_equal(cv.view(np.uint32) & 0x7FC00000, vals.view(np.uint32) & 0x7FC00000) and np.array_equal(cv, vals, equal_nan=True), name
        for q in range(len(idx)):
            n = int(cs["lens"][q])
            if n:
                tv, ti = T.sort_desc(_t(cs["preds"][q:q + 1, :n]))
                assert np.array_equal(ti.numpy()[0], idx[q, :n]), f"torch_ref {name} row {q}"
                assert np.array_equal(tv.numpy()[0], vals[q, :n], equal_nan=True)
        nan = np.isnan(vals)
        for q in range(len(idx)):                                             # NaN first, in index order
            k = int(nan[q].sum())
            assert nan[q, :k].all() and (np.diff(idx[q, :k]) > 0).all()
