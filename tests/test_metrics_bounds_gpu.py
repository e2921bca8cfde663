"""GPU: the evaluation kernels (csrc/metrics.hip: ptr_sort_desc, ptr_metrics_at_ks, the batch-maximum kernels) against float64 with
ELEMENT-WISE error bounds (tests/metrics_ref.py), through functional.metrics_at_ks / sort_desc.  The inputs are the builders of
metrics_ref.py, the very cases tests/test_metrics_cpu.py ran the fp32 references on to set C_METRIC.

  A  every wave tiling (L = 1 .. 4096), ragged and full, presorted or not, five kinds of scores, cut-offs up to 2 L in order and shuffled
  B  all 15 metric subsets: inside the bounds, and bit-identical to the same columns of the all-four call
  C  Permutation and fractional labels, explicit / fractional / batch-maximum max_label, the three batch-maximum routes
  D  lists without a relevant document, empty lists, relevant documents beyond every cut-off, the reference's edge fixture
  E  NaN and infinite scores: the sort's order (NaN first, index ascending) and the metrics on it
  F  a query alone, in its batch, in halves, repeated: the same bits
  G  the Evaluator's methods on padded batches against the float64 mean over the kept queries
Each gate prints its worst err/E as a MEASURED line before it asserts (run with -s)."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

import golden_util as G
import metrics_ref as MR
from f64_bounds import U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CM = MR.C_METRIC


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def run(cs, which=None, rows=None):
    """functional.metrics_at_ks on one case (optionally on a subset of its rows) -> {name: float32 numpy [B, nk]}."""
    from ptranking_amd import functional as F
    sel = slice(None) if rows is None else rows
    which = tuple(m for m in (which or MR.METRICS) if not (cs["permutation_labels"] and m == "nerr"))
    lens = None if cs["lens"] is None else _t(cs["lens"][sel], torch.int32)
    out = F.metrics_at_ks(_t(cs["preds"][sel]), _t(cs["labels"][sel]), cs["ks"], presort=cs["presort"], max_label=cs["max_label"], lens=lens,
                          which=which, permutation_labels=cs["permutation_labels"])
    torch.cuda.synchronize()
    return {m: v.cpu().numpy() for m, v in out.items()}


def bits(d):
    return {m: np.asarray(v, np.float32).view(np.uint32) for m, v in d.items()}


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert a.keys() == b.keys(), what
    for m in a:
        assert np.array_equal(a[m], b[m]), f"{what}: {m} differs in {int((a[m] != b[m]).sum())} elements"


def gate_case(name, cs):
    return MR.gate_metrics(run(cs), MR.restate(cs), name, CM)


# ---------------------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("L", MR.TILING_LENGTHS)
def test_A_every_tiling_long_walks(L):
    worst = {}
    for name, cs in MR.cases_A(L):
        for m, w in gate_case(name, cs).items():
            worst[m] = max(worst.get(m, 0.0), w)
    print(f"MEASURED A L{L}: worst err/E " + ", ".join(f"{m} {w:.3f}" for m, w in worst.items()))


# ---------------------------------------------------------------------------------------------------------------------------- B
SUBSETS = [s for r in range(1, 5) for s in itertools.combinations(MR.METRICS, r)]


@pytest.mark.parametrize("L", [65, 1500])
def test_B_metric_sets(L):
    assert len(SUBSETS) == 15
    cs = MR.case(6, L, "yahoo", "normal", 6000 + L, ragged=True, ks=[1, 2, 5, 10, 64, 65, 129, 1024, 1025, L - 1, L, L + 1])
    ref = MR.restate(cs)
    full = run(cs)
    MR.gate_metrics(full, ref, f"B L{L} all four", CM)
    for sub in SUBSETS:
        got = run(cs, which=sub)
        assert set(got) == set(sub)
        MR.gate_metrics(got, ref, f"B L{L} {'+'.join(sub)}", CM)
        same_bits(got, {m: full[m] for m in sub}, f"B L{L} {'+'.join(sub)} against the all-four call")


# ---------------------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("name,cs", MR.cases_C(), ids=[n for n, _ in MR.cases_C()])
def test_C_gains_and_normalisers(name, cs):
    gate_case(name, cs)


def test_C_raw_abi_batch_maximum_workspace():
    """The C ABI itself with max_label < 0: the batch maximum goes through the caller's one-float workspace."""
    from ptranking_amd import _lib
    name, cs = [c for c in MR.cases_C() if c[0] == "C max vec"][0]
    B, L = cs["preds"].shape
    p, y = _t(cs["preds"]), _t(cs["labels"])
    ks = (C.c_int32 * len(cs["ks"]))(*cs["ks"])
    ws = torch.full((1,), float("nan"), device=DEV)
    out = {m: torch.full((B, len(cs["ks"])), float("nan"), device=DEV) for m in MR.METRICS}
    _lib.call("ptr_metrics_at_ks", _lib.ptr(p), _lib.ptr(y), None, B, L, ks, len(cs["ks"]), 0, 0, C.c_float(-1.0), _lib.ptr(ws),
              _lib.ptr(out["ndcg"]), _lib.ptr(out["nerr"]), _lib.ptr(out["ap"]), _lib.ptr(out["p"]), _lib.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    assert float(ws.item()) == float(cs["labels"].max())          # the workspace holds the float itself (its ordered image is the float for >= 0)
    MR.gate_metrics({m: v.cpu().numpy() for m, v in out.items()}, MR.restate(cs), "C raw ABI", CM)
    assert _lib.load().ptr_metrics_at_ks(_lib.ptr(p), _lib.ptr(y), None, B, L, ks, len(cs["ks"]), 0, 0, C.c_float(-1.0), None, None,
                                         _lib.ptr(out["nerr"]), None, None, None) != 0           # no workspace: refused before any launch


@pytest.mark.parametrize("where", ["unrolled", "remainder"])
def test_C_batch_maximum_eight_loads_in_flight(where):
    """3700 x 1024 labels without lens: batch_max_vec_kernel's 512 x 256 threads stride 131 072 float4 over 947 200; the threads below
    29 696 take the eight-loads-in-flight trip, everything else is the remainder loop.  Labels are <= 3 with a single 4 planted in
    one region or the other: a dropped element would scale every nERR of the batch by two."""
    from ptranking_amd import functional as F
    B, L = 3700, 1024
    g = np.random.default_rng(77)
    labels = g.choice(4, size=(B, L), p=[0.5, 0.3, 0.15, 0.05]).astype(np.float32)
    preds = g.standard_normal((B, L)).astype(np.float32)
    stride, total4 = 512 * 256, B * L // 4
    assert 7 * stride < total4 < 8 * stride
    first = total4 - 7 * stride                                   # 29 696 threads take the unrolled trip
    e4 = 100 + 3 * stride if where == "unrolled" else (first + 20000) + 2 * stride
    assert (e4 % stride < first) == (where == "unrolled") and e4 < total4
    labels.reshape(-1)[4 * e4 + 2] = 4.0
    ks = [1, 5, 10, 100]
    out = F.metrics_at_ks(_t(preds), _t(labels), ks, which=("nerr",))["nerr"].cpu().numpy()
    q = sorted({0, 100, (4 * e4 + 2) // L, 1234, 2047, 2048, 3000, B - 1})
    ref = MR.metrics(preds, labels, None, ks, max_label=4.0, which=("nerr",), queries=q)
    MR.gate_metrics({"nerr": out}, ref, f"C 3700 x 1024, the 4 in the {where} region", CM)


# ---------------------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("name,cs", MR.cases_D(), ids=[n for n, _ in MR.cases_D()])
def test_D_degenerate_lists(name, cs):
    got = run(cs)
    ref = MR.restate(cs)
    MR.gate_metrics(got, ref, name, CM)
    if "norel_rows" in cs:
        for q in cs["norel_rows"]:
            n = int(cs["lens"][q])
            fit = sum(1 for k in cs["ks"] if k <= n)
            assert fit >= 1
            for m in ("ndcg", "nerr", "ap"):
                assert np.isnan(got[m][q, :fit]).all() and (got[m][q, fit:] == 0).all(), f"{name} {m} row {q}"
            assert (got["p"][q] == 0).all()
        for q in cs["empty_rows"]:
            assert all((got[m][q] == 0).all() for m in MR.METRICS)
        rows = list(cs["neighbour_rows"])                          # the neighbours alone give the same bits
        same_bits({m: v[rows] for m, v in got.items()}, run(cs, rows=rows), f"{name}: neighbours")
    else:
        assert all((got[m] == 0).all() for m in MR.METRICS), "no relevant document above the cut-offs"


def _edge():
    spec = importlib.util.spec_from_file_location("make_golden_metrics_edge", os.path.join(G.GOLDEN_DIR, "make_golden_metrics_edge.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load()


EDGE = _edge()


@pytest.mark.parametrize("name", sorted(EDGE))
def test_D_edge_fixture_under_the_golden_gate(name):
    c = EDGE[name]
    ml = float(c["max_label"])
    cs = dict(preds=c["preds"], labels=c["labels"], lens=None, ks=[int(k) for k in c["ks"]], presort=bool(int(c["presort"])),
              permutation_labels=bool(int(c["permutation"])), max_label=None if np.isnan(ml) else ml)
    got = run(cs)
    got1 = run(dict(cs, ks=[int(c["k1"])]))
    MR.gate_metrics(got, MR.restate(cs), f"edge {name}", CM)
    for m in got:
        for g_, r_, what in ((got[m], c[m], m), (got1[m], c[m + "_k"], m + "@k1")):
            assert np.array_equal(np.isnan(g_), np.isnan(r_)), f"edge {name} {what}: NaN placement"
            G.assert_close(np.nan_to_num(g_, nan=0.0), np.nan_to_num(r_, nan=0.0), f"edge {name} {what}")


# ---------------------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("L", MR.NAN_LENGTHS)
def test_E_nan_and_infinite_scores(L):
    from ptranking_amd import functional as F
    for name, cs in MR.cases_E(L):
        p, lens = _t(cs["preds"]), _t(cs["lens"], torch.int32)
        vals, idx = F.sort_desc(p, lens)
        vals2, idx2 = F.sort_desc(p, lens)
        torch.cuda.synchronize()
        idx_h, vals_h = idx.cpu().numpy(), vals.cpu().numpy()      # to the host BEFORE anything gathers with the indices
        n = cs["lens"].astype(np.int64)[:, None]
        r = np.arange(L)[None, :]
        assert ((idx_h >= 0) & (idx_h < np.maximum(n, 1)) | (r >= n)).all(), f"{name}: an index outside its list"
        assert (idx_h[np.broadcast_to(r >= n, idx_h.shape)] == np.broadcast_to(r, idx_h.shape)[np.broadcast_to(r >= n, idx_h.shape)]).all()
        ref_vals, ref_idx = MR.sort_desc(cs["preds"], cs["lens"])
        bad = int((idx_h != ref_idx).sum())
        print(f"MEASURED {name} sort: {bad} of {idx_h.size} indices differ from the restatement")
        assert bad == 0, f"{name}: idx"
        nan = np.isnan(ref_vals)
        assert np.array_equal(np.isnan(vals_h), nan) and np.array_equal(vals_h.view(np.uint32)[~nan], ref_vals.view(np.uint32)[~nan]), f"{name}: vals"
        assert torch.equal(idx, idx2) and np.array_equal(vals2.cpu().numpy().view(np.uint32), vals_h.view(np.uint32)), f"{name}: repeated sort"
        gathered = np.take_along_axis(cs["preds"], idx_h, axis=1)   # safe now
        assert np.array_equal(gathered.view(np.uint32)[np.broadcast_to(r < n, idx_h.shape)], vals_h.view(np.uint32)[np.broadcast_to(r < n, idx_h.shape)])
        got = run(cs)
        MR.gate_metrics(got, MR.restate(cs), name, CM)
        same_bits(got, run(cs), f"{name}: repeated call")


# ---------------------------------------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("L", [128, 1024, 4096])
def test_F_a_query_does_not_depend_on_its_batch(L):
    from ptranking_amd import functional as F
    cs = MR.case(6, L, "mslr", "normal", 4000 + L, ragged=False, ks=[1, 5, 10, 64, 65, 128, L], max_label=4.0)
    cs["lens"] = np.asarray([L, L - 1, L // 2, 3, L, 65], np.int32)
    full = run(cs)
    MR.gate_metrics(full, MR.restate(cs), f"F L{L}", CM)
    same_bits(full, run(cs), f"F L{L}: repeated")
    halves = [run(cs, rows=slice(0, 3)), run(cs, rows=slice(3, 6))]
    same_bits(full, {m: np.concatenate([h[m] for h in halves]) for m in full}, f"F L{L}: two halves")
    alone = [run(cs, rows=slice(q, q + 1)) for q in range(6)]
    same_bits(full, {m: np.concatenate([a[m] for a in alone]) for m in full}, f"F L{L}: alone")

    def srt(rows):
        v, i = F.sort_desc(_t(cs["preds"][rows]), _t(cs["lens"][rows], torch.int32))
        return v.cpu().numpy().view(np.uint32), i.cpu().numpy()
    v, i = srt(slice(None))
    for parts in ([slice(None)], [slice(0, 3), slice(3, 6)], [slice(q, q + 1) for q in range(6)]):
        got = [srt(r) for r in parts]
        assert np.array_equal(np.concatenate([g_[0] for g_ in got]), v) and np.array_equal(np.concatenate([g_[1] for g_ in got]), i), f"F L{L} sort"
    rv, ri = MR.sort_desc(cs["preds"], cs["lens"])
    assert np.array_equal(i, ri) and np.array_equal(v, rv.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------- G
G_LENGTHS = (3, 5, 9, 10, 11, 40)
G_FEATURES = 24


def _ranker():
    import ptranking_amd as pa
    torch.manual_seed(11)
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
          "pointsf": dict(num_features=G_FEATURES, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None,
                          bn_affine=False, dropout=0.0)}
    ranker = pa.LambdaRank(sf_para_dict=sf, model_para_dict={"sigma": 1.0}, gpu=True, device=DEV)
    ranker.init()
    ranker.eval_mode()
    return ranker


def _queries(lengths, seed):
    g = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(lengths):
        y = g.choice(5, size=n, p=MR.MIXES["yahoo"]).astype(np.float32)
        y[g.integers(n)] = max(1.0, y.max())                   # every list holds a relevant document: the averages are finite
        out.append((f"q{i}", g.standard_normal((n, G_FEATURES)).astype(np.float32), y))
    return out


def _restate_dataset(ranker, data, ks, presort, max_label, which):
    """Per-query float64 rows (and bounds) on the ranker's own predictions, batch by batch: [(ref dict, lens)]."""
    from ptranking_amd.host import scorer_lens
    out = []
    for ids, X, Y, lens in data:
        Xd, ld = X.to(DEV), lens.to(DEV).to(torch.int32)
        with scorer_lens(ranker, ld, Xd):
            preds = ranker.predict(Xd).detach().float().cpu().numpy().reshape(Y.shape)
        ml = max_label if max_label is not None else MR.batch_max_label(Y.cpu().numpy(), lens.cpu().numpy())
        out.append((MR.metrics(preds, Y.cpu().numpy(), lens.cpu().numpy(), ks, presort=presort, max_label=ml, which=which), lens.cpu().numpy()))
    return out


def _gate_average(got, rows, E_rows, what):
    """The average of per-query values: float64 mean, the summed bounds plus the fp32 sum and division."""
    n = len(rows)
    mean = rows.sum(axis=0) / n
    E = (E_rows.sum(axis=0) + CM * U * np.abs(rows).sum(axis=0)) / n + CM * U * np.abs(mean)
    MR.gate_nan(np.asarray(got, np.float64), mean, E, what, CM)


def test_G_evaluator_on_padded_batches():
    from ptranking_amd.batching import PaddedQueryBatches
    ranker = _ranker()
    lengths = [n for n in G_LENGTHS for _ in range(3)]
    data = PaddedQueryBatches(_queries(lengths, 21), DEV, rough_batch_size=64, pad_to=8, presort=False)
    assert sorted({int(n) for _, _, _, lens in data for n in lens}) == list(G_LENGTHS)
    k = 10
    # single-cut-off methods: queries shorter than k are skipped per query
    for m, call in (("ndcg", lambda: ranker.ndcg_at_k(test_data=data, k=k, presort=False)),
                    ("nerr", lambda: ranker.nerr_at_k(test_data=data, k=k, max_label=4.0, presort=False)),
                    ("ap", lambda: ranker.ap_at_k(test_data=data, k=k, presort=False)), ("p", lambda: ranker.p_at_k(test_data=data, k=k))):
        got = call()
        parts = _restate_dataset(ranker, data, [k], False, 4.0, (m,))
        keep = [lens >= k for _, lens in parts]
        rows = np.concatenate([r[m][kp] for (r, _), kp in zip(parts, keep)])
        E_rows = np.concatenate([r["E_" + m][kp] for (r, _), kp in zip(parts, keep)])
        assert len(rows) == sum(1 for n in lengths if n >= k)
        _gate_average(got.numpy(), rows, E_rows, f"G {m}@{k} over the {len(rows)} kept queries")
    ks = [1, 5, 10, 20]
    got = ranker.ndcg_at_ks(test_data=data, ks=ks, presort=False)
    parts = _restate_dataset(ranker, data, ks, False, 4.0, ("ndcg",))
    _gate_average(got.numpy(), np.concatenate([r["ndcg"] for r, _ in parts]), np.concatenate([r["E_ndcg"] for r, _ in parts]), "G ndcg_at_ks")
    res = ranker.adhoc_performance_at_ks(test_data=data, ks=ks, max_label=None, presort=False, need_per_q=True)
    parts = _restate_dataset(ranker, data, ks, False, None, MR.METRICS)
    for j, m in enumerate(MR.METRICS):
        for (r, _), per_q in zip(parts, res[4 + j]):
            MR.gate_metrics({m: per_q.numpy()}, {k_: v for k_, v in r.items() if k_ in (m, "E_" + m, "q", "p_exact")}, f"G per-query {m}", CM)
        _gate_average(res[j].numpy(), np.concatenate([r[m] for r, _ in parts]), np.concatenate([r["E_" + m] for r, _ in parts]), f"G adhoc {m}")


def test_G_every_list_shorter_than_k_is_nan():
    from ptranking_amd.batching import PaddedQueryBatches
    ranker = _ranker()
    data = PaddedQueryBatches(_queries([3, 5, 9, 9, 5], 22), DEV, rough_batch_size=64, pad_to=8, presort=False)
    for got in (ranker.ndcg_at_k(test_data=data, k=10), ranker.nerr_at_k(test_data=data, k=10, max_label=4.0), ranker.ap_at_k(test_data=data, k=10),
                ranker.p_at_k(test_data=data, k=10)):
        assert got.shape == (1,) and bool(torch.isnan(got).all())          # the reference's 0 / 0
