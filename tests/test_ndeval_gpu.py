"""GPU: ptr_ndeval_measures (csrc/ndeval.hip) on the real kernel — every field of every fixture topic as the reference's ndeval printed it
(tests/golden/ndeval.npz), every output element against the float64 restatement tests/ndeval_ref.py (expected difference 0: the same IEEE
operations in the same order), the greedy ideal ranking exactly, bit identity, and the Python surface.

Dispatch forms: (G, DPT) = (64, 1) L <= 64, (64, 2) L <= 128 — one wavefront per query, four queries per workgroup —
and (256, 1) (256, 2) (256, 4) (256, 8) (256, 16) — one workgroup per query, up to PTR_MAX_LIST_LEN = 4096, which is also the LDS limit.

The gate against the restatement is 2^-50 max(1, |ref|): a few ulp of headroom for a host log() that may differ between machines (the 20
discounts are the only transcendental values); NaN must meet NaN.  Each comparison prints its worst difference.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util as GU
import ndeval_ref as NR

pytestmark = pytest.mark.gpu

GATE = 2.0 ** -50
KS_ALL = list(range(1, 21))
TILE_TOP = (64, 128, 256, 512, 1024, 2048, 4096)


def golden():
    if "ndeval" not in GU._CACHE:
        GU._CACHE["ndeval"] = GU._load("ndeval.npz")
    return GU._CACHE["ndeval"]


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def run_abi(preds, rele, ks=KS_ALL, alpha=0.5, beta=0.5, depth=0, lens=None, ntopics=None):
    """ptr_ndeval_measures through the ctypes binding -> (per_k [B, 6, nk], per_q [B, 3], S [B], ideal_order [B, L]) as numpy."""
    from ptranking_amd import _lib
    p, r = dev(preds), dev(rele)
    B, T, L = r.shape
    ld, td = dev(lens, torch.int32), dev(ntopics, torch.int32)
    nk = len(ks)
    per_k = torch.full((B, 6, nk), -7.0, dtype=torch.float64).cuda()
    per_q = torch.full((B, 3), -7.0, dtype=torch.float64).cuda()
    S = torch.full((B,), -7, dtype=torch.int32).cuda()
    ideal = torch.full((B, L), -7, dtype=torch.int32).cuda()
    _lib.call("ptr_ndeval_measures", _lib.ptr(p), _lib.ptr(r), _lib.ptr(ld), _lib.ptr(td), B, T, L, (C.c_int32 * max(nk, 1))(*ks), nk,
              C.c_double(alpha), C.c_double(beta), int(depth), _lib.ptr(per_k), _lib.ptr(per_q), _lib.ptr(S), _lib.ptr(ideal),
              _lib.current_stream(r.device))
    torch.cuda.synchronize()
    return per_k.cpu().numpy(), per_q.cpu().numpy(), S.cpu().numpy(), ideal.cpu().numpy()


def worst(got, ref):
    """max over the elements of |got - ref| / max(1, |ref|); NaN against NaN counts 0, NaN against a number inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    both = np.isnan(got) & np.isnan(ref)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    d = np.where(both, 0.0, np.where(np.isnan(d), np.inf, d))
    return float(d.max()) if d.size else 0.0


def check_against_restatement(what, preds, rele, ks=KS_ALL, alpha=0.5, beta=0.5, depth=0, lens=None, ntopics=None):
    got = run_abi(preds, rele, ks, alpha, beta, depth, lens, ntopics)
    ref = NR.batch(preds, rele, ks, alpha, beta, depth, lens, ntopics)
    wk, wq = worst(got[0], ref[0]), worst(got[1], ref[1])
    print(f"{what}: worst |kernel - restatement| / max(1, |ref|): per_k {wk:.3e}, per_q {wq:.3e} (gate {GATE:.3e})")
    assert np.array_equal(got[2], ref[2]), f"{what}: actual_subtopics {got[2]} vs {ref[2]}"
    assert np.array_equal(got[3], ref[3]), f"{what}: ideal_order differs in {int((got[3] != ref[3]).sum())} places"
    assert wk <= GATE and wq <= GATE, what
    return got


def synth(rng, B, T, L, density, ragged=False, graded=True, decimals=1):
    rele = (rng.random((B, T, L)) < density).astype(np.float32)
    if graded:
        rele *= rng.integers(1, 4, (B, T, L)).astype(np.float32)
    preds = np.round(rng.standard_normal((B, L)) * 2.0, decimals).astype(np.float32)
    lens = ntopics = None
    if ragged:
        lens = rng.integers(1, L + 1, B).astype(np.int32)
        lens[0] = L
        ntopics = rng.integers(1, T + 1, B).astype(np.int32)
        ntopics[-1] = T
        for q in range(B):                                   # junk beyond lens / ntopics: never read
            preds[q, lens[q]:] = np.nan
            rele[q, :, lens[q]:] = np.nan
            rele[q, ntopics[q]:, :] = np.nan
    return preds, rele, lens, ntopics


# ---------------------------------------------------------------------------------------------------------------- 1. what ndeval printed
@pytest.mark.parametrize("run", sorted(golden()["runs"]))
def test_every_fixture_field_as_ndeval_prints_it(run):
    """Topics are batched by tiling bucket (so each form serves the topics of its size), NaN-padded beyond lens / ntopics."""
    g = golden()
    r = g["runs"][run]
    alpha, beta, depth = float(r["alpha"]), float(r["beta"]), int(r["depth_m"])
    tids = [int(t) for t in r["topics"]]
    topics = [g["topics"][f"t{t:03d}"] for t in tids]
    values = np.full((len(tids), 21), -7.0)
    for top in TILE_TOP:
        rows = [i for i, t in enumerate(topics) if top // 2 < t["rele"].shape[1] <= top or (top == 64 and t["rele"].shape[1] <= 64)]
        if not rows:
            continue
        L, T = max(topics[i]["rele"].shape[1] for i in rows), max(topics[i]["rele"].shape[0] for i in rows)
        preds, rele = np.full((len(rows), L), np.nan, np.float32), np.full((len(rows), T, L), np.nan, np.float32)
        lens, nts = np.zeros(len(rows), np.int32), np.zeros(len(rows), np.int32)
        for b, i in enumerate(rows):
            t = topics[i]
            nt, n = t["rele"].shape
            preds[b, :n], rele[b, :nt, :n], lens[b], nts[b] = t["preds"], t["rele"], n, nt
        per_k, per_q, S, _ = run_abi(preds, rele, list(NR.FIELD_KS), alpha, beta, depth, lens, nts)
        for b, i in enumerate(rows):
            res = {m: per_k[b, a] for a, m in enumerate(NR.PER_K)}
            res.update({m: per_q[b, a] for a, m in enumerate(NR.PER_Q)})
            at = lambda m: list(res[m])
            values[i] = at("ERR-IA") + at("nERR-IA") + at("alpha-DCG") + at("alpha-nDCG") + [res["NRBP"], res["nNRBP"], res["MAP-IA"]] + \
                at("P-IA") + at("strec")
            assert S[b] == NR.actual_subtopics(NR.nrel_sub(NR.binarise(topics[i]["rele"])))
    bad = [(tids[i], NR.FIELD_NAMES[c], NR.fmt(values[i, c]), str(r["field_str"][i][c])) for i in range(len(tids)) for c in range(21)
           if not NR.same_field(NR.fmt(values[i, c]), str(r["field_str"][i][c]))]
    assert not bad, f"{len(bad)} of {21 * len(tids)} fields differ from ndeval's output: {bad[:6]}"
    amean = torch.from_numpy(values).mean(dim=0).numpy()                 # torch's summation order across the topics
    want = r["amean_f64"]
    diff = np.where(np.isnan(want) & np.isnan(amean), 0.0, np.abs(amean - want))
    print(f"run {run}: {21 * len(tids)} fields equal; amean worst |diff| {np.nanmax(diff):.3e} (gate 5e-7)")
    assert not np.isnan(diff).any() and diff.max() <= 5e-7


# ---------------------------------------------------------------------------------------------------------------- 2. the restatement
SHAPES = [(1, 1), (2, 31), (19, 32), (20, 8), (21, 1), (63, 32), (64, 31), (65, 8), (128, 32), (129, 31), (256, 1), (257, 32), (512, 8),
          (513, 31), (1024, 32), (1025, 8), (2048, 31), (2049, 32), (4096, 32)]


@pytest.mark.parametrize("L,T", SHAPES)
def test_every_output_element_against_the_restatement(L, T):
    """Full lists and ragged ones per shape; B = 3 is no multiple of the four queries of a one-wavefront workgroup."""
    rng = np.random.default_rng(1000 * T + L)
    B = 3 if L <= 1024 else 2
    density = 0.3 if L <= 256 else 0.08
    preds, rele, _, _ = synth(rng, B, T, L, density)
    check_against_restatement(f"full L={L} T={T}", preds, rele)
    preds, rele, lens, nts = synth(rng, B, T, L, density, ragged=True)
    check_against_restatement(f"ragged L={L} T={T}", preds, rele, alpha=0.3, beta=0.8, lens=lens, ntopics=nts)


@pytest.mark.parametrize("L,T", [(100, 5), (300, 32)])
def test_ragged_nan_padded_batch_per_form(L, T):
    """lens in {0, 1, 2, L - 1, L} and ntopics in {0, 1, T}, one batch for the one-wavefront form and one for the workgroup form."""
    rng = np.random.default_rng(L)
    lens = np.array([0, 1, 2, L - 1, L, L, 2], np.int32)
    nts = np.array([T, 1, T, 0, T, 1, 0], np.int32)
    B = len(lens)
    preds, rele, _, _ = synth(rng, B, T, L, 0.3)
    for q in range(B):
        preds[q, lens[q]:] = np.nan
        rele[q, :, lens[q]:] = np.nan
        rele[q, nts[q]:, :] = np.nan
    per_k, per_q, S, ideal = check_against_restatement(f"edges L={L} T={T}", preds, rele, lens=lens, ntopics=nts)
    assert S[0] == 0 and S[3] == 0 and S[6] == 0 and not per_k[[0, 3, 6]].any() and np.isnan(per_q[[0, 3, 6], 1]).all()
    assert (ideal[0] == -1).all() and ideal[3, :L - 1].tolist() == list(range(L - 2, -1, -1)) and ideal[3, L - 1] == -1


@pytest.mark.parametrize("L", [50, 200])
def test_nan_and_infinite_scores_rank_like_ptr_sort_desc(L):
    rng = np.random.default_rng(L + 7)
    preds, rele, _, _ = synth(rng, 3, 6, L, 0.3)
    preds[0, [3, L - 1]] = np.nan
    preds[0, 7] = np.inf
    preds[1, [0, 5]] = [np.inf, -np.inf]
    preds[2, 11] = -np.inf
    preds[2, [12, 13]] = [0.0, -0.0]
    check_against_restatement(f"non-finite L={L}", preds, rele)


@pytest.mark.parametrize("L", [40, 300])
def test_no_scores_means_the_input_order(L):
    rng = np.random.default_rng(L + 11)
    _, rele, lens, nts = synth(rng, 3, 7, L, 0.2, ragged=True)
    got = check_against_restatement(f"preds=None L={L}", None, rele, lens=lens, ntopics=nts)
    ident = np.tile(-np.arange(L, dtype=np.float32), (3, 1))
    again = run_abi(ident, rele, lens=lens, ntopics=nts)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize("n", [30, 150])
def test_depth_cut_off(n):
    rng = np.random.default_rng(n)
    preds, rele, _, _ = synth(rng, 2, 8, n, 0.3)
    full = run_abi(preds, rele)
    for depth in (1, 10, n, n + 5):
        got = check_against_restatement(f"depth={depth} n={n}", preds, rele, depth=depth)
        assert np.array_equal(got[3], full[3])                           # the ideal side always uses the whole pool
        if depth >= n:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, full))


# ---------------------------------------------------------------------------------------------------------------- 3. bit identity
@pytest.mark.parametrize("L,T", [(100, 7), (700, 32)])
def test_a_query_alone_in_a_batch_and_repeated_is_bit_identical(L, T):
    rng = np.random.default_rng(L)
    preds, rele, lens, nts = synth(rng, 5, T, L, 0.2, ragged=True)
    whole = run_abi(preds, rele, lens=lens, ntopics=nts)
    again = run_abi(preds, rele, lens=lens, ntopics=nts)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again))
    for q in (0, 3, 4):
        alone = run_abi(preds[q:q + 1], rele[q:q + 1], lens=lens[q:q + 1], ntopics=nts[q:q + 1])
        assert all(a[0].tobytes() == b[q].tobytes() for a, b in zip(alone, whole)), q


# ---------------------------------------------------------------------------------------------------------------- 4. the Python surface
def test_functional_surface():
    import ptranking_amd.functional as F_
    rng = np.random.default_rng(5)
    preds, rele, lens, nts = synth(rng, 6, 9, 90, 0.25, ragged=True)
    ks = (5, 10, 20)
    out = F_.ndeval_measures(dev(preds), dev(rele), ks, alpha=0.3, beta=0.8, depth=40, lens=dev(lens, torch.int32), ntopics=dev(nts, torch.int32),
                             return_ideal_order=True)
    per_k, per_q, S, ideal = NR.batch(preds, rele, ks, 0.3, 0.8, 40, lens, nts)
    assert set(out) == set(F_.NDEVAL_MEASURES) | {"actual_subtopics", "ideal_order"}
    for a, m in enumerate(NR.PER_K):
        assert out[m].dtype == torch.float64 and out[m].shape == (6, 3) and out[m].is_cuda and worst(out[m].cpu().numpy(), per_k[:, a]) <= GATE, m
    for a, m in enumerate(NR.PER_Q):
        assert out[m].dtype == torch.float64 and out[m].shape == (6,) and worst(out[m].cpu().numpy(), per_q[:, a]) <= GATE, m
    assert out["ideal_order"].dtype == torch.int64 and np.array_equal(out["ideal_order"].cpu().numpy(), ideal)
    assert np.array_equal(out["actual_subtopics"].cpu().numpy(), S)
    assert "ideal_order" not in F_.ndeval_measures(None, dev(rele))
    order = F_.div_ideal_order(dev(rele), alpha=0.3, lens=dev(lens, torch.int32), ntopics=dev(nts, torch.int32))
    assert order.dtype == torch.int64 and np.array_equal(order.cpu().numpy(), ideal)


def _presorted(rele, order):
    return np.take_along_axis(rele, order[:, None, :].repeat(rele.shape[1], axis=1), axis=2)


def test_the_ideal_order_scores_alpha_ndcg_one():
    """A run in the order div_ideal_order returns has alpha-nDCG = nERR-IA = 1 exactly at every k (the ideal is non-zero wherever S > 0).
    (a) The run is given by scores on the unsorted query: any data, ties included.  (b) The query itself is presorted by the order and
    evaluated with preds=None.  The greedy breaks ties by document INDEX, and presorting renumbers the documents; (b) therefore holds
    exactly for the pools on which the greedy never has to choose between tied documents with different subtopic sets: pools of nested
    subtopic sets (a larger set always scores strictly more), and those random pools that the restatement says are free of such ties."""
    import ptranking_amd.functional as F_
    rng = np.random.default_rng(77)
    B, T, L = 24, 6, 30
    rele = (rng.random((B, T, L)) < 0.3).astype(np.float32)
    order = F_.div_ideal_order(dev(rele), alpha=0.3).cpu().numpy()
    scores = np.empty((B, L), np.float32)
    np.put_along_axis(scores, order, -np.arange(L, dtype=np.float32)[None, :].repeat(B, axis=0), axis=1)
    out = F_.ndeval_measures(dev(scores), dev(rele), KS_ALL, alpha=0.3)
    live = (out["actual_subtopics"] > 0).cpu().numpy()
    assert live.sum() >= B - 2
    assert (out["alpha-nDCG"].cpu().numpy()[live] == 1.0).all() and (out["nERR-IA"].cpu().numpy()[live] == 1.0).all()
    # (b) nested pools: document i covers the subtopics 0 .. size_i - 1, sizes repeated and shuffled, some documents empty
    sizes = rng.integers(0, 33, (4, 80))
    nested = (np.arange(32)[None, :, None] < sizes[:, None, :]).astype(np.float32)
    pools = [(nested, 0.5)]
    # random pools of 10 documents with the subtopic counts 1 .. 10 in random order (no tie in the first round; alpha = 0.3 makes a later
    # one unlikely), kept where the restatement's greedy on the presorted pool returns the identity
    distinct = np.zeros((24, 12, 10), np.float32)
    for q in range(24):
        for i, c in enumerate(rng.permutation(10) + 1):
            distinct[q, rng.choice(12, c, replace=False), i] = 1.0
    free = []
    for q in range(24):
        rel = NR.binarise(distinct[q])
        s = rel[NR.ideal_order(rel, 0.3)]
        if np.array_equal(s[NR.ideal_order(s, 0.3)], s):
            free.append(q)
    assert len(free) >= 12, "the random pools hold too few tie-free queries"
    pools.append((distinct[free], 0.3))
    for r, alpha in pools:
        o = F_.div_ideal_order(dev(r), alpha=alpha).cpu().numpy()
        res = F_.ndeval_measures(None, dev(_presorted(r, o)), KS_ALL, alpha=alpha)
        assert (res["actual_subtopics"] > 0).all()
        assert (res["alpha-nDCG"].cpu().numpy() == 1.0).all() and (res["nERR-IA"].cpu().numpy() == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------- 5. the ranker
F_DIM = 8
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=F_DIM, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False,
                      dropout=0.0)}


def _query(rng, n, T):
    R = (rng.random((T, n)) < 0.2).astype(np.float32) * rng.integers(1, 3, (T, n)).astype(np.float32)      # NOT presorted
    d = (0.5 * rng.standard_normal((n, F_DIM))).astype(np.float32)
    q = rng.standard_normal((1, F_DIM)).astype(np.float32)
    return (f"q{n}_{T}", torch.from_numpy(q), [f"d{i}" for i in range(n)], torch.from_numpy(d), 0.0, {}, torch.from_numpy(np.ascontiguousarray(R)))


def test_ranker_method_equals_the_mean_of_per_query_calls():
    import ptranking_amd as pa
    rng = np.random.default_rng(9)
    data = [_query(rng, int(rng.integers(3, 70)), int(rng.integers(1, 9))) for _ in range(60)]
    data[7] = data[7][:6] + (torch.zeros_like(data[7][6]),)              # a query without a relevant document: its nNRBP is NaN
    batches = pa.DivQueryBatches(data, "cuda:0", rough_batch_size=512, pad_to=16)
    assert len(batches) > 2
    torch.manual_seed(21)
    r = pa.DALETOR(sf_para_dict=copy.deepcopy(SF), model_para_dict=dict(pa.diversity.DEFAULT_DIV_PARAS["DALETOR"]), gpu=True, device="cuda:0")
    r.init()
    ks = [5, 10, 20]
    got, per_q = r.ndeval_performance_at_ks(test_data=batches, ks=ks, alpha=0.5, beta=0.5, need_per_q=True)
    assert set(got) == set(pa.functional.NDEVAL_MEASURES) and len(per_q) == len(batches)
    rows = {m: [] for m in NR.MEASURES}
    r.eval_mode()
    with torch.no_grad():
        for ids, X, rele, lens, nts in batches:
            preds = r._score_batch(X, lens).cpu().numpy()
            for q in range(len(ids)):
                n, nt = int(lens[q]), int(nts[q])
                t = NR.topic(preds[q], rele[q].cpu().numpy(), 0.5, 0.5, 0, n, nt)
                for m in NR.MEASURES:
                    rows[m].append([t[m][k - 1] for k in ks] if m in NR.PER_K else t[m])
    for m in NR.MEASURES:
        want = np.mean(np.array(rows[m], np.float64), axis=0)
        assert got[m].dtype == torch.float64 and got[m].device.type == "cpu" and got[m].shape == np.shape(want), m
        if m == "nNRBP":
            assert np.isnan(want) and bool(torch.isnan(got[m]))          # ndeval's amean includes the 0 / 0 topic
        else:
            assert worst(got[m].numpy(), want) <= 1e-12, m                # sums of 60 values in another order
    plain = r.ndeval_performance_at_ks(test_data=batches, ks=ks)
    assert all(torch.equal(plain[m], got[m]) or m == "nNRBP" for m in got)
    one = r.ndeval_performance_at_ks(test_data=[data[3]], ks=ks)         # the reference's per-query iterable
    t = NR.topic(r.div_predict(data[3][1].cuda(), data[3][3].cuda()).detach().cpu().numpy()[0], data[3][6].numpy(), 0.5, 0.5)
    assert worst(one["alpha-nDCG"].numpy(), [t["alpha-nDCG"][k - 1] for k in ks]) <= GATE and worst(one["NRBP"].numpy(), t["NRBP"]) <= GATE
