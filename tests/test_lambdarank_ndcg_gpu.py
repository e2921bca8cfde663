"""GPU: the truncated, normalised lambdarank (csrc/tree.hip tree_lambdarank_ndcg_kernel) under the element-wise float64 gate of
tests/lambdarank_ndcg_ref.py — a ragged batch whose lengths straddle every form of the dispatch at every truncation level x norm x sigma,
the edge lists, bit-identity across launches and forms, subset launches, NaN containment, the identity with the Delta-nDCG pair kernel,
TreeObjective's three call forms, a whole fit on the native booster and the example.  Each gated test prints its worst needed constant
before it asserts."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import f64_loss_bounds as FB
import lambdarank_ndcg_ref as LR
import tree_ref as TR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
STRADDLE = LR.STRADDLE


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def F_():
    import ptranking_amd.functional as f
    return f


class Batch:
    """A ragged batch on the device, launched the way TreeObjective launches it: one call per length class."""

    def __init__(self, preds, labels, group):
        from ptranking_amd.tree import bucket_queries
        self.preds_host, self.labels_host, self.group = np.asarray(preds, np.float32), np.asarray(labels, np.float32), np.asarray(group)
        self.preds, self.labels = dev(self.preds_host), dev(self.labels_host)
        self.offsets = dev(TR.offsets_of(group), np.int64)
        self.buckets = [(m, dev(idx)) for m, idx in bucket_queries(group)]

    def launch(self, T, norm, sigma, queries=None, max_len=None, fill=None):
        out = None if fill is None else (torch.full_like(self.preds, fill), torch.full_like(self.preds, fill))
        return F_().tree_lambdarank_ndcg_grad_hess(self.preds, self.labels, self.offsets, T, sigma, norm, queries=queries, max_len=max_len, out=out)

    def bucketed(self, T, norm, sigma):
        out = (torch.full_like(self.preds, 7.0), torch.full_like(self.preds, 7.0))
        for max_len, queries in self.buckets:
            F_().tree_lambdarank_ndcg_grad_hess(self.preds, self.labels, self.offsets, T, sigma, norm, queries=queries, max_len=max_len, out=out)
        return out


def host(pair):
    return tuple(t.cpu().numpy() for t in pair)


def named(name):
    return Batch(*LR.gpu_inputs()[name])


@pytest.fixture(scope="module")
def straddle():
    return named("straddle")


# ---------------------------------------------------------------------------------------------------------------- 1. the gate
@pytest.mark.parametrize("T,norm,sigma", LR.CONFIGS)
def test_ragged_batch_across_every_form_under_the_gate(straddle, T, norm, sigma):
    grad, hess = host(straddle.bucketed(T, norm, sigma))
    assert not (grad == 7.0).any() and not (hess == 7.0).any()                # every document was written
    w = LR.gate(grad, hess, LR.reference("straddle", T, norm, sigma), f"straddle T {T} norm {norm} sigma {sigma}")
    print(f"kernel: worst err/E {w:.3f}: needs C_PAIR >= {w * FB.C_PAIR:.2f}")
    assert (hess >= 0).all() and np.isfinite(grad).all()
    ref = LR.reference("straddle", T, norm, sigma)
    off = TR.offsets_of(STRADDLE)
    for a, b in zip(off[:-1], off[1:]):
        # the gradients of a query sum to 0: each element is within its bound of a float64 value, and those sum to 0 (where the
        # restatement compares every document of the list)
        if 0 < b - a <= LR.MAX_ROWS:
            sel = (ref["idx"] >= a) & (ref["idx"] < b)
            assert abs(grad[a:b].astype(np.float64).sum()) <= ref["E_grad"][sel].sum() + 1e-12


# ---------------------------------------------------------------------------------------------------------------- 2. the edge lists
EDGE_CONFIGS = ((1, True, 2.0), (2, False, 1.0), (30, True, 1.0), (5000, True, 2.0), (5000, False, 1.0))


@pytest.mark.parametrize("name", ["equal labels", "no relevant document"])
def test_lists_without_a_pair_are_exactly_zero(name):
    b = named(name)
    for T, norm, sigma in EDGE_CONFIGS:
        grad, hess = host(b.bucketed(T, norm, sigma))
        assert (grad == 0).all() and (hess == 0).all(), (T, norm, sigma)
    one = Batch([0.5], [3.0], [1])
    assert [float(t) for t in one.launch(30, True, 1.0)] == [0.0, 0.0]


@pytest.mark.parametrize("name", ["equal scores", "shorter than T", "offset 1e3"])
def test_edge_lists_under_the_gate(name):
    b = named(name)
    worst = 0.0
    for T, norm, sigma in EDGE_CONFIGS:
        grad, hess = host(b.bucketed(T, norm, sigma))
        worst = max(worst, LR.gate(grad, hess, LR.reference(name, T, norm, sigma), f"{name} T {T} norm {norm} sigma {sigma}"))
    print(f"{name}: needs C_PAIR >= {worst * FB.C_PAIR:.2f}")
    if name == "equal scores":
        # every score the same: rank = original index, no score-distance division, and sigma ds = 0 gives p = 1/2 whatever sigma is
        a = host(b.bucketed(30, False, 1.0))
        c = host(b.bucketed(30, False, 2.0))
        assert np.array_equal(2.0 * a[0], c[0]) and np.array_equal(4.0 * a[1], c[1])
        s, y, group = LR.gpu_inputs()[name]
        off = TR.offsets_of(group)
        n = group[2]
        first = y[off[2]:off[3]].copy()
        grad, _ = host(b.launch(1, False, 1.0))
        top = grad[off[2]:off[3]]
        assert n == 64 and (top[1:][first[1:] == first[0]] == 0).all()          # T = 1: only pairs with document 0, which ranks first
        assert (np.sign(top[1:][first[1:] != first[0]]) == np.sign(first[0] - first[1:][first[1:] != first[0]])).all()


# ---------------------------------------------------------------------------------------------------------------- 3. bit-identity
@pytest.mark.parametrize("T,norm,sigma", [(30, True, 1.0), (2, True, 2.0), (5000, False, 1.0)])
def test_launches_and_forms_agree_bit_for_bit(straddle, T, norm, sigma):
    """All queries in one launch (every list in the one-workgroup form), per length class (each in its own form), the short lists through
    the one-wavefront form as well, the index list in two halves, each query alone, and a repeated launch: the same bits."""
    B = len(STRADDLE)
    fn = F_().tree_lambdarank_ndcg_grad_hess
    sp = straddle
    whole = sp.launch(T, norm, sigma)
    again = sp.launch(T, norm, sigma)
    classes = sp.bucketed(T, norm, sigma)
    fresh = lambda: (torch.full_like(sp.preds, 7.0), torch.full_like(sp.preds, 7.0))
    halves = fresh()
    for part in (np.arange(0, B, 2), np.arange(1, B, 2)):
        fn(sp.preds, sp.labels, sp.offsets, T, sigma, norm, queries=dev(part, np.int32), max_len=int(max(STRADDLE[q] for q in part)), out=halves)
    alone = fresh()
    for q in range(B):
        fn(sp.preds, sp.labels, sp.offsets, T, sigma, norm, queries=dev([q], np.int32), max_len=STRADDLE[q], out=alone)
    for name, other in (("repeated", again), ("per class", classes), ("halves", halves), ("alone", alone)):
        for a, b, what in zip(whole, other, ("grad", "hess")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, what)
    # max_len raised: lists of at most 16 documents through the one-wavefront form, lists of at most 128 through the one-workgroup form
    off = TR.offsets_of(STRADDLE)
    for limit, max_len in ((16, 128), (16, 129), (128, 256)):
        part = [q for q in range(B) if 0 < STRADDLE[q] <= limit]
        raised = fresh()
        fn(sp.preds, sp.labels, sp.offsets, T, sigma, norm, queries=dev(part, np.int32), max_len=max_len, out=raised)
        for q in part:
            for a, b in zip(whole, raised):
                assert torch.equal(a[off[q]:off[q + 1]].view(torch.int32), b[off[q]:off[q + 1]].view(torch.int32)), (limit, max_len, q)


def test_a_subset_launch_writes_only_its_queries(straddle):
    off = TR.offsets_of(STRADDLE)
    grad, hess = host(straddle.launch(30, True, 1.0, queries=dev([5, 9], np.int32), max_len=129, fill=7.0))
    mine = np.zeros(off[-1], bool)
    mine[off[5]:off[6]] = mine[off[9]:off[10]] = True
    assert (grad[~mine] == 7.0).all() and (hess[~mine] == 7.0).all() and not (grad[mine] == 7.0).any() and not (hess[mine] == 7.0).any()
    # a launched query longer than max_len is the caller's error: NaN on it, and on nothing else
    grad, hess = host(straddle.launch(30, True, 1.0, queries=dev([3, 4], np.int32), max_len=16, fill=7.0))
    assert np.isnan(grad[off[4]:off[5]]).all() and np.isnan(hess[off[4]:off[5]]).all() and np.isfinite(grad[off[3]:off[4]]).all()
    assert (grad[off[5]:] == 7.0).all() and (grad[:off[3]] == 7.0).all()
    # without `out`, the documents of queries that are not launched read 0
    grad, _ = host(straddle.launch(30, True, 1.0, queries=dev([5], np.int32), max_len=63))
    assert (grad[:off[5]] == 0).all() and (grad[off[6]:] == 0).all() and (grad[off[5]:off[6]] != 0).any()


# ---------------------------------------------------------------------------------------------------------------- 4. NaN
def test_a_nan_score_or_label_stays_in_its_list():
    s, y, group = LR.gpu_inputs()["nan"]
    clean = host(Batch(s, y, group).bucketed(30, True, 1.0))
    off = TR.offsets_of(group)
    for bad_scores in (True, False):
        s2, y2 = s.copy(), y.copy()
        (s2 if bad_scores else y2)[off[1] + 40] = np.nan
        (s2 if bad_scores else y2)[off[3]] = np.nan
        b2 = Batch(s2, y2, group)
        got = host(b2.bucketed(30, True, 1.0))
        for g, c in zip(got, clean):
            assert np.isnan(g[off[1]:off[2]]).all() and np.isnan(g[off[3]:]).all()
            assert np.array_equal(g[:off[1]], c[:off[1]]) and np.array_equal(g[off[2]:off[3]], c[off[2]:off[3]])
        ref = LR.batch(s2, y2, group, T=30, norm=True, sigma=1.0)               # the restatement agrees: NaN there and nowhere else
        LR.gate(got[0], got[1], ref, "nan lists")
        whole = host(b2.launch(30, True, 1.0))                                   # the one-workgroup form
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(whole, got))


# ---------------------------------------------------------------------------------------------------------------- 5. the identity
def test_no_truncation_no_norm_is_the_delta_ndcg_pair_kernel():
    """T >= n, norm off, sigma 1 against tree_pair_grad_hess('NoTies', 'DeltaNDCG', epsilon 1, 'sum') on lists that hold a relevant
    document: two kernels, each within its own bound of the same float64 value (up to the other's 1e-16 Hessian floor per pair)."""
    s, y, group = LR.gpu_inputs()["identity"]
    b = Batch(s, y, group)
    mine = host(b.bucketed(5000, False, 1.0))
    theirs = (torch.empty_like(b.preds), torch.empty_like(b.preds))
    for max_len, queries in b.buckets:
        F_().tree_pair_grad_hess(b.preds, b.labels, b.offsets, "NoTies", "DeltaNDCG", 1.0, "sum", queries, max_len, theirs)
    theirs = host(theirs)
    ra = LR.reference("identity", 5000, False, 1.0)
    rb = TR.pair(s, y, group, pair_type="NoTies", weighting="DeltaNDCG", eps=1.0, hessian="sum")
    LR.gate(mine[0], mine[1], ra, "identity, this kernel")
    TR.gate(theirs[0], theirs[1], rb, "identity, the pair kernel", FB.C_PAIR)
    n_max = max(group)
    for k, name in enumerate(("grad", "hess")):
        diff = np.abs(mine[k].astype(np.float64) - theirs[k].astype(np.float64))
        bound = ra["E_" + name] + rb["E_" + name] + (n_max * 1e-16 if k else 0.0) + np.abs(ra[name] - rb[name])
        assert (diff <= bound).all(), (name, float((diff - bound).max()))
    assert np.abs(mine[0]).max() > 0


# ---------------------------------------------------------------------------------------------------------------- 6. the Python surface
def test_tree_objective_in_its_three_call_forms():
    import ptranking_amd as pa
    group = np.array(LR.OBJECTIVE_GROUP, np.int32)
    y = LR.gpu_inputs()["objective round 0"][1]
    obj = pa.TreeObjective(y.astype(np.float64), group, "lambdarank_ndcg")
    labels_ptr = obj._own.labels.data_ptr()
    for r, dtype in enumerate((np.float64, np.float32, np.float64)):
        preds = LR.gpu_inputs()[f"objective round {r}"][0].astype(dtype)
        grad, hess = obj(preds)
        assert grad.dtype == hess.dtype == np.float64 and grad.shape == hess.shape == (len(y),)
        LR.gate(grad, hess, LR.reference(f"objective round {r}", 30, True, 1.0), f"TreeObjective round {r}")
        assert (hess >= 0).all()
    assert obj.uploads == 1 and obj._own.labels.data_ptr() == labels_ptr
    with pytest.raises(ValueError, match="documents"):
        obj(np.zeros(3))
    # the settings reach the kernel, through .fobj and .sklearn too; the upload happens once per dataset
    kw = dict(truncation_level=1, sigmoid=2.0, norm=True)
    preds = LR.gpu_inputs()["objective round 1"][0].astype(np.float64)
    want = pa.TreeObjective(y, group, "lambdarank_ndcg", **kw)(preds)
    LR.gate(want[0], want[1], LR.reference("objective round 1", 1, True, 2.0), "TreeObjective T 1 sigma 2")
    data = types.SimpleNamespace(get_label=lambda: y, get_group=lambda: group)
    lazy = pa.TreeObjective(objective="lambdarank_ndcg", **kw)
    a, b = lazy.fobj(preds, data), lazy.fobj(preds, data)
    c, d = lazy.sklearn(y, preds, group), lazy.sklearn(y.copy(), preds, group.astype(np.float64))
    assert lazy.uploads == 2
    for got in (a, b, c, d):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(want[0], obj(preds)[0])


def fit_data(seed=5, queries=48):
    rng = np.random.default_rng(seed)
    group = rng.integers(5, 41, queries)
    n = int(group.sum())
    X = rng.standard_normal((n, 8)).astype(np.float32)
    z = X[:, 2] + 0.3 * rng.standard_normal(n)                                  # a noisy monotone function of one feature
    y = np.digitize(z, np.quantile(z, [0.5, 0.8, 0.93, 0.98])).astype(np.float32)
    return X, y, group


FIT_PARAMS = {"num_trees": 12, "num_leaves": 8, "min_data_in_leaf": 5, "learning_rate": 0.2, "lambdarank_truncation_level": 10}


def test_a_whole_fit_on_the_native_booster(tmp_path, monkeypatch):
    import ptranking_amd as pa
    from ptranking_amd import gbdt
    X, y, group = fit_data()
    seen = []
    update = gbdt.GBDT.update

    def recording(self, grad, hess):
        seen.append((self.scores.clone(), grad.clone(), hess.clone()))
        return update(self, grad, hess)
    monkeypatch.setattr(gbdt.GBDT, "update", recording)
    lm = pa.LambdaMART(FIT_PARAMS, objective="lambdarank_ndcg").fit(X, y, group)
    monkeypatch.setattr(gbdt.GBDT, "update", update)
    assert len(seen) == 12 == len(lm.booster.trees) and lm.booster.trees[0]["feature"].size > 0
    labels, offsets = dev(y), dev(TR.offsets_of(group), np.int64)
    for t, (scores, grad, hess) in enumerate(seen):                             # one launch over all queries against fit's launches per class
        g, h = F_().tree_lambdarank_ndcg_grad_hess(scores, labels, offsets, 10, 1.0, True)
        assert torch.equal(g.view(torch.int32), grad.view(torch.int32)) and torch.equal(h.view(torch.int32), hess.view(torch.int32)), t
    ref = LR.batch(seen[3][0].cpu().numpy(), y, group, T=10, norm=True, sigma=1.0)
    LR.gate(seen[3][1].cpu().numpy(), seen[3][2].cpu().numpy(), ref, "the gradients of round 4")
    assert torch.equal(lm.booster.scores.view(torch.int32), lm.predict(X).view(torch.int32))
    again = pa.LambdaMART(FIT_PARAMS, objective="lambdarank_ndcg").fit(X, y, group)
    assert torch.equal(again.booster.scores.view(torch.int32), lm.booster.scores.view(torch.int32))
    first = pa.LambdaMART.ndcg_at(seen[1][0], labels, group, 5)
    last = pa.LambdaMART.ndcg_at(lm.booster.scores, labels, group, 5)
    print(f"training nDCG@5: {first:.4f} after the first round, {last:.4f} after the last")
    assert last > first
    lm.booster.save_model(tmp_path / "m.npz")
    back = gbdt.GBDT.load_model(tmp_path / "m.npz")
    assert back.params == lm.booster.params and back.params["lambdarank_truncation_level"] == 10
    assert torch.equal(back.predict(X).view(torch.int32), lm.predict(X).view(torch.int32))
    Xv, yv, gv = fit_data(seed=6, queries=24)
    es = pa.LambdaMART(dict(FIT_PARAMS, num_trees=30), objective="lambdarank_ndcg").fit(X, y, group, eval_set=(Xv, yv), eval_group=gv, eval_at=5,
                                                                                       early_stopping_rounds=3)
    assert es.best_iteration is not None and 1 <= es.best_iteration <= len(es.booster.trees) <= 30
    assert es.booster.best_iteration == es.best_iteration and len(es.evals_result) == len(es.booster.trees)
    # the other objectives ignore the three settings: the same trees with and without them
    base = pa.LambdaMART({k: v for k, v in FIT_PARAMS.items() if k != "lambdarank_truncation_level"}).fit(X, y, group, num_boost_round=2)
    same = pa.LambdaMART(dict(FIT_PARAMS, lambdarank_norm=False, sigmoid=3.0)).fit(X, y, group, num_boost_round=2)
    assert torch.equal(base.booster.scores.view(torch.int32), same.booster.scores.view(torch.int32))


def _write_letor(path, n_q, rng, F=6):
    w = rng.standard_normal(F)
    with open(path, "w") as f:
        for q in range(n_q):
            n = int(rng.integers(12, 150))
            X = rng.standard_normal((n, F))
            s = X @ w + 0.3 * rng.standard_normal(n)
            lab = np.clip(np.floor((s - s.mean()) / (s.std() + 1e-9) + 1.5), 0, 4).astype(int)
            for i in range(n):
                f.write(f"{lab[i]} qid:{q + 1} " + " ".join(f"{k + 1}:{X[i, k]:.4f}" for k in range(F)) + "\n")


def test_the_example_runs_with_the_new_objective(tmp_path):
    _write_letor(tmp_path / "train.txt", 40, np.random.default_rng(7))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_lambdamart_native.py"), str(tmp_path / "train.txt"),
                          "--objective", "lambdarank_ndcg", "--rounds", "10", "--num-leaves", "8", "--min-data-in-leaf", "5",
                          "--truncation-level", "20"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    constant = float(out.stdout.split("constant scores: valid nDCG@5 ")[1].split()[0])
    tenth = float(out.stdout.split("round 10: valid nDCG@5 ")[1].split()[0])
    assert tenth > constant and "test nDCG@5" in out.stdout, out.stdout
