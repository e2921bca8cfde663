"""GPU: the cross-entropy nDCG objective, rank_xendcg (csrc/tree.hip tree_xendcg_kernel), under the element-wise float64 gate of
tests/xendcg_ref.py — a ragged batch whose lengths straddle every form of the dispatch with supplied uniforms and with the counter stream,
the dominant, equal-score, offset and edge-uniform lists, the stream against its host restatement, bit-identity across launches and forms,
subset launches, NaN containment, TreeObjective's three call forms, whole fits on the native booster (split in two, refitted, replayed by
a host loop) and the example.  Each gated test prints its worst needed constant before it asserts."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import tree_ref as TR
import xendcg_ref as XR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
STRADDLE = XR.STRADDLE


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def F_():
    import ptranking_amd.functional as f
    return f


def bits(t):
    return t.view(torch.int32)


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


class Batch:
    """A ragged batch on the device, launched the way TreeObjective launches it: one call per length class."""

    def __init__(self, preds, labels, unif, group):
        from ptranking_amd.tree import bucket_queries
        self.group = np.asarray(group)
        self.preds, self.labels = dev(preds, np.float32), dev(labels, np.float32)
        self.unif = None if unif is None else dev(unif, np.float32)
        self.offsets = dev(TR.offsets_of(group), np.int64)
        self.buckets = [(m, dev(idx)) for m, idx in bucket_queries(group)]

    def fresh(self, fill=7.0):
        return (torch.full_like(self.preds, fill), torch.full_like(self.preds, fill))

    def launch(self, queries=None, max_len=None, out=None, stream=None):
        """stream = (seed, draw): the counter stream in place of the supplied uniforms."""
        seed, draw = stream or (5, 0)
        return F_().tree_xendcg_grad_hess(self.preds, self.labels, self.offsets, seed, draw, None if stream else self.unif, queries=queries,
                                          max_len=max_len, out=out)

    def bucketed(self, stream=None):
        out = self.fresh()
        for max_len, queries in self.buckets:
            self.launch(queries, max_len, out, stream)
        return out


def host(pair):
    return tuple(t.cpu().numpy() for t in pair)


def named(name):
    return Batch(*XR.gpu_inputs()[name])


@pytest.fixture(scope="module")
def straddle():
    return named("straddle")


# ---------------------------------------------------------------------------------------------------------------- 1. the gate
def test_ragged_batch_across_every_form_under_the_gate(straddle):
    grad, hess = host(straddle.bucketed())
    assert not (grad == 7.0).any() and not (hess == 7.0).any()                # every document was written
    w = XR.gate(grad, hess, XR.reference("straddle"), "straddle, supplied uniforms")
    print(f"kernel, supplied uniforms: worst err/E {w:.3f}: needs C_LIST >= {w * XR.C:.2f}")
    assert (hess >= 0).all() and np.isfinite(grad).all() and np.isfinite(hess).all()
    # the counter stream: the same gate against the restatement on the host-restated uniforms
    s, y, _, group = XR.gpu_inputs()["straddle"]
    for seed, draw in ((5, 0), (11, 3)):
        grad, hess = host(straddle.bucketed(stream=(seed, draw)))
        assert not (grad == 7.0).any() and not (hess == 7.0).any()
        ref = XR.batch(s, y, XR.uniforms(seed, draw, np.arange(s.size)), group)
        w = XR.gate(grad, hess, ref, f"straddle, the stream at seed {seed} draw {draw}")
        print(f"kernel, stream ({seed}, {draw}): worst err/E {w:.3f}: needs C_LIST >= {w * XR.C:.2f}")
        assert (hess >= 0).all() and np.isfinite(grad).all() and np.isfinite(hess).all()


@pytest.mark.parametrize("name", ["dominant", "equal scores", "offset 1e3", "edge uniforms"])
def test_edge_lists_under_the_gate(name):
    b = named(name)
    grad, hess = host(b.bucketed())
    assert not (grad == 7.0).any() and not (hess == 7.0).any()
    w = XR.gate(grad, hess, XR.reference(name), name)
    print(f"{name}: worst err/E {w:.3f}: needs C_LIST >= {w * XR.C:.2f}")
    assert (hess >= 0).all() and np.isfinite(grad).all() and np.isfinite(hess).all()
    off = TR.offsets_of(b.group)
    for a, e in zip(off[:-1], off[1:]):
        if e - a == 1:
            assert grad[a] == 0 and hess[a] == 0


# ---------------------------------------------------------------------------------------------------------------- 2. the stream
@pytest.mark.parametrize("seed,draw", [(5, 0), (5, 2 ** 32 + 7), (2 ** 40 + 3, 1), (2 ** 40 + 3, 2 ** 33)])
def test_the_stream_is_its_host_restatement_bit_for_bit(straddle, seed, draw):
    n = straddle.preds.numel()
    streamed = straddle.bucketed(stream=(seed, draw))
    uploaded = Batch(straddle.preds.cpu().numpy(), straddle.labels.cpu().numpy(), XR.uniforms(seed, draw, np.arange(n)), STRADDLE).bucketed()
    assert same_bits(streamed, uploaded)
    assert not same_bits(streamed, straddle.bucketed(stream=(seed, draw + 1))) and not same_bits(streamed, straddle.bucketed(stream=(seed + 1, draw)))


# ---------------------------------------------------------------------------------------------------------------- 3. bit-identity
@pytest.mark.parametrize("stream", [None, (5, 4)], ids=["supplied", "stream"])
def test_launches_and_forms_agree_bit_for_bit(straddle, stream):
    """All queries in one launch at max_len 4096 (every list in the one-workgroup form), per length class (each in its own form), the index
    list in two halves, each query alone, the short lists with max_len raised into the other forms, and a repeated launch: the same bits."""
    B = len(STRADDLE)
    sp = straddle
    whole = sp.launch(max_len=4096, stream=stream)
    again = sp.launch(max_len=4096, stream=stream)
    classes = sp.bucketed(stream=stream)
    halves = sp.fresh()
    for part in (np.arange(0, B, 2), np.arange(1, B, 2)):
        sp.launch(dev(part, np.int32), int(max(STRADDLE[q] for q in part)), halves, stream)
    alone = sp.fresh()
    for q in range(B):
        sp.launch(dev([q], np.int32), STRADDLE[q], alone, stream)
    for name, other in (("repeated", again), ("per class", classes), ("halves", halves), ("alone", alone)):
        assert same_bits(whole, other), name
    off = TR.offsets_of(STRADDLE)
    for limit, max_len in ((16, 16), (16, 128), (16, 129), (128, 256)):         # a list of 16 documents through G = 16 / 64 / 256
        part = [q for q in range(B) if 0 < STRADDLE[q] <= limit]
        raised = sp.fresh()
        sp.launch(dev(part, np.int32), max_len, raised, stream)
        for q in part:
            assert same_bits([t[off[q]:off[q + 1]] for t in whole], [t[off[q]:off[q + 1]] for t in raised]), (limit, max_len, q)


def test_a_subset_launch_writes_only_its_queries(straddle):
    off = TR.offsets_of(STRADDLE)
    whole = host(straddle.launch(max_len=4096, stream=(5, 0)))
    grad, hess = host(straddle.launch(dev([5, 9], np.int32), 129, straddle.fresh(), (5, 0)))
    mine = np.zeros(off[-1], bool)
    mine[off[5]:off[6]] = mine[off[9]:off[10]] = True
    assert (grad[~mine] == 7.0).all() and (hess[~mine] == 7.0).all() and not (grad[mine] == 7.0).any() and not (hess[mine] == 7.0).any()
    # a document's uniform does not change with the subset: the same bits as in the launch of everything
    assert np.array_equal(grad[mine], whole[0][mine]) and np.array_equal(hess[mine], whole[1][mine])
    # a launched query longer than max_len is the caller's error: NaN on it, and on nothing else
    grad, hess = host(straddle.launch(dev([3, 4], np.int32), 16, straddle.fresh()))
    assert np.isnan(grad[off[4]:off[5]]).all() and np.isnan(hess[off[4]:off[5]]).all() and np.isfinite(grad[off[3]:off[4]]).all()
    assert (grad[off[5]:] == 7.0).all() and (grad[:off[3]] == 7.0).all()
    # without `out`, the documents of queries that are not launched read 0
    grad, _ = host(straddle.launch(dev([5], np.int32), 63))
    assert (grad[:off[5]] == 0).all() and (grad[off[6]:] == 0).all() and (grad[off[5]:off[6]] != 0).any()


# ---------------------------------------------------------------------------------------------------------------- 4. NaN
@pytest.mark.parametrize("what,value", [("score", np.nan), ("label", np.nan), ("label", -1.0), ("uniform", 1.0)])
def test_a_bad_input_stays_in_its_list(what, value):
    group = XR.NAN_GROUP + [0, 1]
    s, y = TR.tree_inputs(group, seed=13)
    u = XR.draw_uniforms(s.size, np.random.default_rng(3))
    clean = host(Batch(s, y, u, group).bucketed())
    off = TR.offsets_of(group)
    assert clean[0][-1] == 0 and clean[1][-1] == 0                              # n = 1 is exactly 0 (n = 0 owns no output)
    s2, y2, u2 = s.copy(), y.copy(), u.copy()
    {"score": s2, "label": y2, "uniform": u2}[what][off[1] + 40] = value
    b2 = Batch(s2, y2, u2, group)
    got = host(b2.bucketed())
    for g, c in zip(got, clean):
        assert np.isnan(g[off[1]:off[2]]).all()
        assert np.array_equal(g[:off[1]], c[:off[1]]) and np.array_equal(g[off[2]:], c[off[2]:])
    XR.gate(got[0], got[1], XR.batch(s2, y2, u2, group), f"a bad {what}")        # the restatement agrees: NaN there and nowhere else
    whole = host(b2.launch(max_len=4096))                                       # the one-workgroup form
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(whole, got))


# ---------------------------------------------------------------------------------------------------------------- 5. the Python surface
def test_tree_objective_in_its_three_call_forms():
    import ptranking_amd as pa
    group = np.array(XR.OBJECTIVE_GROUP, np.int32)
    _, y = TR.tree_inputs(XR.OBJECTIVE_GROUP, seed=21)
    rounds = [(np.random.default_rng(40 + r).standard_normal(len(y)) * (r + 1)).astype(np.float32) for r in range(3)]
    obj = pa.TreeObjective(y.astype(np.float64), group, "rank_xendcg")
    labels_ptr = obj._own.labels.data_ptr()
    first = []
    for r, dtype in enumerate((np.float64, np.float32, np.float64)):
        assert obj.draw == r
        grad, hess = obj(rounds[r].astype(dtype))
        assert grad.dtype == hess.dtype == np.float64 and grad.shape == hess.shape == (len(y),)
        ref = XR.batch(rounds[r], y, XR.uniforms(5, r, np.arange(len(y))), group)
        XR.gate(grad, hess, ref, f"TreeObjective round {r}")
        assert (hess >= 0).all()
        first.append((grad, hess))
    assert obj.draw == 3 and obj.uploads == 1 and obj._own.labels.data_ptr() == labels_ptr
    with pytest.raises(ValueError, match="documents"):
        obj(np.zeros(3))
    assert obj.draw == 3                                                        # a refused call draws nothing
    # another object with the same seed replays the same rounds bit for bit, through .fobj and .sklearn too; another seed differs
    data = types.SimpleNamespace(get_label=lambda: y, get_group=lambda: group)
    by_fobj, by_sklearn, other = (pa.TreeObjective(objective="rank_xendcg", objective_seed=sd) for sd in (5, 5, 6))
    for r in range(3):
        a = by_fobj.fobj(rounds[r], data)
        b = by_sklearn.sklearn(y, rounds[r], group)
        c = other.sklearn(y, rounds[r], group)
        assert by_fobj.draw == by_sklearn.draw == r + 1
        for got in (a, b):
            assert np.array_equal(got[0], first[r][0]) and np.array_equal(got[1], first[r][1])
        assert not np.array_equal(c[0], first[r][0]) and np.array_equal(c[1], first[r][1])         # the Hessian holds no uniform
    assert by_fobj.uploads == by_sklearn.uploads == 1
    # the same scores in another round draw other uniforms
    assert not np.array_equal(by_fobj.fobj(rounds[0], data)[0], first[0][0])


def fit_data(seed=5, queries=60):
    rng = np.random.default_rng(seed)
    group = rng.integers(5, 41, queries)
    n = int(group.sum())
    X = rng.standard_normal((n, 6)).astype(np.float32)
    z = X[:, 2] + 0.3 * rng.standard_normal(n)                                  # a noisy monotone function of one feature
    y = np.digitize(z, np.quantile(z, [0.5, 0.8, 0.93, 0.98])).astype(np.float32)
    return X, y, group


FIT_PARAMS = {"num_trees": 12, "num_leaves": 8, "min_data_in_leaf": 5, "learning_rate": 0.2}


def same_trees(a, b):
    return len(a.trees) == len(b.trees) and all(sorted(t) == sorted(u) and all(np.array_equal(t[k], u[k]) for k in t) for t, u in zip(a.trees, b.trees))


@pytest.fixture(scope="module")
def fitted():
    import ptranking_amd as pa
    X, y, group = fit_data()
    return X, y, group, pa.LambdaMART(FIT_PARAMS, objective="rank_xendcg").fit(X, y, group)


def test_a_whole_fit_is_reproducible_and_learns(fitted):
    import ptranking_amd as pa
    X, y, group, lm = fitted
    assert len(lm.booster.trees) == 12 and lm.booster.trees[0]["feature"].size > 0
    again = pa.LambdaMART(FIT_PARAMS, objective="rank_xendcg").fit(X, y, group)
    assert same_trees(lm.booster, again.booster) and torch.equal(bits(again.booster.scores), bits(lm.booster.scores))
    assert torch.equal(bits(lm.booster.scores), bits(lm.predict(X)))
    other = pa.LambdaMART(dict(FIT_PARAMS, objective_seed=6), objective="rank_xendcg").fit(X, y, group)
    assert not same_trees(lm.booster, other.booster)
    labels = dev(y)
    zero = pa.LambdaMART.ndcg_at(torch.zeros_like(lm.booster.scores), labels, group, 5)
    last = pa.LambdaMART.ndcg_at(lm.booster.scores, labels, group, 5)
    print(f"training nDCG@5: {zero:.4f} for all-zero scores, {last:.4f} after 12 rounds of rank_xendcg")
    assert last > zero


def test_a_host_loop_reproduces_the_fit(fitted):
    from ptranking_amd import gbdt
    X, y, group, lm = fitted
    labels, offsets = dev(y), dev(TR.offsets_of(group), np.int64)
    booster = gbdt.GBDT(FIT_PARAMS, device=DEV).fit_bins(X, group=np.asarray(group))
    for t in range(12):
        booster.update(*F_().tree_xendcg_grad_hess(booster.scores, labels, offsets, seed=5, draw=t))     # one launch, where fit launches per class
    assert same_trees(lm.booster, booster) and torch.equal(bits(booster.scores), bits(lm.booster.scores))


def test_a_fit_split_in_two_is_the_unsplit_fit(fitted, tmp_path):
    import ptranking_amd as pa
    from ptranking_amd import gbdt
    X, y, group, lm = fitted
    half = pa.LambdaMART(dict(FIT_PARAMS, num_trees=6), objective="rank_xendcg").fit(X, y, group)
    half.booster.save_model(tmp_path / "half.npz")
    assert gbdt.GBDT.load_model(tmp_path / "half.npz").params["objective_seed"] == 5
    rest = pa.LambdaMART(dict(FIT_PARAMS, num_trees=6), objective="rank_xendcg").fit(X, y, group, init_model=str(tmp_path / "half.npz"))
    assert same_trees(lm.booster, rest.booster) and torch.equal(bits(rest.booster.scores), bits(lm.booster.scores))


def test_refit_on_the_training_data_returns_the_models_own_values(fitted):
    X, y, group, lm = fitted
    back = lm.refit(X, y, group, decay_rate=0)
    assert same_trees(lm.booster, back.booster) and torch.equal(bits(back.booster.scores), bits(lm.booster.scores))


def test_the_other_objectives_do_not_see_the_seed(tmp_path):
    """A lambdarank_ndcg fit under another objective_seed: the same trees, scores and, apart from the key itself, the same file."""
    import ptranking_amd as pa
    X, y, group = fit_data()
    params = dict(FIT_PARAMS, num_trees=4, lambdarank_truncation_level=10)
    a = pa.LambdaMART(params, objective="lambdarank_ndcg").fit(X, y, group)
    b = pa.LambdaMART(dict(params, objective_seed=99), objective="lambdarank_ndcg").fit(X, y, group)
    assert same_trees(a.booster, b.booster) and torch.equal(bits(a.booster.scores), bits(b.booster.scores))
    a.booster.save_model(tmp_path / "a.npz")
    b.booster.save_model(tmp_path / "b.npz")
    with np.load(tmp_path / "a.npz") as za, np.load(tmp_path / "b.npz") as zb:
        assert sorted(za.files) == sorted(zb.files)
        for k in za.files:
            if k == "params":
                import json
                pa_, pb_ = json.loads(str(za[k])), json.loads(str(zb[k]))
                assert pa_.pop("objective_seed") == 5 and pb_.pop("objective_seed") == 99 and pa_ == pb_
            else:
                assert za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes(), k


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
                          "--objective", "rank_xendcg", "--rounds", "10", "--num-leaves", "8", "--min-data-in-leaf", "5",
                          "--objective-seed", "7"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    constant = float(out.stdout.split("constant scores: valid nDCG@5 ")[1].split()[0])
    tenth = float(out.stdout.split("round 10: valid nDCG@5 ")[1].split()[0])
    assert tenth > constant and "test nDCG@5" in out.stdout, out.stdout
