"""GPU: the position-debiased lambdarank (csrc/tree.hip tree_lambdarank_ndcg_kernel<G, true>, tree_position_bias_update_kernel) under the
element-wise float64 gate of tests/lambdarank_unbiased_ref.py, its identity with the plain kernel, the partition independence of the
fixed-point reduction, the update rule, NaN lists and a whole fit.  The gated tests print their worst needed constant before they assert."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import f64_loss_bounds as FB
import lambdarank_ndcg_ref as LR
import lambdarank_unbiased_ref as UR
import tree_ref as TR
from test_lambdarank_ndcg_gpu import FIT_PARAMS, Batch, dev, fit_data

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRADDLE = LR.STRADDLE
bits = lambda t: t.view(torch.int32)


def F_():
    import ptranking_amd.functional as f
    return f


def run(b, parts, T, norm, P, biases=None, pos=None, sigma=1.0):
    """The launches `parts` = [(max_len, queries or None)] into fresh outputs -> (grad, hess, cost_acc)."""
    acc = torch.zeros((2, P), device="cuda:0", dtype=torch.int64)
    out = (torch.full_like(b.preds, 7.0), torch.full_like(b.preds, 7.0))
    for max_len, queries in parts:
        F_().tree_lambdarank_unbiased_grad_hess(b.preds, b.labels, b.offsets, acc, biases, pos, T, sigma, norm, queries, max_len, out)
    return out[0], out[1], acc


@pytest.fixture(scope="module")
def straddle():
    return Batch(*LR.gpu_inputs()["straddle"])


@pytest.mark.parametrize("given,P", UR.VARIANTS)
@pytest.mark.parametrize("T,norm", [(T, norm) for T in (2, 30, 5000) for norm in (True, False)])
def test_ragged_batch_across_every_form_under_the_gate(straddle, T, norm, given, P):
    ref = UR.reference(T, norm)[(given, P)]
    pos = dev(UR.given_positions(STRADDLE)) if given else None
    grad, hess, acc = (t.cpu().numpy() for t in run(straddle, straddle.buckets, T, norm, P, dev(UR.draw_biases(P)), pos))
    assert not (grad == 7.0).any() and (hess >= 0).all() and (acc >= 0).all() and acc.sum() > 0
    w = max(TR.gate(grad, hess, ref, f"T {T} norm {norm} given {given} P {P}", UR.C), UR.gate_costs(acc, ref, f"T {T} norm {norm} given {given} P {P}"))
    print(f"kernel: worst err/E {w:.3f}: needs C_PAIR >= {w * FB.C_PAIR:.2f}")


@pytest.mark.parametrize("T,norm,sigma", [(30, True, 1.0), (2, True, 2.0), (5000, False, 1.0)])
def test_unit_and_null_biases_give_the_bits_of_lambdarank_ndcg(straddle, T, norm, sigma):
    want = straddle.bucketed(T, norm, sigma)
    for biases in (None, torch.ones((2, 30), device="cuda:0")):
        got = run(straddle, straddle.buckets, T, norm, 30, biases, dev(UR.given_positions(STRADDLE)), sigma)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1])) and int(got[2].sum()) > 0


@pytest.mark.parametrize("T,norm,P", [(30, True, 30), (5000, False, 256), (2, True, 3)])
def test_the_launch_partition_does_not_reach_a_bit(straddle, T, norm, P):
    B, t, pos = len(STRADDLE), dev(UR.draw_biases(P)), dev(UR.given_positions(STRADDLE))
    part = lambda qs: (int(max(STRADDLE[q] for q in qs)), dev(np.asarray(qs), np.int32))
    whole = run(straddle, [(max(STRADDLE), None)], T, norm, P, t, pos)
    others = {"repeated": [(max(STRADDLE), None)], "per class": straddle.buckets, "halves": [part(range(0, B, 2)), part(range(1, B, 2))],
              "alone": [part([q]) for q in range(B) if STRADDLE[q]]}
    for name, parts in others.items():
        got = run(straddle, parts, T, norm, P, t, pos)
        for a, b, what in zip(whole, got, ("grad", "hess", "cost_acc")):
            assert torch.equal(a.view(torch.int64) if what == "cost_acc" else bits(a), b.view(torch.int64) if what == "cost_acc" else bits(b)), (name, what)


@pytest.mark.parametrize("p_norm", [0.0, 0.5, 1.0])
def test_the_update_rule(p_norm):
    cost = np.array([[4.0, 1.0, 0.0, 2.0 ** -30, 9.0, 2.0 ** -32], [0.0, 3.0, 2.0, 1.0, 0.0, 5.0]])      # a zero cost, the floor; cost-[0] == 0
    acc = dev(np.rint(cost * 2.0 ** 32).astype(np.int64))
    start = np.random.default_rng(2).uniform(0.3, 1.2, cost.shape).astype(np.float32)
    biases = dev(start)
    _, costs = F_().tree_position_bias_update(acc, biases, p_norm, return_costs=True)
    want = UR.update(cost, start, p_norm)
    got = biases.cpu().numpy()
    assert np.array_equal(costs.cpu().numpy(), cost) and int(acc.abs().sum()) == 0
    assert (np.abs(got - want) <= 2.0 ** -24 * want).all() and np.array_equal(got[1], start[1]) and got[0, 2] == start[0, 2]
    assert got[0, 0] == 1.0 and got[0, 3] == np.float32(UR.FLOOR) and got[0, 4] > 1.0


def test_a_nan_list_is_nan_alone_and_adds_nothing_to_the_costs():
    s, y, group = LR.gpu_inputs()["nan"]
    off, pos = TR.offsets_of(group), UR.given_positions(group)
    keep = np.ones(len(s), bool)
    keep[off[1]:off[2]] = keep[off[3]:] = False
    clean = Batch(s[keep], y[keep], [group[0], group[2]])
    want = run(clean, clean.buckets, 30, True, 30, dev(UR.draw_biases(30)), dev(pos[keep]))
    for how in ("score", "label", "position"):
        s2, y2, p2 = s.copy(), y.copy(), pos.copy()
        for at in (off[1] + 40, off[3]):
            {"score": s2, "label": y2, "position": p2}[how][at] = -1 if how == "position" else np.nan
        b = Batch(s2, y2, group)
        for parts in (b.buckets, [(max(group), None)]):
            grad, hess, acc = run(b, parts, 30, True, 30, dev(UR.draw_biases(30)), dev(p2))
            for got, ok in ((grad, want[0]), (hess, want[1])):
                assert torch.isnan(got[~torch.from_numpy(keep)]).all() and torch.equal(bits(got[torch.from_numpy(keep)]), bits(ok)), how
            assert torch.equal(acc, want[2]) and int(acc.sum()) > 0, how


def test_a_whole_fit_threads_the_biases_through_the_rounds(monkeypatch):
    import ptranking_amd as pa
    from ptranking_amd import gbdt
    X, y, group = fit_data()
    pos = np.concatenate([np.random.default_rng(8).permutation(n) for n in group]).astype(np.int64)
    params = dict(FIT_PARAMS, num_trees=6, lambdarank_unbiased=True, lambdarank_bias_positions=12, lambdarank_bias_p_norm=1.0)
    seen, update = [], gbdt.GBDT.update

    def recording(self, grad, hess):
        seen.append((self.scores.clone(), grad.clone(), hess.clone()))
        return update(self, grad, hess)
    monkeypatch.setattr(gbdt.GBDT, "update", recording)
    lm = pa.LambdaMART(params, objective="lambdarank_ndcg").fit(X, y, group, position=pos)
    monkeypatch.setattr(gbdt.GBDT, "update", update)
    labels, offsets, p32 = dev(y), dev(TR.offsets_of(group), np.int64), dev(pos, np.int32)
    biases, acc = torch.ones((2, 12), device="cuda:0"), torch.zeros((2, 12), device="cuda:0", dtype=torch.int64)
    assert len(seen) == 6
    for t, (scores, grad, hess) in enumerate(seen):                              # one launch over all queries against fit's launches per class
        g, h = F_().tree_lambdarank_unbiased_grad_hess(scores, labels, offsets, acc, biases, p32, 10, 1.0, True)
        assert torch.equal(bits(g), bits(grad)) and torch.equal(bits(h), bits(hess)), t
        F_().tree_position_bias_update(acc, biases, 1.0)
    learned = lm.position_biases
    assert np.array_equal(learned, biases.cpu().numpy()) and learned.shape == (2, 12) and (learned[:, 0] == 1).all() and (learned != 1).any()
    again = pa.LambdaMART(params, objective="lambdarank_ndcg").fit(X, y, group, position=pos)
    assert torch.equal(bits(again.booster.scores), bits(lm.booster.scores)) and np.array_equal(again.position_biases, learned)
    off = pa.LambdaMART(dict(FIT_PARAMS, num_trees=6, lambdarank_unbiased=False), objective="lambdarank_ndcg").fit(X, y, group, position=pos)
    base = pa.LambdaMART(dict(FIT_PARAMS, num_trees=6), objective="lambdarank_ndcg").fit(X, y, group)
    assert torch.equal(bits(off.booster.scores), bits(base.booster.scores)) and not torch.equal(bits(base.booster.scores), bits(lm.booster.scores))
    with pytest.raises(ValueError, match="init_model"):
        pa.LambdaMART(params, objective="lambdarank_ndcg").fit(X, y, group, init_model=base)
    obj = pa.TreeObjective(y, group, "lambdarank_ndcg", truncation_level=10, unbiased=True, bias_p_norm=1.0, bias_positions=12, position=pos)
    for scores, grad, hess in seen[:3]:                                          # the same rounds through the LightGBM hook
        g, h = obj(scores.cpu().numpy())
        assert np.array_equal(g, grad.cpu().numpy().astype(np.float64)) and np.array_equal(h, hess.cpu().numpy().astype(np.float64))
    assert obj.position_biases.shape == (2, 12) and obj.uploads == 1


def test_the_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_lambdamart_unbiased.py"), "--queries", "300", "--rounds", "10"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "t+[p]" in out.stdout and out.stdout.count("nDCG@5 on the true grades") == 2, out.stdout
