"""GPU: the WassRank kernel (ptr_wassrank_fwd_bwd, csrc/wassrank.hip) against the reference's float64 outputs (tests/golden/wassrank.npz,
tests/golden/make_golden_wassrank.py), batch semantics, list lengths up to PTR_MAX_LIST_LEN, run-to-run stability and the ranker step."""
import copy
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest
import torch

import golden_util as G
import wassrank_ref as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cases():
    return G._load("wassrank.npz")["wassrank"]


def case_kwargs(c):
    return dict(cost_type=W.COST_TYPES[int(c["cost_type"])], lam=float(c["lam"]), sh_itr=int(c["sh_itr"]), gain_base=float(c["gain_base"]),
                non_rele_gap=float(c["non_rele_gap"]), var_penalty=float(c["var_penalty"]), scale_by_max_label=bool(c["scale"]))


def run(preds, labels, lens=None, cost_type="eg", lam=0.1, sh_itr=20, gain_base=4.0, non_rele_gap=100.0, var_penalty=np.e,
        scale_by_max_label=False):
    """The raw entry point: (loss_out, loss_q [B], grad [B, L]) as numpy."""
    from ptranking_amd import _lib
    p = torch.as_tensor(np.asarray(preds, np.float32)).to(DEV).contiguous()
    y = torch.as_tensor(np.asarray(labels, np.float32)).to(DEV).contiguous()
    B, L = p.shape
    ln = None if lens is None else torch.as_tensor(np.asarray(lens, np.int32)).to(DEV)
    out = torch.full((1,), float("nan"), device=DEV)
    lq = torch.full((B,), float("nan"), device=DEV)
    g = torch.full((B, L), float("nan"), device=DEV)
    _lib.call("ptr_wassrank_fwd_bwd", _lib.ptr(p), _lib.ptr(y), _lib.ptr(ln), B, L, W.COST_TYPES.index(cost_type), C.c_float(gain_base),
              C.c_float(non_rele_gap), C.c_float(var_penalty), C.c_float(lam), int(sh_itr), int(bool(scale_by_max_label)), _lib.ptr(out),
              _lib.ptr(lq), _lib.ptr(g), _lib.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return float(out.item()), lq.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("name", sorted(cases()))
def test_golden_case_against_float64_reference(name):
    """The kernel against the reference's float64 run under the repository's 1e-5 gate (max-norm and element-wise), through the public
    functional API; cases where the reference's own fp32 run is NaN give finite results here."""
    import ptranking_amd as pa
    c = cases()[name]
    p = torch.from_numpy(c["preds"]).to(DEV).requires_grad_(True)
    loss = pa.functional.wassrank_loss(p, torch.from_numpy(c["labels"]).to(DEV), **case_kwargs(c))
    loss.backward()
    lo, g = loss.item(), p.grad.cpu().numpy()
    assert np.isfinite(lo) and np.isfinite(g).all()
    G.assert_close(np.array(lo), c["loss64"], f"{name} loss")
    G.assert_close(g, c["grad64"], f"{name} grad")


def test_stacked_cases_give_the_mean_and_scaled_gradient():
    """B = 1 cases that share length and parameters, stacked into one batch: the mean loss, and each query's grad64 / B."""
    groups = defaultdict(list)
    for name, c in sorted(cases().items()):
        groups[(c["preds"].shape[1], tuple(sorted(case_kwargs(c).items())))].append(c)
    groups = [v for v in groups.values() if len(v) >= 2]
    assert groups
    for grp in groups:
        B = len(grp)
        kw = case_kwargs(grp[0])
        lo, lq, g = run(np.concatenate([c["preds"] for c in grp]), np.concatenate([c["labels"] for c in grp]), **kw)
        ref = np.array([float(c["loss64"]) for c in grp])
        G.assert_close(lq, ref, "loss_q")
        G.assert_close(np.array(lo), ref.mean(), "loss_out")
        G.assert_close(g, np.concatenate([c["grad64"] for c in grp]) / B, "grad")


def test_padded_batch_with_mixed_lens():
    """Queries of 1 .. 512 documents padded to 512: each gives its unpadded result (grad / B) and exactly 0 on padded documents."""
    d = cases()
    names = ["eg_L1", "eg_L2", "eg_L7_s1", "eg_L64_s1", "eg_zero_L64", "eg_equal_L64", "eg_L128_s3", "eg_frac_L256", "eg_L512_s3"]
    B, L = len(names), 512
    rng = np.random.default_rng(9)
    P = rng.standard_normal((B, L)).astype(np.float32) * 50.0        # padding: large values that must not leak in
    Y = np.full((B, L), 4.0, np.float32)
    lens = np.zeros(B, np.int32)
    for q, n in enumerate(names):
        m = d[n]["preds"].shape[1]
        P[q, :m], Y[q, :m], lens[q] = d[n]["preds"][0], d[n]["labels"][0], m
        assert case_kwargs(d[n]) == case_kwargs(d["eg_L7_s1"])
    lo, lq, g = run(P, Y, lens=lens, **case_kwargs(d["eg_L7_s1"]))
    for q, n in enumerate(names):
        m = lens[q]
        G.assert_close(lq[q:q + 1], np.array([float(d[n]["loss64"])]), f"{n} loss_q")
        G.assert_close(g[q, :m], d[n]["grad64"][0] / B, f"{n} grad")
        assert np.all(g[q, m:] == 0.0), n
    G.assert_close(np.array(lo), np.mean([float(d[n]["loss64"]) for n in names]), "loss_out")


@pytest.mark.parametrize("B,L,cost,sample", [(4096, 128, "eg", 6), (64, 1251, "eg", 3), (64, 1251, "ddg", 2), (2, 4096, "eg", 1),
                                             (2, 4096, "p1", 1)])
def test_sizes_against_float64_restatement(B, L, cost, sample):
    rng = np.random.default_rng(B + L)
    P = rng.standard_normal((B, L)).astype(np.float32)
    Y = -np.sort(-rng.choice(5, size=(B, L), p=[0.5147, 0.3250, 0.1339, 0.0183, 0.0081]).astype(np.float32), axis=1)
    lens = rng.integers(max(2, L // 2), L + 1, size=B).astype(np.int32)
    lens[0] = L
    lo, lq, g = run(P, Y, lens=lens, cost_type=cost)
    assert np.isfinite(lq).all() and np.isfinite(g).all() and np.isfinite(lo)
    for q in sorted({0, B - 1, *rng.integers(0, B, size=sample).tolist()}):
        n = lens[q]
        l64, g64 = W.query(P[q, :n], Y[q, :n], cost_type=cost)
        G.assert_close(lq[q:q + 1], np.array([l64]), f"q{q} loss")
        G.assert_close(g[q, :n] * B, g64, f"q{q} grad")
        assert np.all(g[q, n:] == 0.0)


@pytest.mark.parametrize("cost", W.COST_TYPES)
def test_two_launches_are_bit_identical(cost):
    rng = np.random.default_rng(1)
    P = rng.standard_normal((37, 700)).astype(np.float32)
    Y = rng.choice(5, size=(37, 700)).astype(np.float32)
    lens = rng.integers(2, 701, size=37).astype(np.int32)
    a = run(P, Y, lens=lens, cost_type=cost)
    b = run(P, Y, lens=lens, cost_type=cost)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _ranker(sf):
    import ptranking_amd as pa
    torch.manual_seed(5)
    r = pa.WassRank(sf_para_dict=copy.deepcopy(sf), wass_para_dict=dict(pa.DEFAULT_PARAS["WassRank"]), gpu=True, device=DEV)
    r.init()
    r.train_mode()
    return r


def _mslr(B, L, F, seed):
    rng = np.random.default_rng(seed)
    X = torch.from_numpy(rng.standard_normal((B, L, F)).astype(np.float32)).to(DEV)
    Y = rng.choice(5, size=(B, L), p=[0.5147, 0.3250, 0.1339, 0.0183, 0.0081]).astype(np.float32)
    Y[:, 0] = np.maximum(Y[:, 0], 1)
    return X, torch.from_numpy(-np.sort(-Y, axis=1).copy()).to(DEV)


SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=136, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False)}


def test_ranker_step_equals_the_hand_composed_step():
    import ptranking_amd as pa
    from ptranking_amd.scorer import FusedPointScorer
    X, Y = _mslr(16, 128, 136, 3)
    r1, r2 = _ranker(SF), _ranker(SF)
    assert isinstance(r1.point_sf, FusedPointScorer)
    for a, b in zip(r1.get_parameters(), r2.get_parameters()):
        assert torch.equal(a, b)
    torch.manual_seed(7)                                   # the scorer's dropout seed comes from torch's CPU generator
    loss1 = r1.custom_loss_function(r1.forward(X), Y, batch_ids=["q"] * 16, label_type=pa.LABEL_TYPE.MultiLabel)
    wd = r2.wass_para_dict
    torch.manual_seed(7)
    preds = r2.forward(X)
    loss2 = pa.functional.wassrank_loss(preds, Y, cost_type=wd["cost_type"], lam=wd["lam"], sh_itr=wd["sh_itr"], gain_base=wd["gain_base"],
                                        non_rele_gap=wd["non_rele_gap"], var_penalty=wd["var_penalty"], scale_by_max_label=True)
    r2.optimizer.zero_grad()
    loss2.backward()
    r2.optimizer.step()
    torch.cuda.synchronize()
    assert loss1.item() == loss2.item()
    for a, b in zip(r1.get_parameters(), r2.get_parameters()):
        assert torch.equal(a, b)


def test_twenty_steps_stay_finite():
    import ptranking_amd as pa
    X, Y = _mslr(64, 200, 136, 4)
    lens = torch.randint(20, 201, (64,), dtype=torch.int32, generator=torch.Generator().manual_seed(2)).to(DEV)
    r = _ranker(SF)
    losses = []
    for _ in range(20):
        loss = r.custom_loss_function(r.forward(X), Y, lens=lens)
        losses.append(loss.item())
    assert np.isfinite(losses).all(), losses
    assert all(torch.isfinite(p).all() for p in r.get_parameters())
