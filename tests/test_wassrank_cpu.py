"""CPU: WassRank (ptranking/ltr_adhoc/listwise/wassrank/wassRank.py) — the float64 log-domain restatement against the reference's own
outputs (tests/golden/wassrank.npz), the C-ABI entry's argument checks, the drop-in wiring into the reference's driver and the data-parallel
batch-mean step.  The HIP kernel itself is compared against the same fixtures in tests/test_wassrank_gpu.py.  The second half: the
float64 error bounds of tests/wassrank_bounds.py (the gate of tests/test_wassrank_bounds_gpu.py) — the fixtures inside them, planted faults
that golden_util.assert_close lets through and the bounds do not, the screening of the gate's inputs, its coverage of the kernel's 20 forms,
and where C_WASS comes from."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import golden_util as G
import wassrank_bounds as WB
import wassrank_ref as W
from f64_loss_bounds import gate_losses
from launch_form import group_form

REF = os.environ.get("PTRANKING_REF") or "/root/reference"
NEEDS_REF = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "ptranking")),
                               reason="runs the reference's own driver: needs a wildltr/ptranking checkout (PTRANKING_REF)")
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-2,
      "pointsf": dict(num_features=10, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None,
                      bn_affine=False, dropout=0.0)}


def cases():
    return G._load("wassrank.npz")["wassrank"]


def case_kwargs(c):
    return dict(cost_type=W.COST_TYPES[int(c["cost_type"])], lam=float(c["lam"]), sh_itr=int(c["sh_itr"]), gain_base=float(c["gain_base"]),
                non_rele_gap=float(c["non_rele_gap"]), var_penalty=float(c["var_penalty"]), scale_by_max_label=bool(c["scale"]))


def test_golden_covers_the_issue_cases():
    d = cases()
    kws = [case_kwargs(c) for c in d.values()]
    assert {k["cost_type"] for k in kws} == set(W.COST_TYPES)
    assert {c["preds"].shape[1] for c in d.values()} >= {1, 2, 7, 64, 128, 256, 512}
    assert {round(k["lam"], 6) for k in kws} >= {0.01, 0.1, 1.0} and {k["sh_itr"] for k in kws} >= {0, 1, 20, 50}
    assert any(k["scale_by_max_label"] for k in kws)
    assert sum(not bool(c["ref32_finite"]) for c in d.values()) >= 3
    assert all(np.isfinite(c["loss64"]) and np.isfinite(c["grad64"]).all() for c in d.values())


@pytest.mark.parametrize("name", sorted(cases()))
def test_restatement_matches_the_reference(name):
    """float64 restatement == the reference's float64 component run; where the reference's own fp32 custom_loss_function is finite, the
    restatement is at least as close to float64 as it is, and agrees with it within that error."""
    c = cases()[name]
    loss, _, grad = W.batch(c["preds"], c["labels"], **case_kwargs(c))
    G.assert_close(np.array(loss), c["loss64"], f"{name} loss")
    G.assert_close(grad, c["grad64"], f"{name} grad")
    if bool(c["ref32_finite"]):
        e32_l = abs(float(c["loss32"]) - float(c["loss64"]))
        e32_g = np.abs(c["grad32"].astype(np.float64) - c["grad64"])
        assert abs(loss - float(c["loss64"])) <= e32_l + G.tol(c["loss64"])
        assert np.all(np.abs(grad - c["grad64"]) <= e32_g + G.tol(c["grad64"]))
        assert abs(loss - float(c["loss32"])) <= e32_l + G.tol(c["loss32"])
        assert np.max(np.abs(grad - c["grad32"])) <= G.tol(c["grad32"]) + np.max(e32_g)


def test_padded_batch_is_independent_queries():
    d = cases()
    a, b = d["eg_L64_s1"], d["p1_L7_s1"]
    P = np.zeros((2, 64), np.float32)
    Y = np.zeros((2, 64), np.float32)
    P[0], Y[0] = a["preds"][0], a["labels"][0]
    P[1, :7], Y[1, :7] = b["preds"][0], b["labels"][0]
    P[1, 7:], Y[1, 7:] = 5.0, 4.0                          # padding must not leak in
    for kw_case, q in ((a, 0), (b, 1)):
        loss, lq, grad = W.batch(P, Y, lens=np.array([64, 7]), **case_kwargs(kw_case))
        n = 64 if q == 0 else 7
        l1, g1 = W.query(P[q, :n], Y[q, :n], **case_kwargs(kw_case))
        assert lq[q] == pytest.approx(l1, rel=1e-12) and np.allclose(grad[q, :n], g1 / 2, rtol=1e-12, atol=0)
        assert np.all(grad[1, 7:] == 0.0)


def test_abi_errors_need_no_gpu():
    from ptranking_amd import build, _lib
    build.build()
    lib = _lib.load()
    one = ctypes.c_void_p(4096)
    f = ctypes.c_float

    def call(preds=one, labels=one, B=2, L=8, cost=2, lam=0.1, itr=20, lq=one, grad=one):
        return lib.ptr_wassrank_fwd_bwd(preds, labels, None, B, L, cost, f(4.0), f(100.0), f(2.718), f(lam), itr, 0, None, lq, grad, None)

    assert call(preds=None) == 1001 and b"NULL" in lib.ptr_last_error()
    assert call(lq=None) == 1001 and b"NULL" in lib.ptr_last_error()
    assert call(grad=None) == 1001
    assert call(cost=5) == 1001 and b"cost_type" in lib.ptr_last_error()
    assert call(cost=-1) == 1001
    assert call(lam=0.0) == 1001 and b"lam" in lib.ptr_last_error()
    assert call(lam=-1.0) == 1001
    assert call(itr=-1) == 1001 and b"sh_itr" in lib.ptr_last_error()
    assert call(L=4097) == 1002 and b"PTR_MAX_LIST_LEN" in lib.ptr_last_error()
    assert call(B=0) == 0                                 # an empty batch launches nothing


def test_functional_refuses_cpu_tensors_and_unknown_cost():
    import ptranking_amd as pa
    with pytest.raises(NotImplementedError, match="cost_type"):
        pa.functional.wassrank_loss(torch.zeros(1, 4), torch.zeros(1, 4), cost_type="Group")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pa.functional.wassrank_loss(torch.zeros(1, 4), torch.zeros(1, 4))


def test_constructor_and_unsupported_settings():
    import ptranking_amd as pa
    assert "WassRank" in pa.RANKER_NAMES and set(pa.EXTRA_RANKER_NAMES) == {"DASALC", "MDPRank"}
    import inspect
    assert list(inspect.signature(pa.WassRank.__init__).parameters) == \
        ["self", "sf_para_dict", "wass_para_dict", "dict_cost_mats", "dict_std_dists", "gpu", "device"]
    r = pa.WassRank(sf_para_dict=copy.deepcopy(SF), wass_para_dict=dict(pa.DEFAULT_PARAS["WassRank"]), gpu=False, device="cpu")
    assert r.TL_AF == "S"                                 # the stand-alone base returns TL_AF (and so scales by the maximum label)
    for key, val in (("mode", "EntropicOT"), ("smooth_type", "NG")):
        with pytest.raises(NotImplementedError, match=f"{key} {val!r}"):
            pa.WassRank(sf_para_dict=copy.deepcopy(SF), wass_para_dict=dict(pa.DEFAULT_PARAS["WassRank"], **{key: val}), gpu=False, device="cpu")


@NEEDS_REF
def test_default_paras_equal_the_reference():
    import ptranking_amd as pa
    sys.path.insert(0, REF)
    try:
        from ptranking.ltr_adhoc.listwise.wassrank.wassRank import WassRankParameter
        assert pa.DEFAULT_PARAS["WassRank"] == WassRankParameter().default_para_dict()
    finally:
        sys.path.remove(REF)


@NEEDS_REF
def test_install_and_the_drivers_load_ranker(monkeypatch):
    import ptranking_amd as pa
    import ptranking_amd.functional as F_
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    try:
        import ptranking.ltr_adhoc.eval.ltr as ref_ltr
        from ptranking.ltr_adhoc.listwise.wassrank.wassRank import WassRankParameter
        original = ref_ltr.WassRank
        installed = pa.install()
        try:
            assert ref_ltr.WassRank is installed["WassRank"] is not original
            ev = ref_ltr.LTREvaluator()
            ev.declare_global(model_id="WassRank")
            paras = WassRankParameter().default_para_dict()
            sf = copy.deepcopy(SF)
            ranker = ev.load_ranker(sf_para_dict=sf, model_para_dict=paras)
            assert type(ranker) is installed["WassRank"]
            assert ranker.dict_cost_mats is ev.dict_cost_mats and ranker.dict_std_dists is ev.dict_std_dists
            assert ranker.get_tl_af() is None and ranker.TL_AF is None      # the installed base's get_tl_af() returns None: no scaling
            ranker.init()
            seen = {}

            def restated(preds, labels, **kw):
                seen.update(kw)
                return W.wassrank_loss(preds, labels, **kw)

            monkeypatch.setattr(F_, "wassrank_loss", restated)
            rng = np.random.default_rng(4)
            X = torch.from_numpy(rng.standard_normal((3, 6, 10)).astype(np.float32))
            Y = torch.from_numpy(-np.sort(-rng.choice(3, size=(3, 6)).astype(np.float32), axis=1).copy())
            preds = ranker.forward(X)
            loss = ranker.custom_loss_function(preds, Y)                     # batch_ids / lens / label_type are not required
            assert seen["scale_by_max_label"] is False and seen["cost_type"] == "eg" and seen["sh_itr"] == 20
            ref_loss, _, _ = W.batch(preds.detach().numpy(), Y.numpy(), **{k: v for k, v in seen.items() if k != "lens"})
            assert float(loss) == pytest.approx(ref_loss, rel=1e-6)
            for key, val in (("mode", "EntropicOT"), ("smooth_type", "NG")):
                with pytest.raises(NotImplementedError, match=f"{key} {val!r}"):
                    ev.load_ranker(sf_para_dict=sf, model_para_dict=dict(paras, **{key: val}))
        finally:
            pa.uninstall()
        assert ref_ltr.WassRank is original
    finally:
        sys.path.remove(REF)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data(B=9, L=12, F=10):
    rng = np.random.default_rng(3)
    X = torch.from_numpy(rng.standard_normal((B, L, F)).astype(np.float32))
    Y = rng.choice(5, size=(B, L), p=[0.5, 0.3, 0.15, 0.03, 0.02]).astype(np.float32)
    Y[:, 0] = np.maximum(Y[:, 0], 1)
    return X, torch.from_numpy(-np.sort(-Y, axis=1).copy())


def _make():
    import ptranking_amd as pa
    torch.manual_seed(11)
    r = pa.WassRank(sf_para_dict=copy.deepcopy(SF), wass_para_dict=dict(pa.DEFAULT_PARAS["WassRank"]), gpu=False, device="cpu")
    r.init()
    r.train_mode()
    return r


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import ptranking_amd as pa
    import ptranking_amd.functional as F_
    from ptranking_amd import dp
    F_.wassrank_loss = W.wassrank_loss
    rk, ws, _ = dp.init_from_env(backend="gloo")
    assert (rk, ws) == (rank, world) and dp.is_distributed()
    X, Y = _data()
    lo, hi = dp.shard_queries(X.size(0))                    # unequal shards 5 + 4
    r = _make()
    dp.broadcast_parameters(r.get_parameters())
    losses, grads1 = [], None
    for step in range(3):
        loss, _ = r.train_op(X[lo:hi], Y[lo:hi], epoch_k=1, presort=True, label_type=pa.LABEL_TYPE.MultiLabel)
        losses.append(float(loss.detach()))
        if step == 0:
            grads1 = [p.grad.detach().clone() for p in r.get_parameters()]
    torch.save({"params": [p.detach().clone() for p in r.get_parameters()], "losses": losses, "shard": (lo, hi), "grads1": grads1},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_step_equals_single_process_full_batch(tmp_path, monkeypatch):
    import ptranking_amd as pa
    import ptranking_amd.functional as F_
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{i}.pt") for i in range(2))
    assert (r0["shard"], r1["shard"]) == ((0, 5), (5, 9))
    for a, b in zip(r0["params"], r1["params"]):
        assert torch.equal(a, b), "replicas diverged"
    monkeypatch.setattr(F_, "wassrank_loss", W.wassrank_loss)
    X, Y = _data()
    r = _make()
    ref_losses, ref_grads1 = [], None
    for step in range(3):
        loss, _ = r.train_op(X, Y, epoch_k=1, presort=True, label_type=pa.LABEL_TYPE.MultiLabel)
        ref_losses.append(float(loss.detach()))
        if step == 0:
            ref_grads1 = [p.grad.detach().clone() for p in r.get_parameters()]
    gmax = max(float(g.abs().max()) for g in ref_grads1)
    for a, b in zip(r0["grads1"], ref_grads1):
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, gmax)
    for a, b in zip(r0["params"], r.get_parameters()):
        assert float((a - b.detach()).abs().max()) <= 0.1 * 3 * SF["lr"]
    for step in range(3):                                   # the batch-mean loss of the GLOBAL batch on every rank
        assert abs(r0["losses"][step] - ref_losses[step]) <= 1e-4 * abs(ref_losses[step])
        assert abs(r1["losses"][step] - ref_losses[step]) <= 1e-4 * abs(ref_losses[step])


# ------------------------------------------------------------------------------------------------------- the float64 bounds (wassrank_bounds.py)
def _as_batch(out):
    """A wassrank_bounds.query result as the one-query batch wassrank_bounds.with_c takes."""
    return dict(q=np.arange(1), B=1, loss_q=np.array([out["loss"]]), A_loss_q=np.array([out["A_loss"]]), F_loss_q=np.array([out["F_loss"]]),
                grad=out["grad"][None, :], A_grad=out["A_grad"][None, :], F_grad=out["F_grad"][None, :])


def _new_gate(loss, grad, out, what):
    ref, total = WB.with_c(_as_batch(out))
    gate_losses(np.array([loss]), np.asarray(grad)[None, :], ref, what, WB.C_WASS, got_total=loss, total=total)


def _old_gate_excess(loss, grad, out):
    """By what factor golden_util.assert_close's tolerances (the max-norm rule and the element-wise one) are exceeded: <= 1 is accepted."""
    f = 0.0
    for got, ref in ((np.array([loss]), np.array([out["loss"]])), (np.asarray(grad), out["grad"])):
        err = np.abs(got - ref)
        el = G.EL_RTOL * np.abs(ref) + G.EL_FLOOR * max(1.0, float(np.abs(ref).max()))
        f = max(f, float(err.max() / G.tol(ref)), float((err / el).max()))
    return f


def _let_through_then_caught(loss, grad, out, what):
    """The planted fault passes golden_util.assert_close (or misses it by less than a factor of 2) and fails the float64 gate; the clean
    result passes both."""
    excess = _old_gate_excess(loss, grad, out)
    print(f"{what}: exceeds the golden gate's tolerance by a factor of {excess:.3g}")
    assert excess < 2.0, (what, excess)
    if excess <= 1.0:
        G.assert_close(np.array([loss]), np.array([out["loss"]]), what)
        G.assert_close(np.asarray(grad), out["grad"], what)
    _new_gate(out["loss"], out["grad"], out, f"{what} clean")
    with pytest.raises(AssertionError, match="f64 bound failed"):
        _new_gate(loss, grad, out, what)


def test_the_bounds_module_restates_the_same_values():
    rng = np.random.default_rng(0)
    for cost in W.COST_TYPES:
        for n in (0, 1, 2, 17, 65):
            s, y = rng.standard_normal(n).astype(np.float32), rng.choice(5, size=n).astype(np.float32)
            for kw in (dict(), dict(scale_by_max_label=True, lam=1.0, sh_itr=3), dict(gain_base=3.0, non_rele_gap=10.0, var_penalty=0.5)):
                l, g = W.query(s, y, cost_type=cost, **kw)
                o = WB.query(s, y, cost_type=cost, **kw)
                assert abs(l - o["loss"]) <= 1e-12 * max(1.0, abs(l)) and np.allclose(g, o["grad"], rtol=1e-10, atol=1e-15), (cost, n, kw)
                if n <= 1:
                    assert o["A_loss"] == 0.0 and o["F_loss"] == 0.0 and not o["A_grad"].any() and not o["F_grad"].any()
    P, Y, n, ref = WB.case_ref("ragged_L62_eg_scaled")
    lo, lq, g = W.batch(P, Y, n, **WB.CASE_BY_NAME["ragged_L62_eg_scaled"]["kw"])
    assert np.allclose(lq, ref["loss_q"], rtol=1e-12, atol=0) and np.allclose(g, ref["grad"], rtol=1e-10, atol=1e-16)
    pad = np.arange(P.shape[1])[None, :] >= n[:, None]
    assert not ref["A_grad"][pad].any() and not ref["F_grad"][pad].any() and not ref["grad"][pad].any()      # E = 0: exact zeros demanded


@pytest.mark.parametrize("name", sorted(cases()))
def test_every_fixture_lies_inside_the_float64_bound(name):
    """The reference's own float64 run (one shift per query) against the restatement (one maximum per row) under the gate the kernel gets."""
    c = cases()[name]
    out = WB.query(c["preds"][0], c["labels"][0], **case_kwargs(c))
    _new_gate(float(c["loss64"]), c["grad64"][0], out, name)


def test_planted_gradient_element_fault():
    """One gradient element moved by 1e-5 of the largest gradient entry."""
    for name in ("eg_L256_s1", "eg_L512_s1"):
        c = cases()[name]
        out = WB.query(c["preds"][0], c["labels"][0], **case_kwargs(c))
        g = out["grad"].copy()
        g[int(np.argmin(np.abs(g)))] += 1e-5 * np.abs(g).max()
        _let_through_then_caught(out["loss"], g, out, f"{name} planted gradient element")


def test_planted_missing_iteration_fault():
    """19 iterations where 20 were asked for, on a list whose scores sit within 3e-4 of its labels (a nearly converged plan: on the
    fixtures, whose 20th iteration still moves the result by 1e-2, the golden gate notices too)."""
    rng = np.random.default_rng(5)
    y = -np.sort(-rng.choice(5, size=64, p=[.5, .3, .13, .05, .02]).astype(np.float32))
    s = (y + 3e-4 * rng.standard_normal(64)).astype(np.float32)
    kw = dict(cost_type="eg", lam=0.01, sh_itr=20)
    out = WB.query(s, y, **kw)
    l19, g19 = W.query(s, y, **dict(kw, sh_itr=19))
    _let_through_then_caught(l19, g19, out, "one iteration fewer")


def test_planted_eg_diagonal_fault():
    """The eg diagonal costing var_penalty instead of 0 on a list with one document per label.  In the row passes alone (the loss sum keeps
    the right cost) the golden gate lets it through: log u and log v move by a constant that the centred gradient does not see, and the
    loss, 1.7e-39, moves to 1.1e-27 — both under that gate's absolute floor.  With the fault in the loss sum too the loss moves by
    var_penalty times the mass on the diagonal, which either gate rejects (the golden gate by 6e4 and more)."""
    y = np.array([2.0, 1.0, 0.0], np.float32)
    s = np.random.default_rng(1).standard_normal(3).astype(np.float32)
    out = WB.query(s, y, cost_type="eg")
    bad = WB.query(s, y, cost_type="eg", diag_fault="rows")
    _let_through_then_caught(bad["loss"], bad["grad"], out, "eg diagonal in the row passes")
    for yy in ([2.0, 1.0, 0.0], [4.0, 3.0, 2.0, 1.0, 0.0]):
        for lam in (0.1, 1.0):
            yy_, ss = np.array(yy, np.float32), np.random.default_rng(1).standard_normal(len(yy)).astype(np.float32)
            out = WB.query(ss, yy_, cost_type="eg", lam=lam)
            bad = WB.query(ss, yy_, cost_type="eg", lam=lam, diag_fault=True)
            assert _old_gate_excess(bad["loss"], bad["grad"], out) > 1e4
            with pytest.raises(AssertionError, match="f64 bound failed"):
                _new_gate(bad["loss"], bad["grad"], out, "eg diagonal everywhere")


def test_planted_padded_maximum_label_fault():
    """The maximum label taken over the padded width, whose padding holds a label 2e-5 above the list's own maximum of 4."""
    rng = np.random.default_rng(2)
    s = rng.standard_normal(100).astype(np.float32)
    y = -np.sort(-rng.choice(5, size=100, p=[.5, .3, .13, .05, .02]).astype(np.float32))
    y[0] = 4.0
    out = WB.query(s, y, cost_type="eg", scale_by_max_label=True)
    bad = WB.query(s, y, cost_type="eg", scale_by_max_label=True, m_fault=float(np.float32(4.00002)))
    _let_through_then_caught(bad["loss"], bad["grad"], out, "maximum label over the padding")


def test_gate_inputs_screen_the_eg_discontinuities():
    """Every random case keeps each eg gain and gain difference 1e-3 away from 1 (gate_inputs asserts that it moved under 1 % of the
    documents to get there); integer labels and the fractional set need no move at all.  The exact cases are inside the bands by design."""
    for case in WB.GATE_CASES:
        P, Y, n = WB.case_inputs(case)
        kw = case["kw"]
        assert WB.eg_screen_hits(Y, n, kw["gain_base"], kw["non_rele_gap"]) == 0
        assert list(n) == list(case["lens"]) and P.shape == (len(n), case["L"])
        for q, nq in enumerate(n):
            assert np.isnan(P[q, nq:]).all() and np.isfinite(P[q, :nq]).all() and np.all(Y[q, nq:] == WB.PAD_LABEL)
            assert nq == 0 or Y[q, :nq].max() < WB.PAD_LABEL
        rng = np.random.default_rng(case["seed"])                  # the screen moved nothing: the labels are the raw draws
        assert set(np.unique(Y[np.arange(P.shape[1])[None, :] < n[:, None]])) <= (set(range(5)) if case["labels"] == "mslr" else
                                                                                   set(np.float32(WB.FRAC_LABELS).tolist()))
    assert WB.eg_ambiguous(np.array([0.0, 1.0, 2.0]), 2.0, 25.0).tolist() == [False, True, False]      # gain exactly 1
    assert WB.eg_ambiguous(np.array([0.0, 0.5, 1.0]), 4.0, 100.0).tolist() == [False, True, False]
    assert WB.eg_ambiguous(np.array([0.5, 0.50001]), 4.0, 100.0).all()                                   # 4^y - 1 within 3e-5 of 1
    assert WB.eg_ambiguous(np.array([1.0, 1.161036, 3.0]), 4.0, 100.0).tolist() == [True, True, False]   # gains 3 and 4.0005: 1.0005 apart
    for spec in WB.EXACT_EG:
        P, Y, n = WB.exact_eg_inputs(spec)
        assert WB.eg_screen_hits(Y, n, spec["gain_base"], 100.0) > 0
        g, k = WB.eg_keys(np.asarray(spec["labels"]), spec["gain_base"], 100.0)
        assert g[1] == 1.0 and k[1] == 1.0 and k[0] == -100.0          # the restatement takes the `gain >= 1` branch


def test_the_gate_cases_reach_every_form_of_the_kernel():
    """The forms of ptr_wassrank_fwd_bwd, asked of the library: 64 threads x 1 column up to 64 documents of padded width, 64 x 2 up to 128,
    128 x 2 up to 256, 256 x 2 beyond; five costs each.  The ragged batches reach all 20 with scaling off and on, list lengths 0, 1, 2 and
    a ragged width in each; the widest form runs one, two and three column tiles, with one, two and four waves alive in the last."""
    form = lambda L: group_form("ptr_wassrank_fwd_bwd", L)
    assert [form(L) for L in (1, 64, 65, 128, 129, 256, 257, 4096)] == [(64, 1)] * 2 + [(64, 2)] * 2 + [(128, 2)] * 2 + [(256, 2)] * 2
    forms = {(64, 1), (64, 2), (128, 2), (256, 2)}
    for scale in (False, True):
        seen = {(c["kw"]["cost_type"], form(c["L"])) for c in WB.RAGGED_CASES if c["kw"]["scale_by_max_label"] is scale}
        assert seen == {(cost, f) for cost in W.COST_TYPES for f in forms}
    for c in WB.RAGGED_CASES:
        assert {0, 1, 2} <= set(c["lens"]) and max(c["lens"]) == c["L"]
    assert any(c["L"] % 4 for c in WB.RAGGED_CASES)
    for cost in W.COST_TYPES:
        wide = [c for c in WB.RAGGED_CASES if c["kw"]["cost_type"] == cost and form(c["L"]) == (256, 2)]
        tiles = {-(-n // 512) for c in wide for n in c["lens"] if n > 1}      # trips of the column-tile loop: 256 x 2 columns a tile
        assert tiles == {1, 2, 3}, (cost, tiles)
        last = {(-(-n // 512), -(-min((n - 1) % 512 + 1, 256) // 64)) for c in wide for n in c["lens"] if n > 1}
        assert {(2, 1), (2, 2), (2, 4), (3, 1), (1, 4)} <= last, (cost, last)
    sweep = WB.SWEEP_CASES
    assert {form(c["L"]) for c in sweep} == {(64, 2), (256, 2)}
    for L in WB.SWEEP_LENS:
        here = [c for c in sweep if c["L"] == L]
        assert {(c["kw"]["lam"], c["kw"]["sh_itr"]) for c in here if c["kw"]["cost_type"] == "eg"} >= \
            {(lam, itr) for lam in WB.SWEEP_LAMS for itr in WB.SWEEP_ITRS}
        assert {c["kw"]["cost_type"] for c in here} == set(W.COST_TYPES)
        assert {(c["kw"]["gain_base"], c["kw"]["non_rele_gap"], c["kw"]["var_penalty"]) for c in here} >= set(WB.ALT_EG)
        assert any(c["labels"] == "frac" for c in here) and any(c["sigmas"] == (10.0,) for c in here)
    assert len({c["name"] for c in WB.GATE_CASES}) == len(WB.GATE_CASES)


def test_c_wass_is_twice_the_fp32_need_rounded_up_to_a_half():
    """C_WASS is not chosen: it is 2 x what the fp32 eager-torch evaluation of the same formulas needs of these bounds on the very batches of
    the GPU gate, rounded up to a half — that value, or one step above it where another machine's torch sums in another order and needs less."""
    need = WB.measure_fp32_need()
    print("MEASURED fp32 need of the eager-torch evaluation per output: " + ", ".join(f"{k} {v:.2f} ({n})" for k, (v, n) in need.items()))
    derived = WB.constant_from_need(max(v for v, _ in need.values()))
    assert 0.0 <= WB.C_WASS - derived <= 0.5, (need, derived, WB.C_WASS)
