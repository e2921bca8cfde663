"""CPU: WassRank (ptranking/ltr_adhoc/listwise/wassrank/wassRank.py) — the float64 log-domain restatement against the reference's own
outputs (tests/golden/wassrank.npz), the C-ABI entry's argument checks, the drop-in wiring into the reference's driver and the data-parallel
batch-mean step.  The HIP kernel itself is compared against the same fixtures in tests/test_wassrank_gpu.py."""
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
import wassrank_ref as W

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
