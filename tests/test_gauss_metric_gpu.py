"""GPU: the Gaussian expected-rank metric objectives (csrc/gaussmetric.hip, ptr_gaussmetric_fwd_bwd) — P, AP, nERR and nDCG on the expected
ranks of documents with normal scores, every form (opt_ideal x top_k), every kernel instantiation, both gradients.

  1. every run of tests/golden/gauss_metric.npz (the reference's own get_expected_rank -> *_as_opt_objective -> autograd) through the C ABI
     under golden_util.assert_close against the reference's FLOAT64; `pos` is exactly the reference's sort order; NaN placement and valid_q
     exactly;
  2. the float64 gate (tests/gauss_metric_ref.py, c = C_GAUSS): ranks, loss_q, every element of both gradients and the batch total, each
     under its own bound, on ragged NaN-padded batches (gauss_metric_ref.GATE_BATCHES: every register width, every workgroup form, a mean
     offset of 1e3, the learned-head and the saturated variance regimes).  The re-sorted forms threefold: pos is the (rank, index) order of
     the kernel's own ranks; an adjacent pair in that order inverts the float64 ranks only within the two rank bounds; loss and gradients
     against the restatement evaluated WITH the kernel's pos;
  3. const_std against filled vars, bit identity alone / in a batch / in halves / repeated, all-equal documents, autograd;
  4. the ProbSmoothMetric ranker: one-query steps, 20 steps per metric and mode, a filtered batch, two ranks on one GPU, the example.
"""
import copy
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gauss_metric_ref as GR
import golden_util as GU
from f64_loss_bounds import batch_total, gate_nan
from gauss_metric_ref import C_GAUSS, NAMES

pytestmark = pytest.mark.gpu

GOLDEN = GU._load("gauss_metric.npz")
CASES = [(fam, name) for fam in ("main", "edge") for name in GOLDEN[fam]]


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def run_abi(mus, vars_, labels, lens, metric, opt_ideal, top_k, max_label=None, const_std=None, own_loss=True):
    """One call of the entry point on numpy inputs -> dict of numpy outputs.  vars_ None: the constant-variance form (grad_var NULL)."""
    from ptranking_amd import _lib
    m, y = dev(np.atleast_2d(mus)), dev(np.atleast_2d(labels))
    v = None if vars_ is None else dev(np.atleast_2d(vars_))
    B, L = m.shape
    ln = None if lens is None else dev(lens, torch.int32)
    new = lambda *s: torch.full(s, 7.0, device="cuda")
    loss, lq, vq, rk, ws, gm = new(1), new(max(B, 1)), new(max(B, 1)), new(max(B, 1), L), new(1), new(max(B, 1), L)
    gv = None if v is None else new(max(B, 1), L)
    ps = torch.full((max(B, 1), L), 7, device="cuda", dtype=torch.int32)
    _lib.call("ptr_gaussmetric_fwd_bwd", _lib.ptr(m), _lib.ptr(v), _lib.ptr(y), _lib.ptr(ln), B, L, NAMES.index(metric), int(bool(opt_ideal)),
              int(top_k or 0), C.c_float(0.0 if const_std is None else const_std), C.c_float(-1.0 if max_label is None else max_label),
              _lib.ptr(loss) if own_loss else None, _lib.ptr(lq), _lib.ptr(vq), _lib.ptr(rk), _lib.ptr(ps), _lib.ptr(ws), _lib.ptr(gm), _lib.ptr(gv),
              _lib.current_stream(m.device))
    torch.cuda.synchronize()
    return dict(loss=float(loss[0]), loss_q=lq[:B].cpu().numpy(), valid_q=vq[:B].cpu().numpy(), ranks=rk[:B].cpu().numpy(), pos=ps[:B].cpu().numpy(),
                grad_mu=gm[:B].cpu().numpy(), grad_var=None if gv is None else gv[:B].cpu().numpy(), max_label_ws=float(ws[0]))


# ------------------------------------------------------------------------------------------------------------------------ 1. golden
@pytest.mark.parametrize("fam,name", CASES)
def test_golden_against_the_reference_float64(fam, name):
    case = GOLDEN[fam][name]
    const = float(case["const_std"]) if "const_std" in case else None
    order = np.atleast_2d(case["order"])
    for k, (m, oi, tk) in enumerate(case["combos"]):
        what = f"{fam}/{name} {NAMES[m]} opt_ideal={oi} top_k={tk}"
        r64, valid = case["res64"][k], case["valid"][k]
        ml = None if name == "batch3" else float(case["max_label"])
        out = run_abi(case["mus"], case.get("vars"), case["labels"], None, NAMES[m], oi, int(tk), ml, const)
        got = np.concatenate([[out["loss"]], out["grad_mu"].reshape(-1)] + ([] if const else [out["grad_var"].reshape(-1)]))
        assert np.array_equal(np.isnan(got), np.isnan(r64)), f"{what}: NaN placement, got {got}, reference {r64}"
        fin = np.isfinite(r64)
        assert np.isfinite(got[fin]).all(), what
        if fin.any():
            GU.assert_close(got[fin], r64[fin], what)
        GU.assert_close(out["ranks"], np.atleast_2d(case["ranks64"]), f"{what} ranks")
        assert np.array_equal(out["valid_q"], valid), f"{what}: valid_q {out['valid_q']} vs {valid}"
        # pos_i = the place of document i in the reference's torch.sort of the ranks (the input index under opt_ideal)
        want = np.argsort(order, axis=1) if not oi else np.broadcast_to(np.arange(order.shape[1]), order.shape)
        assert np.array_equal(out["pos"], want), f"{what}: pos {out['pos']} vs {want}"
        if name == "batch3" and NAMES[m] == "nERR":
            assert out["max_label_ws"] == float(case["max_label"])
        assert np.all(out["loss_q"][valid == 0] == 0.0) and np.all(out["grad_mu"][valid == 0] == 0.0), what
        if not const:
            assert np.all(out["grad_var"][valid == 0] == 0.0), what


# ------------------------------------------------------------------------------------------------------------------------ 2. float64 gate
TOP_KS = (None, 1, 10, 5000)
OUTPUTS = ("ranks", "loss_q", "grad_mu", "grad_var", "loss_out")


@pytest.fixture(scope="module")
def gate_data():
    """The inputs and the metric-independent half of the float64 reference (expected ranks, pair derivatives, their bounds), computed once."""
    out = []
    for k, (L, lens, regime) in enumerate(GR.GATE_BATCHES):
        m, v, y, n = GR.gate_inputs(L, lens, regime, seed=900 + k)
        out.append((L, regime, m, v, y, n, GR.stages(m, v, n, C_GAUSS)))
    return out


def check_order(out, st, n, opt_ideal, what):
    """pos: the input index under opt_ideal; else exactly the (rank ascending, index ascending) order of the kernel's OWN ranks, in which an
    adjacent pair inverts the float64 ranks only within the sum of the two documents' rank bounds.  -1 on padding."""
    L = out["pos"].shape[1]
    for q, nq in enumerate(n):
        assert np.all(out["pos"][q, nq:] == -1), f"{what}: pos on padding"
        if nq == 0:
            continue
        if opt_ideal:
            assert np.array_equal(out["pos"][q, :nq], np.arange(nq)), f"{what}: pos under opt_ideal"
            continue
        assert np.array_equal(out["pos"][q, :nq], GR.positions(out["ranks"][q, :nq])), f"{what}: pos is not the order of the kernel's ranks (query {q})"
        order = np.argsort(out["pos"][q, :nq])
        r64, E = st[q].r[order], st[q].E_r[order]
        inv = r64[:-1] - r64[1:]
        assert np.all(inv <= E[:-1] + E[1:]), f"{what}: an inversion of the float64 ranks beyond the rank bounds (query {q}, worst {inv.max():.3e})"


def gate_outputs(out, ref, what, c=C_GAUSS):
    """ranks, loss_q, every element of both gradients and the batch total under their own bounds; valid_q exactly.  Worst err/E per output."""
    q = ref["q"]
    total = batch_total(ref, c)
    w = dict(ranks=gate_nan(out["ranks"], ref["ranks"], ref["E_ranks"], f"{what} ranks", c),
             loss_q=gate_nan(out["loss_q"][q], ref["loss_q"], ref["E_loss_q"], f"{what} loss_q", c),
             grad_mu=gate_nan(out["grad_mu"][q], ref["grad_mu"], ref["E_grad_mu"], f"{what} grad_mu", c),
             grad_var=gate_nan(out["grad_var"][q], ref["grad_var"], ref["E_grad_var"], f"{what} grad_var", c),
             loss_out=gate_nan(np.array([out["loss"]]), np.array([total[0]]), np.array([total[1]]), f"{what} loss_out", c))
    assert np.array_equal(out["valid_q"], ref["valid_q"]), f"{what}: valid_q"
    return w


@pytest.mark.parametrize("opt_ideal", [True, False])
@pytest.mark.parametrize("metric", NAMES)
def test_float64_gate_on_every_form(gate_data, metric, opt_ideal):
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for L, regime, m, v, y, n, st in gate_data:
        for tk in TOP_KS:
            what = f"{metric} opt_ideal={opt_ideal} top_k={tk} L={L} {regime}"
            out = run_abi(m, v, y, n, metric, opt_ideal, tk, None)
            check_order(out, st, n, opt_ideal, what)
            ref = GR.batch(st, y, n, metric, tk, opt_ideal, None, pos=out["pos"])
            w = gate_outputs(out, ref, what)
            worst = {k: max(worst[k], w[k]) for k in OUTPUTS}
            pad = np.arange(L)[None, :] >= n[:, None]
            assert np.all(out["grad_mu"][pad] == 0.0) and np.all(out["grad_var"][pad] == 0.0) and np.all(out["ranks"][pad] == 0.0)
    print(f"MEASURED {metric} opt_ideal={opt_ideal}, needed constant per output (C_GAUSS = {C_GAUSS:g}): "
          + ", ".join(f"{k} {worst[k] * C_GAUSS:.2f}" for k in OUTPUTS))


# ------------------------------------------------------------------------------------------------------------------------ 3. identities
def plain_inputs(L, lens, regime, seed):
    m, v, y, n = GR.gate_inputs(L, lens, regime, seed)
    return np.nan_to_num(m, nan=0.0), np.nan_to_num(v, nan=1.0), np.nan_to_num(y, nan=0.0), n


@pytest.mark.parametrize("L,lens", [(64, [64, 1, 17, 0]), (1024, [1024, 513, 2])])
@pytest.mark.parametrize("metric,opt_ideal,top_k", [("AP", False, 10), ("nERR", True, None)])
def test_const_std_is_bit_identical_to_filled_vars(L, lens, metric, opt_ideal, top_k):
    m, _, y, n = plain_inputs(L, lens, "wide", seed=61)
    std = 0.7
    fill = np.full(m.shape, np.float32(float(np.float32(std)) ** 2), np.float32)     # the double product of the fp32 const_std, rounded once
    a = run_abi(m, None, y, n, metric, opt_ideal, top_k, 4.0, const_std=std)
    b = run_abi(m, fill, y, n, metric, opt_ideal, top_k, 4.0)
    assert a["grad_var"] is None
    for k in ("loss_q", "grad_mu", "ranks", "pos", "valid_q"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["loss"] == b["loss"]


@pytest.mark.parametrize("L,lens", [(128, [128, 65, 1, 90, 0, 127, 3, 100]), (1024, [1024, 513, 700]), (4096, [0, 1, 2, 64, 130, 2049])])
@pytest.mark.parametrize("metric,opt_ideal,top_k", [("AP", False, 10), ("nERR", True, None), ("P", False, None), ("nDCG", False, 1)])
def test_a_query_alone_in_a_batch_in_halves_and_repeated_is_bit_identical(L, lens, metric, opt_ideal, top_k):
    m, v, y, n = plain_inputs(L, lens, "wide", seed=77)
    keys = ("loss_q", "grad_mu", "grad_var", "ranks", "pos", "valid_q")
    full = run_abi(m, v, y, n, metric, opt_ideal, top_k, 4.0)
    again = run_abi(m, v, y, n, metric, opt_ideal, top_k, 4.0)
    h = len(lens) // 2
    halves = [run_abi(m[a:b], v[a:b], y[a:b], n[a:b], metric, opt_ideal, top_k, 4.0) for a, b in ((0, h), (h, len(lens)))]
    for k in keys:
        assert np.array_equal(full[k], again[k], equal_nan=True), k
        assert np.array_equal(full[k], np.concatenate([halves[0][k], halves[1][k]]), equal_nan=True), k
    for q in range(len(lens)):
        one = run_abi(m[q:q + 1], v[q:q + 1], y[q:q + 1], n[q:q + 1], metric, opt_ideal, top_k, 4.0)
        for k in keys:
            assert np.array_equal(full[k][q:q + 1], one[k], equal_nan=True), (k, q)


@pytest.mark.parametrize("L,n", [(128, 70), (600, 600)])
def test_all_equal_documents_rank_by_index(L, n):
    """Ties: every mean and every variance equal.  Every pair has Phi = 1 / 2 exactly: the expected ranks are (n + 1) / 2, the hard positions
    the indices, so the re-sorted forms return the bits of the ideal-order forms."""
    from f64_loss_bounds import labels_like
    m, v = np.full((1, L), 1000.25, np.float32), np.full((1, L), 0.3, np.float32)
    y = np.zeros((1, L), np.float32)
    y[0, :n] = -np.sort(-labels_like(1, n, "mslr", np.random.default_rng(3))[0])
    y[0, 0] = max(y[0, 0], 1.0)
    lens = np.asarray([n], np.int32)
    st = GR.stages(m, v, lens, C_GAUSS)
    for metric in NAMES:
        for tk in (None, 10):
            ideal = run_abi(m, v, y, lens, metric, True, tk, 4.0)
            assert np.all(ideal["ranks"][0, :n] == (n + 1) / 2.0)
            gate_outputs(ideal, GR.batch(st, y, lens, metric, tk, True, 4.0), f"ties {metric} top_k={tk} ideal")
            resort = run_abi(m, v, y, lens, metric, False, tk, 4.0)
            assert np.array_equal(resort["pos"][0, :n], np.arange(n))
            gate_outputs(resort, GR.batch(st, y, lens, metric, tk, False, 4.0, pos=resort["pos"]), f"ties {metric} top_k={tk} re-sorted")
            if not (metric == "AP" and tk is None):                 # (the re-sorted full-list AP is the reference's other formula)
                for k in ("loss_q", "grad_mu", "grad_var", "ranks"):
                    assert np.array_equal(ideal[k], resort[k]), (metric, tk, k)


def test_autograd_scales_both_gradients_and_runs_through_an_exp_head():
    import ptranking_amd.functional as F
    m, v, y, n = plain_inputs(128, [128, 65, 90], "wide", seed=78)
    lens = dev(n, torch.int32)
    for metric, oi, tk in (("AP", False, 10), ("nERR", True, None)):
        raw = run_abi(m, v, y, n, metric, oi, tk, None, own_loss=False)
        mu, var = dev(m).requires_grad_(True), dev(v).requires_grad_(True)
        loss, parts = F.gaussian_metric_objective(mu, var, dev(y), metric, top_k=tk, opt_ideal=oi, lens=lens, return_parts=True)
        (loss * -2.5).backward()
        assert torch.equal(mu.grad, dev(raw["grad_mu"]) * -2.5) and torch.equal(var.grad, dev(raw["grad_var"]) * -2.5)
        for k in ("loss_q", "ranks", "valid_q", "pos"):
            assert np.array_equal(parts[k].cpu().numpy(), raw[k]), k
        assert parts["ranks"].shape == (3, 128) and parts["pos"].dtype == torch.int32
        plain = F.gaussian_metric_objective(dev(m), dev(v), dev(y), metric, top_k=tk, opt_ideal=oi, lens=lens)
        assert not plain.requires_grad and torch.equal(plain, loss.detach())
        # through an exp head: d loss / d s = d loss / d var * exp(s)
        s = torch.log(dev(v)).requires_grad_(True)
        var2 = torch.exp(s)
        out = run_abi(m, var2.detach().cpu().numpy(), y, n, metric, oi, tk, None)
        F.gaussian_metric_objective(dev(m), var2, dev(y), metric, top_k=tk, opt_ideal=oi, lens=lens).backward()
        assert torch.equal(s.grad, dev(out["grad_var"]) * var2.detach())
        # the constant-variance form is differentiable in the means alone
        mu2 = dev(m).requires_grad_(True)
        F.gaussian_metric_objective(mu2, None, dev(y), metric, top_k=tk, opt_ideal=oi, lens=lens, const_std=0.5).backward()
        assert torch.equal(mu2.grad, dev(run_abi(m, None, y, n, metric, oi, tk, None, const_std=0.5)["grad_mu"]))
    with pytest.raises(ValueError):
        F.gaussian_metric_objective(dev(m), dev(v), dev(y), "MRR")
    with pytest.raises(ValueError):
        F.gaussian_metric_objective(dev(m), None, dev(y), "AP")


# ------------------------------------------------------------------------------------------------------------------------ 4. the ranker
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=24, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False, dropout=0.0)}
KW = dict(epoch_k=1, presort=True)


def _data(B=12, L=64, F=24):
    rng = np.random.default_rng(5)
    Y = rng.choice(5, size=(B, L), p=[0.5, 0.3, 0.15, 0.03, 0.02]).astype(np.float32)
    Y[:, 0] = np.maximum(Y[:, 0], 1)
    Y = -np.sort(-Y, axis=1)
    X = rng.standard_normal((B, L, F)).astype(np.float32)
    X[:, :, :4] += 0.5 * Y[:, :, None]
    return torch.from_numpy(X), torch.from_numpy(Y.copy())


def _make(lr=1e-3, **over):
    import ptranking_amd as pa
    torch.manual_seed(21)
    sf = copy.deepcopy(SF)
    sf["lr"] = lr
    r = pa.ProbSmoothMetric(sf_para_dict=sf, model_para_dict={**pa.DEFAULT_PARAS["ProbSmoothMetric"], **over}, gpu=True, device="cuda:0")
    r.init()
    r.train_mode()
    return r


def _flat_grad(r):
    return torch.cat([p.grad.detach().reshape(-1) for g in r.optimizer.param_groups for p in g["params"]])


def _flat_params(r):
    return torch.cat([p.detach().reshape(-1) for g in r.optimizer.param_groups for p in g["params"]])


@pytest.mark.parametrize("metric,opt_ideal,top_k,head", [("AP", False, 10, dict(limit_delta=0.01)), ("nERR", True, 5, dict(limit_delta=None)),
                                                         ("nDCG", False, None, dict(const_std=0.5))])
def test_one_query_steps_add_up_to_the_batched_step(metric, opt_ideal, top_k, head):
    """The parameter gradient of a batched step is the sum of the gradients of the one-query steps (the loss is a sum over queries): within
    the 2e-5 of the largest element that the data-parallel tests hold a split batch to."""
    import ptranking_amd as pa
    X, Y = _data()
    r = _make(metric=metric, opt_ideal=opt_ideal, top_k=top_k, max_label=4.0, **head)
    assert r.forward(X[:1].cuda()).shape == ((1, 64) if "const_std" in head else (1, 64, 2))
    loss, _ = r.train_op(X.cuda(), Y.cuda(), label_type=pa.LABEL_TYPE.MultiLabel, **KW)
    ref = _flat_grad(r).clone()
    total, lsum = torch.zeros_like(ref), 0.0
    for q in range(X.size(0)):
        one = _make(metric=metric, opt_ideal=opt_ideal, top_k=top_k, max_label=4.0, **head)
        lq, _ = one.train_op(X[q:q + 1].cuda(), Y[q:q + 1].cuda(), label_type=pa.LABEL_TYPE.MultiLabel, **KW)
        total += _flat_grad(one)
        lsum += float(lq)
    assert float((total - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    assert abs(lsum - float(loss)) <= 1e-5 * max(1.0, abs(float(loss)))


@pytest.mark.parametrize("metric", NAMES)
@pytest.mark.parametrize("opt_ideal", [True, False])
def test_twenty_steps_do_not_increase_the_loss(metric, opt_ideal):
    import ptranking_amd as pa
    X, Y = _data(B=32)
    Xd, Yd = X.cuda(), Y.cuda()
    r = _make(lr=2e-3, metric=metric, opt_ideal=opt_ideal, top_k=10, max_label=4.0)
    losses = []
    for step in range(20):
        loss, stop = r.train_op(Xd, Yd, label_type=pa.LABEL_TYPE.MultiLabel, **KW)
        assert stop is False and torch.isfinite(loss).all()
        losses.append(float(loss))
    print(f"{metric} opt_ideal={opt_ideal}: loss {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert losses[-1] <= losses[0]


@pytest.mark.parametrize("sort_id", ["ExpRele", "RiskAware", "RERAR"])
def test_predict_returns_the_scores_of_sort_id(sort_id):
    import ptranking_amd.functional as F
    X, _ = _data(B=3)
    r = _make(sort_id=sort_id, limit_delta=None)
    r.eval_mode()
    with torch.no_grad():
        comp = r.forward(X.cuda())
        mus, vars_ = comp[:, :, 0], torch.exp(comp[:, :, 1])
        got = r.predict(X.cuda())
        if sort_id == "ExpRele":
            want = mus
        elif sort_id == "RiskAware":
            want = mus - 0.1 * vars_
        else:
            want = 1.0 / F.expected_ranks(mus.contiguous(), vars_.contiguous())
    assert got.shape == (3, 64) and torch.equal(got, want)


def test_a_batch_the_filter_drops_entirely_still_steps_with_a_zero_gradient():
    import ptranking_amd as pa
    X, _ = _data(B=4)
    Y = torch.zeros(4, 64)
    r = _make(metric="P", opt_ideal=False, top_k=5)
    before = _flat_params(r).clone()
    loss, _ = r.train_op(X.cuda(), Y.cuda(), label_type=pa.LABEL_TYPE.MultiLabel, **KW)
    assert float(loss) == 0.0 and float(_flat_grad(r).abs().max()) == 0.0
    assert not torch.equal(before, _flat_params(r))                 # the step is taken: weight decay alone moves the parameters


def test_the_example_runs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "train_prob_smooth_metric.py"), "--queries", "64", "--steps", "10"], cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "after" in out.stdout and "nan" not in out.stdout.lower(), out.stdout


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", PTR_DP_BACKEND="gloo")
    import ptranking_amd as pa
    from ptranking_amd import dp
    dp.init_from_env()
    X, Y = _data()
    lo, hi = dp.shard_queries(X.size(0))
    r = _make(metric="nERR", opt_ideal=False, top_k=10, max_label=4.0)
    loss, _ = r.train_op(X[lo:hi].cuda(), Y[lo:hi].cuda(), label_type=pa.LABEL_TYPE.MultiLabel, **KW)
    missing = None
    if rank == 0:                                                    # the batch maximum is rank-local: without max_label the ranker refuses
        try:
            _make(metric="nERR", opt_ideal=True, top_k=None).custom_loss_function(torch.zeros(1, 4, 2, device="cuda"), torch.zeros(1, 4, device="cuda"),
                                                                                  presort=True, label_type=pa.LABEL_TYPE.MultiLabel)
        except ValueError as e:
            missing = str(e)
    torch.save({"flat": _flat_params(r).cpu(), "grads": _flat_grad(r).cpu(), "missing": missing}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_match_the_full_batch(tmp_path):
    import ptranking_amd as pa
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{i}.pt") for i in range(2))
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["grads"], r1["grads"])
    assert r0["missing"] and "max_label" in r0["missing"]
    X, Y = _data()
    r = _make(metric="nERR", opt_ideal=False, top_k=10, max_label=4.0)
    r.train_op(X.cuda(), Y.cuda(), label_type=pa.LABEL_TYPE.MultiLabel, **KW)
    ref = _flat_grad(r).cpu()
    assert float((r0["grads"] - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
