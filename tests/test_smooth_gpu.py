"""GPU: the smooth-rank metric objectives (csrc/smoothmetric.hip, ptr_smoothmetric_fwd_bwd) — P, AP, nERR and nDCG on the smooth ranks of
ApproxNDCG, every form (opt_ideal x top_k), every kernel instantiation.

  1. every run of tests/golden/smooth_metric.npz (the reference's own get_approx_ranks -> *_as_opt_objective -> autograd) through the C ABI
     under golden_util.assert_close against the reference's FLOAT64; the edge family pins NaN placement and valid_q exactly;
  2. the float64 gate (tests/smooth_ref.py, c = C_APPROX): ranks, loss_q, every gradient element and the batch total, each under its own
     bound, on ragged batches (NaN in the padding, a common score offset of 1e3) that reach every ring width and every LDS form;
  3. nDCG / opt_ideal / no cut-off is ApproxNDCG's per-query form; bit identity alone / in a batch / in halves / repeated; ties; autograd;
  4. the SmoothMetric ranker: one-query steps, 20 steps per metric, two data-parallel ranks on one GPU, the example.
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

import f64_loss_bounds as FB
import golden_util as GU
import smooth_ref as SR
from f64_loss_bounds import C_APPROX, MAX_SCREENED, batch_total, gate_nan

pytestmark = pytest.mark.gpu

NAMES = ("P", "AP", "nERR", "nDCG")
GOLDEN = GU._load("smooth_metric.npz")
CASES = [(fam, name) for fam in ("main", "edge") for name in GOLDEN[fam]]


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def run_abi(preds, labels, lens, metric, opt_ideal, top_k, alpha, max_label=None, own_loss=True):
    """One call of the entry point on numpy inputs -> dict of numpy outputs (loss, loss_q, valid_q, ranks, grad)."""
    from ptranking_amd import _lib
    p, y = dev(np.atleast_2d(preds)), dev(np.atleast_2d(labels))
    B, L = p.shape
    ln = None if lens is None else dev(lens, torch.int32)
    new = lambda *s: torch.full(s, 7.0, device="cuda")
    loss, lq, vq, rk, ws, g = new(1), new(max(B, 1)), new(max(B, 1)), new(max(B, 1), L), new(1), new(max(B, 1), L)
    _lib.call("ptr_smoothmetric_fwd_bwd", _lib.ptr(p), _lib.ptr(y), _lib.ptr(ln), B, L, NAMES.index(metric), int(bool(opt_ideal)), int(top_k or 0),
              C.c_float(alpha), C.c_float(-1.0 if max_label is None else max_label), _lib.ptr(loss) if own_loss else None, _lib.ptr(lq),
              _lib.ptr(vq), _lib.ptr(rk), _lib.ptr(ws), _lib.ptr(g), _lib.current_stream(p.device))
    torch.cuda.synchronize()
    return dict(loss=float(loss[0]), loss_q=lq[:B].cpu().numpy(), valid_q=vq[:B].cpu().numpy(), ranks=rk[:B].cpu().numpy(), grad=g[:B].cpu().numpy(),
                max_label_ws=float(ws[0]))


# ------------------------------------------------------------------------------------------------------------------------ 1. golden
@pytest.mark.parametrize("fam,name", CASES)
def test_golden_against_the_reference_float64(fam, name):
    case = GOLDEN[fam][name]
    for k, (m, oi, tk) in enumerate(case["combos"]):
        what = f"{fam}/{name} {NAMES[m]} opt_ideal={oi} top_k={tk}"
        r64, valid = case["res64"][k], case["valid"][k]
        # max_label: given for the one-query cases; the batch case leaves it to the device (the batch maximum)
        ml = None if name == "batch3" else float(case["max_label"])
        out = run_abi(case["preds"], case["labels"], None, NAMES[m], oi, int(tk), float(case["alpha"]), ml)
        got = np.concatenate([[out["loss"]], out["grad"].reshape(-1)])
        assert np.array_equal(np.isnan(got), np.isnan(r64)), f"{what}: NaN placement, got {got}, reference {r64}"
        fin = np.isfinite(r64)
        assert np.isfinite(got[fin]).all(), what
        if fin.any():
            GU.assert_close(got[fin], r64[fin], what)
        assert np.array_equal(out["valid_q"], valid), f"{what}: valid_q {out['valid_q']} vs {valid}"
        if name == "batch3" and NAMES[m] == "nERR":
            assert out["max_label_ws"] == float(case["max_label"])
        lq = out["loss_q"]
        assert np.all(lq[valid == 0] == 0.0) and np.all(out["grad"][valid == 0] == 0.0), what


# ------------------------------------------------------------------------------------------------------------------------ 2. float64 gate
ALPHA = 10.0
# (L, lens).  The ring kernels by width (L <= 64, 128, 192, 256, 384, 512: 1, 2, 3, 4, 6, 8 documents per lane); the LDS forms (L <= 1024, 2048,
# 4096: 4, 8, 16 documents per thread), each with short lists inside the wide padded batch — the production shape — down to 0, 1 and 2
# documents; the last batch is ONE batch of every length class at L = 4096.
GATE_BATCHES = [(64, [0, 1, 2, 63, 64]), (128, [65, 128]), (192, [129, 192]), (256, [256, 200]), (384, [257, 384]), (512, [512, 300]),
                (1024, [0, 1, 2, 40, 513, 1024]), (2048, [1, 2, 64, 1025, 2048]),
                (4096, [0, 1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1251, 2048, 4096])]
TOP_KS = (None, 1, 10, 5000)
OUTPUTS = ("ranks", "loss_q", "grad", "loss_out")


def gate_inputs(L, lens, seed):
    """A ragged batch [len(lens), L]: every query drawn at its own length by f64_loss_bounds.pair_inputs (scores with a common offset of 1e3,
    presorted labels, its pairs screened), NaN in the padding."""
    n = np.asarray(lens, np.int32)
    s, y = np.full((len(lens), L), np.nan, np.float32), np.full((len(lens), L), np.nan, np.float32)
    moved = 0.0
    for q, nq in enumerate(lens):
        if nq > 0:
            sq, yq, _, frac = FB.pair_inputs(1, nq, sigma=ALPHA, seed=seed * 100 + q, offset=1e3, lens="full", specials=False, sort_labels=True,
                                                every_relevant=True)
            s[q, :nq], y[q, :nq] = sq[0], -np.sort(-yq[0])
            moved += frac * nq
    assert moved <= MAX_SCREENED * max(1, int(n.sum())), moved
    return s, y, n


@pytest.fixture(scope="module")
def gate_data():
    """The inputs and the metric-independent half of the float64 reference (smooth ranks, pair derivatives, their bounds), computed once."""
    out = []
    for k, (L, lens) in enumerate(GATE_BATCHES):
        s, y, n = gate_inputs(L, lens, seed=40 + k)
        out.append((L, s, y, n, SR.stages(s, n, ALPHA, C_APPROX)))
    return out


def gate_outputs(out, ref, what, c=C_APPROX):
    """ranks, loss_q, every gradient element and the batch total under their own bounds; valid_q exactly.  Returns the worst err/E per output."""
    q = ref["q"]
    total = batch_total(ref, c)
    w = dict(ranks=gate_nan(out["ranks"], ref["ranks"], ref["E_ranks"], f"{what} ranks", c),
             loss_q=gate_nan(out["loss_q"][q], ref["loss_q"], ref["E_loss_q"], f"{what} loss_q", c),
             grad=gate_nan(out["grad"][q], ref["grad"], ref["E_grad"], f"{what} grad", c),
             loss_out=gate_nan(np.array([out["loss"]]), np.array([total[0]]), np.array([total[1]]), f"{what} loss_out", c))
    assert np.array_equal(out["valid_q"], ref["valid_q"]), f"{what}: valid_q"
    return w


@pytest.mark.parametrize("opt_ideal", [True, False])
@pytest.mark.parametrize("metric", NAMES)
def test_float64_gate_on_every_form(gate_data, metric, opt_ideal):
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for L, s, y, n, st in gate_data:
        for tk in TOP_KS:
            ref = SR.smooth(st, y, n, metric, tk, opt_ideal, None)
            out = run_abi(s, y, n, metric, opt_ideal, tk, ALPHA, None)
            w = gate_outputs(out, ref, f"{metric} opt_ideal={opt_ideal} top_k={tk} L={L}")
            worst = {k: max(worst[k], w[k]) for k in OUTPUTS}
            assert np.all(out["grad"][np.arange(L)[None, :] >= n[:, None]] == 0.0) and np.all(out["ranks"][np.arange(L)[None, :] >= n[:, None]] == 0.0)
    print(f"MEASURED {metric} opt_ideal={opt_ideal}, needed constant per output (C_APPROX = {C_APPROX:g}): "
          + ", ".join(f"{k} {worst[k] * C_APPROX:.2f}" for k in OUTPUTS))


def test_ndcg_ideal_form_is_approxndcg_per_query(gate_data):
    """metric='nDCG', opt_ideal=True, top_k=None and F.approxndcg_loss(couple_batch=False) pass the SAME float64 bounds on the same batch."""
    import ptranking_amd.functional as F
    L, s, y, n, st = gate_data[1]
    s2, y2 = np.nan_to_num(s, nan=0.0), np.nan_to_num(y, nan=0.0)
    ref = SR.smooth(st, y2, n, "nDCG", None, True, None)
    out = run_abi(s2, y2, n, "nDCG", True, None, ALPHA)
    gate_outputs(out, ref, "smooth nDCG")
    p = dev(s2).requires_grad_(True)
    loss, parts = F.approxndcg_loss(p, dev(y2), alpha=ALPHA, presort=True, couple_batch=False, lens=dev(n, torch.int32), return_parts=True)
    loss.backward()
    lq = -(parts["dcg_q"] * parts["inv_idcg_q"]).cpu().numpy()
    FB.gate_losses(lq, p.grad.cpu().numpy(), ref, "approxndcg per query", C_APPROX, got_total=float(loss), total=batch_total(ref, C_APPROX))


# ------------------------------------------------------------------------------------------------------------------------ 3. identities
@pytest.mark.parametrize("L,lens", [(128, [128, 65, 1, 90, 0, 127, 3, 100]), (1024, [1024, 513, 700]), (4096, [0, 1, 2, 64, 130, 2049])])
@pytest.mark.parametrize("metric,opt_ideal,top_k", [("AP", False, 10), ("nERR", True, None), ("P", False, None), ("nDCG", False, 1)])
def test_a_query_alone_in_a_batch_in_halves_and_repeated_is_bit_identical(L, lens, metric, opt_ideal, top_k):
    s, y, n = gate_inputs(L, lens, seed=77)
    s, y = np.nan_to_num(s, nan=0.0), np.nan_to_num(y, nan=0.0)
    keys = ("loss_q", "grad", "ranks", "valid_q")
    full = run_abi(s, y, n, metric, opt_ideal, top_k, ALPHA, 4.0)
    again = run_abi(s, y, n, metric, opt_ideal, top_k, ALPHA, 4.0)
    h = len(lens) // 2
    halves = [run_abi(s[a:b], y[a:b], n[a:b], metric, opt_ideal, top_k, ALPHA, 4.0) for a, b in ((0, h), (h, len(lens)))]
    for k in keys:
        assert np.array_equal(full[k], again[k], equal_nan=True), k
        assert np.array_equal(full[k], np.concatenate([halves[0][k], halves[1][k]]), equal_nan=True), k
    for q in range(len(lens)):
        one = run_abi(s[q:q + 1], y[q:q + 1], n[q:q + 1], metric, opt_ideal, top_k, ALPHA, 4.0)
        for k in keys:
            assert np.array_equal(full[k][q:q + 1], one[k], equal_nan=True), (k, q)


@pytest.mark.parametrize("L,n", [(128, 70), (600, 600)])
def test_all_equal_scores_rank_by_index(L, n):
    """Ties: every score equal.  The smooth ranks are exactly 1 + (n - 1) / 2, the hard positions are the indices, so the re-sorted forms
    return the bits of the ideal-order forms, and both pass the float64 gate."""
    s = np.full((1, L), 1000.25, np.float32)
    y = np.zeros((1, L), np.float32)
    y[0, :n] = -np.sort(-FB.labels_like(1, n, "mslr", np.random.default_rng(3))[0])
    y[0, 0] = max(y[0, 0], 1.0)
    lens = np.asarray([n], np.int32)
    st = SR.stages(s, lens, ALPHA, C_APPROX)
    for metric in NAMES:
        for tk in (None, 10):
            ideal = run_abi(s, y, lens, metric, True, tk, ALPHA, 4.0)
            assert np.all(ideal["ranks"][0, :n] == 1.0 + (n - 1) / 2.0)
            gate_outputs(ideal, SR.smooth(st, y, lens, metric, tk, True, 4.0), f"ties {metric} top_k={tk} ideal")
            resort = run_abi(s, y, lens, metric, False, tk, ALPHA, 4.0)
            gate_outputs(resort, SR.smooth(st, y, lens, metric, tk, False, 4.0), f"ties {metric} top_k={tk} re-sorted")
            if not (metric == "AP" and tk is None):                 # (the re-sorted full-list AP is the reference's other formula)
                for k in ("loss_q", "grad", "ranks"):
                    assert np.array_equal(ideal[k], resort[k]), (metric, tk, k)


def test_autograd_scales_the_kernel_gradient_and_no_grad_skips_it():
    import ptranking_amd.functional as F
    s, y, n = gate_inputs(128, [128, 65, 90], seed=78)
    s, y = np.nan_to_num(s, nan=0.0), np.nan_to_num(y, nan=0.0)
    lens = dev(n, torch.int32)
    for metric, oi, tk in (("AP", False, 10), ("nERR", True, None)):
        raw = run_abi(s, y, n, metric, oi, tk, ALPHA, None, own_loss=False)
        p = dev(s).requires_grad_(True)
        loss, parts = F.smooth_metric_objective(p, dev(y), metric, alpha=ALPHA, top_k=tk, opt_ideal=oi, lens=lens, return_parts=True)
        (loss * -2.5).backward()
        assert torch.equal(p.grad, dev(raw["grad"]) * -2.5)
        assert np.array_equal(parts["loss_q"].cpu().numpy(), raw["loss_q"]) and np.array_equal(parts["ranks"].cpu().numpy(), raw["ranks"])
        assert np.array_equal(parts["valid_q"].cpu().numpy(), raw["valid_q"]) and parts["ranks"].shape == (3, 128)
        plain = F.smooth_metric_objective(dev(s), dev(y), metric, alpha=ALPHA, top_k=tk, opt_ideal=oi, lens=lens)
        assert not plain.requires_grad and torch.equal(plain, loss.detach())
    with pytest.raises(ValueError):
        F.smooth_metric_objective(dev(s), dev(y), "MRR")


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
    r = pa.SmoothMetric(sf_para_dict=sf, model_para_dict={**pa.DEFAULT_PARAS["SmoothMetric"], **over}, gpu=True, device="cuda:0")
    r.init()
    r.train_mode()
    return r


@pytest.mark.parametrize("metric,opt_ideal,top_k", [("AP", False, 10), ("nERR", True, 5)])
def test_one_query_steps_add_up_to_the_batched_step(metric, opt_ideal, top_k):
    """The parameter gradient of a batched step is the sum of the gradients of the one-query steps (the loss is a sum over queries): within
    the 2e-5 of the largest element that the data-parallel tests hold a split batch to."""
    import ptranking_amd as pa
    X, Y = _data()
    r = _make(metric=metric, opt_ideal=opt_ideal, top_k=top_k, max_label=4.0)
    loss, _ = r.train_op(X.cuda(), Y.cuda(), label_type=pa.LABEL_TYPE.MultiLabel, **KW)
    ref = r.point_sf.flat.grad.detach().clone()
    total, lsum = torch.zeros_like(ref), 0.0
    for q in range(X.size(0)):
        one = _make(metric=metric, opt_ideal=opt_ideal, top_k=top_k, max_label=4.0)
        lq, _ = one.train_op(X[q:q + 1].cuda(), Y[q:q + 1].cuda(), label_type=pa.LABEL_TYPE.MultiLabel, **KW)
        total += one.point_sf.flat.grad.detach()
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


def test_a_batch_the_filter_drops_entirely_still_steps_with_a_zero_gradient():
    import ptranking_amd as pa
    X, _ = _data(B=4)
    Y = torch.zeros(4, 64)
    r = _make(metric="P", opt_ideal=False, top_k=5)
    before = r.point_sf.flat.detach().clone()
    loss, _ = r.train_op(X.cuda(), Y.cuda(), label_type=pa.LABEL_TYPE.MultiLabel, **KW)
    assert float(loss) == 0.0 and float(r.point_sf.flat.grad.abs().max()) == 0.0
    # the step IS taken (no host sync tells the ranker to skip it, as the reference's callers do): the optimiser's weight decay (1e-3, the
    # reference's default) alone moves the parameters
    assert r.optimizer.state[r.point_sf.flat]["step"] == 1 and not torch.equal(before, r.point_sf.flat.detach())


def test_the_example_runs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "train_smooth_metric.py"), "--queries", "64", "--steps", "10"], cwd=root,
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
            _make(metric="nERR", opt_ideal=True, top_k=None).custom_loss_function(torch.zeros(1, 4, device="cuda"), torch.zeros(1, 4, device="cuda"),
                                                                                  presort=True, label_type=pa.LABEL_TYPE.MultiLabel)
        except ValueError as e:
            missing = str(e)
    torch.save({"flat": r.point_sf.flat.detach().cpu(), "grads": r.point_sf.flat.grad.detach().cpu(), "missing": missing}, os.path.join(out_dir, f"rank{rank}.pt"))
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
    ref = r.point_sf.flat.grad.detach().cpu()
    assert float((r0["grads"] - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
