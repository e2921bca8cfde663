"""CPU: the device Plackett-Luce sampler and the fused multi-sample MDPRank loss (csrc/plsample.hip) — the float64 restatement
(tests/plsample_ref.py) against the reference's own runs (tests/golden/plsample.npz) and a float64 re-run of the reference's formulas,
central differences, the law of the Gumbel order, the counter hash, the ABI and the Python surface."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import plsample_ref as PR
from golden_util import _load, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=12, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False)}
NEW = ("ptr_pl_uniforms", "ptr_pl_sample", "ptr_mdprank_sample_fwd_bwd")


@pytest.fixture(scope="module")
def golden():
    return _load("plsample.npz")


def torch_f64(preds, labels, unif, top_k, gamma, T, perm=None):
    """sampling_utils.py:66-81 and mdprank.py:45-71 re-run in float64 torch with autograd -> (inds, sorted logits, loss, grad).  Unlike the
    reference on float64 tensors this is float64 THROUGHOUT (its discount row is an fp32 arange)."""
    p = torch.from_numpy(np.asarray(preds, np.float64)).requires_grad_(True)
    uu = torch.from_numpy((np.asarray(unif, np.float32) + np.float32(1e-20)).astype(np.float64))
    g = -torch.log(-torch.log(uu) + 1e-20)
    logits = p + g if T == 1.0 else (p + g) / T
    srt, inds = torch.sort(logits, dim=1, descending=True)
    if labels is None:
        return inds.numpy(), srt.detach().numpy(), None, None
    y = torch.gather(torch.from_numpy(np.asarray(labels, np.float64)), 1, inds)
    k = y.size(1) if not top_k else int(top_k)
    rewards = (torch.pow(2.0, y) - 1.0)[:, :k] / torch.log2(2.0 + torch.arange(k, dtype=torch.float64).view(1, -1))
    G = torch.flip(torch.cumsum(torch.flip(rewards, dims=[1]), dim=1), dims=[1])
    if gamma != 1.0:
        G = G * torch.cumprod(torch.ones(k, dtype=torch.float64).view(1, -1) * gamma, dim=1)
    m, _ = torch.max(srt, dim=1, keepdim=True)
    cs = torch.flip(torch.cumsum(torch.flip(torch.exp(srt - m), dims=[1]), dim=1), dims=[1])
    loss = torch.sum((torch.log(cs) + m)[:, :k] * G - srt[:, :k] * G)
    loss.backward()
    return inds.numpy(), srt.detach().numpy(), loss.detach().item(), p.grad.numpy()


def test_restatement_reproduces_every_sampler_fixture(golden):
    cases = golden["sampler"]
    assert len(cases) == 8 * 3 * 3 * 2
    for name, c in sorted(cases.items()):
        T, S = float(c["temperature"]), c["unif"].shape[0]
        perm, act, ok, _ = PR.sample(c["preds"], c["unif"][None], None, T, "STPL")
        assert ok.all(), name
        assert np.array_equal(perm[0], c["inds"]), name                       # exact
        for s in range(S):
            inds64, srt64, _, _ = torch_f64(c["preds"], None, c["unif"][s:s + 1], None, 1.0, T)
            assert np.array_equal(inds64[0], c["inds"][s]), name
            assert np.allclose(act[0, s], srt64[0], rtol=1e-12, atol=0.0), name
        if not int(c["only_indices"]):
            assert_close(act[0], c["logits"], name)                           # the reference's fp32 values


def test_restatement_reproduces_every_mdprank_fixture(golden):
    cases = golden["mdprank"]
    assert len(cases) == 3 * 3 * 2
    for name, c in sorted(cases.items()):
        top_k, gamma, T = int(c["top_k"]), float(c["gamma"]), float(c["temperature"])
        ref = PR.mdprank_sampled(c["preds"], c["labels"], c["unif"][None], None, top_k, gamma, T, "STPL")
        assert ref["ok"].all() and np.array_equal(ref["perm"][:, 0], c["perm"]), name
        inds64, _, loss64, grad64 = torch_f64(c["preds"], c["labels"], c["unif"], top_k, gamma, T)
        assert np.array_equal(inds64, c["perm"]), name
        assert abs(ref["loss_q"][0] - loss64) <= 1e-12 * abs(loss64), name
        assert np.allclose(ref["grad"], grad64, rtol=1e-12, atol=1e-12 * np.abs(grad64).max()), name
        assert_close(np.array([ref["loss_q"].sum()]), np.array([c["loss"]]), name + " loss")
        assert_close(ref["grad"], c["grad"], name + " grad")
        # the reference's own fp32 run sits inside the restatement's bound, a 1e-4 relative fault does not
        E = ref["E_grad"]
        assert (np.abs(c["grad"].astype(np.float64) - ref["grad"]) <= E).all(), name
        assert abs(float(c["loss"]) - ref["loss_q"][0]) <= ref["E_loss_q"][0] + 2.0 ** -24 * abs(ref["loss_q"][0]), name
        if np.abs(ref["grad"]).max() > 0:                                      # (a sampled top_k without a relevant document: all zero)
            assert not (np.abs(ref["grad"] * (1.0 + 1e-4) - ref["grad"]) <= E).all(), name


def test_the_adjacent_gap_condition_holds_for_the_stored_fixtures(golden):
    n = 0
    for fam in ("sampler", "mdprank"):
        for name, c in golden[fam].items():
            for row in np.atleast_2d(c["unif"]):
                key, _, _ = PR.keys_f64(c["preds"][0], row, 1.0, "STPL")
                assert PR.gap_ok(key), (fam, name)
                if key.size > 1:
                    srt = -np.sort(-key)
                    assert np.min(srt[:-1] - srt[1:]) > 2.0 ** -16 * np.max(np.abs(key))
                n += 1
    assert n == 8 * 3 * 2 * (1 + 1 + 5) + 18


@pytest.mark.parametrize("dist,T,S,top_k,gamma", [("PL", 1.0, 1, 10, 1.0), ("PL", 0.5, 3, None, 0.9), ("STPL", 1.0, 2, 3, 0.5), ("STPL", 2.0, 3, 10, 0.9)])
def test_restatement_gradient_is_the_derivative_of_its_loss(dist, T, S, top_k, gamma):
    g = np.random.default_rng(5)
    n = 9
    s = g.standard_normal((1, n)).astype(np.float32)
    y = -np.sort(-g.integers(0, 5, size=(1, n)).astype(np.float32))
    u = g.random((1, S, n), dtype=np.float32)
    assert PR.redraw(s, u, None, T, dist) == (0, 0)
    ref = PR.mdprank_sampled(s, y, u, None, top_k, gamma, T, dist)
    h = 1e-6
    for i in range(n):
        lo, hi = s.astype(np.float64).copy(), s.astype(np.float64).copy()
        lo[0, i] -= h
        hi[0, i] += h
        f = lambda v: PR.mdprank_sampled(v, y, u, None, top_k, gamma, T, dist, perm=ref["perm"])["loss_q"][0]
        fd = (f(hi) - f(lo)) / (2 * h)
        assert abs(fd - ref["grad"][0, i]) <= 1e-7 * max(1.0, np.abs(ref["grad"]).max()), (i, fd, ref["grad"][0, i])
    if dist == "PL":       # T only shapes the draw: the gradient carries no 1 / T
        again = PR.mdprank_sampled(s, y, u, None, top_k, gamma, 1.0, dist, perm=ref["perm"])
        assert np.array_equal(again["grad"], ref["grad"])


def _gumbel_order_probability(keys_shift, pi):
    """P(s_pi0 + g_0 > s_pi1 + g_1 > s_pi2 + g_2) for independent standard Gumbels, by quadrature of the densities (no sampling):
    H(x) = int_{-inf}^{x} f(t - s_b) F(t - s_c) dt on a grid, then int f(x - s_a) H(x) dx."""
    a, b, c = (keys_shift[i] for i in pi)
    x = np.linspace(-12.0, 45.0, 400001)
    f = lambda t: np.exp(-t - np.exp(-t))
    F = lambda t: np.exp(-np.exp(-t))
    inner = f(x - b) * F(x - c)
    dx = x[1] - x[0]
    H = np.concatenate([[0.0], np.cumsum(0.5 * (inner[1:] + inner[:-1]) * dx)])
    outer = f(x - a) * H
    return float(np.sum(0.5 * (outer[1:] + outer[:-1]) * dx))


def test_the_gumbel_orders_law_is_the_sequential_draws_law_at_three_documents():
    for s, T in (([1.0, 0.5, -1.0], 1.0), ([0.3, -0.2, 2.0], 0.5), ([0.0, 0.0, 0.0], 1.0), ([2.0, -3.0, 0.5], 2.0)):
        pr = PR.pl_probabilities(np.array(s), T)              # torch.multinomial without replacement: w_i / (remaining mass), in turn
        assert abs(sum(pr.values()) - 1.0) < 1e-12 and len(pr) == 6
        shift = np.array(s) / T
        total = 0.0
        for pi in itertools.permutations(range(3)):
            got = _gumbel_order_probability(shift, pi)
            total += got
            assert abs(got - pr[pi]) < 1e-8, (s, T, pi, got, pr[pi])
        assert abs(total - 1.0) < 1e-8


def test_host_uniforms_are_24_bit_keyed_by_the_global_query_and_well_spread():
    u = PR.uniforms_host(64, 33, 3, seed=2 ** 40 + 17, q0=5)
    assert u.dtype == np.float32 and u.shape == (64, 3, 33) and u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))
    whole = PR.uniforms_host(64, 33, 3, seed=2 ** 40 + 17, q0=5)
    assert np.array_equal(PR.uniforms_host(20, 33, 3, seed=2 ** 40 + 17, q0=5 + 44), whole[44:])        # a shard draws the whole batch's
    assert np.array_equal(PR.uniforms_host(3, 33, 3, seed=2 ** 40 + 17, q0=2 ** 33 + 1), PR.uniforms_host(4, 33, 3, seed=2 ** 40 + 17, q0=2 ** 33)[1:])
    assert not np.array_equal(PR.uniforms_host(64, 33, 3, seed=2 ** 40 + 18, q0=5), whole)
    big = PR.uniforms_host(512, 64, 8, seed=99).astype(np.float64)
    cnt = np.bincount((big * 64).astype(int).ravel(), minlength=64)
    chi = ((cnt - big.size / 64) ** 2 / (big.size / 64)).sum()
    assert chi < 140.0                                         # chi^2 with 63 degrees of freedom: 1 - 1e-6 quantile is 139.5


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from ptranking_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in zip(NEW, (7, 13, 18)):
        proto = re.search(rf"{name}\s*\(([^)]*)\)", src).group(1)
        assert proto.count(",") + 1 == len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name)
    assert re.search(r"#define PTR_PL_DIST_PL 0\b", src) and re.search(r"#define PTR_PL_DIST_STPL 1\b", src)
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == lib.ptr_abi_version() == _lib.ABI_VERSION
    assert "plsample.hip" in build.SOURCES


def test_every_argument_error_needs_no_gpu(lib):
    f, one = ctypes.c_float, ctypes.c_void_p(16)

    def sample(preds=one, B=1, L=8, S=1, T=1.0, dist=0, perm=one):
        return lib.ptr_pl_sample(preds, None, B, L, S, f(T), dist, 0, 0, None, perm, None, None)

    def fused(preds=one, labels=one, B=1, L=8, S=1, gamma=1.0, T=1.0, dist=0, loss_q=one, grad=one):
        return lib.ptr_mdprank_sample_fwd_bwd(preds, labels, None, B, L, S, 10, f(gamma), f(T), dist, 0, 0, None, None, loss_q, grad, None, None)

    def unif(B=1, L=8, S=1, out=one):
        return lib.ptr_pl_uniforms(B, L, S, 0, 0, out, None)

    common = ((dict(S=0), b"samples"), (dict(S=-3), b"samples"), (dict(L=4097), b"PTR_MAX_LIST_LEN"), (dict(L=0), b"shape"), (dict(B=-1), b"shape"))
    shaped = common + ((dict(T=0.0), b"temperature"), (dict(T=-1.0), b"temperature"), (dict(T=float("nan")), b"temperature"),
                       (dict(dist=2), b"distribution"), (dict(dist=-1), b"distribution"), (dict(preds=None), b"NULL"))
    for bad, word in shaped + ((dict(perm=None), b"NULL"),):
        assert sample(**bad) == 1001 and word in lib.ptr_last_error(), bad
    for bad, word in shaped + ((dict(labels=None), b"NULL"), (dict(loss_q=None), b"NULL"), (dict(grad=None), b"NULL"), (dict(gamma=0.0), b"gamma"),
                               (dict(gamma=float("nan")), b"gamma")):
        assert fused(**bad) == 1001 and word in lib.ptr_last_error(), bad
    for bad, word in common + ((dict(out=None), b"NULL"),):
        assert unif(**bad) == 1001 and word in lib.ptr_last_error(), bad
    assert sample(B=0, preds=None, perm=None) == 0 and unif(B=0, out=None) == 0          # an empty batch launches nothing


def test_cpu_tensors_and_bad_arguments_raise():
    import ptranking_amd.functional as F
    p, y = torch.zeros(2, 4), torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.sample_rankings_pl(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.mdprank_sampled_loss(p, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.pl_uniforms(2, 4, device="cpu")
    assert F.PL_DISTRIBUTIONS["PL"] == 0 and F.PL_DISTRIBUTIONS["STPL"] == 1
    for name in ("pl_uniforms", "sample_rankings_pl", "PL_DISTRIBUTIONS"):
        assert name in F.__all__
    assert callable(F.mdprank_sampled_loss)


def test_public_ranker_names_and_defaults_are_unchanged():
    import ptranking_amd as pa
    assert pa.RANKER_NAMES == ("RankNet", "LambdaRank", "LambdaLoss", "ApproxNDCG", "ListNet", "ListMLE", "STListNet", "RankCosine", "RankMSE",
                               "SoftRank", "WassRank")
    assert pa.EXTRA_RANKER_NAMES == ("DASALC", "MDPRank")
    assert pa.DEFAULT_PARAS["MDPRank"] == dict(model_id="MDPRank", temperature=1.0, gamma=1.0, top_k=10, distribution='PL')


def test_mdprank_parses_the_new_keys():
    import ptranking_amd as pa
    d = pa.MDPRank(sf_para_dict=SF, model_para_dict=pa.DEFAULT_PARAS["MDPRank"], gpu=False, device="cpu")
    assert (d.sampler, d.samples_per_query) == ("torch", 1)
    r = pa.MDPRank(sf_para_dict=SF, model_para_dict=dict(pa.DEFAULT_PARAS["MDPRank"], sampler="device", samples_per_query=4), gpu=False, device="cpu")
    assert (r.sampler, r.samples_per_query, r.distribution) == ("device", 4, "PL")
    for bad in (dict(sampler="host"), dict(sampler="device", samples_per_query=0), dict(samples_per_query=2)):
        with pytest.raises(ValueError):
            pa.MDPRank(sf_para_dict=SF, model_para_dict=dict(pa.DEFAULT_PARAS["MDPRank"], **bad), gpu=False, device="cpu")


@pytest.mark.parametrize("dist,T,with_lens", [("PL", 1.0, False), ("PL", 0.5, True), ("STPL", 1.0, True), ("STPL", 2.0, False)])
def test_the_default_route_draws_what_it_drew_before(dist, T, with_lens, monkeypatch):
    """sampler='torch': the same torch calls in the same order under the same generator state -> the same ranking and action scores handed to
    functional.mdprank_loss (replayed here from the reference's construction, sampling_utils.py:31-81, plus the padding rules)."""
    import ptranking_amd as pa
    from ptranking_amd import rankers
    seen = {}

    def fake_loss(action, labels, perm, top_k=10, gamma=1.0, lens=None):
        seen.update(action=action.detach().clone(), perm=perm.clone(), top_k=top_k, gamma=gamma, lens=lens)
        return action.sum() * 0.0

    monkeypatch.setattr(rankers.F_, "mdprank_loss", fake_loss)
    monkeypatch.setattr(rankers.F_, "mdprank_sampled_loss", lambda *a, **k: pytest.fail("the default route took the device sampler"))
    r = pa.MDPRank(sf_para_dict=SF, model_para_dict=dict(pa.DEFAULT_PARAS["MDPRank"], distribution=dist, temperature=T, top_k=5, gamma=0.9),
                   gpu=False, device="cpu")
    monkeypatch.setattr(r, "_fused_step", lambda loss: loss)
    g = torch.Generator().manual_seed(3)
    preds, labels = torch.randn(4, 12, generator=g), torch.zeros(4, 12)
    lens = torch.tensor([12, 5, 1, 9], dtype=torch.int32) if with_lens else None
    torch.manual_seed(11)
    r.custom_loss_function(preds.clone().requires_grad_(True), labels, presort=True, lens=lens)
    torch.manual_seed(11)
    det = preds.clone()
    if lens is not None:
        det = det.masked_fill(torch.arange(12)[None, :] >= lens[:, None], -1e30)
    if dist == "PL":
        t = det / T if T != 1.0 else det
        perm = torch.multinomial(torch.exp(t - t.max(dim=1, keepdim=True)[0]).clamp_min(1e-38), num_samples=12, replacement=False)
        if lens is not None:
            perm = torch.gather(perm, 1, torch.sort((perm >= lens[:, None]).to(torch.int8), dim=1, stable=True)[1])
        action = preds
    else:
        noise = -torch.log(-torch.log(torch.rand(det.size()) + 1e-20) + 1e-20)
        perm = torch.sort(det + noise if T == 1.0 else (det + noise) / T, dim=1, descending=True)[1]
        action = preds + noise if T == 1.0 else (preds + noise) / T
    assert torch.equal(seen["perm"], perm) and torch.equal(seen["action"], action)
    assert (seen["top_k"], seen["gamma"]) == (5, 0.9) and (seen["lens"] is lens)


def test_the_device_route_passes_a_per_call_seed_and_the_query_offset(monkeypatch):
    import ptranking_amd as pa
    from ptranking_amd import rankers
    calls = []
    monkeypatch.setattr(rankers.F_, "mdprank_sampled_loss", lambda p, y, **k: calls.append(k) or p.sum() * 0.0)
    r = pa.MDPRank(sf_para_dict=SF, model_para_dict=dict(pa.DEFAULT_PARAS["MDPRank"], distribution="STPL", temperature=2.0, sampler="device",
                                                          samples_per_query=4), gpu=False, device="cpu")
    monkeypatch.setattr(r, "_fused_step", lambda loss: loss)
    p, y = torch.zeros(3, 6), torch.zeros(3, 6)
    r.custom_loss_function(p, y, presort=True)
    r.custom_loss_function(p, y, presort=True, q0=40)
    a, b = calls
    assert (a["samples"], a["distribution"], a["temperature"], a["top_k"], a["gamma"]) == (4, "STPL", 2.0, 10, 1.0)
    assert (a["q0"], b["q0"]) == (0, 40) and b["seed"] == a["seed"] + 1 == 137 * 0x9E3779B1 + 2
