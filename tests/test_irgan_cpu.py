"""CPU: the adversarial frame's IRGAN point and pair kernels (csrc/irgan.hip) and machines (ptranking_amd/adversarial.py) — the float64
restatement (tests/irgan_ref.py) against the reference's own runs (tests/golden/irgan.npz, tests/golden/make_golden_irgan.py), the laws of
the sampling rules, the gate constant's rule, the ABI, every argument error, and the Python surface."""
import ctypes
import itertools
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import irgan_ref as IR
from golden_util import _load, assert_close
from plsample_ref import uniforms_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
NEW = (("ptr_irgan_sample", 15), ("ptr_irgan_point_gen_fwd_bwd", 18), ("ptr_irgan_sel_fwd_bwd", 15))
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=12, num_layers=3, AF="R", TL_AF="S", apply_tl_af=True, BN=False, bn_type=None, bn_affine=False)}


@pytest.fixture(scope="module")
def golden():
    return _load("irgan.npz")


# ------------------------------------------------------------------------------------------------------------- restatement vs the reference
def test_fixture_holds_every_family(golden):
    assert {f: len(c) for f, c in golden.items()} == dict(gen_point=12, gen_pair=24, point_d=10, point_g=10, pair_d=16, pair_g=16)
    assert {float(c["temperature"]) for c in golden["point_g"].values()} == {0.5, 1.0}


def test_restatement_reproduces_the_generator_step_of_irgan_point(golden):
    for name, c in sorted(golden["point_g"].items()):
        n, P = c["g_preds"].size, int(c["num_pos"])
        assert c["choose_inds"].size == 5 * P and c["choose_inds"].max() < n
        counts = np.bincount(c["choose_inds"], minlength=n)[None]
        ref = IR.point_generator(c["g_preds"][None], c["d_preds"][None], [P], None, float(c["temperature"]), 0.5, counts)
        assert_close(np.array([ref["loss_q"][0]]), c["loss"], name + " loss")
        assert_close(ref["grad"][0], c["grad"], name + " grad")
        # the reference's own fp32 run (log(softmax), per-draw terms) sits inside the restatement's bound at the rule's cap, c = 4
        assert (np.abs(c["grad"].astype(np.float64) - ref["grad"][0]) <= 4.0 * ref["E_grad"][0] / IR.C_IRGAN + 1e-30).all(), name


def test_restatement_reproduces_the_discriminator_losses(golden):
    for name, c in sorted(golden["point_d"].items()):
        V = c["d_sel"].size // 2
        ref = IR.selected(c["d_sel"][None], [V], "POINT_D")
        assert_close(np.array([ref["loss_q"][0]]), c["loss"], name + " loss")
        assert_close(ref["grad"][0], c["grad"], name + " grad")
    for name, c in sorted(golden["pair_d"].items()):
        V = c["d_pos"].size
        mode = "PAIR_D_SVM" if name.startswith("svm") else "PAIR_D_LOG"
        ref = IR.selected(np.concatenate([c["d_pos"], c["d_neg"]])[None], [V], mode)
        assert_close(np.array([ref["loss_q"][0]]), c["loss"], name + " loss")
        assert_close(ref["grad"][0], np.concatenate([c["grad_pos"], c["grad_neg"]]), name + " grad")


def test_restatement_reproduces_the_generator_step_of_irgan_pair(golden):
    for name, c in sorted(golden["pair_g"].items()):
        V = c["neg_inds"].size
        mode = "PAIR_G_SVM" if name.startswith("svm") else "PAIR_G_LOG"
        ref = IR.selected(c["g_preds"][None], [V], mode, d_sel=np.concatenate([c["d_pos"], c["d_neg"]])[None], neg_idx=c["neg_inds"][None],
                          T=float(c["temperature"]))
        assert_close(np.array([ref["loss_q"][0]]), c["loss"], name + " loss")
        assert_close(ref["grad"][0], c["grad"], name + " grad")
        assert len(set(c["neg_inds"].tolist())) == V                          # torch.multinomial(replacement=False)


def test_the_samplers_outputs_have_the_shape_of_the_references_draws(golden):
    """What per_query_generation returned (torch.randperm, torch.multinomial) and what the restatement draws obey the same rules: V, the
    ranges, distinctness.  (The reference's generator cannot be replayed from uniforms; the LAW is checked below.)"""
    rng = np.random.default_rng(3)
    for fam, mode in (("gen_point", "POINT_D"), ("gen_pair", "PAIR_D")):
        for name, c in sorted(golden[fam].items()):
            n, P, S = int(c["n"]), int(c["num_pos"]), int(c["S"])
            V = min(P, S) if mode == "POINT_D" else min(P, n - P, S)
            assert c["pos_inds"].size == c["neg_inds"].size == V, name
            if V == 0:
                continue
            pos, neg, nsel, _ = IR.sample(c["g_preds"][None], [P], None, S, mode, float(c["temperature"]), rng.random((1, 2, n), dtype=np.float32))
            assert nsel[0] == V
            for p_, n_ in ((c["pos_inds"], c["neg_inds"]), (pos[0, :V], neg[0, :V])):
                assert len(set(p_.tolist())) == V and p_.max() < P and n_.min() >= 0 and n_.max() < n
                if mode == "PAIR_D":
                    assert len(set(n_.tolist())) == V and n_.min() >= P


# ------------------------------------------------------------------------------------------------------------- laws of the sampling rules
def test_the_inverse_cdf_rule_names_each_document_with_its_probability():
    """Exact: the set of u that names document i is the interval [C_{i-1}, C_i) / C_{n-1}; its length is the document's probability."""
    s = np.array([1.0, -2.0, 0.5, 3.0, -300.0, 0.0, 1.5], np.float32)
    p = IR.sample_probabilities(s, 0, "POINT_D", 0.5)
    u = (np.arange(2 ** 16) + 0.5) / 2 ** 16
    z = s.astype(np.float64) / 0.5
    idx, _ = IR.inverse_cdf(np.exp(z - z.max()), u)
    freq = np.bincount(idx, minlength=7) / u.size
    assert np.abs(freq - p).max() <= 2.0 ** -15 and freq[4] == 0.0            # the underflowed document is never named
    idx, _ = IR.inverse_cdf(np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.5, 1.0 - 2.0 ** -24]))
    assert idx.tolist() == [1, 1, 1]                                          # zero weights at either end
    idx, _ = IR.inverse_cdf(np.array([2.0, 0.0, 0.0]), np.array([0.999999]))
    assert idx.tolist() == [0]


def test_gumbel_rounds_have_the_sequential_law_without_replacement():
    """Two rounds over four documents, by quadrature-free enumeration: P(first = a, second = b) of the Gumbel order is w_a / W * w_b / (W - w_a),
    estimated from 2^17 fixed draws within 4 sigma."""
    s = np.array([0.3, -0.4, 1.1, 0.0], np.float32)
    rng = np.random.default_rng(11)
    N = 2 ** 17
    u = rng.random((N, 4))
    key = s.astype(np.float64)[None, :] + IR.gumbel(u.astype(np.float32))
    first_two = np.argsort(-key, axis=1)[:, :2]
    w = np.exp(s.astype(np.float64))
    for a, b in itertools.permutations(range(4), 2):
        want = w[a] / w.sum() * w[b] / (w.sum() - w[a])
        got = np.mean((first_two[:, 0] == a) & (first_two[:, 1] == b))
        assert abs(got - want) <= 4.0 * np.sqrt(want * (1 - want) / N), (a, b, got, want)


def test_largest_uniform_keys_are_a_uniform_subset():
    rng = np.random.default_rng(5)
    N, P, V = 2 ** 15, 5, 2
    u = rng.random((N, P), dtype=np.float32)
    first = np.array([IR.order(u[i])[:V] for i in range(N)])
    for a, b in itertools.permutations(range(P), 2):
        got = np.mean((first[:, 0] == a) & (first[:, 1] == b))
        assert abs(got - 1.0 / 20) <= 4.0 * np.sqrt(0.05 * 0.95 / N)


def test_restatement_gradients_are_the_derivatives_of_its_losses():
    rng = np.random.default_rng(9)
    n, P = 9, 3
    g = rng.standard_normal((1, n)).astype(np.float32)
    d = rng.random((1, n)).astype(np.float32)
    counts = rng.integers(0, 4, size=(1, n))
    ref = IR.point_generator(g, d, [P], None, 0.5, 0.5, counts)
    h = 1e-6
    for i in range(n):
        lo, hi = g.astype(np.float64).copy(), g.astype(np.float64).copy()
        lo[0, i] -= h
        hi[0, i] += h
        f = lambda v: _gen_loss64(v[0], d[0], P, 0.5, 0.5, counts[0])
        assert abs((f(hi) - f(lo)) / (2 * h) - ref["grad"][0, i]) <= 1e-6 * max(1.0, np.abs(ref["grad"]).max())


def _gen_loss64(g, d, P, T, lam, c):
    """The generator's loss written out in numpy, independent of the restatement's torch graph."""
    z = g / T
    p = np.exp(z - z.max())
    p /= p.sum()
    q = (1 - lam) * p
    q[:P] += lam / P
    return -np.sum(c * 2.0 * (d.astype(np.float64) - 0.5) * np.log(p) * p / q) / c.sum()


def test_host_uniform_layout_matches_the_kernels_streams():
    """irgan_uniforms is pl_uniforms with samples = streams: [B, streams, L], stream s index i."""
    u = uniforms_host(3, 7, 5, seed=2 ** 40 + 3, q0=11)
    assert u.shape == (3, 5, 7) and np.array_equal(uniforms_host(1, 7, 5, seed=2 ** 40 + 3, q0=13)[0], u[2])


def test_gate_constant_follows_the_fp32_restatement():
    """C_IRGAN by the project's rule for C_METRIC: the need of the float32 CPU restatement on the GPU test's own cases (err / E at c = 1),
    doubled, rounded up to a half, capped at 4."""
    import test_irgan_gpu as G
    need = G.fp32_restatement_need()
    want = min(4.0, np.ceil(2.0 * need * 2.0) / 2.0)
    print(f"MEASURED fp32 CPU restatement: needs c >= {need:.3f} -> C_IRGAN {want}")
    assert IR.C_IRGAN == want, (need, want)


# ------------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from ptranking_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in NEW:
        proto = re.search(rf"{name}\s*\(([^)]*)\)", src).group(1)
        assert proto.count(",") + 1 == len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name)
    for i, n in enumerate(("POINT_D", "PAIR_D", "PAIR_G")):
        assert re.search(rf"#define PTR_IRGAN_{n} {i}\b", src)
    for i, n in enumerate(("POINT_D", "PAIR_D_SVM", "PAIR_D_LOG", "PAIR_G_SVM", "PAIR_G_LOG")):
        assert re.search(rf"#define PTR_IRGAN_SEL_{n} {i}\b", src)
    assert re.search(r"#define PTR_IRGAN_MAX_SAMPLES 64\b", src)
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == lib.ptr_abi_version() == _lib.ABI_VERSION
    assert "irgan.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "irgan.hip"))


def test_every_argument_error_needs_no_gpu(lib):
    f, one = ctypes.c_float, ctypes.c_void_p(16)

    def sample(preds=one, num_pos=one, B=1, L=8, S=5, mode=0, T=0.5, pos=one, neg=one, nsel=one):
        return lib.ptr_irgan_sample(preds, None, num_pos, B, L, S, mode, f(T), 0, 0, None, pos, neg, nsel, None)

    def gen(g=one, d=one, num_pos=one, B=1, L=8, T=0.5, lam=0.5, dpp=5, loss_q=one, valid=one, grad=one):
        return lib.ptr_irgan_point_gen_fwd_bwd(g, d, None, num_pos, B, L, f(T), f(lam), dpp, 0, 0, None, None, loss_q, valid, grad, None, None)

    def sel(x=one, d_sel=one, neg=one, nsel=one, B=1, L=8, S=5, mode=0, T=0.5, loss_q=one, valid=one, grad=one):
        return lib.ptr_irgan_sel_fwd_bwd(x, d_sel, neg, nsel, None, B, L, S, mode, f(T), None, loss_q, valid, grad, None)

    shape = ((dict(L=4097), b"PTR_MAX_LIST_LEN"), (dict(L=0), b"shape"), (dict(B=-1), b"shape"), (dict(T=0.0), b"temperature"),
             (dict(T=-1.0), b"temperature"), (dict(T=float("nan")), b"temperature"), (dict(T=float("inf")), b"temperature"))
    samples = ((dict(S=0), b"samples"), (dict(S=65), b"samples"), (dict(S=-1), b"samples"))
    for bad, word in shape + samples + ((dict(mode=3), b"mode"), (dict(mode=-1), b"mode"), (dict(preds=None), b"NULL"), (dict(num_pos=None), b"NULL"),
                                        (dict(pos=None), b"NULL"), (dict(neg=None), b"NULL"), (dict(nsel=None), b"NULL")):
        assert sample(**bad) == 1001 and word in lib.ptr_last_error(), bad
    for bad, word in shape + ((dict(lam=-0.1), b"lambda"), (dict(lam=1.0), b"lambda"), (dict(lam=float("nan")), b"lambda"), (dict(dpp=0), b"draws_per_pos"),
                              (dict(dpp=65), b"draws_per_pos"), (dict(g=None), b"NULL"), (dict(d=None), b"NULL"), (dict(num_pos=None), b"NULL"),
                              (dict(loss_q=None), b"NULL"), (dict(valid=None), b"NULL"), (dict(grad=None), b"NULL")):
        assert gen(**bad) == 1001 and word in lib.ptr_last_error(), bad
    for bad, word in shape + samples + ((dict(mode=5), b"mode"), (dict(mode=-1), b"mode"), (dict(x=None), b"NULL"), (dict(nsel=None), b"NULL"),
                                        (dict(mode=3, d_sel=None), b"NULL"), (dict(mode=4, neg=None), b"NULL"), (dict(loss_q=None), b"NULL"),
                                        (dict(valid=None), b"NULL"), (dict(grad=None), b"NULL")):
        assert sel(**bad) == 1001 and word in lib.ptr_last_error(), bad
    # an empty batch launches nothing; the discriminator's forms need neither d_sel nor neg_idx
    assert sample(B=0, preds=None, num_pos=None, pos=None, neg=None, nsel=None) == 0
    assert gen(B=0, g=None, d=None, num_pos=None, loss_q=None, valid=None, grad=None) == 0
    assert sel(B=0, x=None, d_sel=None, neg=None, nsel=None, loss_q=None, valid=None, grad=None) == 0


def test_launch_forms_answer_without_a_gpu():
    from launch_form import launch_form
    for entry in ("ptr_irgan_sample", "ptr_irgan_point_gen_fwd_bwd"):
        assert [launch_form(entry, L)[:2] for L in (1, 256, 257, 4096)] == [(64, 4), (64, 4), (256, 1), (256, 1)]
    assert [launch_form("ptr_irgan_sel_fwd_bwd", m, 4096)[:2] for m in range(5)] == [(64, 4)] * 3 + [(256, 1)] * 2
    assert launch_form("ptr_irgan_sel_fwd_bwd", 4, 256)[:2] == (64, 4)


# ------------------------------------------------------------------------------------------------------------- the Python surface
def test_functional_surface_and_cpu_tensors():
    import ptranking_amd.functional as F
    for name in ("irgan_uniforms", "irgan_sample", "irgan_point_generator", "irgan_selected", "IRGAN_SAMPLE_MODES", "IRGAN_SELECTED_MODES"):
        assert name in F.__all__ and hasattr(F, name)
    assert not [n for n in F.__all__ if "irgan" in n.lower() and n.endswith("_loss")]
    assert F.IRGAN_SAMPLE_MODES == IR.SAMPLE_MODES and F.IRGAN_SELECTED_MODES == IR.SEL_MODES
    p, k = torch.zeros(2, 4), torch.ones(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.irgan_sample(p, k, 5, "POINT_D")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.irgan_point_generator(p, p, k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.irgan_selected(p, k, "POINT_D")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.irgan_uniforms(2, 4, 2, device="cpu")
    with pytest.raises(ValueError):
        F.irgan_sample(p, k, 65, "POINT_D")
    with pytest.raises(ValueError):
        F.irgan_sample(p, k, 5, "LIST")


def test_the_loss_names_of_functional_are_unchanged():
    import ptranking_amd.functional as F
    assert {n for n in F.__all__ if n.endswith("_loss")} == {"ranknet_loss", "lambdarank_loss", "lambdaloss_loss", "approxndcg_loss", "listnet_loss",
                                                             "listmle_loss", "stlistnet_loss", "rankmse_loss", "rankcosine_loss", "softrank_loss",
                                                             "mdprank_loss", "wassrank_loss", "alphadcg_loss", "divprob_loss"}


def test_ranker_names_and_the_default_install_are_unchanged():
    import ptranking_amd as pa
    assert pa.AD_RANKER_NAMES == ("IRGAN_Point", "IRGAN_Pair") == pa.adversarial.AD_RANKER_NAMES
    assert pa.RANKER_NAMES == ("RankNet", "LambdaRank", "LambdaLoss", "ApproxNDCG", "ListNet", "ListMLE", "STListNet", "RankCosine", "RankMSE",
                               "SoftRank", "WassRank")
    assert pa.EXTRA_RANKER_NAMES == ("DASALC", "MDPRank") and pa.DIV_RANKER_NAMES == ("DALETOR",)
    assert pa.METRIC_RANKER_NAMES == ("SmoothMetric",) and pa.PROB_RANKER_NAMES == ("ProbSmoothMetric",)
    assert not set(pa.AD_RANKER_NAMES) & set(pa.RANKER_NAMES + pa.EXTRA_RANKER_NAMES + pa.DIV_RANKER_NAMES)


def _fake_modules(monkeypatch, names):
    mods = {}
    for n in names:
        m = types.ModuleType(n)
        monkeypatch.setitem(sys.modules, n, m)
        mods[n] = m
    return mods


def test_install_adversarial_round_trip_on_a_stand_in_driver(monkeypatch):
    import ptranking_amd as pa
    mods = _fake_modules(monkeypatch, ["fake_ad_ltr"])
    ad = mods["fake_ad_ltr"]
    ad.IRGAN_Point, ad.IRGAN_List = "reference point", "reference list"
    done = pa.install_adversarial(ltr_module="fake_ad_ltr")
    try:
        assert set(done) == {"IRGAN_Point", "IRGAN_Pair"}
        assert ad.IRGAN_Point is pa.IRGAN_Point and ad.IRGAN_Pair is pa.IRGAN_Pair and ad.IRGAN_List == "reference list"
        with pytest.raises(KeyError):
            pa.install_adversarial(names=("IRGAN_List",), ltr_module="fake_ad_ltr")
    finally:
        pa.uninstall()
    assert ad.IRGAN_Point == "reference point" and not hasattr(ad, "IRGAN_Pair")


def test_the_default_install_binds_no_adversarial_name(monkeypatch):
    import ptranking_amd as pa
    mods = _fake_modules(monkeypatch, ["ptranking", "ptranking.base", "ptranking.base.adhoc_ranker", "fake_irgan_adhoc_ltr"])
    mods["ptranking.base.adhoc_ranker"].AdhocNeuralRanker = pa.host.PointScorerRanker
    done = pa.install(ltr_module="fake_irgan_adhoc_ltr")
    try:
        assert set(done) == set(pa.RANKER_NAMES)
        assert not any(hasattr(mods["fake_irgan_adhoc_ltr"], n) for n in pa.AD_RANKER_NAMES)
    finally:
        pa.uninstall()


def test_constructor_asserts_and_parameters():
    import ptranking_amd as pa
    import copy
    ad = pa.adversarial.DEFAULT_AD_PARAS
    data = dict(train_presort=True)
    no_af = copy.deepcopy(SF)
    no_af["pointsf"]["apply_tl_af"] = False
    with pytest.raises(AssertionError):
        pa.IRGAN_Point(None, data, sf_para_dict=no_af, ad_para_dict=ad["IRGAN_Point"], gpu=False, device="cpu")
    m = pa.IRGAN_Point(None, data, sf_para_dict=copy.deepcopy(SF), ad_para_dict=ad["IRGAN_Point"], gpu=False, device="cpu")
    assert m.get_discriminator().sf_para_dict["pointsf"]["TL_AF"] == "S" and m.get_generator().weight_decay == 1e-3
    assert (m.d_epoches, m.g_epoches, m.temperature, m.ad_training_order, m.samples_per_query) == (1, 1, 0.5, "DG", 5)
    sf = copy.deepcopy(no_af)
    p = pa.IRGAN_Pair(None, data, sf_para_dict=sf, ad_para_dict=ad["IRGAN_Pair"], gpu=False, device="cpu")
    assert sf["pointsf"]["apply_tl_af"] is True                               # irgan_pair.py:62 sets it in the caller's dict
    assert p.get_generator().sf_para_dict["pointsf"]["apply_tl_af"] is True and p.get_discriminator().sf_para_dict["pointsf"]["apply_tl_af"] is False
    assert (p.d_loss_mode, p.g_loss_mode) == ("PAIR_D_SVM", "PAIR_G_SVM")
    with pytest.raises(NotImplementedError):
        pa.IRGAN_Pair(None, data, sf_para_dict=copy.deepcopy(SF), ad_para_dict=dict(ad["IRGAN_Pair"], loss_type="hinge"), gpu=False, device="cpu")
    for bad in (dict(samples_per_query=0), dict(samples_per_query=65), dict(ad_training_order="DD")):
        with pytest.raises(ValueError):
            pa.IRGAN_Point(None, data, sf_para_dict=copy.deepcopy(SF), ad_para_dict=dict(ad["IRGAN_Point"], **bad), gpu=False, device="cpu")
    with pytest.raises(AssertionError):
        pa.IRGAN_Point(None, dict(train_presort=False), sf_para_dict=copy.deepcopy(SF), ad_para_dict=ad["IRGAN_Point"], gpu=False,
                       device="cpu").fill_global_buffer([], dict_buffer={})


def test_fill_global_buffer_counts_positives_and_refuses_unsorted_lists():
    import ptranking_amd as pa
    import copy
    m = pa.IRGAN_Point(None, dict(train_presort=True), sf_para_dict=copy.deepcopy(SF), ad_para_dict=pa.adversarial.DEFAULT_AD_PARAS["IRGAN_Point"],
                       gpu=False, device="cpu")
    X = torch.zeros(3, 4, 12)
    Y = torch.tensor([[2.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 9.0]])
    lens = torch.tensor([4, 2, 3], dtype=torch.int32)
    buf = {}
    m.fill_global_buffer([(["a", "b", "c"], X, Y, lens), (["d"], X[:1].clone(), Y[:1], lens[:1])], dict_buffer=buf)
    (n0, q0, x0), (n1, q1, x1) = buf.values()
    assert n0.tolist() == [2, 0, 3] and n0.dtype == torch.int32 and (q0, q1) == (0, 3) and n1.tolist() == [2]
    # an entry keeps its batch's tensor: the address in its key cannot pass to another dataset's batch while the buffer lives
    assert x0 is X and list(buf) == [(X.data_ptr(), (3, 4, 12)), (x1.data_ptr(), (1, 4, 12))]
    assert pa.adversarial.buffered(buf, (["a", "b", "c"], X, Y, lens))[1] == 0
    with pytest.raises(KeyError):
        pa.adversarial.buffered(buf, (["z"], X.clone(), Y, lens))
    # an unsorted list is refused before anything is written: a sorted batch ahead of it leaves no entry behind
    kept = dict(buf)
    for target in ({}, buf):
        with pytest.raises(ValueError, match="presorted"):
            m.fill_global_buffer([(["f"], X[:2].clone(), Y[:2], lens[:2]), (["e"], X[:1].clone(), torch.tensor([[0.0, 1.0, 0.0, 0.0]]), lens[:1])],
                                 dict_buffer=target)
        assert list(target) == (list(kept) if target is buf else [])


def test_selected_batch_is_compact_and_zero_padded():
    import ptranking_amd as pa
    X = torch.arange(2 * 5 * 2, dtype=torch.float32).view(2, 5, 2) + 1.0
    pos = torch.tensor([[1, 0, 0], [0, 0, 0]])
    neg = torch.tensor([[4, 3, 0], [0, 0, 0]])
    Xs, lens = pa.adversarial._IRGANMachine.selected_batch(X, pos, neg, torch.tensor([2, 0], dtype=torch.int32))
    assert lens.tolist() == [4, 0] and Xs.shape == (2, 6, 2)
    assert torch.equal(Xs[0, :4], X[0, [1, 0, 4, 3]]) and not Xs[0, 4:].any() and not Xs[1].any()
