"""CPU: the adversarial frame's list machines — kernels (csrc/adlist.hip) and classes (ptranking_amd/adversarial.py): the float64
restatement (tests/adlist_ref.py) against the reference's own runs (tests/golden/adlist.npz, tests/golden/make_golden_adlist.py), central
differences on its gradients, the gate constant's rule, the ABI, every argument error, and the Python surface."""
import copy
import ctypes
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import adlist_ref as AR
import test_adlist_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
NEW = (("ptr_adlist_sample", 14), ("ptr_adlist_fwd_bwd", 25))
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=12, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False)}


# ------------------------------------------------------------------------------------------------------------- restatement vs the reference
def test_fixture_covers_what_it_should():
    z, cases = G.golden_cases()
    assert {f["n"] for f, _, _ in cases} == {1, 2, 3, 17, 64, 65, 130} and {f["S"] for f, _, _ in cases} == {1, 5}
    for n in (1, 2, 3, 17, 64, 65, 130):
        assert {f["top_k"] for f, _, _ in cases if f["n"] == n} == {None, 1, 2, 5, n + 3}
    total = sum(f["n"] for f, _, _ in cases)
    for prob in ("PL", "BT"):
        assert z[f"D/{prob}/loss64"].shape == (9, len(cases)) and z[f"G/{prob}/loss32"].shape == (12, len(cases))
        assert z[f"D/{prob}/grad32"].shape == (9, total) and z[f"G/{prob}/grad64"].shape == (12, total)
        assert z[f"D/{prob}/grad32"].dtype == np.float32 and z[f"G/{prob}/grad64"].dtype == np.float64
    assert os.path.getsize(G.GOLDEN) < 1024 * 1024
    for f, _, _ in cases:                                                     # the screen: one order, probabilities pairwise distinct
        for k in range(f["S"]):
            pi, _ = AR.gen_order(f["x"], f["unif"][k])
            assert np.array_equal(pi[:f["K"]], f["gen"][k])


@pytest.mark.parametrize("prob", ("PL", "BT"))
@pytest.mark.parametrize("mode", ("D", "G"))
def test_restatement_reproduces_every_golden_run(mode, prob):
    """Every finite float64 run of the reference to 1e-9 of its scale (JS to 1e-6: the reference's log 2 is a float32 constant), every finite
    float32 run to 2e-4; the tolerance achieved is printed."""
    z, cases = G.golden_cases()
    worst64 = worst_js = worst32 = 0.0
    for f, cols, i in cases:
        x, kw = G.golden_call(f, mode)
        for row, (family, reward, f_div) in G.golden_rows(mode):
            for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
                lg, gg = z[f"{mode}/{prob}/loss{tag}"][row, i], z[f"{mode}/{prob}/grad{tag}"][row, cols]
                if not (np.isfinite(lg) and np.isfinite(gg).all()):
                    continue
                r = AR.loss(x, mode, prob, family, reward, f_div, dtype=dtype, bounds=False, **kw)
                if mode == "G":
                    assert np.array_equal(r["gen_idx"][0, :, :f["K"]], f["gen"])
                scale = max(1.0, abs(lg), float(np.abs(gg).max()))
                err = max(abs(r["loss_q"][0] - lg), float(np.abs(r["grad"][0] - gg).max())) / scale
                if tag == "32":
                    worst32 = max(worst32, err)
                elif family == "IRFGAN" and f_div == "JS":
                    worst_js = max(worst_js, err)
                else:
                    worst64 = max(worst64, err)
    print(f"MEASURED restatement vs golden {mode} {prob}: float64 {worst64:.2e} (JS {worst_js:.2e}), float32 {worst32:.2e}")
    assert worst64 < 1e-9 and worst_js < 1e-6 and worst32 < 2e-4


@pytest.mark.parametrize("prob", ("PL", "BT"))
@pytest.mark.parametrize("mode", ("D", "G"))
def test_gradients_by_central_differences(mode, prob):
    z, cases = G.golden_cases()
    f = next(f for f, _, _ in cases if f["n"] == 17 and f["top_k"] == 5)
    x, kw = G.golden_call(f, mode)
    for family, reward, f_div in G.variants(mode):
        r = AR.loss(x, mode, prob, family, reward, f_div, bounds=False, **kw)
        h = 1e-6
        for j in range(f["n"]):
            xp, xm = x.astype(np.float64).copy(), x.astype(np.float64).copy()
            xp[0, j] += h
            xm[0, j] -= h
            # float64 inputs: the restatement rounds to fp32 at the door, so difference its torch core directly
            lp = _loss64(xp, mode, prob, family, reward, f_div, kw)
            lm = _loss64(xm, mode, prob, family, reward, f_div, kw)
            tol = 1e-6 * max(1.0, abs(r["grad"][0, j])) + 8 * 2.0 ** -52 * abs(lp) / h      # truncation, and the two losses' own rounding over 2 h
            assert abs((lp - lm) / (2 * h) - r["grad"][0, j]) < tol, (mode, prob, family, reward, f_div, j)


def _loss64(x64, mode, prob, family, reward, f_div, kw):
    """The restatement's loss on float64 inputs (no rounding to fp32), with the rankings of the unperturbed call."""
    xs = torch.tensor(x64[0], dtype=torch.float64)
    sgn = -1.0 if family == "IRFGAN" else 1.0
    if mode == "D":
        S, K = kw["std_idx"].shape[1], int(kw["kq"][0])
        ls = 0.0
        for s in range(S):
            for which, idx in ((0, kw["std_idx"]), (1, kw["gen_idx"])):
                lp = AR.lp_torch(prob, xs[torch.tensor(idx[0, s, :K])])
                if family == "IRFGAN":
                    ls = ls + (AR.conj(f_div, lp, "stable") if which else -AR.act(f_div, lp, "stable")) / S
                else:
                    ls = ls - (torch.log(1.0 - lp) if which else lp)
        return float(ls)
    S, n = kw["S"], x64.shape[1]
    K = AR.kq_of(kw["top_k"], n)
    ls = 0.0
    for s in range(S):
        pi, _ = AR.gen_order(x64[0].astype(np.float32), kw["unif"][0, s])
        g64, _ = AR.gumbel_E(kw["unif"][0, s])
        y = torch.softmax((xs + torch.tensor(g64)) / kw["T"], dim=0)
        top = torch.tensor(pi[:K])
        R = AR.reward_torch(family, reward, f_div, AR.lp_torch(prob, torch.tensor(kw["d_preds"][0], dtype=torch.float64)[top]))
        ls = ls + sgn * AR.lp_torch("PL", y[top]) * R / S
    return float(ls)


def test_sampler_restatement_rules():
    y = np.array([2, 0, 2, -1, 2, 1], np.float32)
    u = np.array([0.25, 0.9, 0.75, 0.99, 0.75, 0.1], np.float32)
    assert AR.std_order(y, u).tolist() == [2, 4, 0, 5, 1, 3]                 # label, then the key, then the index; -1 last
    s = np.array([[0.0, 1.0, 0.5, np.nan], [0.3, 0.2, 0.1, 0.0]], np.float32)
    unif = np.full((2, 4, 4), 0.5, np.float32)
    std, gen, kq, pinned = AR.sample(s, np.zeros((2, 4), np.float32), np.array([4, 3], np.int32), 2, 5, unif)
    assert kq.tolist() == [0, 3] and std.shape == (2, 2, 5) and gen[1, 0].tolist() == [0, 1, 2, 0, 0] and std[1, 1].tolist() == [0, 1, 2, 0, 0]
    assert not gen[0].any() and AR.kq_of(None, 7) == 7 and AR.kw_of(None, 9) == 9 and AR.kq_of(9, 7) == 7 and AR.kw_of(9, 7) == 9
    counts = {}
    rng = np.random.default_rng(1)
    for _ in range(3000):                                                     # uniform among ties
        o = tuple(AR.std_order(np.array([1, 1, 1, 0], np.float32), rng.random(4, dtype=np.float32))[:3])
        counts[o] = counts.get(o, 0) + 1
    assert len(counts) == 6 and min(counts.values()) > 400


def test_gate_constant_follows_the_fp32_restatement():
    """C_ADLIST by the project's rule for C_METRIC: the need of the float32 CPU restatement on the GPU test's own cases (err / E at c = 1),
    doubled, rounded up to a half, capped at 4."""
    need = G.fp32_restatement_need()
    want = min(4.0, np.ceil(2.0 * need * 2.0) / 2.0)
    print(f"MEASURED fp32 CPU restatement: needs c >= {need:.3f} -> C_ADLIST {want}")
    assert AR.C_ADLIST == want, (need, want)


def test_cases_keep_every_query_where_the_values_fit_fp32():
    for case in G.CASES:
        for mode in ("D", "G"):
            for prob in ("PL", "BT"):
                for variant in G.variants(mode):
                    G.kept(case, mode, prob, variant)


# ------------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from ptranking_amd import _lib, build
    import ptranking_amd.functional as F
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in NEW:
        proto = re.search(rf"{name}\s*\(([^)]*)\)", src).group(1)
        assert proto.count(",") + 1 == len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name)
    for table, prefix in ((F.ADLIST_MODES, "PTR_ADLIST_"), (F.ADLIST_PROBS, "PTR_ADLIST_"), (F.ADLIST_FAMILIES, "PTR_ADLIST_")):
        for n, i in table.items():
            assert re.search(rf"#define {prefix}{n} {i}\b", src)
    for (n, i), c_name in zip(F.ADLIST_REWARDS.items(), ("NEG_EXP", "NEG_LP", "EXP_1M", "LOG_1M")):
        assert re.search(rf"#define PTR_ADLIST_REWARD_{c_name} {i}\b", src)
    assert (F.ADLIST_MODES, F.ADLIST_PROBS, F.ADLIST_FAMILIES, F.ADLIST_REWARDS) == (AR.MODES, AR.PROBS, AR.FAMILIES, AR.REWARDS)
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == lib.ptr_abi_version() == _lib.ABI_VERSION
    assert "adlist.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "adlist.hip"))
    assert [F.adlist_reward(r, d) for r, d in ((True, True), (True, False), (False, True), (False, False))] == list(F.ADLIST_REWARDS)


def test_every_argument_error_needs_no_gpu(lib):
    one = ctypes.c_void_p(16)
    f32, u64, i64 = ctypes.c_float, ctypes.c_uint64, ctypes.c_int64

    def sample(preds=one, labels=one, B=1, L=8, S=5, top_k=2, std=one, gen=one, kq=one):
        return lib.ptr_adlist_sample(preds, labels, None, B, L, S, top_k, u64(0), i64(0), None, std, gen, kq, None)

    def loss(x=one, d_preds=one, std=one, gen=one, kq=one, B=1, L=8, S=5, top_k=2, mode=0, prob=0, family=0, reward=0, f_div=1, T=1.0, loss_q=one,
             valid=one, grad=one):
        return lib.ptr_adlist_fwd_bwd(x, d_preds, std, gen, kq, None, B, L, S, top_k, mode, prob, family, reward, f_div, f32(T), u64(0), i64(0), None,
                                      None, loss_q, valid, grad, None, None)

    shape = ((dict(L=4097), b"PTR_MAX_LIST_LEN"), (dict(L=0), b"shape"), (dict(B=-1), b"shape"), (dict(S=0), b"samples"), (dict(S=65), b"samples"),
             (dict(S=-1), b"samples"), (dict(top_k=4097), b"top_k"))
    for bad, word in shape + tuple((dict([(k, None)]), b"NULL") for k in ("preds", "labels", "std", "gen", "kq")):
        assert sample(**bad) == 1001 and word in lib.ptr_last_error(), bad
    for bad, word in shape + ((dict(mode=2), b"mode"), (dict(mode=-1), b"mode"), (dict(prob=2), b"prob"), (dict(prob=-1), b"prob"), (dict(family=2), b"family"),
                              (dict(family=-1), b"family"), (dict(reward=4), b"reward"), (dict(reward=-1), b"reward"), (dict(f_div=8), b"f_div"),
                              (dict(f_div=-1), b"f_div"), (dict(T=0.0), b"temperature"), (dict(T=-1.0), b"temperature"), (dict(T=float("inf")), b"temperature"),
                              (dict(T=float("nan")), b"temperature"), (dict(x=None), b"NULL"), (dict(std=None), b"NULL"), (dict(gen=None), b"NULL"),
                              (dict(kq=None), b"NULL"), (dict(mode=1, d_preds=None), b"NULL"), (dict(loss_q=None), b"NULL"), (dict(valid=None), b"NULL"),
                              (dict(grad=None), b"NULL")):
        assert loss(**bad) == 1001 and word in lib.ptr_last_error(), bad
    # an empty batch launches nothing; D needs no d_preds and G none of the rankings: the checks pass and B = 0 never reaches a launch
    assert sample(B=0, preds=None, labels=None, std=None, gen=None, kq=None) == 0 and sample(B=0, top_k=0) == 0 and sample(B=0, top_k=-3) == 0
    assert loss(B=0, x=None, d_preds=None, std=None, gen=None, kq=None, loss_q=None, valid=None, grad=None) == 0
    assert loss(B=0, mode=0, d_preds=None) == 0 and loss(B=0, mode=1, std=None, gen=None, kq=None) == 0


def test_launch_forms_answer_without_a_gpu():
    from launch_form import launch_form
    for entry in ("ptr_adlist_sample", "ptr_adlist_fwd_bwd"):
        assert [launch_form(entry, L)[:2] for L in (1, 256, 257, 4096)] == [(64, 4), (64, 4), (256, 1), (256, 1)]


# ------------------------------------------------------------------------------------------------------------- the Python surface
def test_functional_surface_and_cpu_tensors():
    import ptranking_amd.functional as F
    for name in ("adlist_uniforms", "adlist_sample", "ADLIST_MODES", "ADLIST_PROBS", "ADLIST_FAMILIES", "ADLIST_REWARDS"):
        assert name in F.__all__ and hasattr(F, name)
    assert callable(F.adlist_loss) and list(inspect.signature(F.adlist_loss).parameters)[:2] == ["x", "mode"]
    p, i, k = torch.zeros(2, 4), torch.zeros(2, 5, 2, dtype=torch.int64), torch.ones(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.adlist_sample(p, p, 5, top_k=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.adlist_loss(p, "D", std_idx=i, gen_idx=i, kq=k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.adlist_loss(p, "G", d_preds=p, samples_per_query=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.adlist_uniforms(2, 4, 5, device="cpu")
    for bad in (dict(mode="L"), dict(prob="SR"), dict(family="WGAN"), dict(reward="exp"), dict(f_div="Wasserstein")):
        with pytest.raises(ValueError):
            F.adlist_loss(p, **dict(dict(mode="D", std_idx=i, gen_idx=i, kq=k), **bad))
    with pytest.raises(NotImplementedError, match="math.pi"):
        F.adlist_loss(p, "D", f_div="JSW", std_idx=i, gen_idx=i, kq=k)
    with pytest.raises(ValueError):
        F.adlist_sample(p, p, 65)
    with pytest.raises(ValueError, match="needs"):
        F.adlist_loss(p, "D")
    with pytest.raises(ValueError, match="needs"):
        F.adlist_loss(p, "G", d_preds=p)


def test_ranker_names_and_defaults():
    import ptranking_amd as pa
    assert pa.LIST_AD_RANKER_NAMES == ("IRGAN_List", "IRFGAN_List") == pa.adversarial.LIST_AD_RANKER_NAMES
    assert pa.AD_RANKER_NAMES == ("IRGAN_Point", "IRGAN_Pair") and pa.EXTRA_AD_RANKER_NAMES == ("IRFGAN_Point", "IRFGAN_Pair")
    ad = pa.adversarial.DEFAULT_AD_PARAS
    assert ad["IRGAN_List"] == dict(model_id="IRGAN_List", d_epoches=1, g_epoches=1, temperature=0.2, ad_training_order="DG", samples_per_query=10,
                                    top_k=2, PL_D=True, repTrick=False, dropLog=True)                       # irgan_list.py:420-433
    assert ad["IRFGAN_List"] == dict(model_id="IRFGAN_List", d_epoches=1, g_epoches=1, f_div_id="KL", temperature=0.2, ad_training_order="GD",
                                     samples_per_query=10, top_k=10, PL_D=True, repTrick=True, dropLog=True)   # irfgan_list.py:405-420


def _machine(name, data=None, sf=None, eval_dict=None, optimal_train=False, **ad):
    import ptranking_amd as pa
    return getattr(pa, name)(eval_dict, dict(train_presort=True) if data is None else data, sf_para_dict=copy.deepcopy(SF) if sf is None else sf,
                             ad_para_dict=dict(pa.adversarial.DEFAULT_AD_PARAS[name], **ad), optimal_train=optimal_train, gpu=False, device="cpu")


def test_class_surface_and_signatures():
    import ptranking_amd as pa
    for cls in (pa.IRGAN_List, pa.IRFGAN_List):
        assert list(inspect.signature(cls.__init__).parameters) == ["self", "eval_dict", "data_dict", "sf_para_dict", "ad_para_dict", "optimal_train",
                                                                    "gpu", "device"]
        assert inspect.signature(cls.__init__).parameters["optimal_train"].default is False
        assert inspect.signature(cls.mini_max_train).parameters["per_query_ad_training"].default is True
        assert inspect.signature(cls.get_generator).parameters["super"].default is False
        for m in ("pre_check", "burn_in", "fill_global_buffer", "mini_max_train", "train_discriminator", "train_generator", "reset_generator",
                  "reset_discriminator", "get_generator", "get_discriminator", "per_query_generation"):
            assert callable(getattr(cls, m)), (cls, m)
        assert issubclass(cls, pa.adversarial._IRGANMachine)
    sf = copy.deepcopy(SF)
    m = _machine("IRGAN_List", sf=sf)
    d_sf, g_sf = m.get_discriminator().sf_para_dict["pointsf"], m.get_generator().sf_para_dict["pointsf"]
    assert (d_sf["apply_tl_af"], d_sf["TL_AF"]) == (True, "S") and g_sf["apply_tl_af"] is False and sf["pointsf"]["apply_tl_af"] is False
    assert (m.top_k, m.temperature, m.samples_per_query, m.PL_discriminator, m.replace_trick_4_generator, m.drop_discriminator_log_4_reward) == \
        (2, 0.2, 10, True, False, True) and m.optimal_train is False
    assert m._loss_kw == dict(prob="PL", family="IRGAN", f_div="KL", top_k=2, reward="exp_1m")
    f = _machine("IRFGAN_List", f_div_id="GAN", PL_D=False, top_k=None)
    assert f._loss_kw == dict(prob="BT", family="IRFGAN", f_div="GAN", top_k=None, reward="neg_exp") and f.ad_training_order == "GD"
    assert m.get_generator().weight_decay == 1e-3 and m.burn_in(train_data=[]) is None
    m.fill_global_buffer([], dict_buffer={})
    with pytest.raises(AssertionError):
        _machine("IRGAN_List", data=dict(train_presort=False)).fill_global_buffer([], dict_buffer={})


def test_every_refused_configuration():
    for name in ("IRGAN_List", "IRFGAN_List"):
        with pytest.raises(NotImplementedError, match="optimal_train"):
            _machine(name, optimal_train=True)
        sf = copy.deepcopy(SF)
        sf["sf_id"], sf["listsf"] = "listsf", {}
        with pytest.raises(NotImplementedError, match="point scorers"):
            _machine(name, sf=sf)
        m = _machine(name)
        with pytest.raises(NotImplementedError):
            m.mini_max_train(train_data=[], generator=m.get_generator(), discriminator=m.get_discriminator(), per_query_ad_training=False)
        for piece in (m.get_generator, m.get_discriminator):
            with pytest.raises(NotImplementedError, match="optimal_train"):
                piece(super=True)
        with pytest.raises(AssertionError):                                  # pre_check keeps the reference's assert
            _machine(name, eval_dict=dict(mask_label=True), top_k=None)
        _machine(name, eval_dict=dict(mask_label=True), top_k=3)
        _machine(name, eval_dict=dict(mask_label=False), top_k=None)
        for bad in (dict(samples_per_query=0), dict(samples_per_query=65), dict(ad_training_order="DD"), dict(top_k=0), dict(f_div_id="Wasserstein")):
            with pytest.raises(ValueError):
                _machine(name, **bad)
        with pytest.raises(NotImplementedError, match="math.pi"):
            _machine(name, f_div_id="JSW")


def test_install_adversarial_list_round_trip(monkeypatch):
    import ptranking_amd as pa
    ad = types.ModuleType("fake_adlist_ltr")
    monkeypatch.setitem(sys.modules, "fake_adlist_ltr", ad)
    ad.IRGAN_List, ad.IRGAN_Point = "reference list", "reference point"
    try:
        done = pa.install_adversarial_list(ltr_module="fake_adlist_ltr")
        assert set(done) == {"IRGAN_List", "IRFGAN_List"} and ad.IRGAN_List is pa.IRGAN_List and ad.IRFGAN_List is pa.IRFGAN_List
        assert ad.IRGAN_Point == "reference point"
        pa.uninstall()
        assert ad.IRGAN_List == "reference list" and not hasattr(ad, "IRFGAN_List")
        done = pa.install_adversarial_list(names=("IRFGAN_List",), ltr_module="fake_adlist_ltr")
        assert set(done) == {"IRFGAN_List"} and ad.IRGAN_List == "reference list" and ad.IRFGAN_List is pa.IRFGAN_List
        with pytest.raises(KeyError):
            pa.install_adversarial_list(names=("IRGAN_Pair",), ltr_module="fake_adlist_ltr")
        for missing in ("IRGAN_List", "IRFGAN_List"):                         # install_adversarial still refuses both names
            with pytest.raises(KeyError):
                pa.install_adversarial(names=(missing,), ltr_module="fake_adlist_ltr", extras=True)
        assert set(pa.install_adversarial(ltr_module="fake_adlist_ltr", extras=True)) == {"IRGAN_Point", "IRGAN_Pair", "IRFGAN_Point", "IRFGAN_Pair"}
    finally:
        pa.uninstall()
    assert ad.IRGAN_List == "reference list" and ad.IRGAN_Point == "reference point" and not hasattr(ad, "IRFGAN_List")
    assert "install_adversarial_list" in dir(pa)
