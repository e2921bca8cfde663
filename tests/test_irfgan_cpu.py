"""CPU: the adversarial frame's IRFGAN point and pair kernels (csrc/irfgan.hip) and machines (ptranking_amd/adversarial.py) — the float64
restatement (tests/irfgan_ref.py) against the reference's own runs (tests/golden/irfgan.npz, tests/golden/make_golden_irfgan.py), the
gate constant's rule, the ABI, every argument error, and the Python surface."""
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

import irfgan_ref as FR
import test_irfgan_gpu as G
from golden_util import _load, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
NEW = (("ptr_irfgan_point_sample", 13), ("ptr_irfgan_pair_sample", 18), ("ptr_irfgan_fwd_bwd", 16))
KINDS = ("point_d", "pair_d", "point_g", "pair_g")
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=12, num_layers=3, AF="R", TL_AF="S", apply_tl_af=True, BN=False, bn_type=None, bn_affine=False)}


# ------------------------------------------------------------------------------------------------------------- restatement vs the reference
def test_fixture_holds_every_family():
    g = _load("irfgan.npz")
    assert set(g) == set(KINDS) | {"weights"}
    for kind in KINDS:
        assert set(g[kind]) == {"moderate", "steep"}
        for family, c in g[kind].items():
            rows = c["shape"]
            assert c["loss32"].shape == c["loss64"].shape == (8, len(rows)) and c["loss32"].dtype == np.float32 and c["grad64"].dtype == np.float64
            assert {int(r[-1]) for r in rows} == {1, 2, 5}
            if kind.endswith("_g"):
                assert {int(r[0]) for r in rows} == {1, 2, 3, 17, 64, 65, 130, 300}
            v = {"point_d": lambda: np.concatenate([c["x_true"], c["x_fake"]]), "pair_d": lambda: np.concatenate([c["th"] - c["tt"], c["fh"] - c["ft"]]),
                 "point_g": lambda: c["d_fake"], "pair_g": lambda: c["d_head"] - c["d_tail"]}[kind]()          # the argument of activation_f
            bound = 3.0 if family == "moderate" else 30.0
            assert np.abs(v).max() <= bound * (1.0 + 1e-6) and np.abs(v).max() > 0.95 * bound
    pair = g["pair_g"]["moderate"]
    assert (pair["head"] == pair["tail"]).any()
    assert {"all_equal", "all_positive", "ties"} <= set(g["weights"])


def _literal_vs_golden(kind, family):
    c, cases = G.golden_cases(kind, family)
    for fields, cols, i, n, V in cases:
        x, nsel, mode, d_fake, idx_a, idx_b = G.golden_call(kind, fields, n, V)
        for fi, f_div in enumerate(G.DIVS):
            yield (f"{kind} {family} {f_div} n{n} V{V}", (x, nsel, mode, f_div, dict(d_fake=d_fake, idx_a=idx_a, idx_b=idx_b)),
                   c["loss64"][fi, i], c["grad64"][fi, cols], c["loss32"][fi, i], c["grad32"][fi, cols])


@pytest.mark.parametrize("kind", KINDS)
def test_literal_restatement_reproduces_every_float64_run(kind):
    """conjugate_f(activation_f(v)) composed as the reference composes it, in float64: 1e-12 relative on every loss and gradient entry the
    reference's float64 run left finite (a non-finite entry must be non-finite here too).  A gradient entry that is the residue of
    cancelling terms (the reference's 1e-18 beside entries of 0.25, where the true value is 0) has no digits to be relative to: such an
    entry is held to 2^-50 of the run's largest entry or of 1, the size of a term on inputs of order 1: four float64 roundings of the
    terms it is the difference of."""
    for family in ("moderate", "steep"):
        for what, (x, nsel, mode, f_div, kw), loss64, grad64, _, _ in _literal_vs_golden(kind, family):
            ref = FR.loss(x, nsel, mode, f_div, form="literal", **kw)
            got, want = np.concatenate([[ref["loss"]], ref["grad"][0]]), np.concatenate([[loss64], grad64])
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(got), fin), what
            scale = max(1.0, np.abs(want[fin]).max()) if fin.any() else 1.0
            assert (np.abs(got - want)[fin] <= 1e-12 * np.abs(want[fin]) + 2.0 ** -50 * scale).all(), what


@pytest.mark.parametrize("kind", KINDS)
def test_closed_forms_equal_the_composition_on_the_moderate_family(kind):
    """1e-9 between the composition and the closed form, in float64.  Seven divergences meet it with the reference's lines as written.
    JS meets it with log 2 taken in float64 ('literal64'): the reference writes torch.log(torch.tensor(2.0)), a float32 tensor 1.9e-9 above
    log 2, and its conjugate turns that into 1.9e-9 (1 + e^v).  MEASURED with the constant as written: 1.9e-8 in the discriminators'
    losses and gradients, 3.7e-8 (pair) and 1.1e-7 (point) in the generators' (bounded here by 1e-6); the kernel's table
    (include/ptranking_amd.h) is the divergence itself."""
    worst = 0.0
    for what, (x, nsel, mode, f_div, kw), *_ in _literal_vs_golden(kind, "moderate"):
        lit, st = FR.loss(x, nsel, mode, f_div, form="literal64", **kw), FR.loss(x, nsel, mode, f_div, **kw)
        for k in ("loss_q", "grad"):
            assert (np.abs(lit[k] - st[k]) <= 1e-9 * np.maximum(1.0, np.abs(lit[k]))).all(), (what, k)
        if f_div == "JS":
            written = FR.loss(x, nsel, mode, f_div, form="literal", **kw)
            worst = max(worst, max(float(np.abs(written[k] - st[k]).max()) for k in ("loss_q", "grad")))
        else:
            assert np.array_equal(FR.loss(x, nsel, mode, f_div, form="literal", **kw)["grad"], lit["grad"])
    print(f"MEASURED {kind}: the reference's float32 log 2 moves its float64 JS by up to {worst:.2e}")
    assert 1e-10 < worst < 1e-6


def test_the_references_fp32_composition_breaks_on_the_steep_family():
    """From the fixture: under SH, JS and GAN the reference's fp32 run holds inf or NaN on the steep family, and under SH and GAN (and NC in
    the discriminator's losses) it does so where its own float64 run is finite.  (Its float64 JS is NaN there too: see the float32 log 2
    above.)"""
    for kind in KINDS:
        broken, rescued = set(), set()
        for what, (x, nsel, mode, f_div, kw), loss64, grad64, loss32, grad32 in _literal_vs_golden(kind, "steep"):
            if not (np.isfinite(loss32) and np.isfinite(grad32).all()):
                broken.add(f_div)
                if np.isfinite(loss64) and np.isfinite(grad64).all():
                    rescued.add(f_div)
        assert {"SH", "JS", "GAN"} <= broken and {"SH", "GAN"} <= rescued, (kind, broken, rescued)
        assert not {"TVar", "KL", "PC"} & broken


def test_true_pair_weights_equal_the_references_matrices():
    for name, c in sorted(_load("irfgan.npz")["weights"].items()):
        P = int(np.ravel(c["num_pos"])[0])
        w = FR.pair_weights(c["labels"], P)
        assert w.shape == c["w"].shape == (P, c["labels"].size)
        assert_close(w, c["w"], name)
        assert (w >= 0).all() and ((w > 0) == (c["w"] > 0)).all()
        if name in ("all_equal", "no_positive", "one"):
            assert w.sum() == 0.0


def test_pair_restatement_names_set_bits_and_ordered_pairs():
    """The restatement on random uniforms: true pairs have y_head > y_tail and follow the flat inverse CDF, fake pairs are set bits, and
    r = M - 1 is reached by a uniform of 1 - 2^-24."""
    rng = np.random.default_rng(2)
    y = np.array([[3, 2, 2, 1, 0, 0, 0, 0]], np.float32)
    s = rng.standard_normal((1, 8)).astype(np.float32)
    ud, ub = rng.random((1, 2, 16), dtype=np.float32), rng.random((1, 8, 8), dtype=np.float32)
    ud[0, 1, 0], ud[0, 1, 1] = 0.0, 1.0 - 2.0 ** -24
    r = FR.pair_sample(s, y, [4], None, 16, ud, ub)
    bits = ub[0].astype(np.float64) < FR._sg(s[0].astype(np.float64)[:, None] - s[0][None, :])
    assert r["nsel"][0] == 16 and r["count"][0] == bits.sum()
    assert (y[0, r["true_head"][0]] > y[0, r["true_tail"][0]]).all() and bits[r["fake_head"][0], r["fake_tail"][0]].all()
    flat = np.flatnonzero(bits.reshape(-1))
    assert r["fake_head"][0, 0] * 8 + r["fake_tail"][0, 0] == flat[0] and r["fake_head"][0, 1] * 8 + r["fake_tail"][0, 1] == flat[-1]
    for bad_y in ([[2, 2, 2, 2, 2, 2, 2, 2]], [[0] * 8]):
        assert FR.pair_sample(s, np.array(bad_y, np.float32), [4], None, 16, ud, ub)["nsel"][0] == 0
    law, alive = FR.fake_pair_law(np.array([0.5, -0.4, 0.1]))
    assert abs(law.sum() - 1.0) < 1e-12 and 0.99 < alive < 1.0
    assert abs(FR.point_fake_law(np.array([0.1, 0.7, -0.2]), 2).sum() - 1.0) < 1e-12


def test_gate_constant_follows_the_fp32_restatement():
    """C_IRFGAN by the project's rule for C_METRIC: the need of the float32 CPU restatement on the GPU test's own cases (err / E at c = 1),
    doubled, rounded up to a half, capped at 4."""
    need = G.fp32_restatement_need()
    want = min(4.0, np.ceil(2.0 * need * 2.0) / 2.0)
    print(f"MEASURED fp32 CPU restatement: needs c >= {need:.3f} -> C_IRFGAN {want}")
    assert FR.C_IRFGAN == want, (need, want)


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
    for n, i in F.IRFGAN_MODES.items():
        assert re.search(rf"#define PTR_IRFGAN_{n} {i}\b", src)
    for n, i in F.F_DIVERGENCES.items():
        assert re.search(rf"#define PTR_FDIV_{n.upper()} {i}\b", src)
    assert F.IRFGAN_MODES == FR.MODES and F.F_DIVERGENCES == FR.F_DIVS
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == lib.ptr_abi_version() == _lib.ABI_VERSION
    assert "irfgan.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "irfgan.hip"))


def test_every_argument_error_needs_no_gpu(lib):
    one = ctypes.c_void_p(16)

    def point(preds=one, num_pos=one, B=1, L=8, S=5, pos=one, neg=one, nsel=one):
        return lib.ptr_irfgan_point_sample(preds, None, num_pos, B, L, S, 0, 0, None, pos, neg, nsel, None)

    def pair(preds=one, labels=one, num_pos=one, B=1, L=8, S=5, th=one, tt=one, fh=one, ft=one, nsel=one):
        return lib.ptr_irfgan_pair_sample(preds, labels, None, num_pos, B, L, S, 0, 0, None, None, th, tt, fh, ft, nsel, None, None)

    def loss(x=one, d_fake=one, idx_a=one, idx_b=one, nsel=one, B=1, L=8, S=5, mode=0, f_div=1, loss_q=one, valid=one, grad=one):
        return lib.ptr_irfgan_fwd_bwd(x, d_fake, idx_a, idx_b, nsel, None, B, L, S, mode, f_div, None, loss_q, valid, grad, None)

    shape = ((dict(L=4097), b"PTR_MAX_LIST_LEN"), (dict(L=0), b"shape"), (dict(B=-1), b"shape"), (dict(S=0), b"samples"), (dict(S=65), b"samples"),
             (dict(S=-1), b"samples"))
    for bad, word in shape + tuple((dict([(k, None)]), b"NULL") for k in ("preds", "num_pos", "pos", "neg", "nsel")):
        assert point(**bad) == 1001 and word in lib.ptr_last_error(), bad
    for bad, word in shape + tuple((dict([(k, None)]), b"NULL") for k in ("preds", "labels", "num_pos", "th", "tt", "fh", "ft", "nsel")):
        assert pair(**bad) == 1001 and word in lib.ptr_last_error(), bad
    for bad, word in shape + ((dict(mode=4), b"mode"), (dict(mode=-1), b"mode"), (dict(f_div=8), b"f_div"), (dict(f_div=-1), b"f_div"), (dict(x=None), b"NULL"),
                              (dict(nsel=None), b"NULL"), (dict(mode=2, d_fake=None), b"NULL"), (dict(mode=3, idx_a=None), b"NULL"),
                              (dict(mode=3, idx_b=None), b"NULL"), (dict(loss_q=None), b"NULL"), (dict(valid=None), b"NULL"), (dict(grad=None), b"NULL")):
        assert loss(**bad) == 1001 and word in lib.ptr_last_error(), bad
    # an empty batch launches nothing; the discriminator's modes need none of d_fake, idx_a, idx_b, and POINT_G no idx_b: the shape check passes
    # and the launch itself is what these calls never reach (B = 0)
    assert point(B=0, preds=None, num_pos=None, pos=None, neg=None, nsel=None) == 0
    assert pair(B=0, preds=None, labels=None, num_pos=None, th=None, tt=None, fh=None, ft=None, nsel=None) == 0
    assert loss(B=0, x=None, d_fake=None, idx_a=None, idx_b=None, nsel=None, loss_q=None, valid=None, grad=None) == 0


def test_launch_forms_answer_without_a_gpu():
    from launch_form import launch_form
    for entry in ("ptr_irfgan_point_sample", "ptr_irfgan_pair_sample"):
        assert [launch_form(entry, L)[:2] for L in (1, 256, 257, 4096)] == [(64, 4), (64, 4), (256, 1), (256, 1)]
    assert [launch_form("ptr_irfgan_fwd_bwd", m, 4096)[:2] for m in range(4)] == [(64, 4)] * 2 + [(256, 1)] * 2
    assert launch_form("ptr_irfgan_fwd_bwd", 3, 256)[:2] == (64, 4)


# ------------------------------------------------------------------------------------------------------------- the Python surface
def test_functional_surface_and_cpu_tensors():
    import ptranking_amd.functional as F
    for name in ("irfgan_uniforms", "irfgan_point_sample", "irfgan_pair_sample", "IRFGAN_MODES", "F_DIVERGENCES"):
        assert name in F.__all__ and hasattr(F, name)
    assert callable(F.irfgan_loss) and list(inspect.signature(F.irfgan_loss).parameters)[:4] == ["x", "nsel", "mode", "f_div"]
    p, k, i = torch.zeros(2, 4), torch.ones(2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.irfgan_point_sample(p, k, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.irfgan_pair_sample(p, p, k, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.irfgan_loss(p, k, "POINT_D", "KL")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.irfgan_loss(p, k, "PAIR_G", "GAN", d_fake=p, idx_a=i, idx_b=i)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.irfgan_uniforms(2, 4, device="cpu")
    with pytest.raises(ValueError):
        F.irfgan_point_sample(p, k, 65)
    with pytest.raises(ValueError):
        F.irfgan_loss(p, k, "LIST_D", "KL")
    with pytest.raises(ValueError):
        F.irfgan_loss(p, k, "POINT_D", "Wasserstein")
    with pytest.raises(NotImplementedError, match="math.pi"):
        F.irfgan_loss(p, k, "POINT_D", "JSW")


def test_ranker_names_and_defaults():
    import ptranking_amd as pa
    assert pa.EXTRA_AD_RANKER_NAMES == ("IRFGAN_Point", "IRFGAN_Pair") == pa.adversarial.EXTRA_AD_RANKER_NAMES
    assert pa.AD_RANKER_NAMES == ("IRGAN_Point", "IRGAN_Pair") and not set(pa.AD_RANKER_NAMES) & set(pa.EXTRA_AD_RANKER_NAMES)
    ad = pa.adversarial.DEFAULT_AD_PARAS
    assert ad["IRFGAN_Point"]["f_div_id"] == ad["IRFGAN_Pair"]["f_div_id"] == "KL" and ad["IRFGAN_Pair"]["samples_per_query"] == 5


def _machine(name, data=None, sf=None, **ad):
    import ptranking_amd as pa
    return getattr(pa, name)(None, dict(train_presort=True) if data is None else data, sf_para_dict=copy.deepcopy(SF) if sf is None else sf,
                             ad_para_dict=dict(pa.adversarial.DEFAULT_AD_PARAS[name], **ad), gpu=False, device="cpu")


def test_class_surface_and_signatures():
    import ptranking_amd as pa
    assert list(inspect.signature(pa.IRFGAN_Point.__init__).parameters) == ["self", "eval_dict", "data_dict", "sf_para_dict", "ad_para_dict", "gpu", "device"]
    assert list(inspect.signature(pa.IRFGAN_Pair.__init__).parameters) == ["self", "eval_dict", "data_dict", "sf_para_dict", "ad_para_dict", "g_key", "sigma",
                                                                             "gpu", "device"]
    sig = inspect.signature(pa.IRFGAN_Pair.__init__).parameters
    assert sig["g_key"].default == "BT" and sig["sigma"].default == 1.0
    assert inspect.signature(pa.IRFGAN_Point.mini_max_train).parameters["single_step"].default is True
    assert "single_step" not in inspect.signature(pa.IRFGAN_Pair.mini_max_train).parameters
    for cls in (pa.IRFGAN_Point, pa.IRFGAN_Pair):
        for m in ("fill_global_buffer", "mini_max_train", "train_discriminator_generator_single_step", "reset_generator", "reset_discriminator",
                  "get_generator", "get_discriminator"):
            assert callable(getattr(cls, m)), (cls, m)
        assert issubclass(cls, pa.adversarial._IRGANMachine)
    sf = copy.deepcopy(SF)
    p = _machine("IRFGAN_Pair", sf=sf, f_div_id="JS")
    assert p.get_generator().sf_para_dict["pointsf"]["apply_tl_af"] is True and p.get_discriminator().sf_para_dict["pointsf"]["apply_tl_af"] is False
    assert sf["pointsf"]["apply_tl_af"] is True and (p.f_div_id, p.samples_per_query, p.g_key, p.sigma) == ("JS", 5, "BT", 1.0)
    assert p.get_generator().weight_decay == 1e-3
    m = _machine("IRFGAN_Point")
    assert m.get_discriminator().sf_para_dict == m.get_generator().sf_para_dict and m.f_div_id == "KL"
    with pytest.raises(AssertionError):
        pa.IRFGAN_Pair(None, dict(train_presort=True), sf_para_dict=copy.deepcopy(SF), ad_para_dict=pa.adversarial.DEFAULT_AD_PARAS["IRFGAN_Pair"],
                       g_key="SR", gpu=False, device="cpu")


def test_what_the_reference_cannot_run_raises():
    for name in ("IRFGAN_Point", "IRFGAN_Pair"):
        with pytest.raises(NotImplementedError, match="math.pi"):
            _machine(name, f_div_id="JSW")
        with pytest.raises(ValueError):
            _machine(name, f_div_id="Wasserstein")
        for bad in (0, 65):
            with pytest.raises(ValueError):
                _machine(name, samples_per_query=bad)
    m = _machine("IRFGAN_Point")
    with pytest.raises(NotImplementedError, match="d_epoches"):
        m.mini_max_train(train_data=[], generator=m.get_generator(), discriminator=m.get_discriminator(), global_buffer={}, single_step=False)
    for piece in ("generate_data", "train_discriminator", "train_generator"):
        with pytest.raises(NotImplementedError):
            getattr(m, piece)(train_data=[])


def test_fill_global_buffer_of_the_pair_machine():
    import ptranking_amd as pa
    m = _machine("IRFGAN_Pair")
    X = torch.zeros(4, 4, 12)
    Y = torch.tensor([[2.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 9.0], [3.0, 3.0, 0.0, 0.0]])
    lens = torch.tensor([4, 2, 3, 2], dtype=torch.int32)
    buf = {}
    m.fill_global_buffer([(list("abcd"), X, Y, lens), (["e"], X[:1].clone(), Y[:1], lens[:1])], dict_buffer=buf)
    (n0, q0, x0, d0), (n1, q1, x1, d1) = buf.values()
    assert n0.tolist() == [2, 0, 3, 2] and n0.dtype == torch.int32 and (q0, q1) == (0, 4) and x0 is X
    assert d0.tolist() == [True, False, False, False] and d1.tolist() == [True]       # two distinct labels among the REAL documents
    assert list(buf) == [(X.data_ptr(), (4, 4, 12)), (x1.data_ptr(), (1, 4, 12))]
    for Ybad, word in ((torch.tensor([[1.0, 0.0, -1.0, 0.0]]), "below 0"), (torch.tensor([[1.0, 2.0, 0.0, 0.0]]), "sorted"),
                       (torch.tensor([[2.0, 0.0, 1.0, 0.0]]), "sorted")):
        for target in ({}, buf):
            kept = list(target)
            with pytest.raises(ValueError, match=word):
                m.fill_global_buffer([(["f"], X[:2].clone(), Y[:2], lens[:2]), (["g"], X[:1].clone(), Ybad, torch.tensor([3], dtype=torch.int32))],
                                     dict_buffer=target)
            assert list(target) == kept
    # padding is not judged: a label behind lens may be anything
    m.fill_global_buffer([(["h"], X[:1].clone(), torch.tensor([[1.0, 0.0, 5.0, -1.0]]), torch.tensor([2], dtype=torch.int32))], dict_buffer={})
    with pytest.raises(AssertionError):
        _machine("IRFGAN_Pair", data=dict(train_presort=False)).fill_global_buffer([], dict_buffer={})
    # the point machine keeps IRGAN's rule: the positives in front
    with pytest.raises(ValueError, match="presorted"):
        _machine("IRFGAN_Point").fill_global_buffer([(["i"], X[:1].clone(), torch.tensor([[0.0, 1.0, 0.0, 0.0]]), lens[:1])], dict_buffer={})


def test_compact_batch_is_compact_and_zero_padded():
    import ptranking_amd as pa
    X = torch.arange(2 * 6 * 2, dtype=torch.float32).view(2, 6, 2) + 1.0
    a, b = torch.tensor([[1, 0, 0], [0, 0, 0]]), torch.tensor([[4, 3, 0], [0, 0, 0]])
    c, d = torch.tensor([[5, 5, 0], [0, 0, 0]]), torch.tensor([[2, 1, 0], [0, 0, 0]])
    Xs, lens = pa.adversarial._IRFGANMachine.compact_batch(X, [a, b, c, d], torch.tensor([2, 0], dtype=torch.int32))
    assert lens.tolist() == [8, 0] and Xs.shape == (2, 12, 2)
    assert torch.equal(Xs[0, :8], X[0, [1, 0, 4, 3, 5, 5, 2, 1]]) and not Xs[0, 8:].any() and not Xs[1].any()
    Xs, lens = pa.adversarial._IRFGANMachine.compact_batch(X, [a, b], torch.tensor([3, 1], dtype=torch.int32))
    old = pa.adversarial._IRGANMachine.selected_batch(X, a, b, torch.tensor([3, 1], dtype=torch.int32))
    assert torch.equal(Xs, old[0]) and torch.equal(lens, old[1])


def _fake_modules(monkeypatch, names):
    mods = {}
    for n in names:
        m = types.ModuleType(n)
        monkeypatch.setitem(sys.modules, n, m)
        mods[n] = m
    return mods


def test_install_adversarial_round_trip_with_extras(monkeypatch):
    import ptranking_amd as pa
    ad = _fake_modules(monkeypatch, ["fake_irfgan_ad_ltr"])["fake_irfgan_ad_ltr"]
    ad.IRFGAN_Point, ad.IRGAN_List, ad.IRFGAN_List = "reference f-point", "reference list", "reference f-list"
    try:
        done = pa.install_adversarial(ltr_module="fake_irfgan_ad_ltr")                     # the default binds no IRFGAN name
        assert set(done) == {"IRGAN_Point", "IRGAN_Pair"} and ad.IRFGAN_Point == "reference f-point" and not hasattr(ad, "IRFGAN_Pair")
        pa.uninstall()
        done = pa.install_adversarial(ltr_module="fake_irfgan_ad_ltr", extras=True)
        assert set(done) == {"IRGAN_Point", "IRGAN_Pair", "IRFGAN_Point", "IRFGAN_Pair"}
        assert ad.IRFGAN_Point is pa.IRFGAN_Point and ad.IRFGAN_Pair is pa.IRFGAN_Pair and ad.IRGAN_Pair is pa.IRGAN_Pair
        pa.uninstall()
        assert ad.IRFGAN_Point == "reference f-point" and not hasattr(ad, "IRFGAN_Pair") and not hasattr(ad, "IRGAN_Pair")
        done = pa.install_adversarial(names=("IRFGAN_Pair",), ltr_module="fake_irfgan_ad_ltr")
        assert set(done) == {"IRFGAN_Pair"} and ad.IRFGAN_Pair is pa.IRFGAN_Pair and ad.IRFGAN_Point == "reference f-point"
        for missing in ("IRGAN_List", "IRFGAN_List"):
            with pytest.raises(KeyError):
                pa.install_adversarial(names=(missing,), ltr_module="fake_irfgan_ad_ltr", extras=True)
    finally:
        pa.uninstall()
    assert ad.IRFGAN_Point == "reference f-point" and ad.IRFGAN_List == "reference f-list" and not hasattr(ad, "IRFGAN_Pair")
