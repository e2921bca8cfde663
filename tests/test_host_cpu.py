"""CPU: host-side mirror of the reference's plugin surface (class shapes, constructor signatures, error behaviour) and
the install() drop-in wiring into the reference's ltr module (when the reference is importable)."""
import inspect
import os
import sys

import pytest
import torch

import ptranking_amd as pa
from ptranking_amd import host, rankers

# The wildltr/ptranking checkout for the tests that run the reference's own driver code (its sources are not part of this
# repository): $PTRANKING_REF, else the build container's copy.  Where there is none (the GPU machines) those tests skip.
REF = os.environ.get("PTRANKING_REF") or "/root/reference"
NEEDS_REF = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "ptranking")),
                               reason="runs the reference's own driver: needs a wildltr/ptranking checkout (PTRANKING_REF)")
SF = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
      "pointsf": dict(num_features=12, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False)}


def test_constructor_signatures_match_the_reference():
    """lambdarank.py:23, ranknet.py:20, lambdaloss.py:67, approxNDCG.py:74, listmle.py:70 vs listnet.py:19."""
    for name in ("RankNet", "LambdaRank", "LambdaLoss", "ApproxNDCG", "ListMLE"):
        assert list(inspect.signature(getattr(pa, name).__init__).parameters) == \
            ["self", "sf_para_dict", "model_para_dict", "gpu", "device"], name
    assert list(inspect.signature(pa.ListNet.__init__).parameters) == ["self", "sf_para_dict", "gpu", "device"]
    for name in pa.RANKER_NAMES:
        cls = getattr(pa, name)
        for meth in ("init", "train", "train_op", "custom_loss_function", "forward", "predict", "save", "load", "validation",
                     "ndcg_at_k", "ndcg_at_ks", "nerr_at_k", "ap_at_k", "p_at_k", "adhoc_performance_at_ks", "stop_training",
                     "eval_mode", "train_mode", "uniform_eval_setting", "get_tl_af", "config_optimizer", "get_parameters"):
            assert callable(getattr(cls, meth)), (name, meth)


def test_evaluator_signatures_match_the_reference():
    ev = host.DeviceEvaluator
    assert list(inspect.signature(ev.ndcg_at_k).parameters) == ["self", "test_data", "k", "label_type", "presort", "device"]
    assert list(inspect.signature(ev.ap_at_k).parameters) == ["self", "test_data", "k", "presort", "device"]
    assert list(inspect.signature(ev.p_at_k).parameters) == ["self", "test_data", "k", "device"]
    assert list(inspect.signature(ev.adhoc_performance_at_ks).parameters) == \
        ["self", "test_data", "ks", "label_type", "max_label", "presort", "device", "need_per_q"]
    assert list(inspect.signature(ev.validation).parameters) == \
        ["self", "vali_data", "vali_metric", "k", "presort", "max_label", "label_type", "device"]


def test_standalone_ranker_builds_the_reference_scorer():
    r = pa.LambdaRank(sf_para_dict=SF, model_para_dict={"sigma": 1.0}, gpu=False, device="cpu")
    r.init()
    names = [n for n, _ in r.point_sf.named_children()]
    assert names == ["dr_1", "ff_2", "act_2", "dr_2", "ff_3", "act_3", "dr_3", "ff_4", "act_4", "ff_5"]   # base/utils.py:299-322
    assert sum(p.numel() for p in r.get_parameters()) == 12 * 100 + 100 + 2 * (100 * 100 + 100) + 100 + 1
    assert isinstance(r.optimizer, torch.optim.Adam) and r.optimizer.defaults["weight_decay"] == 1e-3
    assert r.scheduler.step_size == 20 and r.scheduler.gamma == 0.5                                        # ranker.py:525
    assert r.forward(torch.randn(3, 7, 12)).shape == (3, 7)
    assert r.stop_check_freq == 10 and r.sigma == 1.0
    # NaN / all-zero detection (ranker.py:547-561)
    assert r.stop_training(torch.zeros(2, 3)) is True
    assert r.stop_training(torch.tensor([[1.0, float("nan")]])) is True
    assert r.stop_training(torch.ones(2, 3)) is False


def test_reference_error_behaviour_is_preserved():
    r = pa.LambdaRank(sf_para_dict=SF, model_para_dict={"sigma": 1.0}, gpu=False, device="cpu")
    p, y = torch.zeros(1, 4), torch.zeros(1, 4)
    with pytest.raises(AssertionError):      # lambdarank.py:34
        r.custom_loss_function(p, y, presort=True)
    with pytest.raises(AssertionError):      # lambdarank.py:36
        r.custom_loss_function(p, y, presort=False, label_type=pa.LABEL_TYPE.MultiLabel)
    with pytest.raises(AssertionError):
        r.custom_loss_function(p, y, presort=True, label_type=pa.LABEL_TYPE.Permutation)
    with pytest.raises(NotImplementedError):
        pa.LambdaLoss(sf_para_dict=SF, model_para_dict=dict(k=5, sigma=1.0, loss_type="ARP_Loss1"), gpu=False, device="cpu")
    with pytest.raises(NotImplementedError):
        bad = dict(SF, opt="SGD")
        rr = pa.ListNet(sf_para_dict=bad, gpu=False, device="cpu")
        rr.init()
    with pytest.raises(AssertionError):      # adhoc_ranker.py:18
        pa.RankNet(sf_para_dict=dict(SF, sf_id="treesf"), model_para_dict={"sigma": 1.0})
    with pytest.raises(NotImplementedError):  # list_ranker.py:330-331
        bad_enc = dict(num_features=8, ff_dims=[8], n_heads=2, encoder_layers=1, encoder_type="Performer", BN=False)
        rr = pa.RankNet(sf_para_dict=dict(SF, sf_id="listsf", listsf=bad_enc), model_para_dict={"sigma": 1.0}, gpu=False, device="cpu")
        rr.init()
    with pytest.raises(NotImplementedError):
        r.validation(vali_data=[], vali_metric="MRR")
    ll = pa.LambdaLoss(sf_para_dict=SF, model_para_dict=pa.DEFAULT_PARAS["LambdaLoss"], gpu=False, device="cpu")
    assert (ll.k, ll.sigma, ll.loss_type) == (5, 1.0, "NDCG_Loss2")
    ap = pa.ApproxNDCG(sf_para_dict=SF, model_para_dict=pa.DEFAULT_PARAS["ApproxNDCG"], gpu=False, device="cpu")
    ed = dict(do_validation=True, vali_metric="AP")
    ap.uniform_eval_setting(eval_dict=ed)
    assert ed["vali_metric"] == "nDCG"       # approxNDCG.py:78-81


def test_label_type_accepts_the_reference_enum_by_name():
    assert host.is_multilabel(pa.LABEL_TYPE.MultiLabel) and not host.is_multilabel(pa.LABEL_TYPE.Permutation)

    class Fake:
        name = "MultiLabel"
    assert host.is_multilabel(Fake())


@NEEDS_REF
def test_install_drops_into_the_reference_driver():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    try:
        import ptranking.ltr_adhoc.eval.ltr as ref_ltr
        from ptranking.base.adhoc_ranker import AdhocNeuralRanker
        from ptranking.data.data_utils import LABEL_TYPE as REF_LABEL_TYPE
        original = ref_ltr.LambdaRank
        installed = pa.install()
        try:
            assert set(installed) == set(pa.RANKER_NAMES) and not (set(installed) & set(pa.EXTRA_RANKER_NAMES))
            for n, cls in installed.items():
                assert getattr(ref_ltr, n) is cls and issubclass(cls, AdhocNeuralRanker)
                assert cls.custom_loss_function is not getattr(original if n == "LambdaRank" else AdhocNeuralRanker,
                                                               "custom_loss_function")
            # the reference's own factory instantiates OUR class with ITS calling convention (ltr.py:164-171)
            ev = ref_ltr.LTREvaluator()
            sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
                  "pointsf": dict(num_features=8, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False,
                                  bn_type=None, bn_affine=False)}
            for model_id, paras in (("LambdaRank", {"model_id": "LambdaRank", "sigma": 1.0}), ("ListNet", {"model_id": "ListNet"}),
                                    ("ApproxNDCG", {"model_id": "ApproxNDCG", "alpha": 10})):
                ranker = ev.load_ranker(sf_para_dict=sf, model_para_dict=paras)
                assert type(ranker) is installed[model_id]
                ranker.init()                       # the REFERENCE's scorer construction
                assert ranker.forward(torch.randn(2, 5, 8)).shape == (2, 5)
            assert host.is_multilabel(REF_LABEL_TYPE.MultiLabel)
            # listsf: the reference's init() path builds OUR modules (fused attention / LayerNorm) with the reference's key names
            lsf = {"sf_id": "listsf", "opt": "Adam", "lr": 1e-3,
                   "listsf": dict(num_features=8, ff_dims=[16, 16], AF="R", TL_AF="GE", apply_tl_af=False, BN=False, bn_type="BN2",
                                  bn_affine=False, n_heads=2, encoder_layers=1, encoder_type="AllRank")}
            lr = installed["LambdaRank"](sf_para_dict=lsf, model_para_dict={"sigma": 1.0}, gpu=False, device="cpu")
            lr.init()
            from ptranking_amd import listsf as LS
            from ptranking.base.list_ranker import ListNeuralRanker
            assert isinstance(lr.list_sf["encoder"], LS.Encoder) and isinstance(lr.list_sf["encoder"].layers[0].mhsa, LS.MultiheadAttention)
            ref = ListNeuralRanker(sf_para_dict=lsf, gpu=False, device="cpu")
            ref.init()
            for part in ("head_ffnns", "encoder", "tail_ffnns"):
                assert set(lr.list_sf[part].state_dict()) == set(ref.list_sf[part].state_dict()), part
            assert len(lr.get_parameters()) == len(ref.get_parameters())
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                lr.forward(torch.randn(2, 6, 8))
        finally:
            pa.uninstall()
        assert ref_ltr.LambdaRank is original
    finally:
        sys.path.remove(REF)


def _stand_in_ptranking(root):
    """A minimal package with the two module paths install() binds into (ptranking/ltr_adhoc/eval/ltr.py, ptranking/base/adhoc_ranker.py):
    ltr.py holds placeholders for the six ranker names its driver imports; the base class is this package's own standalone one."""
    files = {"ptranking/__init__.py": "", "ptranking/base/__init__.py": "", "ptranking/ltr_adhoc/__init__.py": "",
             "ptranking/ltr_adhoc/eval/__init__.py": "",
             "ptranking/base/adhoc_ranker.py": "from ptranking_amd.rankers import PointScorerRanker\n\n\n"
                                                "class AdhocNeuralRanker(PointScorerRanker):\n    pass\n",
             "ptranking/ltr_adhoc/eval/ltr.py": "".join(f"class {n}:\n    pass\n\n\n" for n in pa.RANKER_NAMES)}
    for rel, text in files.items():
        path = root / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(text)
    return str(root)


@pytest.fixture
def stand_in_ptranking(tmp_path, monkeypatch):
    monkeypatch.setattr(sys, "dont_write_bytecode", True)
    monkeypatch.syspath_prepend(_stand_in_ptranking(tmp_path / "stand_in"))
    for m in [m for m in sys.modules if m == "ptranking" or m.startswith("ptranking.")]:
        monkeypatch.delitem(sys.modules, m)
    yield
    for m in [m for m in sys.modules if m == "ptranking" or m.startswith("ptranking.")]:
        del sys.modules[m]


def test_install_rebinds_and_uninstall_restores_the_ranker_names(stand_in_ptranking):
    """install() puts the fused classes into the driver module under the reference's names, built on the module's AdhocNeuralRanker;
    uninstall() puts the module's own classes back."""
    import ptranking.ltr_adhoc.eval.ltr as ltr
    from ptranking.base.adhoc_ranker import AdhocNeuralRanker
    original = {n: getattr(ltr, n) for n in pa.RANKER_NAMES}
    installed = pa.install()
    try:
        assert set(installed) == set(pa.RANKER_NAMES) and not (set(installed) & set(pa.EXTRA_RANKER_NAMES))
        for n, cls in installed.items():
            assert getattr(ltr, n) is cls and cls is not original[n] and issubclass(cls, AdhocNeuralRanker)
        r = ltr.LambdaRank(sf_para_dict=SF, model_para_dict={"sigma": 1.0}, gpu=False, device="cpu")
        r.init()
        assert r.forward(torch.randn(2, 5, 12)).shape == (2, 5)
    finally:
        pa.uninstall()
    assert {n: getattr(ltr, n) for n in pa.RANKER_NAMES} == original
    assert not any(hasattr(ltr, n) for n in pa.EXTRA_RANKER_NAMES)


def test_padded_batches_with_batch_normalisation_are_rejected():
    """PaddedQueryBatches zero-pads rows; with BN they would enter the statistics — the loops must refuse, not drift."""
    import torch
    from ptranking_amd import host

    class R:
        pass

    r = R()
    r.point_sf = torch.nn.Sequential(torch.nn.Linear(4, 4), host._BatchNormOverDocs(4))
    lens = torch.tensor([3, 2], dtype=torch.int32)
    host._reject_padding_with_batchnorm(r, None)                 # equal-length batches: fine
    with pytest.raises(NotImplementedError, match="batch normalisation"):
        host._reject_padding_with_batchnorm(r, lens)
    r2 = R()
    r2.point_sf = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.ReLU())
    host._reject_padding_with_batchnorm(r2, lens)                # no BN: padding is masked by the kernels


@NEEDS_REF
def test_reference_kfold_cv_eval_runs_on_the_installed_ranker(tmp_path, monkeypatch):
    """the REFERENCE's own driver loop (ptranking/ltr_adhoc/eval/ltr.py:291-369 — load_ranker -> init -> train ->
    scheduler.step -> validation (ValidationTape: save of the best epoch) -> load of the optimal checkpoint -> CVTape.fold_evaluation)
    executed on the class install() put into its module, on CPU, with only `ptranking_amd.functional`'s two device entry points
    replaced by the oracle (test infrastructure) and the data loader replaced by synthetic batches."""
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import ptranking_amd.functional as F_
    from oracle import torch_ref as T
    try:
        import ptranking.ltr_adhoc.eval.ltr as ref_ltr
        from ptranking.data.data_utils import LABEL_TYPE as REF_LABEL_TYPE
        installed = pa.install()
        try:
            calls = {"loss": 0, "metrics": 0}

            def lambdarank_loss(preds, labels, sigma=1.0, lens=None):
                calls["loss"] += 1
                return T.lambdarank_loss(preds, labels, sigma=sigma)

            def metrics_at_ks(preds, labels, ks, presort=False, max_label=None, lens=None, which=("ndcg", "nerr", "ap", "p"),
                              permutation_labels=False):
                calls["metrics"] += 1
                out = T.evaluate_at_ks(preds, labels, list(ks), presort, max_label=max_label)
                return {m: out[m] for m in which}

            monkeypatch.setattr(F_, "lambdarank_loss", lambdarank_loss)
            monkeypatch.setattr(F_, "metrics_at_ks", metrics_at_ks)

            gen = torch.Generator().manual_seed(5)

            def batches(n, B=4, L=12, F=8):
                out = []
                for _ in range(n):
                    X = torch.randn(B, L, F, generator=gen)
                    Y = torch.sort(torch.randint(0, 5, (B, L), generator=gen).float(), dim=1, descending=True)[0]
                    Y[:, 0] = torch.clamp(Y[:, 0], min=1.0)
                    out.append((list(range(B)), X, Y))
                return out

            folds = {k: (batches(3), batches(2), batches(2)) for k in (1, 2)}
            ev = ref_ltr.LTREvaluator()
            ev.dir_run = str(tmp_path) + "/"
            monkeypatch.setattr(ev, "display_information", lambda *a, **k: None)
            monkeypatch.setattr(ev, "check_consistency", lambda *a, **k: None)
            monkeypatch.setattr(ev, "setup_eval", lambda *a, **k: None)
            monkeypatch.setattr(ev, "load_data", lambda eval_dict, data_dict, fold_k: folds[fold_k])
            data_dict = dict(data_id="synthetic", fold_num=2, label_type=REF_LABEL_TYPE.MultiLabel, max_rele_level=4, train_presort=True,
                             validation_presort=True, test_presort=True)
            eval_dict = dict(epochs=3, loss_guided=False, vali_k=5, log_step=1, cutoffs=[1, 3, 5], do_validation=True, vali_metric="nDCG",
                             do_summary=False, do_log=False)
            sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-2,
                  "pointsf": dict(num_features=8, num_layers=3, AF="R", TL_AF="S", apply_tl_af=False, BN=False, bn_type=None, bn_affine=False)}
            scores = ev.kfold_cv_eval(data_dict=data_dict, eval_dict=eval_dict, sf_para_dict=sf,
                                      model_para_dict={"model_id": "LambdaRank", "sigma": 1.0})
            scores = torch.as_tensor(scores)
            assert scores.shape == (3,) and bool(torch.isfinite(scores).all()) and bool((scores > 0).all()) and bool((scores <= 1).all())
            assert calls["loss"] == 2 * 3 * 3                     # folds x epochs x train batches went through OUR custom_loss_function
            assert calls["metrics"] >= 2 * (3 * 2 + 2)            # per-epoch validation + the final test evaluation of every fold
        finally:
            pa.uninstall()
    finally:
        sys.path.remove(REF)


def test_strict_device_is_the_default_and_extras_are_opt_in(monkeypatch, stand_in_ptranking):
    """VERDICT r4 housekeeping: (a) without PTR_STRICT_DEVICE=0 a CPU tensor in a FusedLinear is an error, not torch's F.linear; (b) install()
    leaves the rankers SURVEY.md 2 marks out of scope (DASALC, MDPRank) alone unless asked."""
    import torch
    import ptranking_amd as pa
    from ptranking_amd import _lib, linear
    lin = linear.FusedLinear(4, 3)
    monkeypatch.delenv("PTR_STRICT_DEVICE", raising=False)
    with pytest.raises(_lib.NativeLibraryError):
        lin(torch.zeros(2, 4))
    monkeypatch.setenv("PTR_STRICT_DEVICE", "0")
    assert lin(torch.zeros(2, 4)).shape == (2, 3)
    assert "MDPRank" not in pa.RANKER_NAMES and "DASALC" not in pa.RANKER_NAMES and set(pa.EXTRA_RANKER_NAMES) == {"DASALC", "MDPRank"}
    installed = pa.install(extras=True)
    try:
        assert set(installed) == set(pa.RANKER_NAMES) | set(pa.EXTRA_RANKER_NAMES)
    finally:
        pa.uninstall()


@pytest.mark.parametrize("opt,kind,hyper,h12,keys", [
    ("Adam", 1, dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-3), (0.8, 0.99), ("exp_avg", "exp_avg_sq")),
    ("Adagrad", 2, dict(lr=2e-2, lr_decay=0.1, eps=1e-9, weight_decay=1e-3), (0.1, 0.0), ("sum",)),
    ("RMS", 3, dict(lr=3e-2, alpha=0.9, eps=1e-7, weight_decay=1e-3), (0.9, 0.0), ("square_avg",)),
])
def test_flat_optimiser_bookkeeping_without_a_gpu(opt, kind, hyper, h12, keys):
    """The bookkeeping the three flat optimisers share (scorer.FlatOptimizer) on a CPU parameter: `fused_step_args` returns PTR_OPT_* and the
    group's values in ABI order, creates exactly torch's state keys, counts `step` up by one per call and `undo_step` takes it back by one;
    state_dict() -> load_state_dict() round-trips."""
    from ptranking_amd.scorer import FLAT_OPTIMIZERS, FLAT_VIEW_OPTIMIZERS, FlatOptimizer
    cls = FLAT_OPTIMIZERS[opt]
    assert issubclass(cls, FlatOptimizer) and issubclass(FLAT_VIEW_OPTIMIZERS[opt], cls)
    assert [c for c in FLAT_OPTIMIZERS.values() if issubclass(cls, c)] == [cls]          # no flat optimiser is another one's subclass
    p = torch.nn.Parameter(torch.arange(5, dtype=torch.float32))
    o = cls([p], **hyper)
    assert not o.state[p]
    for t in (1, 2, 3):
        k, lr, h1, h2, eps, wd, step, s1, s2 = o.fused_step_args(p)
        assert (k, lr, h1, h2, eps, wd, step) == (kind, hyper["lr"], h12[0], h12[1], hyper["eps"], hyper["weight_decay"], t)
        st = o.state[p]
        assert set(st) == {"step", *keys} and st["step"] == t
        assert s1 is st[keys[0]] and (s2 is st[keys[1]] if len(keys) == 2 else s2 is None)
        assert all(st[key].shape == p.shape and st[key].dtype == torch.float32 and not st[key].any() for key in keys)
    o.undo_step(p)
    assert o.state[p]["step"] == 2 and o.fused_step_args(p)[6] == 3
    o.state[p][keys[0]].copy_(torch.arange(5.0) + 1)
    q = torch.nn.Parameter(torch.zeros(5))
    o2 = cls([q], **{**hyper, "lr": 1.0})
    o2.load_state_dict(o.state_dict())
    assert set(o2.state[q]) == {"step", *keys} and o2.state[q]["step"] == 3 and o2.param_groups[0]["lr"] == hyper["lr"]
    assert all(torch.equal(o2.state[q][key], o.state[p][key]) for key in keys)
    assert o2.fused_step_args(q)[:7] == (kind, hyper["lr"], h12[0], h12[1], hyper["eps"], hyper["weight_decay"], 4)
