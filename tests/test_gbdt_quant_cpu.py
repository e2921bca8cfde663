"""Quantized-gradient training without a GPU: the parameters, the model-file key rule, and the restatement's own invariants."""
import json

import numpy as np
import pytest

import gbdt_quant_ref as Q
from test_gbdt_cst_cpu import host_booster, members

DEFAULTS = {"use_quantized_grad": False, "num_grad_quant_bins": 4, "stochastic_rounding": True, "quant_train_renew_leaf": False, "quant_seed": 0}


def test_defaults_and_validation():
    from ptranking_amd import gbdt
    assert set(gbdt.QUANT_KEYS) == set(DEFAULTS)
    for k, v in DEFAULTS.items():
        assert gbdt.DEFAULT_PARAMS[k] == v and type(gbdt.DEFAULT_PARAMS[k]) is type(v) and k not in gbdt.IGNORED_PARAMS, k
        assert gbdt.GBDT({k: v}).params == gbdt.GBDT().params
    p = gbdt._params({"use_quantized_grad": np.bool_(True), "num_grad_quant_bins": np.int64(256), "quant_seed": 2 ** 64 - 1})
    assert p["use_quantized_grad"] is True and p["num_grad_quant_bins"] == 256 and type(p["num_grad_quant_bins"]) is int
    for bad in (0, 1, 3, 6, 512, 4.0, "4", True, None):                                   # no power of two in 2 .. 256
        with pytest.raises(ValueError, match="num_grad_quant_bins"):
            gbdt._params({"num_grad_quant_bins": bad})
    for k in ("use_quantized_grad", "stochastic_rounding", "quant_train_renew_leaf"):
        for bad in (1, 0, "true", None):
            with pytest.raises(ValueError, match=f"{k} must be True or False"):
                gbdt._params({k: bad})
    for bad in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match="quant_seed"):
            gbdt._params({"quant_seed": bad})
    with pytest.raises(ValueError, match="quant_train_renew_leaf is not available under monotone_constraints"):
        gbdt._params({"use_quantized_grad": True, "quant_train_renew_leaf": True, "monotone_constraints": [0, 1]})


def test_the_keys_are_in_a_model_file_only_under_the_switch(tmp_path):
    from ptranking_amd import gbdt
    files = []
    for k, extra in enumerate(({}, {"use_quantized_grad": False, "num_grad_quant_bins": 16, "quant_seed": 9})):
        host_booster(dict({"max_bin": 8}, **extra)).save_model(tmp_path / f"{k}.npz")
        files.append(members(tmp_path / f"{k}.npz"))
    assert files[0] == files[1]                                                           # off: the file written before the keys existed
    with np.load(tmp_path / "1.npz", allow_pickle=False) as z:
        assert not set(json.loads(str(z["params"]))) & set(gbdt.QUANT_KEYS) and int(z["format"]) == 1
    assert {k: gbdt.GBDT.load_model(tmp_path / "1.npz").params[k] for k in DEFAULTS} == DEFAULTS       # and it loads with the defaults
    on = host_booster({"max_bin": 8, "use_quantized_grad": True, "num_grad_quant_bins": 16, "quant_train_renew_leaf": True, "quant_seed": 9})
    on.save_model(tmp_path / "on.npz")
    with np.load(tmp_path / "on.npz", allow_pickle=False) as z:
        assert set(gbdt.QUANT_KEYS) <= set(json.loads(str(z["params"]))) and int(z["format"]) == 1
    assert gbdt.GBDT.load_model(tmp_path / "on.npz").params == on.params


@pytest.mark.parametrize("B", [2, 4, 256])
def test_the_restatement_keeps_its_bounds(B):
    rng = np.random.default_rng(B)
    g, h = (rng.standard_normal(4000) * 3).astype(np.float32), rng.random(4000).astype(np.float32)
    g[:2], h[0] = (np.abs(g).max(), -np.abs(g).max()), h.max()
    for stochastic in (True, False):
        qg, qh, (eg, eh), flag = Q.quantize_low(g, h, B, stochastic, 3, 1)
        assert flag == 0 and np.abs(qg).max() <= B // 2 and 0 <= qh.min() and qh.max() <= B
        if not stochastic:
            assert np.array_equal(qg, np.rint(np.ldexp(g.astype(np.float64), eg))) and np.array_equal(qh, np.rint(np.ldexp(h.astype(np.float64), eh)))
    assert Q.quantize_low(np.zeros(3, np.float32), np.zeros(3, np.float32), B, True, 0, 0)[2] == (0, 0)
    assert Q.quantize_low(np.array([np.nan, 1], np.float32), np.ones(2, np.float32), B, False, 0, 0)[3] == 1
