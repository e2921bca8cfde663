"""CPU: NeuralNDCG without a GPU — the argument errors of the C entry point and of the Python surface, the symbol's declaration, export and
binding, the opt-in ranker name, and two properties of the float64 restatement (tests/neuralndcg_ref.py) that pin the rule itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import neuralndcg_ref as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ptranking_amd.h")
ENTRY = "ptr_neuralndcg_fwd_bwd"


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbol_is_declared_exported_and_bound_and_the_names_are_public(lib):
    from ptranking_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(ENTRY + r"\s*\(([^)]*)\)", src).group(1)
    assert proto.count(",") + 1 == len(_lib.SIGNATURES[ENTRY]) == 14 and hasattr(lib, ENTRY) and "neuralndcg.hip" in build.SOURCES
    assert int(re.search(r"#define PTR_ABI_VERSION (\d+)", src).group(1)) == 8 == lib.ptr_abi_version() == _lib.ABI_VERSION


def test_every_argument_error_of_the_entry_point_needs_no_gpu(lib):
    f, one = ctypes.c_float, ctypes.c_void_p(16)

    def args(preds=one, labels=one, B=1, L=8, tau=1.0, iters=50, loss_q=one, grad=one, ws=None):
        return (preds, labels, None, B, L, f(tau), iters, 0, 1, None, loss_q, grad, ws, None)
    for bad, word in ((dict(preds=None), b"NULL"), (dict(labels=None), b"NULL"), (dict(loss_q=None), b"NULL"), (dict(grad=None), b"NULL"),
                      (dict(tau=0.0), b"tau"), (dict(tau=-1.0), b"tau"), (dict(tau=float("nan")), b"tau"), (dict(iters=-1), b"iters"),
                      (dict(L=1025), b"1024"), (dict(L=0), b"shape"), (dict(L=1024), b"workspace")):
        assert getattr(lib, ENTRY)(*args(**bad)) == 1001 and word in lib.ptr_last_error(), bad
    assert getattr(lib, ENTRY)(*args(B=0, preds=None, labels=None, loss_q=None, grad=None)) == 0       # an empty batch launches nothing


def test_python_argument_errors_need_no_gpu():
    import ptranking_amd.functional as F
    z = torch.zeros(2, 4)
    for p, y, kw in ((z, z, dict(temperature=0.0)), (z, z, dict(temperature=-1.0)), (z, z, dict(iters=-1)),
                     (torch.zeros(2, 1025), torch.zeros(2, 1025), {}), (z, torch.zeros(2, 5), {}), (torch.zeros(4), torch.zeros(4), {}),
                     (z, z, dict(lens=torch.zeros(3, dtype=torch.int32)))):
        with pytest.raises(ValueError):
            F.neuralndcg_loss(p, y, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.neuralndcg_loss(z, z)
    import ptranking_amd as pa
    assert callable(pa.functional.neuralndcg_loss) and pa.SORT_RANKER_NAMES == ("NeuralNDCG",) and "NeuralNDCG" not in pa.RANKER_NAMES
    assert pa.NeuralNDCG is pa.rankers.NeuralNDCG and pa.DEFAULT_PARAS["NeuralNDCG"]["iters"] == 50 and "NeuralNDCG" in pa.make_ranker_classes()
    cut = pa.functional.neuralndcg_form(128, 50)["cutover"]
    assert 128 < cut < 1024 and [pa.functional.neuralndcg_form(L, 50)["resident"] for L in (cut, cut + 1)] == [1, 0]


@pytest.mark.parametrize("top_k", [None, 1, 5, 40])
def test_at_tau_1e_3_on_untied_scores_the_loss_is_the_true_ndcg_of_the_score_order(top_k):
    rng = np.random.default_rng(3)
    s, y = rng.permutation(37) * 0.25 - 3.0, rng.integers(0, 5, 37).astype(np.float64)
    k = min(top_k or 37, 37)
    d, g = 1.0 / np.log2(np.arange(37) + 2.0), 2.0 ** y - 1.0
    want = (g[np.argsort(-s)][:k] * d[:k]).sum() / (np.sort(g)[::-1][:k] * d[:k]).sum()
    got = R.ndcg_query(torch.from_numpy(s), torch.from_numpy(y), tau=1e-3, iters=50, top_k=top_k)
    assert abs(float(got) - want) <= 1e-9


def test_fifty_iterations_leave_a_doubly_stochastic_matrix():
    """On 8 documents a unit apart: the rule fixes T, and the columns of 29 standard-normal scores at tau = 1 are still 2e-4 away."""
    s = torch.tensor([3.0, 0.0, 6.0, 4.0, 1.0, 7.0, 2.0, 5.0], dtype=torch.float64)
    P = R.ndcg_query(s, torch.ones(8), iters=50, return_matrix=True)
    assert (P.sum(0) - 1).abs().max() <= 1e-6 and (P.sum(1) - 1).abs().max() <= 1e-6
