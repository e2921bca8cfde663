"""CPU: PL-Rank without a GPU — ptr_plrank_fwd_bwd's argument errors and empty batch, the refusal of CPU tensors, the names, the launch form."""
import ctypes

import pytest
import torch

ENTRY = "ptr_plrank_fwd_bwd"


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import _lib, build
    build.build()
    return _lib.load()


def _args(preds=16, labels=16, B=1, L=8, S=4, value_q=16, grad=16):
    p = lambda a: ctypes.c_void_p(a) if a else None
    return (p(preds), p(labels), None, B, L, S, 10, 1, 0, 0, None, None, p(value_q), p(grad), None, None)


@pytest.mark.parametrize("bad, word", [(dict(B=-1), b"shape"), (dict(L=0), b"shape"), (dict(L=1025), b"PLRANK_MAX_LEN=1024"), (dict(S=0), b"samples"),
                                       (dict(preds=0), b"NULL"), (dict(labels=0), b"NULL"), (dict(value_q=0), b"NULL"), (dict(grad=0), b"NULL")])
def test_argument_errors_need_no_gpu(lib, bad, word):
    assert getattr(lib, ENTRY)(*_args(**bad)) == 1001 and word in lib.ptr_last_error()
    assert getattr(lib, ENTRY)(*_args(B=0, preds=0, labels=0, value_q=0, grad=0)) == 0      # an empty batch launches nothing


def test_public_names_and_the_launch_form():
    import ptranking_amd as pa
    F = pa.functional
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.plrank_objective(torch.zeros(2, 4), torch.zeros(2, 4))
    assert "plrank_objective" in F.__all__ and F.PLRANK_MAX_LEN == 1024
    assert pa.POLICY_RANKER_NAMES == ("PLRank",) and "PLRank" not in pa.RANKER_NAMES and pa.PLRank is pa.rankers.PLRank
    forms = {(L, S): F.plrank_form(L, S) for L in (1, 64, 65, 130, 257, 1024) for S in (1, 3, 9)}
    assert [forms[L, 9]["DPT"] for L in (1, 64, 65, 130, 257, 1024)] == [1, 1, 2, 4, 8, 16]
    assert [forms[130, S]["waves"] for S in (1, 3, 9)] == [1, 3, 4]
    assert all(f["lds_bytes"] == (3 + 3 * f["waves"]) * 256 * f["DPT"] + 16 <= 64 * 1024 for f in forms.values())
