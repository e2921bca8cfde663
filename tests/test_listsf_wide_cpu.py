"""CPU: the public surface of the wide-head attention forms (heads of 129 .. PTR_MHSA_MAX_HEAD_DIM floats, csrc/listsf_wide.hip): argument
checks of the C ABI before any launch, the module's limit, the forms the library launches for tests/test_listsf_wide_gpu.py's case
list, and the reference-generated fixture (tests/golden/make_golden_listsf_wide.py) against the oracle's restatement."""
import ctypes
import importlib
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import golden_util as G
from launch_form import launch_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")
CSRC = os.path.join(ROOT, "ptranking_amd", "csrc")
INVALID, UNSUPPORTED = 1001, 1002


def _limit():
    return int(re.search(r"#define PTR_MHSA_MAX_HEAD_DIM (\d+)", open(HEADER).read()).group(1))


def _maker():
    spec = importlib.util.spec_from_file_location("make_golden_listsf_wide", os.path.join(G.GOLDEN_DIR, "make_golden_listsf_wide.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _calls(lib):
    one = ctypes.c_void_p(4096)
    f, u = ctypes.c_float, ctypes.c_uint64

    def fwd(B, F, H, L=8, ptr=one):
        return lib.ptr_mhsa_forward(ptr, ptr, ptr, F, None, B, L, F, H, f(0.0), u(0), 0, ptr, ptr, None)

    def bwd(B, F, H, L=8, ptr=one):
        return lib.ptr_mhsa_backward(ptr, ptr, ptr, F, ptr, ptr, ptr, None, B, L, F, H, f(0.0), u(0), 0, ptr, ptr, ptr, ptr, None, None)
    return fwd, bwd


def test_wide_heads_pass_the_argument_checks_without_a_gpu():
    """An empty batch at the Yahoo! shape (700 features, 2 heads: dh 350) succeeds — before this the head dimension was refused first."""
    from ptranking_amd import _lib
    lib = _lib.load()
    fwd, bwd = _calls(lib)
    assert fwd(0, 700, 2) == 0 and bwd(0, 700, 2) == 0
    assert fwd(0, _limit(), 1) == 0 and bwd(0, _limit(), 1) == 0
    assert fwd(2, 700, 2, ptr=None) == INVALID and b"NULL" in lib.ptr_last_error()          # past the head-dimension check, at the pointers


def test_heads_beyond_the_limit_are_refused_and_the_message_names_it():
    from ptranking_amd import _lib
    lib = _lib.load()
    fwd, bwd = _calls(lib)
    lim = _limit()
    for call in (fwd, bwd):
        for F, H in ((lim + 1, 1), (2 * (lim + 1), 2), (700, 1)):
            assert call(0, F, H) == UNSUPPORTED
            msg = lib.ptr_last_error()
            assert b"PTR_MHSA_MAX_HEAD_DIM" in msg and str(lim).encode() in msg and str(F // H).encode() in msg, msg


def test_module_accepts_heads_up_to_the_limit():
    from ptranking_amd import listsf as LS
    lim = _limit()
    assert LS.MAX_HEAD_DIM == lim and lim >= 352
    m = LS.MultiheadAttention(700, 2)
    assert m.w_q.weight.shape == (700, 700) and m.n_heads == 2
    LS.MultiheadAttention(lim, 1)
    with pytest.raises(NotImplementedError, match=f"head dimension {lim + 1} > {lim} is not covered by the fused kernels"):
        LS.MultiheadAttention(lim + 1, 1)
    with pytest.raises(NotImplementedError, match=str(lim)):
        LS.MultiheadAttention(700, 1)                                  # Yahoo! with ONE head stays out of reach


def _wide_form(Bn, L, F, H, mode, ds, packed):
    """The wide form ptr_mhsa_forward / ptr_mhsa_backward launch for a case of 16-byte aligned arrays: DT column tiles (10 .. 22), the
    stored-dS backward or the recomputing one, floats per global access; the chunks of 16 streamed rows and the blocks of 64 rows of L."""
    dh = F // H
    assert 128 < dh <= _limit()
    ld = 3 * F if packed else F
    wide, DT, _, _, store_ds, access = launch_form("ptr_mhsa_backward", L, dh, ld, ds, 16)[:6]
    assert wide and launch_form("ptr_mhsa_forward", L, dh, ld, ds, 16)[:2] == (wide, DT)
    return dict(DT=DT, ds=bool(store_ds), access=access, L=L, dh=dh, mode=mode, packed=packed, chunks=-(-L // 16), blocks=-(-L // 64))


def test_wide_bound_cases_hit_every_dispatch_form():
    """tests/test_listsf_wide_gpu.py's case list launches every wide kernel form: each DT with the recomputing backward (dQ, dK / dV) and
    with the stored-dS backward (dK / dV storing dS, dQ from dS), 16-, 8- and 4-byte accesses, packed and separate, every mode."""
    Gm = importlib.import_module("test_listsf_wide_gpu")
    forms = [_wide_form(*c) for c in Gm.WIDE_CASES]
    assert {(f["DT"], f["ds"]) for f in forms} == {(dt, ds) for dt in range(10, 23, 2) for ds in (False, True)}
    assert all(f["L"] >= 128 for f in forms if f["ds"])               # the product passes the dS scratch from 128 keys on (listsf.py _ds_scratch)
    assert {f["access"] for f in forms} == {4, 2, 1}
    assert {f["packed"] for f in forms if f["access"] == 4} == {True, False} and True in {f["packed"] for f in forms if f["access"] == 2}
    assert {f["access"] for f in forms if f["DT"] == 22} >= {4, 2}          # the Yahoo! head of 350 takes the 8-byte accesses
    assert {f["mode"] for f in forms} == {"eval", "dropout", "lens", "dropout+lens"}
    assert {129, 132, 136, 150, 176, 192, 220, 256, 350, 352} <= {f["dh"] for f in forms}
    assert {7, 32, 33, 64, 65, 128, 129, 257, 513, 1031} <= {f["L"] for f in forms}
    assert min(f["chunks"] for f in forms) == 1 and max(f["blocks"] for f in forms) >= 17      # one chunk of 16; many blocks of 64
    assert {1, 2, 3} <= {c[0] for c in Gm.WIDE_CASES}
    # the issue's fifteen cases are all there
    for c in [(2, 7, 258, 2, "eval", False, False), (3, 33, 264, 2, "lens", False, False), (2, 65, 136, 1, "dropout", False, False),
              (3, 128, 136, 1, "lens", True, False), (2, 129, 300, 2, "dropout+lens", True, False), (2, 32, 300, 2, "dropout+lens", False, True),
              (2, 64, 176, 1, "eval", False, False), (2, 257, 384, 2, "lens", True, False), (2, 64, 256, 1, "eval", False, False),
              (2, 130, 512, 2, "dropout+lens", True, True), (2, 129, 700, 2, "eval", False, False), (3, 257, 700, 2, "dropout+lens", True, False),
              (2, 513, 700, 2, "dropout", False, False), (1, 64, 352, 1, "eval", False, False), (2, 1031, 352, 1, "dropout+lens", True, False)]:
        assert c in Gm.WIDE_CASES, c


def test_build_compiles_the_wide_source():
    from ptranking_amd import build
    assert "listsf_wide.hip" in build.SOURCES and os.path.exists(os.path.join(CSRC, "listsf_wide.hip"))


def test_wide_fixture_loads_and_rewrites_byte_for_byte(tmp_path):
    """The committed archives hold the cases the maker lists, none exceeds the largest fixture there was (step.npz), and writing the
    loaded arrays again through the maker's writer reproduces every archive byte for byte (fixed member dates, sorted members)."""
    M = _maker()
    fams = M.load()
    assert sorted(fams["mhsa"]) == ["c0_d136", "c1_d176"] and sorted(fams["listsf"]) == ["AttnDIN_d136"]
    for (Bn, L, F, H), name in zip(M.MHSA_CASES, sorted(fams["mhsa"])):
        c = fams["mhsa"][name]
        assert c["x"].shape == (Bn, L, F) and int(c["n_heads"]) == H and F // H > 128
        assert {"x", "R", "y", "dx", "sd/w_q.weight", "sd/fc.bias", "grad/w_q.weight", "grad/w_k.bias", "grad/w_v.weight", "grad/fc.weight"} <= set(c)
    total = 0
    for f in M.FILES.values():
        path = os.path.join(G.GOLDEN_DIR, f)
        total += os.path.getsize(path)
        assert os.path.getsize(path) <= 1 << 20, f
        z = np.load(path, allow_pickle=False)
        again = str(tmp_path / f)
        M.write_npz(again, {k: z[k] for k in z.files})
        assert open(again, "rb").read() == open(path, "rb").read(), f
    assert total <= os.path.getsize(os.path.join(G.GOLDEN_DIR, "step.npz"))


@pytest.mark.parametrize("name", ["c0_d136", "c1_d176"])
def test_oracle_restatement_reproduces_the_wide_mhsa_fixture(name):
    from oracle import torch_ref as T
    c = _maker().load()["mhsa"][name]
    sd = {k: _t(v).requires_grad_(True) for k, v in G.sub(c, "sd").items()}
    x = _t(c["x"]).requires_grad_(True)
    y = T.mhsa_ref(x, sd, int(c["n_heads"]))
    (y * _t(c["R"])).sum().backward()
    G.assert_close(y.detach().numpy(), c["y"], "y"); G.assert_close(x.grad.numpy(), c["dx"], "dx")
    for k, v in G.sub(c, "grad").items():
        G.assert_close(sd[k].grad.numpy(), v, k)


def test_module_mirror_loads_the_wide_ranker_fixture():
    from ptranking_amd import listsf as LS
    M = _maker()
    c = M.load()["listsf"]["AttnDIN_d136"]
    mods = LS.build_listsf(**M.RANKER)
    for part, m in mods.items():
        ref_sd = {k: _t(v) for k, v in G.sub(G.sub(c, "sd"), part).items()}
        assert set(m.state_dict().keys()) == set(ref_sd.keys()), part
        m.load_state_dict(ref_sd)
    assert c["preds"].shape == (2, 9) and c["x"].shape == (2, 9, 136)
