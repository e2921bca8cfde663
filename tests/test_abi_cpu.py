"""CPU: the C-ABI library loads and exports every symbol include/ptranking_amd.h declares; the product path refuses to
run without a GPU (no CPU fallback) and never touches oracle/."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from launch_form import launch_form, ring_or_tiling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptranking_amd.h")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ptr_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib_path():
    from ptranking_amd import build
    return build.build()


def test_header_declares_the_expected_entry_points():
    syms = declared_symbols()
    for must in ("ptr_lambdarank_fwd_bwd", "ptr_ranknet_fwd_bwd", "ptr_lambdaloss_fwd_bwd", "ptr_approxndcg_fwd_bwd",
                 "ptr_listnet_fwd_bwd", "ptr_listmle_fwd_bwd", "ptr_sort_desc", "ptr_metrics_at_ks", "ptr_last_error"):
        assert must in syms


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"{lib_path} lacks {missing}"
    lib.ptr_abi_version.restype = ctypes.c_int
    assert lib.ptr_abi_version() == int(re.search(r"#define PTR_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    lib.ptr_last_error.restype = ctypes.c_char_p
    assert isinstance(lib.ptr_last_error(), bytes)


def test_python_binding_matches_header(lib_path):
    from ptranking_amd import _lib
    declared = set(declared_symbols())
    bound = set(_lib.SIGNATURES)
    assert declared <= bound, f"unbound: {sorted(declared - bound)}"
    assert bound - declared <= _lib.OPTIONAL | declared
    handle = _lib.load()
    # the C prototypes and the ctypes argtypes agree on arity
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in declared:
        proto = re.search(name + r"\s*\(([^)]*)\)", src).group(1).strip()
        n = 0 if proto in ("void", "") else proto.count(",") + 1
        assert n == len(_lib.SIGNATURES[name]), name
    assert handle.ptr_abi_version() == _lib.ABI_VERSION
    assert _lib.MAX_LIST_LEN == int(re.search(r"#define PTR_MAX_LIST_LEN (\d+)", src).group(1))


def test_argument_errors_need_no_gpu(lib_path):
    """Argument validation happens before any launch, so it can be exercised on a GPU-less box."""
    from ptranking_amd import _lib
    lib = _lib.load()
    rc = lib.ptr_lambdarank_fwd_bwd(None, None, None, 4, 8, ctypes.c_float(1.0), None, None, None, None)
    assert rc == 1001 and b"NULL" in lib.ptr_last_error()
    one = ctypes.c_void_p(16)
    rc = lib.ptr_sort_desc(one, None, 2, 10 ** 6, one, one, None)
    assert rc == 1002 and b"PTR_MAX_LIST_LEN" in lib.ptr_last_error()
    rc = lib.ptr_lambdaloss_fwd_bwd(one, one, None, 1, 8, 5, ctypes.c_float(1.0), ctypes.c_float(5.0), 7, 1, None, one, one, None)
    assert rc == 1001 and b"loss_type" in lib.ptr_last_error()
    rc = lib.ptr_approxndcg_fwd_bwd(one, one, None, 1, 8, ctypes.c_float(-1.0), 1, 1, ctypes.c_float(0.0), one, one, one, one, one, None)
    assert rc == 1001 and b"alpha" in lib.ptr_last_error()
    ks = (ctypes.c_int32 * 40)(*range(1, 41))
    rc = lib.ptr_metrics_at_ks(one, one, None, 1, 8, ks, 40, 1, 0, ctypes.c_float(4.0), None, one, None, None, None, None)
    assert rc == 1002
    rc = lib.ptr_metrics_at_ks(one, one, None, 1, 8, ks, 3, 1, 1, ctypes.c_float(4.0), None, one, one, None, None, None)
    assert rc == 1002 and b"nERR" in lib.ptr_last_error()          # nERR is undefined for LABEL_TYPE.Permutation
    rc = lib.ptr_metrics_at_ks(one, one, None, 1, 8, ks, 3, 1, 7, ctypes.c_float(4.0), None, one, None, None, None, None)
    assert rc == 1001 and b"label_type" in lib.ptr_last_error()


def test_launch_form_answers_without_a_gpu_and_refuses_what_it_does_not_know():
    from ptranking_amd import _lib
    lib = _lib.load()
    assert launch_form("ptr_wassrank_fwd_bwd", 200)[:3] == (128, 2, 0)
    args, out = (ctypes.c_int64 * 2)(200, 0), (ctypes.c_int32 * 8)()
    assert lib.ptr_launch_form(b"ptr_sort_desc", args, 1, out, 8) == 1001 and b"ptr_sort_desc" in lib.ptr_last_error()
    assert lib.ptr_launch_form(b"ptr_wassrank_fwd_bwd", args, 2, out, 8) == 1001 and b"takes 1" in lib.ptr_last_error()
    assert lib.ptr_launch_form(b"ptr_wassrank_fwd_bwd", args, 1, out, 1) == 1001
    assert lib.ptr_launch_form(None, args, 1, out, 8) == 1001 and lib.ptr_launch_form(b"ptr_wassrank_fwd_bwd", args, 1, None, 8) == 1001


def test_x6_entry_point_validates_without_a_gpu():
    """ABI v3: `ptr_mlp_x6_ws_bytes` / `ptr_mlp_forward_x6` — the configurations the bf16x6 forward does not serve report 0 bytes /
    PTR_ERR_UNSUPPORTED, bad arguments PTR_ERR_INVALID_ARG, an empty batch succeeds, all before any launch."""
    from ptranking_amd import _lib
    lib = _lib.load()
    lib.ptr_mlp_x6_ws_bytes.restype = ctypes.c_size_t
    assert lib.ptr_mlp_x6_ws_bytes(136, 3) == 13 * 21504 + 16384          # 5 + 4 + 4 slices of the weight image + the trace area
    assert lib.ptr_mlp_x6_ws_bytes(46, 3) == 0 and lib.ptr_mlp_x6_ws_bytes(136, 1) == 0 and lib.ptr_mlp_x6_ws_bytes(136, 9) == 0
    one = ctypes.c_void_p(4096)
    args = lambda R, F, NL, p, X=one, acts=one: (X, one, R, F, NL, 1, ctypes.c_float(p), ctypes.c_uint64(1), one, acts, one, None)
    assert lib.ptr_mlp_forward_x6(*args(8, 46, 3, 0.1)) == 1002 and b"bf16x6" in lib.ptr_last_error()
    assert lib.ptr_mlp_forward_x6(*args(8, 136, 3, 1.5)) == 1001 and b"dropout" in lib.ptr_last_error()
    assert lib.ptr_mlp_forward_x6(*args(8, 136, 3, 0.1, X=None)) == 1001 and b"NULL" in lib.ptr_last_error()
    assert lib.ptr_mlp_forward_x6(*args(8, 136, 3, 0.1, X=ctypes.c_void_p(4100))) == 1001 and b"aligned" in lib.ptr_last_error()
    assert lib.ptr_mlp_forward_x6(*args(8, 136, 3, 0.1, acts=None)) == 1001           # a training forward stores its activations
    assert lib.ptr_mlp_forward_x6(*args(2 ** 23, 136, 3, 0.1)) == 1002 and b"4 GB" in lib.ptr_last_error()
    assert lib.ptr_mlp_forward_x6(*args(0, 136, 3, 0.1)) == 0


def test_opt_step_loss_validates_without_a_gpu():
    """ABI v4: `ptr_opt_step_loss` (the data-parallel step's optimiser step + loss-slot sum in one launch) checks its arguments before any launch."""
    from ptranking_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(4096)
    f = ctypes.c_float
    args = lambda kind=1, n=8, step=1, p=one, s2=one, lq=one, nq=4: (p, one, ctypes.c_int64(n), kind, f(1e-3), f(0.9), f(0.999), f(1e-8), f(1e-3), step,
                                                                     one, s2, lq, nq, one, None)
    assert lib.ptr_opt_step_loss(*args(kind=7)) == 1001 and b"optimiser" in lib.ptr_last_error()
    assert lib.ptr_opt_step_loss(*args(step=0)) == 1001
    assert lib.ptr_opt_step_loss(*args(p=None)) == 1001
    assert lib.ptr_opt_step_loss(*args(s2=None)) == 1001            # Adam needs both moment buffers
    assert lib.ptr_opt_step_loss(*args(lq=None)) == 1001            # a loss sum needs its slots
    assert lib.ptr_opt_step_loss(one, one, ctypes.c_int64(0), 1, f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), 1, one, one, None, 0, None, None) == 0


def test_train_step_descriptor_layout_and_validation_without_a_gpu():
    """ABI v5: `ptr_train_step` takes ONE descriptor; the ctypes mirror has the header's size, and a descriptor of another size, an unknown
    loss or missing scratch is refused before any launch."""
    from ptranking_amd import _lib
    lib = _lib.load()
    hdr = open(HEADER).read()
    body = re.search(r"typedef struct ptr_train_step_desc \{(.*?)\} ptr_train_step_desc;", hdr, flags=re.S).group(1)
    names = re.findall(r"[\s\*,]([A-Za-z_0-9]+)(?:\[4\])?\s*(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.TrainStepDesc._fields_], names          # same fields, same order
    assert ctypes.sizeof(_lib.TrainStepDesc) == 256
    d = _lib.TrainStepDesc()
    assert lib.ptr_train_step(None, None) == 1001
    d.struct_bytes = 8
    assert lib.ptr_train_step(ctypes.addressof(d), None) == 1001 and b"descriptor of 8 bytes" in lib.ptr_last_error()
    d.struct_bytes = ctypes.sizeof(_lib.TrainStepDesc)
    d.B, d.L, d.loss_kind = 2, 8, 0
    assert lib.ptr_train_step(ctypes.addressof(d), None) == 1001 and b"unknown loss" in lib.ptr_last_error()
    d.loss_kind = 2
    assert lib.ptr_train_step(ctypes.addressof(d), None) == 1001 and b"NULL scratch" in lib.ptr_last_error()


def test_product_path_fails_loudly_on_cpu_tensors():
    import ptranking_amd as pa
    p, y = torch.zeros(2, 8), torch.zeros(2, 8)
    for fn in (pa.functional.lambdarank_loss, pa.functional.ranknet_loss, pa.functional.listnet_loss,
               pa.functional.approxndcg_loss, pa.functional.lambdaloss_loss):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(p, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pa.functional.metrics_at_ks(p, y, [1, 5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pa.functional.sort_desc(p)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "ptranking_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
                assert "liboracle" not in text, f


def test_missing_library_is_a_loud_error(monkeypatch, tmp_path):
    from ptranking_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.NativeLibraryError, match="no CPU / eager fallback"):
        _lib.load()


def _documented_switches():
    """The PTR_* variables of INTEGRATION.md §6 (first column of its table), without the ones only the tests read."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc.split("## 6. Run-time switches", 1)[1].split("\n## ", 1)[0]
    rows = [line.split("|")[1] for line in sec.splitlines() if line.startswith("| `")]
    names = {n for col in rows if "(tests)" not in col for n in re.findall(r"`(PTR_[A-Z0-9_]+)`", col)}
    assert names, "INTEGRATION.md §6 lists no switches"
    return names


def test_runtime_switches_are_read_in_one_place_and_documented():
    """Every PTR_* variable the library reads goes through ptr::env_int (ptr_device.h) or os.environ in the package, and INTEGRATION.md §6
    lists exactly those; getenv itself appears only in ptr_device.h."""
    pkg = os.path.join(ROOT, "ptranking_amd")
    csrc = os.path.join(pkg, "csrc")
    read = set()
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h", ".cpp")):
            continue
        src = open(os.path.join(csrc, f)).read()
        if f != "ptr_device.h":
            assert "getenv(" not in src, f"{f} reads the environment itself; use ptr::env_int"
        read |= set(re.findall(r'env_int\("(PTR_[A-Z0-9_]+)"', src))
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            for line in open(os.path.join(pkg, f)):
                if "os.environ" in line:
                    read |= set(re.findall(r'"(PTR_[A-Z0-9_]+)"', line))
    assert read == _documented_switches(), (sorted(read - _documented_switches()), sorted(_documented_switches() - read))


def test_bf16x6_split_and_wave_primitives_have_one_home():
    """The bf16x6 numeric contract is written once: the packed fp32 -> bf16 conversion under the three-plane split and the transpose-read
    that feeds the six products live in ptr_x6.h, the global -> LDS DMA in ptr_device.h, and no other file of csrc/ spells them out again
    (comments stripped: several file headers name the instructions in prose).  A private copy compiles, passes its own kernel's tolerance
    gate and breaks the bit-identity between kernels only in combination."""
    csrc = os.path.join(ROOT, "ptranking_amd", "csrc")
    owners = {r"__builtin_convertvector\s*\([^;]*bf\w*\s*\)": "ptr_x6.h",
              r"__builtin_amdgcn_ds_read_tr16_b64": "ptr_x6.h",
              r"global_load_lds_dwordx4": "ptr_device.h"}
    found = {pat: set() for pat in owners}
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h", ".cpp")):
            continue
        code = open(os.path.join(csrc, f)).read()
        code = re.sub(r"/\*.*?\*/", "", code, flags=re.S)
        code = re.sub(r"//[^\n]*", "", code)
        for pat in owners:
            if re.search(pat, code):
                found[pat].add(f)
    for pat, owner in owners.items():
        assert found[pat] == {owner}, f"{pat} belongs in csrc/{owner} alone, found in {sorted(found[pat])}"


def _attn_form(Bn, L, F, H, mode, ds, packed):
    """The forms ptr_mhsa_forward / ptr_mhsa_backward launch for a case of 16-byte aligned arrays: D column tiles, row tiles per forward wave,
    waves and stored dS of the dK / dV kernel, float4 accesses or scalar ones."""
    dh = F // H
    wide, D, row_tiles, dkv_waves, store_ds, access = launch_form("ptr_mhsa_backward", L, dh, 3 * F if packed else F, ds, 16)[:6]
    assert not wide and launch_form("ptr_mhsa_forward", L, dh, 3 * F if packed else F, ds, 16)[:6] == (wide, D, row_tiles, dkv_waves, store_ds, access)
    return dict(fwd=(D, row_tiles), dkv=(D, dkv_waves, bool(store_ds)), vec=access == 4, L=L, dh=dh, mode=mode, packed=packed)


def _ln_form(R, F):
    """NI of the LayerNorm kernels and the trips of their row loops: four rows per workgroup and trip, one per wave."""
    ni, fwd_blocks, bwd_blocks = launch_form("ptr_layernorm_forward", R, F)[:3]
    assert launch_form("ptr_layernorm_backward", R, F)[:3] == (ni, fwd_blocks, bwd_blocks)
    return dict(ni=ni, fwd_trips=-(-R // (4 * fwd_blocks)), bwd_trips=-(-R // (4 * bwd_blocks)))


def test_listsf_bound_cases_hit_every_dispatch_form():
    """tests/test_listsf_bounds_gpu.py's case lists launch every attention and LayerNorm kernel form at least once."""
    import importlib
    G = importlib.import_module("test_listsf_bounds_gpu")
    attn, ln = _attn_form, _ln_form
    forms = [attn(*c) for c in G.ATTN_CASES]
    want_fwd = {(D, rt) for D in range(1, 9) for rt in ((1, 2) if D <= 5 else (1,))}
    # the product passes the dS scratch from 128 keys on (listsf.py _ds_scratch), where D >= 7 takes the 8-wave dK / dV kernel
    want_dkv = {(D, nw, ds) for D in range(1, 9) for nw in ((4, 8) if D >= 7 else (4,)) for ds in (False, True) if not (D >= 7 and nw == 4 and ds)}
    assert want_fwd - {f["fwd"] for f in forms} == set()
    assert want_dkv - {f["dkv"] for f in forms} == set()
    assert {f["vec"] for f in forms} == {True, False}
    assert {f["packed"] for f in forms if f["vec"]} == {True, False} and True in {f["packed"] for f in forms if not f["vec"]}
    assert all(f["L"] >= 128 for f in forms if f["dkv"][2])
    assert {f["mode"] for f in forms} == {"eval", "dropout", "lens", "dropout+lens"}
    assert {7, 32, 33, 64, 65, 128, 129, 256, 257, 513, 1031} <= {f["L"] for f in forms}
    assert {4, 16, 17, 40, 64, 68, 90, 100, 112, 128} <= {f["dh"] for f in forms}
    lns = [(ln(R, F), R, F) for R, F in G.LN_CASES]
    assert {f["ni"] for f, _, _ in lns} == {0, 1, 2, 3, 4}
    for ni in range(5):
        assert max(f["fwd_trips"] for f, _, _ in lns if f["ni"] == ni) >= 2, f"NI={ni}: no forward row loop with a second trip"
        assert max(f["bwd_trips"] for f, _, _ in lns if f["ni"] == ni) >= 8, f"NI={ni}: backward row loop takes few trips"
    assert {F for _, _, F in lns} == {2, 24, 64, 65, 128, 136, 200, 256, 257, 700}
    assert (262144, 136) in G.LN_CASES and 1 in {R for _, R, _ in lns}


def _lambdarank_form(B, L, sigma, ring, monkeypatch):
    """("ring", DPT, "full" or "shrunk": its workgroup against the one a batch that fills the device gets) or ("lds", G, DPT)."""
    monkeypatch.setenv("PTR_LAMBDARANK_RING", str(ring))
    kind, G, DPT, QPB = launch_form("ptr_lambdarank_fwd_bwd", B, L, sigma > 0)[:4]
    if kind != 1:
        assert kind == 0
        return ("lds", G, DPT)
    return ("ring", DPT, "full" if QPB == launch_form("ptr_lambdarank_fwd_bwd", 2 ** 30, L, 1)[3] else "shrunk")


def _ranknet_form(L):
    kind, G, DPT, _ = launch_form("ptr_ranknet_fwd_bwd", 1, L)[:4]
    return ("half-wave",) if kind == 2 else ("lds", G, DPT)


def _approx_form(L, ring, monkeypatch):
    monkeypatch.setenv("PTR_APPROX_RING", str(ring))
    return ring_or_tiling("ptr_approxndcg_fwd_bwd", L)


def _listwise_form(L, unaligned):
    """("vec", V, G) of ListNet's register kernel or ("lds",); ListMLE takes its register kernel for the same calls, with the same V."""
    vec, G, V = launch_form("ptr_listnet_fwd_bwd", L, not unaligned)[:3]
    assert launch_form("ptr_listmle_fwd_bwd", L, not unaligned)[:3] == (vec, 64, V)
    return ("vec", V, G) if vec else ("lds",)


def _ring_z(labels, n, dpt):
    """Z of the LambdaRank ring kernel (ptr_ring.h): trailing slots (documents 64k..64k+63) whose real documents all carry one label,
    the same one from slot to slot; empty slots count."""
    z, zlab, have = 0, None, False
    for k in range(dpt - 1, -1, -1):
        real = labels[64 * k:min(64 * (k + 1), n)]
        empty = 64 * k >= n
        pure = empty or bool((real == real[0]).all())
        if not (empty or (pure and (not have or real[0] == zlab))):
            break
        if not empty:
            zlab, have = real[0], True
        z += 1
    return z


def test_loss_bound_cases_hit_every_dispatch_form(monkeypatch):
    """tests/test_loss_bounds_gpu.py's case lists launch every form of the LambdaRank, RankNet, ApproxNDCG, ListNet, ListMLE, LambdaLoss
    and SoftRank kernels."""
    import importlib
    G = importlib.import_module("test_loss_bounds_gpu")
    lambdarank = lambda B, L, s, r: _lambdarank_form(B, L, s, r, monkeypatch)
    ranknet, approx, listwise = _ranknet_form, lambda L, r: _approx_form(L, r, monkeypatch), _listwise_form
    tilings = {(64, 1), (64, 2), (256, 1), (256, 2), (256, 4), (256, 8), (256, 16)}
    lr = {lambdarank(B, L, s, r) for B, L, s, _, _, _, r, _ in G.LAMBDARANK_CASES}
    # every ring form, its workgroup shrunk (B < waves x CUs) and full
    assert {("ring", d, w) for d in (1, 2, 4, 8) for w in ("full", "shrunk")} <= lr
    assert {("lds",) + t for t in tilings} <= lr
    assert any(c[2] == 0 for c in G.LAMBDARANK_CASES) and any(c[6] == 0 for c in G.LAMBDARANK_CASES)
    assert any(L > 512 for _, L, *_ in G.LAMBDARANK_CASES)
    # the ring kernel's equal-label skip, computed from the generated inputs: for DPT 2, 4 and 8, queries with no skipped slot (Z = 0),
    # with trailing slots of real documents of one grade (label-sorted lists), and with empty trailing slots only
    zs = {}
    for c in G.LAMBDARANK_CASES:
        B, L, s, _, _, _, r, _ = c
        f = lambdarank(B, L, s, r)
        if f[0] != "ring" or f[1] == 1:
            continue
        p, y, n, _ = G.lambdarank_inputs(c)
        for q in range(B):
            z = _ring_z(y[q], int(n[q]), f[1])
            real = 0 < z < f[1] and n[q] - 64 * (f[1] - z) >= 32    # a skipped run of >= 32 real documents (z = DPT: degenerate())
            zs.setdefault(f[1], set()).add("none" if z == 0 else "all" if z == f[1] else "real" if real else "empty")
    assert all(zs.get(d, set()) >= {"none", "real", "empty"} for d in (2, 4, 8)), zs
    assert any(B >= 4096 and L == 128 for B, L, *_ in G.LAMBDARANK_CASES)
    rn = {ranknet(L) for _, L, *_ in G.RANKNET_CASES}
    assert {("half-wave",)} | {("lds",) + t for t in tilings} <= rn
    ap = {approx(L, r) for _, L, _, _, _, r, _ in G.APPROX_CASES}
    assert {("ring", d) for d in (1, 2, 3, 4, 6, 8)} | {("lds",) + t for t in tilings} <= ap
    assert {(c, o == 1.0) for _, _, _, c, o, _, _ in G.APPROX_CASES} >= {(1, False), (1, True), (0, False)}
    assert {pre for _, _, pre, *_ in G.APPROX_CASES} == {0, 1}
    lw = {listwise(L, u) for _, L, _, u in G.LISTWISE_CASES}
    assert {("vec", 1, 16), ("vec", 1, 32), ("vec", 1, 64), ("vec", 2, 64), ("vec", 4, 64), ("lds",)} <= lw
    lds = [(L, u) for _, L, _, u in G.LISTWISE_CASES if listwise(L, u) == ("lds",)]
    assert any(L % 4 for L, _ in lds) and any(L > 1024 for L, _ in lds) and any(u for _, u in lds)
    import f64_loss_bounds as FL                     # ListMLE's two routes: per wavefront, max - min of the scores below 24 or not
    for B, L, off, _ in G.LISTWISE_CASES:
        p, _, n = FL.listwise_inputs(B, L, seed=L + B, offset=1000.0 if off else 0.0)
        spread = [float(p[q, :n[q]].max() - p[q, :n[q]].min()) for q in range(B) if n[q] > 1]
        assert min(spread) < 24.0 < max(spread), (B, L)
    assert any(B % 4 for B, *_ in G.APPROX_CASES) and any(B % 16 for B, *_ in G.LAMBDARANK_CASES)      # B not a multiple of a workgroup
    _check_lambdaloss_softrank_stlistnet_cases()


def _lambdaloss_route(L, k, loss_type, presort, unaligned):
    """("topk", V) or ("generic", G, DPT) of ptr_lambdaloss_fwd_bwd."""
    topk, G, V = launch_form("ptr_lambdaloss_fwd_bwd", L, k, loss_type, presort, not unaligned)[:3]
    return ("topk", V) if topk else ("generic", G, V)


def _topk_libm_queries(case, p, y, n):
    """Queries of a top-k case that leave the fast route: an active pair among the kk best with |sigma ds| > 80."""
    _, L, k, _, _, sigma, _ = case
    out = []
    for q in range(p.shape[0]):
        nq = int(n[q])
        s, lab = p[q, :nq].astype(np.float64), y[q, :nq]
        if np.isnan(s).any():                        # a NaN score: the list's outputs are NaN by either route
            out.append(False)
            continue
        o = np.lexsort((np.arange(nq), -s))[:min(k, nq)]
        x = sigma * np.abs(s[o][:, None] - s[o][None, :])
        out.append(bool(((lab[o][:, None] != lab[o][None, :]) & ~(x <= 80.0)).any()))
    return out


def _check_lambdaloss_softrank_stlistnet_cases():
    """tests/test_loss_bounds_gpu.py's LambdaLoss cases launch all ten forms of ptr_lambdaloss_fwd_bwd, every route that sends a top-k
    eligible call to the generic kernel, both arithmetic routes of the top-k kernel, a batch whose wavefronts must walk; the SoftRank
    cases every dispatch_tiling form."""
    import importlib
    G = importlib.import_module("test_loss_bounds_gpu")
    route = lambda c: _lambdaloss_route(c[1], c[2], c[3], c[4], "u" in c[6])
    gen = {route(c) for c in G.LAMBDALOSS_GENERIC_CASES}
    assert gen == {("generic", 64, 1), ("generic", 64, 2), ("generic", 64, 4), ("generic", 256, 2), ("generic", 256, 4), ("generic", 256, 8),
                   ("generic", 256, 16)}
    assert {route(c) for c in G.LAMBDALOSS_TOPK_CASES} == {("topk", 1), ("topk", 2), ("topk", 4)}
    assert route(G.LAMBDALOSS_PERSISTENT) == ("topk", 1)
    # each reason that keeps a small cut-off off the top-k kernel, alone
    elig = lambda c, **kw: _lambdaloss_route(**{**dict(L=c[1], k=c[2], loss_type=c[3], presort=c[4], unaligned="u" in c[6]), **kw})[0] == "topk"
    why = set()
    for c in G.LAMBDALOSS_GENERIC_CASES:
        why |= {r for r, kw in (("k", dict(k=11)), ("L%4", dict(L=64)), ("unaligned", dict(unaligned=False)), ("loss1", dict(loss_type=1)),
                                ("presort", dict(presort=1))) if elig(c, **kw)}
    assert why == {"k", "L%4", "unaligned", "loss1", "presort"}, why
    assert {c[3] for c in G.LAMBDALOSS_GENERIC_CASES} == {0, 1, 2} and {c[4] for c in G.LAMBDALOSS_GENERIC_CASES} == {0, 1}
    assert all(c[0] % 4 for c in G.LAMBDALOSS_GENERIC_CASES) and all(c[0] <= 96 for c in G.LAMBDALOSS_GENERIC_CASES + G.LAMBDALOSS_TOPK_CASES)
    ks = {("1" if c[2] == 1 else "2" if c[2] == 2 else "5" if c[2] == 5 else "L" if c[2] == c[1] else "2L" if c[2] == 2 * c[1] else
           "odd" if c[2] % 2 else "even") for c in G.LAMBDALOSS_GENERIC_CASES}
    assert ks >= {"1", "2", "5", "odd", "even", "L", "2L"}
    assert {c[2] for c in G.LAMBDALOSS_TOPK_CASES} >= {1, 2, 5, 11} and all(c[3] in (1, 2) and c[4] == 1 for c in G.LAMBDALOSS_TOPK_CASES)
    # the top-k kernel's two arithmetic routes, full lists (the mask-free path), lists shorter than k, ties inside a lane's four documents
    for c in G.LAMBDALOSS_TOPK_CASES:
        p, y, n, _, n_small, _ = G.lambdaloss_inputs(c)
        libm = _topk_libm_queries(c, p, y, n)
        assert any(libm) and not all(libm) if "x" in c[6] else not any(libm), c
        assert "x" not in c[6] or n_small > 0, c     # the libm-route case also holds entries with p < eps
    full = {1 if L <= 256 else 2 for c in G.LAMBDALOSS_TOPK_CASES for L in [c[1]]
            if L in (256, 512) and (G.lambdaloss_inputs(c)[2] == L).any()}
    assert full == {1, 2}
    c = G.LAMBDALOSS_TOPK_CASES[0]
    assert (G.lambdaloss_inputs(c)[2] < c[2]).any()
    tied = False
    for c in G.LAMBDALOSS_TOPK_CASES:
        if "q" in c[6] and c[1] <= 256:
            p, _, n, *_ = G.lambdaloss_inputs(c)
            tied |= any(len(set(p[q, 4 * j:4 * j + 4].tolist())) < 4 for q in range(c[0]) for j in range(int(n[q]) // 4))
    assert tied
    # 8192 wavefronts (256 CUs x 4 SIMDs x 8) is all the device holds: every one walks at least three queries, kk changing on the way
    Bp = G.LAMBDALOSS_PERSISTENT[0]
    assert Bp >= 3 * 256 * 4 * 8 and Bp % 4
    _, _, n, order = G.lambdaloss_persistent_inputs()
    assert set(n.tolist()) == set(range(9)) and len(set(order.tolist())) == 256 and (np.diff(np.minimum(n, 5)) != 0).mean() > 0.5
    tilings = {(64, 1), (64, 2), (256, 1), (256, 2), (256, 4), (256, 8), (256, 16)}
    assert {ring_or_tiling("ptr_softrank_fwd_bwd", L)[1:] for _, L, *_ in G.SOFTRANK_CASES} == tilings
    assert {d for _, _, d, _, _ in G.SOFTRANK_CASES} == {2.0, 0.3} and any(o for *_, o in G.SOFTRANK_CASES)
    assert {("none" if k == 0 else "> n" if k > L else "cut") for _, L, _, k, _ in G.SOFTRANK_CASES} == {"none", "> n", "cut"}
    assert {L for _, L, *_ in G.STLISTNET_CASES} == {64, 63, 128, 1500} and {T for _, _, T, _, _ in G.STLISTNET_CASES} == {1.0, 2.0, 0.5}
