"""CPU: the pieces of the synchronised 'BN' statistics that need no GPU — the C ABI's argument checks (before any launch), the gather
helper under a two-rank gloo group, the switch, and the float64 restatement (tests/syncbn_ref.py) against whole-batch statistics and
autograd of the whole batch."""
import ctypes
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import syncbn_ref as S

INVALID = 1001


@pytest.fixture(scope="module")
def lib():
    from ptranking_amd import build, _lib
    build.build()
    return _lib.load()


def test_new_entry_points_are_declared_bound_and_exported(lib):
    from ptranking_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ptranking_amd.h")).read()
    for name in ("ptr_bn_slot_floats", "ptr_bn_stats_partial", "ptr_bn_stats_combine", "ptr_bnact_backward_sums", "ptr_bnact_backward_apply"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION >= 7 and lib.ptr_abi_version() == _lib.ABI_VERSION
    assert lib.ptr_bn_slot_floats(100) == 204 and lib.ptr_bn_slot_floats(1) == 6 and lib.ptr_bn_slot_floats(0) == 0
    assert "2^24" in hdr                                  # the float-count limit is stated where the slot layout is


def test_argument_errors_need_no_gpu(lib):
    """group_rows > 0 (per-query 'BN2' has nothing to exchange), NULL pointers, W <= 0 and a bad lens / rows_per_query pair are refused
    with PTR_ERR_INVALID_ARG before any launch."""
    one = ctypes.c_void_p(4096)
    f, u64 = ctypes.c_float, ctypes.c_uint64
    R, N = 64, 8

    def partial(z=one, group=0, lens=None, rpq=0, ws=one, slot=one, R=R):
        return lib.ptr_bn_stats_partial(z, N, R, N, group, lens, rpq, ws, slot, None)

    def combine(slots=one, W=2, stride=2 * N + 4, mean=one, rstd=one, cnt=one):
        return lib.ptr_bn_stats_combine(slots, W, stride, N, f(1e-5), mean, rstd, cnt, None)

    def sums(z=one, da=one, group=0, lens=None, rpq=0, mean=one, rstd=one, ws=one, out=one):
        return lib.ptr_bnact_backward_sums(z, da, N, R, N, group, lens, rpq, mean, rstd, one, one, 5, f(0.0), u64(1), 1, ws, out, None)

    def apply(z=one, da=one, group=0, lens=None, rpq=0, mean=one, rstd=one, s=one, W=2, cnt=one, ws=one, dz=one):
        return lib.ptr_bnact_backward_apply(z, da, N, R, N, group, lens, rpq, mean, rstd, one, one, 5, f(0.0), u64(1), 1, s, W, cnt, ws, dz, None)

    for fn in (partial, sums, apply):
        assert fn(group=8) == INVALID and b"per-query" in lib.ptr_last_error(), fn.__name__
        assert fn(z=None) == INVALID and b"NULL" in lib.ptr_last_error(), fn.__name__
        assert fn(lens=one, rpq=0) == INVALID and b"rows_per_query" in lib.ptr_last_error(), fn.__name__
        assert fn(lens=one, rpq=7) == INVALID, fn.__name__                    # 64 rows are no multiple of 7
    assert partial(slot=None) == INVALID and partial(ws=None) == INVALID
    assert partial(R=0) == INVALID and b"empty" in lib.ptr_last_error()     # an empty shard stays unsupported
    assert combine(W=0) == INVALID and combine(W=-3) == INVALID
    assert combine(slots=None) == INVALID and combine(mean=None) == INVALID and combine(rstd=None) == INVALID and combine(cnt=None) == INVALID
    assert combine(stride=2 * N) == INVALID                                  # no room for the count
    assert sums(da=None) == INVALID and sums(mean=None) == INVALID and sums(out=None) == INVALID and sums(ws=None) == INVALID
    assert apply(W=0) == INVALID and apply(W=-1) == INVALID
    assert apply(s=None) == INVALID and apply(cnt=None) == INVALID and apply(dz=None) == INVALID and apply(ws=None) == INVALID


# ---------------------------------------------------------------------------------------------------------------- the gather helper
def _gather_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      PTR_DP_BACKEND="gloo")
    from ptranking_amd import dp
    dp.init_from_env()
    g = torch.Generator().manual_seed(100 + rank)
    floats = 37
    mine = torch.randn(floats, generator=g) * (10.0 ** (3 * rank - 2))       # uneven contents: the ranks' values differ by 1e3
    mine[5] = 0.0
    buf, own = dp.new_slots(floats, "cpu")
    own.copy_(mine)
    before_bn, timing_before = dp.BN_COLLECTIVES, dp.TIMING
    dp.TIMING = []
    out = dp.gather_slots(buf)
    torch.save({"mine": mine, "all": out.clone(), "bn_collectives": dp.BN_COLLECTIVES - before_bn, "grad_allreduces": len(dp.TIMING)},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dp.TIMING = timing_before
    dist.barrier()
    dist.destroy_process_group()


def test_gather_slots_is_a_bit_exact_gather_counted_on_its_own(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_gather_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{i}.pt") for i in range(2))
    stacked = torch.stack([r0["mine"], r1["mine"]])
    assert not torch.equal(r0["mine"], r1["mine"])
    for r in (r0, r1):
        assert torch.equal(r["all"], stacked)
        assert r["bn_collectives"] == 1 and r["grad_allreduces"] == 0


def test_gather_slots_refuses_a_buffer_of_another_shape():
    from ptranking_amd import dp
    with pytest.raises(ValueError, match="gather_slots"):
        dp.gather_slots(torch.zeros(3, 5))               # no process group: world size 1


def test_switch_walks_every_fused_stack_and_defaults_to_off():
    import ptranking_amd as pa
    from ptranking_amd import dp
    from ptranking_amd.linear import FusedStack
    assert FusedStack.sync_batch_norm is False
    sf = {"sf_id": "pointsf", "opt": "Adam", "lr": 1e-3,
          "pointsf": dict(num_features=8, num_layers=3, AF="GE", TL_AF="S", apply_tl_af=True, BN=True, bn_type="BN", bn_affine=True, dropout=0.0)}
    r = pa.LambdaRank(sf_para_dict=sf, model_para_dict=dict(pa.DEFAULT_PARAS["LambdaRank"]), gpu=False, device="cpu")
    r.init()
    assert isinstance(r.point_sf, FusedStack) and not r.point_sf.sync_batch_norm
    assert dp.sync_batch_norm(r) == 1 and r.point_sf.sync_batch_norm is True
    assert not r.point_sf._sync_wanted()                   # no process group: the switch alone changes nothing
    assert dp.sync_batch_norm(r, False) == 1 and r.point_sf.sync_batch_norm is False


# ---------------------------------------------------------------------------------------------------------------- the float64 restatement
@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("padded", [False, True])
def test_restatement_matches_whole_batch_statistics_and_autograd(W, padded):
    """W uneven pieces, one of them without a real row: combined slots = whole-batch mean / rstd; dz from the global sums and
    dgamma / dbeta as the sum of the pieces' local sums = autograd of the whole batch (float64, to rounding)."""
    torch.manual_seed(W)
    R, N = 300, 7
    z = (torch.randn(R, N, dtype=torch.float64) * torch.logspace(-2, 2, N, dtype=torch.float64) + 50.0)
    dy = torch.randn(R, N, dtype=torch.float64)
    gamma = torch.randn(N, dtype=torch.float64)
    real = torch.ones(R, dtype=torch.bool)
    if padded:
        real = torch.rand(R) > 0.3
    empty = W - 1 if W > 1 else None
    pieces = S.split_rows(R, W, empty=empty, seed=W)
    assert len({hi - lo for lo, hi in pieces}) == len(pieces) or W == 8        # uneven
    rows = []
    for w, (lo, hi) in enumerate(pieces):
        if w == empty:                                   # the empty piece: rows of its own that are ALL padding
            rows.append((torch.full((5, N), 3.0, dtype=torch.float64), torch.zeros(5, N, dtype=torch.float64), torch.zeros(5, dtype=torch.bool)))
        else:
            rows.append((z[lo:hi], dy[lo:hi], real[lo:hi]))
    slots = [S.partial(zz, rr) for zz, _, rr in rows]
    if empty is not None:
        assert slots[empty][2] == 0 and float(slots[empty][0].abs().max()) == 0
    mean, rstd, n = S.combine(slots)
    zr = z[real]
    assert n == float(real.sum())
    assert torch.allclose(mean, zr.mean(0), rtol=1e-13, atol=0)
    assert torch.allclose(rstd, 1.0 / torch.sqrt(zr.var(0, unbiased=False) + S.EPS), rtol=1e-12, atol=0)
    # whole batch by autograd: y = gamma * xhat + beta over the real rows, loss = sum dy * y
    zz = zr.clone().requires_grad_(True)
    g = gamma.clone().requires_grad_(True)
    b = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    xh = (zz - zz.mean(0)) / torch.sqrt(zz.var(0, unbiased=False) + S.EPS)
    ((g * xh + b) * dy[real]).sum().backward()
    sums = [S.backward_sums(zz_, dd, mean, rstd, rr) for zz_, dd, rr in rows]
    dz = torch.cat([S.backward_apply(zz_, dd, mean, rstd, gamma, sums, n, rr) for w, (zz_, dd, rr) in enumerate(rows) if w != empty])
    assert torch.allclose(dz[real], zz.grad, rtol=1e-9, atol=1e-12 * float(zz.grad.abs().max()))
    assert float(dz[~real].abs().max()) == 0 if padded else True
    assert torch.allclose(sum(s[0] for s in sums), b.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(sum(s[1] for s in sums), g.grad, rtol=1e-9, atol=1e-10)
    if empty is not None:
        assert float(S.backward_apply(*rows[empty][:2], mean, rstd, gamma, sums, n, rows[empty][2]).abs().max()) == 0
