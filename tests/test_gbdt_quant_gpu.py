"""Quantized-gradient training on the device against plain numpy (tests/gbdt_quant_ref.py, gbdt_ref.py), bit for bit: no tolerances."""
import numpy as np
import pytest
import torch

import gbdt_quant_ref as Q
import gbdt_ref as R
from launch_form import launch_form
from test_gbdt_sample_gpu import bits, dev, fit_data  # noqa: F401  (fit_data is a fixture)

pytestmark = pytest.mark.gpu
BOUNDS = (128, 256)                                                                       # B = 256: the shortest flush period


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("stochastic", [True, False])
@pytest.mark.parametrize("B", [2, 4, 256])
@pytest.mark.parametrize("n", [1, 257, 5000])
def test_quantizer_equals_the_restatement(n, B, stochastic):
    from ptranking_amd import functional as F
    rng = np.random.default_rng(n + B)
    g, h = rng.standard_normal(n).astype(np.float32), rng.random(n).astype(np.float32)
    g *= np.float32(3.0) / np.abs(g).max()
    g[0] = 3.0                                                                            # the exact maximum, with both signs, and zeros
    if n > 2:
        g[1], g[2], h[2] = -3.0, 0.0, 0.0
    half = np.clip(g, -0.5, 0.5)                                                          # max|g| = 0.5: fr = 0.5 exactly
    for gg, hh in ((g, h), (half, np.zeros(n, np.float32)), (half, np.full(n, 0.5, np.float32))):
        want = Q.quantize_low(gg, hh, B, stochastic, 11, 4)
        qg, qh, expo, flag = F.gbdt_quantize_low(dev(gg), dev(hh), B, stochastic, 11, 4)
        assert np.array_equal(host(qg), want[0]) and np.array_equal(host(qh), want[1]) and tuple(host(expo)) == want[2] and int(flag) == 0
        again, other = F.gbdt_quantize_low(dev(gg), dev(hh), B, stochastic, 11, 4), F.gbdt_quantize_low(dev(gg), dev(hh), B, stochastic, 11, 5)
        assert torch.equal(again[0], qg) and torch.equal(again[1], qh)                    # equal draws repeat
        if stochastic and n >= 257 and gg is g:
            assert not torch.equal(other[0], qg) and not torch.equal(other[1], qh)        # different draws differ
    for bad in (np.nan, np.inf):
        gb = g.copy()
        gb[n // 2] = bad
        want = Q.quantize_low(gb, h, B, stochastic, 11, 4)
        qg, qh, expo, flag = F.gbdt_quantize_low(dev(gb), dev(h), B, stochastic, 11, 4)
        assert int(flag) == 1 and want[3] == 1 and int(qg[n // 2]) == 0 and int(qh[n // 2]) == 0
        assert np.array_equal(host(qg), want[0]) and np.array_equal(host(qh), want[1]) and tuple(host(expo)) == want[2]


@pytest.mark.parametrize("max_bin", [2, 255, 256])
@pytest.mark.parametrize("nf", [1, 16, 17, 33])
@pytest.mark.parametrize("m", [257, 2049])
def test_packed_histogram_equals_numpy_and_the_int64_kernel(m, nf, max_bin):
    from ptranking_amd import functional as F
    rng = np.random.default_rng(m + nf + max_bin)
    n = m + 40
    b = rng.integers(0, max_bin, (n, nf)).astype(np.uint8)
    b[rng.integers(0, n, 9), rng.integers(0, nf, 9)] = 255                                # bins >= max_bin (below 256) are skipped
    qg, qh = rng.integers(-128, 129, n).astype(np.int32), rng.integers(-256, 257, n).astype(np.int32)
    qg[:4], qh[:4] = (128, -128, 128, -128), (256, 256, -256, -256)
    lst = rng.permutation(n)[:m].astype(np.int32)
    lst[[3, m // 2]], lst[[7, m - 1]] = -1, n + 5                                         # entries outside the matrix are skipped
    bd, gd, hd = dev(np.pad(b, ((0, 0), (0, -nf % 16)))), dev(qg), dev(qh)
    for rows in (None, lst):
        valid = np.arange(m) if rows is None else rows[(rows >= 0) & (rows < n)]
        want = R.histogram(b, qg, qh, valid, 256)[:, :max_bin]                            # a bin >= max_bin lands behind the slice
        kw = dict(m=m) if rows is None else {}
        got = F.gbdt_histogram(bd, gd, hd, None if rows is None else dev(rows), nf, max_bin, bounds=BOUNDS, **kw)
        assert np.array_equal(host(got), want)
        assert torch.equal(got, F.gbdt_histogram(bd, gd, hd, None if rows is None else dev(rows), nf, max_bin, **kw))


def test_packed_histogram_flushes_before_a_field_overflows():
    # B = 256, every row in bin 0 of constant features, values at the bounds, more than 3 R rows in one workgroup: no flush, no fit
    from ptranking_amd import functional as F
    nf, max_bin = 16 * 1024, 2                                                            # 1024 tiles: the chunk cap is one chunk
    R_ = launch_form("ptr_gbdt_histogram_packed", 1, nf, max_bin, *BOUNDS)[5]
    m = 3 * R_ + 300
    kind, _, tiles, chunks, lds, flush = launch_form("ptr_gbdt_histogram_packed", m, nf, max_bin, *BOUNDS)[:6]
    assert kind == 2 and flush == R_ == 4095 and -(-m // chunks) > 3 * R_ and lds == 16 * max_bin * 8
    bd = torch.zeros((m, nf), device="cuda", dtype=torch.uint8)
    for g, h in ((128, 256), (-128, 256), (-128, -256)):
        gd, hd = torch.full((m,), g, device="cuda", dtype=torch.int32), torch.full((m,), h, device="cuda", dtype=torch.int32)
        one = R.histogram(np.zeros((m, 1), np.uint8), host(gd), host(hd), None, max_bin)
        got = F.gbdt_histogram(bd, gd, hd, None, nf, max_bin, bounds=BOUNDS)
        assert np.array_equal(host(got), np.broadcast_to(one, (nf, max_bin, 3)))
        assert torch.equal(got, F.gbdt_histogram(bd, gd, hd, None, nf, max_bin))


def test_packed_segments_mix_every_form_in_one_call():
    from ptranking_amd import functional as F
    nf, max_bin = 16 * 512, 4                                                             # 512 tiles: two chunks per call, so a chunk exceeds R rows
    counts = [1, 256, 257, 9000]
    form = launch_form("ptr_gbdt_histogram_segments_packed", counts[3], nf, max_bin, counts[2] + counts[3], *BOUNDS)
    assert form[0] == 2 and form[5] > form[7] == 4095 and launch_form("ptr_gbdt_histogram_segments_packed", 256, nf, max_bin, 0, *BOUNDS)[0] == 1
    rng = np.random.default_rng(5)
    n = sum(counts) + 100
    bd = torch.from_numpy(rng.integers(0, max_bin, (n, nf), dtype=np.uint8)).cuda()
    qg, qh = rng.integers(-128, 129, n).astype(np.int32), rng.integers(-256, 257, n).astype(np.int32)
    rows = rng.permutation(n).astype(np.int32)
    starts = np.concatenate([[50], 50 + np.cumsum(counts)[:-1]])
    segs = np.stack([starts, counts, [3, 0, 2, 1]], axis=1)
    pool = F.gbdt_histogram_segments(bd, dev(qg), dev(qh), dev(rows), segs, nf, max_bin, torch.zeros((4, nf, max_bin, 3), device="cuda", dtype=torch.int64),
                                     bounds=BOUNDS)
    cols = [0, 17, nf - 1]
    sub = host(bd[:, cols])
    for s, c, slot in segs:
        part = rows[s:s + c]
        assert np.array_equal(host(pool[slot][cols]), R.histogram(sub, qg, qh, part, max_bin))          # numpy, on three columns
        assert torch.equal(pool[slot], F.gbdt_histogram(bd, dev(qg), dev(qh), dev(part), nf, max_bin))   # the int64 kernel, on all


@pytest.mark.parametrize("nleaves", [1, 31, 1025])
def test_leaf_sums_rows_equals_numpy(nleaves):
    from ptranking_amd import functional as F
    rng = np.random.default_rng(nleaves)
    chunk = launch_form("ptr_gbdt_leaf_sums_rows", 10 ** 6, nleaves)[2]
    sizes = rng.integers(0, 40, nleaves)
    sizes[:3] = [3 * chunk + 5] if nleaves == 1 else [0, 1, 3 * chunk + 5]                # empty, one row, longer than a workgroup's share
    n = int(sizes.sum()) + 10
    assert launch_form("ptr_gbdt_leaf_sums_rows", int(sizes.sum()), nleaves)[1] > 1       # the long leaf is split over workgroups
    rows = rng.permutation(n)[:int(sizes.sum())].astype(np.int32)
    rows[[5, rows.size - 1]] = -1, n                                                      # skipped
    qg, qh = (rng.integers(-2 ** 30, 2 ** 30, n).astype(np.int32) for _ in range(2))
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    want = np.zeros((nleaves, 3), np.int64)
    for l in range(nleaves):
        part = rows[offsets[l]:offsets[l + 1]]
        part = part[(part >= 0) & (part < n)]
        want[l] = qg[part].astype(np.int64).sum(), qh[part].astype(np.int64).sum(), part.size
    assert np.array_equal(host(F.gbdt_leaf_sums_rows(dev(rows), dev(offsets), dev(qg), dev(qh))), want)


BASE = {"max_bin": 31, "num_leaves": 8, "min_data_in_leaf": 10, "learning_rate": 0.3, "use_quantized_grad": True, "quant_seed": 5}
BAG = {"bagging_fraction": 0.5, "bagging_freq": 1}
ROUNDS = 3


def run_fit(d, params, rounds=ROUNDS, init_model=None):
    # squared error; the restatement runs under the same device gradients -> (booster, [(tree, restated tree, restated scores)], reads per update)
    import ptranking_amd as pa
    booster = pa.GBDT(params).fit_bins(d["X"], group=d["group"], **({} if init_model is None else {"init_model": init_model}))
    yd, ones, n = dev(d["y"]), torch.ones(d["X"].shape[0], device="cuda"), d["X"].shape[0]
    ref, out, reads = host(booster.scores).copy(), [], []
    for _ in range(rounds):
        g, t, before = booster.scores - yd, len(booster.trees), booster.host_reads
        tree = booster.update(g, ones)
        reads.append(booster.host_reads - before)
        want, _, add = Q.grow(d["bins"], host(g), np.ones(n, np.float32), d["edges"], d["nbins"], booster.params, t, d["qid"])
        ref = ref + add
        out.append((tree, want, ref.copy()))
    return booster, out, reads


def same_tree(got, want):
    return (all(np.array_equal(got[k], want[k]) for k in ("feature", "left", "right"))
            and np.array_equal(bits(got["threshold"]), bits(want["threshold"])) and np.array_equal(bits(got["value"]), bits(want["value"])))


@pytest.mark.parametrize("bag", [False, True])
@pytest.mark.parametrize("policy", ["leafwise", "depthwise"])
def test_quantized_fits_equal_the_restatement(fit_data, policy, bag, tmp_path):
    params = dict(BASE, grow_policy=policy, **(BAG if bag else {}))
    runs = {renew: run_fit(fit_data, dict(params, quant_train_renew_leaf=renew)) for renew in (False, True)}
    for renew, (booster, out, reads) in runs.items():
        for t, (got, want, ref) in enumerate(out):
            assert same_tree(got, want) and got["feature"].size > 0, (renew, t)
        assert np.array_equal(bits(booster.scores), bits(out[-1][2])) and torch.equal(booster.predict(fit_data["X"]), booster.scores)
    none = {"value": np.zeros(1, np.float32)}
    assert same_tree({**runs[True][1][0][0], **none}, {**runs[False][1][0][0], **none})   # tree 0: the structure does not depend on renewal
    assert runs[True][2][0] == runs[False][2][0] + 1                                      # and renewal costs exactly one more read for it
    if all(o[0]["feature"].size == 7 for r in runs.values() for o in r[1]) and policy == "leafwise":
        assert runs[True][0].host_reads == runs[False][0].host_reads + ROUNDS             # full trees read alike: one more per tree
    # a fit split by save_model / init_model equals the unsplit fit
    first, _, _ = run_fit(fit_data, dict(params, quant_train_renew_leaf=True), rounds=2)
    first.save_model(tmp_path / "two.npz")
    cont, out, _ = run_fit(fit_data, dict(params, quant_train_renew_leaf=True), rounds=1, init_model=tmp_path / "two.npz")
    whole = runs[True][0]
    assert len(cont.trees) == ROUNDS and all(same_tree(a, b) for a, b in zip(cont.trees, whole.trees)) and torch.equal(cont.scores, whole.scores)


def test_lambdamart_trains_under_the_keys(fit_data, monkeypatch):
    import ptranking_amd as pa
    from ptranking_amd import gbdt as G
    d, seen, real = fit_data, [], G.GBDT.update
    monkeypatch.setattr(G.GBDT, "update", lambda self, g, h: (seen.append((host(g).copy(), host(h).copy())), real(self, g, h))[1])
    y = np.clip(np.round(d["y"] + 1), 0, 4).astype(np.float32)
    params = dict(BASE, num_grad_quant_bins=16, quant_train_renew_leaf=True, min_sum_hessian_in_leaf=1e-6)
    model = pa.LambdaMART(params, objective="lambdarank_ndcg").fit(d["X"], y, np.full(100, 30), num_boost_round=2)
    assert len(model.booster.trees) == len(seen) == 2 and model.booster.trees[0]["feature"].size > 0
    for t, (g, h) in enumerate(seen):
        assert same_tree(model.booster.trees[t], Q.grow(d["bins"], g, h, d["edges"], d["nbins"], model.booster.params, t)[0]), t


@pytest.mark.parametrize("B", [2, 4, 256])
def test_launch_forms_report_the_packed_tile(B):
    for max_bin in (2, 255, 256):
        one = launch_form("ptr_gbdt_histogram_packed", 5000, 33, max_bin, B // 2, B)
        seg = launch_form("ptr_gbdt_histogram_segments_packed", 5000, 33, max_bin, 5000, B // 2, B)
        assert one[:5] == launch_form("ptr_gbdt_histogram", 5000, 33, max_bin)[:4] + (16 * max_bin * 8,)      # 8 bytes per cell of the 16-feature tile
        assert seg[4] == 16 * max_bin * 8 and one[5] == seg[7] == (2 ** 20 - 1) // B
    assert launch_form("ptr_gbdt_histogram_packed", 256, 33, 255, B // 2, B)[:5] == (1, 16, 3, 0, 0)                 # up to 256 rows: the direct form
