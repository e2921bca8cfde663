"""Plain-numpy restatement of the row sampling of the native booster (ptranking_amd/csrc/gbdt.hip: ptr_gbdt_bag_mask, ptr_gbdt_goss,
ptr_gbdt_partition_mask, ptr_gbdt_add_tree_binned) and of GBDT.update under bagging_fraction / bagging_freq / bagging_by_query and
data_sample_strategy='goss' (ptranking_amd/gbdt.py).  include/ptranking_amd.h states the rules.  Test infrastructure, never imported by the
package.  Nothing here is LightGBM's: the rules are this project's own.

    u(draw, unit) = pl_uniform(pl_query_keys(seed, draw), unit): tests/plsample_ref.py's integer hash, a multiple of 2^-24 in [0, 1)
    bagging       unit in the bag iff u(t // bagging_freq, unit) < float32(bagging_fraction); unit = the row, or its query
    GOSS          key = |g h| (one fp32 product), K = max(1, floor(n top_rate)), tau = the K-th largest key (a NaN key counts as the
                  smallest); key >= tau: kept as it is; otherwise kept iff u(t, row) < float32(other_rate / (1 - top_rate)) and then
                  g, h times float32((1 - top_rate) / other_rate); the first floor(1 / learning_rate) trees use every row
    growth        on the bag alone, in row order (an order-preserving subset handed to the unsampled restatement gives the same tree)
    scores        every row, in the bag or not, gets the leaf value of the walk over its bins
"""
import math

import numpy as np

import gbdt_level_ref as LR
import gbdt_ref as R
from plsample_ref import M32, _lowbias32

NAN_BITS = 0x7F800000                                  # |g h| bit patterns above this one are NaNs


# ---- the uniforms
def uniforms(seed, draw, units):
    """u(draw, unit) for an array of units (int; taken modulo 2^32 as the device's uint32 cast does) -> float32."""
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    u64 = np.uint64
    lo, hi = u64(seed & M32), u64(seed >> 32)
    qlo, qhi = np.array([draw & M32], u64), np.array([draw >> 32], u64)
    mul = lambda a, c: (a * u64(c)) & u64(M32)
    ka = _lowbias32(lo ^ _lowbias32((hi + mul(qlo, 0x9E3779B1) + mul(qhi, 0xC2B2AE3D)) & u64(M32)))
    kb = _lowbias32(hi ^ _lowbias32((lo + mul(qlo, 0x85EBCA77) + mul(qhi, 0x27D4EB2F) + u64(0x68E31DA4)) & u64(M32)))
    i = (np.asarray(units).astype(np.int64) & M32).astype(u64)
    h = _lowbias32((ka + mul(i, 0x85EBCA77)) & u64(M32))
    t = ((h ^ kb) * u64(0x2C1B3C6D)) & u64(M32)
    return ((t >> u64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def group_qid(group):
    """The query of every row, int32 [n], from the documents per query."""
    group = np.asarray(group).reshape(-1).astype(np.int64)
    return np.repeat(np.arange(group.size, dtype=np.int32), group)


# ---- the masks
def bag_mask(n, seed, draw, fraction, qid=None):
    """uint8 [n], 1 = in the bag."""
    units = np.arange(n) if qid is None else np.asarray(qid)
    return (uniforms(seed, draw, units) < np.float32(fraction)).astype(np.uint8)


def goss_keys(g, h):
    """(the uint32 bit patterns of |g h|, which of them are NaN)."""
    with np.errstate(all="ignore"):
        prod = np.asarray(g, np.float32) * np.asarray(h, np.float32)
    bits = prod.view(np.uint32) & np.uint32(0x7FFFFFFF)
    return bits, bits > NAN_BITS


def goss_top_k(n, top_rate):
    return min(max(1, int(math.floor(n * float(top_rate)))), n)


def select_kth_largest(bits, k):
    """The k-th largest (k from 1) of uint32 keys, exactly: np.partition on the integers."""
    bits = np.asarray(bits, np.uint32)
    return int(np.partition(bits, bits.size - k)[bits.size - k])


def goss(g, h, top_rate, other_rate, seed, draw):
    """-> (g', h' float32, mask uint8, info = (tau's bit pattern, the size of the top set, the number kept))."""
    g, h = np.asarray(g, np.float32), np.asarray(h, np.float32)
    n = g.size
    bits, nan = goss_keys(g, h)
    tau = select_kth_largest(np.where(nan, np.uint32(0), bits), goss_top_k(n, top_rate))
    top = ~nan & (bits >= np.uint32(tau))
    p = np.float32(other_rate / (1.0 - top_rate))
    w = np.float32((1.0 - top_rate) / other_rate)
    keep = top | (uniforms(seed, draw, np.arange(n)) < p)
    scaled = keep & ~top
    with np.errstate(all="ignore"):
        g2, h2 = np.where(scaled, g * w, g).astype(np.float32), np.where(scaled, h * w, h).astype(np.float32)
    return g2, h2, keep.astype(np.uint8), (tau, int(top.sum()), int(keep.sum()))


# ---- the partition and the walk
def partition_mask(mask, rows=None, m=None):
    """-> (the kept rows of the list in their order, then the others in theirs; how many were kept).  rows None: 0 .. m - 1.  A row index
    outside the mask is not kept."""
    mask = np.asarray(mask)
    rows = np.arange(mask.size if m is None else m, dtype=np.int32) if rows is None else np.asarray(rows, np.int32)
    inside = (rows >= 0) & (rows < mask.size)
    keep = np.zeros(rows.size, bool)
    keep[inside] = mask[rows[inside]] != 0
    return np.concatenate([rows[keep], rows[~keep]]).astype(np.int32), int(keep.sum())


def split_bins(tree, edges, nbins):
    """The split bin of every node: the index of its threshold among its feature's edges."""
    out = np.zeros(tree["feature"].size, np.int32)
    for k, (f, thr) in enumerate(zip(tree["feature"], tree["threshold"])):
        b = int(np.searchsorted(edges[f, :nbins[f] - 1], thr))
        assert edges[f, b] == thr
        out[k] = b
    return out


def walk_binned(bins, feature, bin, left, right, value):
    """The leaf value one tree gives every binned row -> float32 [n]; NaN for a malformed tree (a child index out of range, a cycle)."""
    n, nn = bins.shape[0], len(feature)
    out = np.zeros(n, np.float32)
    for r in range(n):
        node = 0 if nn else ~0
        for _ in range(nn):
            if node < 0 or node >= nn:
                break
            f = feature[node]
            if f < 0 or f >= bins.shape[1]:
                break
            node = left[node] if bins[r, f] <= bin[node] else right[node]
        out[r] = value[~node] if node < 0 and ~node <= nn else np.nan
    return out


# ---- sampled growth
def sampling(params):
    if params.get("data_sample_strategy", "bagging") == "goss":
        return "goss"
    return "bagging" if params.get("bagging_freq", 0) > 0 and params.get("bagging_fraction", 1.0) < 1.0 else None


def tree_mask(params, t, g, h, qid=None):
    """Tree t (from 0) -> (g', h', mask or None for a tree on every row)."""
    seed = params.get("bagging_seed", 3)
    kind = sampling(params)
    if kind == "goss":
        if t < int(math.floor(1.0 / params.get("learning_rate", 0.1))):
            return g, h, None
        g2, h2, mask, _ = goss(g, h, params.get("top_rate", 0.2), params.get("other_rate", 0.1), seed, t)
        return g2, h2, mask
    if kind == "bagging":
        by_query = params.get("bagging_by_query", False)
        return g, h, bag_mask(g.size, seed, t // params["bagging_freq"], params["bagging_fraction"], qid if by_query else None)
    return g, h, None


def grow(bins, g, h, edges, nbins, params, t, qid=None):
    """One tree of GBDT.update under the sampling parameters -> (tree, mask or None, the leaf value of every row by the binned walk).  The
    quantization runs over all rows of g', h'; the bag's rows, in order, go to the unsampled restatement of the growth policy."""
    p = params
    g2, h2, mask = tree_mask(p, t, np.asarray(g, np.float32), np.asarray(h, np.float32), qid)
    qg, qh, expo, flag = R.quantize(g2, h2)
    assert flag == 0
    bag = np.arange(bins.shape[0]) if mask is None else np.nonzero(mask)[0]
    grower = LR.grow_tree if p.get("grow_policy", "leafwise") == "depthwise" else R.grow_tree
    out = grower(bins[bag], qg[bag], qh[bag], expo, edges, nbins, p["max_bin"], p["num_leaves"], p.get("learning_rate", 0.1), p.get("lambda_l2", 0.0),
                 p.get("min_data_in_leaf", 20), p.get("min_sum_hessian_in_leaf", 1e-3), p.get("min_gain_to_split", 0.0), p.get("max_depth", -1))
    tree, leaf_rows, margin = out[0], out[1], out[2]
    add = walk_binned(bins, tree["feature"], split_bins(tree, edges, nbins), tree["left"], tree["right"], tree["value"])
    for rows, v in zip(leaf_rows, tree["value"]):                       # in the bag the walk is the leaf the growth put the row in
        assert (add[bag[rows]].view(np.int32) == np.float32(v).view(np.int32)).all()
    return tree, mask, add, margin
