"""Plain-numpy restatement of the gradient-boosted tree kernels (ptranking_amd/csrc/gbdt.hip) and of the leaf-wise growth of
ptranking_amd/gbdt.py: one function per entry point.  Test infrastructure, never imported by the package.  Nothing here is LightGBM's: that
library is not installed where this project is tested, and the binning and tie rules are this project's own.

`fault` arguments plant one wrong rule each, so that tests can show that a comparison against this file is able to fail."""
import numpy as np

REC = 9


# ---- binning
def bin_edges(X, max_bin):
    """-> (edges float32 [F, max_bin - 1] padded with +inf, nbins int32 [F]).  At most max_bin distinct values: an edge between every two
    neighbours.  Otherwise edge k (1 .. max_bin - 1) follows the first distinct value whose cumulative count reaches k n / max_bin.  An edge
    is the fp32 midpoint, or the lower value where that midpoint rounds up to the upper one."""
    X = np.asarray(X, np.float32)
    n, nf = X.shape
    edges = np.full((nf, max_bin - 1), np.inf, np.float32)
    nbins = np.ones(nf, np.int32)
    for f in range(nf):
        col = np.sort(X[:, f])
        vals = [col[0]]
        cum = []
        for i in range(1, n):
            if col[i] != col[i - 1]:
                vals.append(col[i])
                cum.append(i)
        cum.append(n)
        if len(vals) <= max_bin:
            cut = list(range(len(vals) - 1))
        else:
            cut = []
            for k in range(1, max_bin):
                target = k * (n / max_bin)
                i = next(j for j, c in enumerate(cum) if c >= target)
                if i < len(vals) - 1 and i not in cut:
                    cut.append(i)
        for j, i in enumerate(cut):
            lo, hi = vals[i], vals[i + 1]
            mid = np.float32((np.float64(lo) + np.float64(hi)) * 0.5)
            edges[f, j] = lo if mid >= hi else mid
        nbins[f] = len(cut) + 1
    return edges, nbins


def bin_matrix(X, edges, nbins):
    """bins [n, F] uint8 (no pad columns): the number of the feature's first nbins - 1 edges below x."""
    X = np.asarray(X, np.float32)
    out = np.zeros(X.shape, np.uint8)
    for f in range(X.shape[1]):
        out[:, f] = (edges[f, :nbins[f] - 1][None, :] < X[:, f][:, None]).sum(axis=1)
    return out


# ---- quantization
def exponent(mx, fault=None):
    """The largest integer e with mx 2^e < 2^30; 0 for mx == 0."""
    if mx == 0:
        return 0
    e = 30 - int(np.frexp(np.float64(mx))[1])
    assert mx * 2.0 ** e < 2.0 ** 30 <= mx * 2.0 ** (e + 1)
    return e + (1 if fault == "exponent" else 0)


def quantize(g, h, fault=None):
    """-> (qg int32, qh int32, (e_g, e_h), flag).  A non-finite entry sets the flag and its row is written as 0, 0."""
    g, h = np.asarray(g, np.float32), np.asarray(h, np.float32)
    fin = np.isfinite(g) & np.isfinite(h)
    eg = exponent(np.abs(g[fin]).max() if fin.any() else 0.0, fault)
    eh = exponent(np.abs(h[fin]).max() if fin.any() else 0.0, fault)
    qg = np.where(fin, np.rint(np.ldexp(np.where(fin, g, 0).astype(np.float64), eg)), 0).astype(np.int64)
    qh = np.where(fin, np.rint(np.ldexp(np.where(fin, h, 0).astype(np.float64), eh)), 0).astype(np.int64)
    return qg.astype(np.int32), qh.astype(np.int32), (eg, eh), int(not fin.all())


# ---- histograms
def histogram(bins, qg, qh, rows, max_bin, hist=None):
    """hist [F, max_bin, 3] int64 += (sum qg, sum qh, count) of the rows; rows None: all."""
    nf = bins.shape[1]
    hist = np.zeros((nf, max_bin, 3), np.int64) if hist is None else hist
    rows = np.arange(bins.shape[0]) if rows is None else np.asarray(rows, np.int64)
    if rows.size == 0:
        return hist
    cell = ((np.arange(nf, dtype=np.int64) * max_bin)[None, :] + bins[rows, :nf].astype(np.int64)).reshape(-1)      # (feature, bin) of every entry
    flat = hist.reshape(nf * max_bin, 3)
    np.add.at(flat[:, 0], cell, np.repeat(qg[rows].astype(np.int64), nf))
    np.add.at(flat[:, 1], cell, np.repeat(qh[rows].astype(np.int64), nf))
    np.add.at(flat[:, 2], cell, 1)
    return hist


# ---- the split scan
def gains(hist, nbins, expo, l2, min_data, min_hess, min_gain, fault=None):
    """gain [F, max_bin] float64 of every candidate (feature, bin), -inf where it is not valid, with the prefix sums [F, max_bin, 3].
    The kernel's order of operations: gain = ((GL GL) / (HL + l2) + (GR GR) / (HR + l2)) - (G G) / (H + l2)."""
    hist = np.asarray(hist, np.int64)
    nf, mb, _ = hist.shape
    pre = np.cumsum(hist, axis=1)
    tot = pre[0, -1]
    G, H = np.ldexp(np.float64(tot[0]), -expo[0]), np.ldexp(np.float64(tot[1]), -expo[1])
    GL, HL = np.ldexp(pre[:, :, 0].astype(np.float64), -expo[0]), np.ldexp(pre[:, :, 1].astype(np.float64), -expo[1])
    GR = np.ldexp((tot[0] - pre[:, :, 0]).astype(np.float64), -expo[0])
    HR = np.ldexp((tot[1] - pre[:, :, 1]).astype(np.float64), -expo[1])
    CL, CR = pre[:, :, 2], tot[2] - pre[:, :, 2]
    floor_h = max(min_hess, 2.0 ** -40)
    ok = (np.arange(mb)[None, :] < (np.asarray(nbins)[:, None] - 1))
    ok &= (CL > min_data) & (CR > min_data) if fault == "min_data" else (CL >= min_data) & (CR >= min_data)
    ok &= (HL >= floor_h) & (HR >= floor_h)
    with np.errstate(all="ignore"):
        gain = ((GL * GL) / (HL + l2) + (GR * GR) / (HR + l2)) - (G * G) / (H + l2)
    ok &= gain >= min_gain
    return np.where(ok, gain, -np.inf), pre, tot


def best_split(hist, nbins, expo, l2=0.0, min_data=1, min_hess=1e-3, min_gain=0.0, fault=None):
    """-> dict(gain, feature, bin, left (g, h, count), right (g, h, count), runner_up): the highest gain, ties to the lowest feature, then
    the lowest bin; runner_up: the best gain among the candidates with other left sums (-inf when there is none)."""
    gain, pre, tot = gains(hist, nbins, expo, l2, min_data, min_hess, min_gain, fault)
    best = gain.max() if gain.size else -np.inf
    if not best > -np.inf:
        return {"gain": -np.inf, "feature": -1, "bin": -1, "left": (0, 0, 0), "right": (0, 0, 0), "runner_up": -np.inf}
    fs, bs = np.nonzero(gain == best)
    k = int(np.argmax(fs)) if fault == "tie" else 0              # np.nonzero is row-major: entry 0 is the lowest feature, then the lowest bin
    f, b = int(fs[k]), int(bs[k])
    # the runner-up is sought among the candidates with OTHER integer left sums: a candidate with the winner's sums (an empty bin next to it, a
    # twin column) has its gain computed from the same inputs by the same operations, bit-equal here and on the device, and the tie rule decides.
    # The same holds for the complementary partition (left and right sums exchanged): the two quotients are the same and a + b == b + a.
    same = (pre == pre[f, b]).all(axis=-1) | (pre == (tot - pre[f, b])).all(axis=-1)
    rest = np.where(same, -np.inf, gain)
    left = tuple(int(v) for v in pre[f, b])
    return {"gain": float(best), "feature": f, "bin": b, "left": left, "right": tuple(int(t) - v for t, v in zip(tot, left)),
            "runner_up": float(rest.max())}


def record(split):
    """The 9 int64 of the device's split record."""
    return np.array([np.float64(split["gain"]).view(np.int64), split["feature"], split["bin"], *split["left"], *split["right"]], np.int64)


def margin(split):
    """Relative distance of the best gain from the runner-up (inf when there is no runner-up or no split)."""
    if not split["gain"] > -np.inf or not split["runner_up"] > -np.inf:
        return np.inf
    return abs(split["gain"] - split["runner_up"]) / max(abs(split["gain"]), 1e-300)


# ---- partition, leaf values
def partition(bins, rows, feature, b, fault=None):
    """-> (left rows in their order, then right rows in theirs; left count)."""
    rows = np.asarray(rows, np.int32)
    left = bins[rows, feature] <= b
    lrows = rows[left][::-1] if fault == "unstable" else rows[left]
    return np.concatenate([lrows, rows[~left]]).astype(np.int32), int(left.sum())


def leaf_value(g_sum, h_sum, expo, l2, lr):
    G, H = np.ldexp(np.float64(g_sum), -expo[0]), np.ldexp(np.float64(h_sum), -expo[1])
    return np.float32(-G / (H + l2) * lr) if H + l2 > 0.0 else np.float32(0.0)


# ---- leaf-wise growth
def grow_tree(bins, qg, qh, expo, edges, nbins, max_bin, num_leaves, lr=0.1, l2=0.0, min_data=1, min_hess=1e-3, min_gain=0.0, max_depth=-1,
              fault=None):
    """One tree: split the leaf with the largest gain (ties: the older leaf) until num_leaves or no valid split.  The left child keeps its
    parent's leaf number, the right child gets the next one; node k is the k-th split.  As in GBDT.update, only the child with fewer rows
    (ties: the left one) has its histogram summed from its rows; its sibling's is the parent's minus that one.
    fault: "newest_leaf" splits the newest leaf, not the best one; "no_l2" leaves lambda_l2 out of the leaf values; "larger_hist" takes the
    larger child's histogram as the smaller's (the two exchanged).
    -> (tree dict of feature / threshold / left / right / value, the leaves' row lists, the smallest margin of any search)."""
    n = bins.shape[0]
    none = {"gain": -np.inf, "runner_up": -np.inf}

    def splittable(count, depth):
        return count >= 2 * max(min_data, 1) and not (max_depth > 0 and depth >= max_depth)

    def search(hist):
        return best_split(hist, nbins, expo, l2, min_data, min_hess, min_gain)

    all_rows = np.arange(n, dtype=np.int32)
    tot = (int(qg.astype(np.int64).sum()), int(qh.astype(np.int64).sum()))
    root_hist = histogram(bins, qg, qh, all_rows, max_bin)
    leaves = [{"rows": all_rows, "depth": 0, "parent": -1, "side": 0, "sums": tot, "hist": root_hist,
               "split": search(root_hist) if splittable(n, 0) else none}]
    worst = margin(leaves[0]["split"])
    feature, threshold, left, right = [], [], [], []
    while len(leaves) < num_leaves:
        li = len(leaves) - 1 if fault == "newest_leaf" else max(range(len(leaves)), key=lambda i: (leaves[i]["split"]["gain"], -i))
        leaf = leaves[li]
        s = leaf["split"]
        if not s["gain"] > -np.inf:
            break
        out, cl = partition(bins, leaf["rows"], s["feature"], s["bin"])
        assert cl == s["left"][2] or fault == "larger_hist"
        node = len(feature)
        feature.append(s["feature"]); threshold.append(edges[s["feature"], s["bin"]]); left.append(~li); right.append(~len(leaves))
        if leaf["parent"] >= 0:
            (left if leaf["side"] == 0 else right)[leaf["parent"]] = node
        kids = [{"rows": rows, "depth": leaf["depth"] + 1, "parent": node, "side": side, "sums": sums[:2], "hist": None, "split": none}
                for side, rows, sums in ((0, out[:cl], s["left"]), (1, out[cl:], s["right"]))]
        can = [splittable(c["rows"].size, c["depth"]) for c in kids]
        if len(leaves) + 1 < num_leaves and any(can):
            small, large = (kids[0], kids[1]) if kids[0]["rows"].size <= kids[1]["rows"].size else (kids[1], kids[0])
            small["hist"] = histogram(bins, qg, qh, small["rows"], max_bin)
            large["hist"] = leaf["hist"] - small["hist"]
            if fault == "larger_hist":
                small["hist"], large["hist"] = large["hist"], small["hist"]
            for c, ok in zip(kids, can):
                if ok:
                    c["split"] = search(c["hist"])
                    worst = min(worst, margin(c["split"]))
        leaf["hist"] = None
        leaves[li] = kids[0]
        leaves.append(kids[1])
    value = np.array([leaf_value(c["sums"][0], c["sums"][1], expo, 0.0 if fault == "no_l2" else l2, lr) for c in leaves], np.float32)
    tree = {"feature": np.array(feature, np.int32), "threshold": np.array(threshold, np.float32), "left": np.array(left, np.int32),
            "right": np.array(right, np.int32), "value": value}
    return tree, [c["rows"] for c in leaves], worst


def add_leaf_values(scores, leaf_rows, value):
    for rows, v in zip(leaf_rows, value):
        scores[rows] = scores[rows] + np.float32(v)
    return scores


def predict(X, trees):
    """fp32 sum of the leaf values in tree order; left on x <= threshold."""
    X = np.asarray(X, np.float32)
    out = np.zeros(X.shape[0], np.float32)
    for i in range(X.shape[0]):
        s = np.float32(0.0)
        for t in trees:
            node = 0 if t["feature"].size else ~0
            while node >= 0:
                node = t["left"][node] if X[i, t["feature"][node]] <= t["threshold"][node] else t["right"][node]
            s = np.float32(s + t["value"][~node])
        out[i] = s
    return out


def exact_greedy_root(X, g, h, l2=0.0, min_data=1, min_hess=1e-3, min_gain=0.0):
    """Brute force over raw thresholds (every distinct value but the largest of every feature), float64 sums of g and h in row order:
    -> (gain, feature, threshold value, left mask)."""
    X, g, h = np.asarray(X, np.float64), np.asarray(g, np.float64), np.asarray(h, np.float64)
    G, H = g.sum(), h.sum()
    best = (-np.inf, -1, None, None)
    for f in range(X.shape[1]):
        for v in np.unique(X[:, f])[:-1]:
            m = X[:, f] <= v
            GL, HL, GR, HR = g[m].sum(), h[m].sum(), g[~m].sum(), h[~m].sum()
            if m.sum() < min_data or (~m).sum() < min_data or HL < max(min_hess, 2.0 ** -40) or HR < max(min_hess, 2.0 ** -40):
                continue
            gain = GL * GL / (HL + l2) + GR * GR / (HR + l2) - G * G / (H + l2)
            if gain >= min_gain and gain > best[0]:
                best = (gain, f, v, m)
    return best
