"""Plain-numpy restatement of quantized-gradient training (ptr_gbdt_quantize_low of ptranking_amd/csrc/gbdt.hip, and GBDT.update under
use_quantized_grad of ptranking_amd/gbdt.py); include/ptranking_amd.h states the rules.  Test infrastructure; nothing here is LightGBM's.

    scales      max|g| = fr 2^ex, fr in [0.5, 1): e_g = log2(B / 2) - ex; max|h|: e_h = log2(B) - ex; 0 for a maximum of zero
    rounding    x = g 2^e (exact in fp32); stochastic: q = floor(float64(x) + float64(u)), u = u(2 draw, row) for g and u(2 draw + 1, row)
                for h of gbdt_sample_ref.uniforms under quant_seed; deterministic: q = rint(x)
    growth      tree t draws with draw = t and grows on (qg, qh, expo) by the unquantized restatements; renewed leaves: leaf_value of the
                sums of the 30-bit gbdt_ref.quantize pair over the leaf's rows
"""
import numpy as np

import gbdt_level_ref as LR
import gbdt_ref as R
import gbdt_sample_ref as S


def exponent(mx, top):
    return 0 if mx == 0 else top - int(np.frexp(np.float64(mx))[1])


def quantize_low(g, h, levels, stochastic, seed, draw):
    """-> (qg int32, qh int32, (e_g, e_h), flag), as gbdt_ref.quantize."""
    g, h = np.asarray(g, np.float32), np.asarray(h, np.float32)
    lb = int(levels).bit_length() - 1
    assert 2 <= levels <= 256 and 1 << lb == levels
    fin = np.isfinite(g) & np.isfinite(h)
    expo = (exponent(np.abs(g[fin]).max() if fin.any() else 0.0, lb - 1), exponent(np.abs(h[fin]).max() if fin.any() else 0.0, lb))
    out = []
    for k, (v, e) in enumerate(zip((g, h), expo)):
        x = np.ldexp(np.where(fin, v, np.float32(0.0)).astype(np.float32), e)
        assert x.dtype == np.float32 and (np.ldexp(x.astype(np.float64), -e) == np.where(fin, v, 0.0)).all()       # exact
        if stochastic:
            q = np.floor(x.astype(np.float64) + S.uniforms(seed, 2 * draw + k, np.arange(g.size)).astype(np.float64))
        else:
            q = np.rint(x)
        out.append(np.where(fin, q, 0).astype(np.int32))
    return out[0], out[1], expo, int(not fin.all())


def grow(bins, g, h, edges, nbins, params, t, qid=None):
    """One tree of GBDT.update under the quantization and sampling parameters -> (tree, mask or None, every row's leaf value by the walk)."""
    p = params
    g2, h2, mask = S.tree_mask(p, t, np.asarray(g, np.float32), np.asarray(h, np.float32), qid)
    if p.get("use_quantized_grad", False):
        qg, qh, expo, flag = quantize_low(g2, h2, p.get("num_grad_quant_bins", 4), p.get("stochastic_rounding", True), p.get("quant_seed", 0), t)
    else:
        qg, qh, expo, flag = R.quantize(g2, h2)
    assert flag == 0
    bag = np.arange(bins.shape[0]) if mask is None else np.nonzero(mask)[0]
    grower = LR.grow_tree if p.get("grow_policy", "leafwise") == "depthwise" else R.grow_tree
    out = grower(bins[bag], qg[bag], qh[bag], expo, edges, nbins, p["max_bin"], p["num_leaves"], p.get("learning_rate", 0.1), p.get("lambda_l2", 0.0),
                 p.get("min_data_in_leaf", 20), p.get("min_sum_hessian_in_leaf", 1e-3), p.get("min_gain_to_split", 0.0), p.get("max_depth", -1))
    tree, leaf_rows = out[0], out[1]
    if p.get("use_quantized_grad", False) and p.get("quant_train_renew_leaf", False):
        g30, h30, e30, _ = R.quantize(g2, h2)
        tree["value"] = np.array([R.leaf_value(int(g30[bag[rows]].astype(np.int64).sum()), int(h30[bag[rows]].astype(np.int64).sum()), e30,
                                               p.get("lambda_l2", 0.0), p.get("learning_rate", 0.1)) for rows in leaf_rows], np.float32)
    add = S.walk_binned(bins, tree["feature"], S.split_bins(tree, edges, nbins), tree["left"], tree["right"], tree["value"])
    return tree, mask, add
