"""CPU: the float64 restatement of the position-debiased lambdarank against lambdarank_ndcg_ref, its cost symmetry, the eager fp32 form
under the gate (its needed constant printed), and what the C ABI and the Python surface refuse before any launch."""
import ctypes

import numpy as np
import pytest

import f64_loss_bounds as FB
import lambdarank_ndcg_ref as LR
import lambdarank_unbiased_ref as UR
import tree_ref as TR

GROUP = [1, 2, 17, 40, 70, 3]
S, Y = TR.tree_inputs(GROUP, seed=9)
CONFIGS = [(T, norm) for T in (2, 30, 5000) for norm in (True, False)]


@pytest.mark.parametrize("T,norm", CONFIGS)
def test_unit_biases_restate_lambdarank_ndcg_and_the_two_costs_sum_alike(T, norm):
    mine, theirs = UR.batch(S, Y, GROUP, [(None, 7, None)], T=T, norm=norm, sigma=2.0)[0], LR.batch(S, Y, GROUP, T=T, norm=norm, sigma=2.0)
    for k in ("grad", "hess"):
        assert np.allclose(mine[k], theirs[k], rtol=1e-12, atol=1e-300) and (mine["E_" + k] >= theirs["E_" + k]).all(), k
    assert np.abs(mine["grad"]).max() > 0 and mine["cost"][0].sum() > 0
    assert abs(mine["cost"][0].sum() - mine["cost"][1].sum()) <= 1e-12 * mine["cost"][0].sum()     # every pair: once as hi, once as lo


@pytest.mark.parametrize("T,norm", CONFIGS)
@pytest.mark.parametrize("given,P", [(False, 3), (True, 30), (True, 256)])
def test_the_eager_fp32_form_passes_the_gate(T, norm, given, P):
    pos, t = UR.given_positions(GROUP) if given else None, UR.draw_biases(P)
    ref = UR.batch(S, Y, GROUP, [(pos, P, t)], T=T, norm=norm, sigma=1.0)[0]
    grad, hess, cost, off = np.zeros(S.size), np.zeros(S.size), np.zeros((2, P)), TR.offsets_of(GROUP)
    for a, e in zip(off[:-1], off[1:]):
        g, h, c = UR.eager_query(S[a:e], Y[a:e], None if pos is None else pos[a:e], P, t, T, 1.0, norm)
        grad[a:e], hess[a:e], cost = g, h, cost + c
    w = max(TR.gate(grad, hess, ref, "eager", UR.C), FB.gate_nan(cost, ref["cost"], ref["E_cost"], "eager costs", UR.C))
    print(f"eager fp32: worst err/E {w:.3f}: needs C_PAIR >= {w * UR.C:.2f}")
    assert not np.array_equal(grad, LR.eager_batch(S, Y, GROUP, T=T, norm=norm, sigma=1.0)[0])        # the biases reach the result


def test_update_rule_and_settings():
    cost = np.array([[4.0, 1.0, 0.0, 1e-9], [0.0, 3.0, 2.0, 1.0]])
    out = UR.update(cost, np.full((2, 4), 0.7), 1.0)
    assert np.allclose(out[0], [1.0, 0.5, 0.7, UR.FLOOR]) and (out[1] == 0.7).all()
    import ptranking_amd.functional as F
    from ptranking_amd import gbdt, tree
    assert F.position_bias_settings(0, None, 5000) == (0.0, 256) and F.position_bias_settings(0.5, 3) == (0.5, 3)
    for bad in (dict(bias_p_norm=-1.0), dict(bias_p_norm=float("nan")), dict(bias_positions=0), dict(bias_positions=257), dict(bias_positions=True)):
        with pytest.raises(ValueError):
            F.position_bias_settings(**bad)
    with pytest.raises(ValueError, match="negative"):
        tree.positions_of([0, -1, 2], 3)
    with pytest.raises(ValueError, match="documents"):
        tree.positions_of([0, 1], 3)
    assert tree.positions_of([2.0, 0.0], 2).dtype == np.int32 and gbdt._params({})["lambdarank_unbiased"] is False
    with pytest.raises(ValueError):
        gbdt._params({"lambdarank_unbiased": 1})
    assert set(gbdt.UNBIASED_KEYS) <= set(gbdt.DEFAULT_PARAMS)


def test_argument_errors_come_before_any_launch():
    from ptranking_amd import _lib
    from launch_form import launch_form
    lib, one, f = _lib.load(), ctypes.c_void_p(4096), ctypes.c_float
    call = lambda npos=3, acc=one: lib.ptr_tree_lambdarank_unbiased_grad_hess(one, one, None, one, 1, None, 1, 8, 30, f(1.0), 1, None, npos, acc, one, one, None)
    upd = lambda npos=3, acc=one, pn=0.5, t=one: lib.ptr_tree_position_bias_update(acc, npos, ctypes.c_double(pn), t, None, None)
    for fn, kw, word in ((call, dict(npos=0), b"npos"), (call, dict(npos=257), b"npos"), (call, dict(acc=None), b"cost_acc"),
                         (upd, dict(npos=300), b"npos"), (upd, dict(acc=None), b"cost_acc"), (upd, dict(pn=-0.1), b"p_norm"),
                         (upd, dict(pn=float("nan")), b"p_norm"), (upd, dict(t=None), b"biases")):
        assert fn(**kw) == 1001 and word in lib.ptr_last_error(), kw
    assert launch_form("ptr_tree_lambdarank_unbiased_grad_hess", 16)[:2] == (16, 16) and launch_form("ptr_tree_lambdarank_unbiased_grad_hess", 129)[0] == 256
