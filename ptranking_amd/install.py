"""Drop the fused rankers into an installed wildltr/ptranking so that its unchanged pipeline driver picks them up.

`LTREvaluator.load_ranker` instantiates rankers through `globals()[model_id]` of the module
ptranking/ltr_adhoc/eval/ltr.py (:156-178), so rebinding the names of RANKER_NAMES in that module is all a drop-in needs:

    import ptranking_amd
    ptranking_amd.install()          # RankNet, LambdaRank, LambdaLoss, ApproxNDCG, ListNet, ListMLE, STListNet, RankCosine, RankMSE,
                                     # SoftRank, WassRank -> fused HIP versions
    LTREvaluator(cuda=0).run(model_id='LambdaRank', ...)   # the reference's own driver, data layer, config, tapes

The installed classes derive from the reference's own AdhocNeuralRanker (ptranking/base/adhoc_ranker.py:7), i.e. the
scorers (pointsf AND listsf), optimiser config, save/load stay the reference's code; only `custom_loss_function`,
the train loop's host syncs and the Evaluator metric methods are replaced.  `<Model>Parameter` classes are left alone.
WassRank is built by load_ranker with its own calling convention (ltr.py:173-174), which the installed class keeps; a WassRank
configuration with mode='EntropicOT' (or smooth_type='NG') now raises NotImplementedError instead of running the reference's torch code.
"""
import importlib
import sys

from .rankers import EXTRA_RANKER_NAMES, METRIC_RANKER_NAMES, PROB_RANKER_NAMES, RANKER_NAMES, make_ranker_classes

_saved = {}


def install(names=RANKER_NAMES, ltr_module="ptranking.ltr_adhoc.eval.ltr", extras=False):
    """Rebind `names` inside the reference's ltr module; returns {name: installed class}.  extras=True adds the rankers SURVEY.md 2 marks
    out of scope (EXTRA_RANKER_NAMES: DASALC, MDPRank), which the default drop-in leaves alone.  SmoothMetric (METRIC_RANKER_NAMES) has no
    reference class to replace: it is bound only when named, install(names=RANKER_NAMES + METRIC_RANKER_NAMES), and uninstall() removes it; so is
    ProbSmoothMetric (PROB_RANKER_NAMES), install(names=RANKER_NAMES + PROB_RANKER_NAMES)."""
    if extras:
        names = tuple(names) + tuple(n for n in EXTRA_RANKER_NAMES if n not in names)
    mod = importlib.import_module(ltr_module)
    base = importlib.import_module("ptranking.base.adhoc_ranker").AdhocNeuralRanker
    classes = make_ranker_classes(base)
    done = {}
    for n in names:
        if n not in classes:
            raise KeyError(f"{n} is not one of {RANKER_NAMES + EXTRA_RANKER_NAMES + METRIC_RANKER_NAMES + PROB_RANKER_NAMES}")
        _saved.setdefault((ltr_module, n), getattr(mod, n, None))
        setattr(mod, n, classes[n])
        done[n] = classes[n]
    return done


def install_diversification(names=None, ltr_module="ptranking.ltr_diversification.eval.ltr_diversification", extras=False):
    """Rebind DIV_RANKER_NAMES (DALETOR) inside the reference's diversification driver module, which looks its rankers up by name the same
    way (ltr_diversification.py:387-389); returns {name: installed class}.  The installed DALETOR is the stand-alone class of
    ptranking_amd.diversity (pointsf scorer on the fused kernels; sf_id='listsf' raises NotImplementedError).  extras=True adds
    EXTRA_DIV_RANKER_NAMES (DivProbRanker: pointsf, opt_ideal, no cluster / Portfolio; its pairwise objectives are the exact cross entropy,
    not the reference's fp32 arithmetic), which the default drop-in and an explicit `names` leave alone, as install(extras=True) does for
    the ad-hoc rankers.  uninstall() restores."""
    from .diversity import DALETOR, DIV_RANKER_NAMES, EXTRA_DIV_RANKER_NAMES, DivProbRanker
    classes = {"DALETOR": DALETOR}
    names = DIV_RANKER_NAMES if names is None else tuple(names)
    if extras:
        classes["DivProbRanker"] = DivProbRanker
        names = names + tuple(n for n in EXTRA_DIV_RANKER_NAMES if n not in names)
    mod = importlib.import_module(ltr_module)
    done = {}
    for n in names:
        if n not in classes:
            raise KeyError(f"{n} is not one of {DIV_RANKER_NAMES + (EXTRA_DIV_RANKER_NAMES if extras else ())}")
        _saved.setdefault((ltr_module, n), getattr(mod, n, None))
        setattr(mod, n, classes[n])
        done[n] = classes[n]
    return done


def install_adversarial(names=None, ltr_module="ptranking.ltr_adversarial.eval.ltr_adversarial", extras=False):
    """Rebind AD_RANKER_NAMES (IRGAN_Point, IRGAN_Pair) inside the reference's adversarial driver module, which looks its machines up by
    name (ltr_adversarial.py: globals()[model_id]); returns {name: installed class}.  The installed machines are the stand-alone classes of
    ptranking_amd.adversarial: the reference's constructor and method names on PaddedQueryBatches (AdLTREvaluator's own file handling and
    grid search are not replaced).  extras=True adds EXTRA_AD_RANKER_NAMES (IRFGAN_Point, IRFGAN_Pair), which the default leaves alone;
    an explicit `names` may name them too.  The default install() binds none of them.  uninstall() restores."""
    from .adversarial import AD_RANKER_NAMES, EXTRA_AD_RANKER_NAMES, IRFGAN_Pair, IRFGAN_Point, IRGAN_Pair, IRGAN_Point
    classes = {"IRGAN_Point": IRGAN_Point, "IRGAN_Pair": IRGAN_Pair, "IRFGAN_Point": IRFGAN_Point, "IRFGAN_Pair": IRFGAN_Pair}
    names = AD_RANKER_NAMES if names is None else tuple(names)
    if extras:
        names = names + tuple(n for n in EXTRA_AD_RANKER_NAMES if n not in names)
    mod = importlib.import_module(ltr_module)
    done = {}
    for n in names:
        if n not in classes:
            raise KeyError(f"{n} is not one of {AD_RANKER_NAMES + EXTRA_AD_RANKER_NAMES}")
        _saved.setdefault((ltr_module, n), getattr(mod, n, None))
        setattr(mod, n, classes[n])
        done[n] = classes[n]
    return done


def install_adversarial_list(names=None, ltr_module="ptranking.ltr_adversarial.eval.ltr_adversarial"):
    """Rebind LIST_AD_RANKER_NAMES (IRGAN_List, IRFGAN_List) inside the reference's adversarial driver module, as install_adversarial does
    for the point and pair machines (which it leaves alone, as install_adversarial leaves these); returns {name: installed class}.  `names`
    picks a subset.  The default install() binds neither.  uninstall() restores."""
    from .adversarial import LIST_AD_RANKER_NAMES, IRFGAN_List, IRGAN_List
    classes = {"IRGAN_List": IRGAN_List, "IRFGAN_List": IRFGAN_List}
    names = LIST_AD_RANKER_NAMES if names is None else tuple(names)
    mod = importlib.import_module(ltr_module)
    done = {}
    for n in names:
        if n not in classes:
            raise KeyError(f"{n} is not one of {LIST_AD_RANKER_NAMES}")
        _saved.setdefault((ltr_module, n), getattr(mod, n, None))
        setattr(mod, n, classes[n])
        done[n] = classes[n]
    return done


def install_tree(util_module="ptranking.ltr_tree.util.lightgbm_util", user_modules=("ptranking.ltr_tree.lambdamart.lightgbm_lambdaMART",)):
    """Rebind the six custom LightGBM objectives (ptranking_amd.tree.DROP_IN_NAMES: lightgbm_custom_obj_{ranknet,lambdarank,listnet} and
    their *_fobj forms) inside the reference's lightgbm_util module, and inside each of `user_modules` that is ALREADY imported: the
    reference's LightGBMLambdaMART imports the six names by value (lightgbm_lambdaMART.py:14-16), so a binding made there before
    install_tree() would keep the Python loops; a module imported afterwards picks the new names up from lightgbm_util itself.  The
    installed functions return what the reference's return (unweighted 'lambdarank', the rank-signed Hessian; ptranking_amd/tree.py), from
    one fused kernel.  Returns {name: installed function}; uninstall() restores."""
    from . import tree
    done = {n: getattr(tree, n) for n in tree.DROP_IN_NAMES}
    mods = [importlib.import_module(util_module)] + [sys.modules[m] for m in user_modules if m in sys.modules]
    for mod in mods:
        for n, fn in done.items():
            if mod.__name__ != util_module and not hasattr(mod, n):
                continue
            _saved.setdefault((mod.__name__, n), getattr(mod, n, None))
            setattr(mod, n, fn)
    return done


def uninstall(ltr_module=None):
    """Restore the reference's own classes and functions: in `ltr_module`, or (default) in every module install(), install_diversification(),
    install_adversarial(), install_adversarial_list() or install_tree() touched."""
    for m in sorted({m for m, _ in _saved} if ltr_module is None else {ltr_module}):
        _uninstall_module(m)


def _uninstall_module(ltr_module):
    mod = importlib.import_module(ltr_module)
    for (m, n), cls in list(_saved.items()):
        if m != ltr_module:
            continue
        if cls is not None:
            setattr(mod, n, cls)
        elif hasattr(mod, n):          # the name did not exist before install() (e.g. DASALC is never imported by ltr.py)
            delattr(mod, n)
        del _saved[(m, n)]
