"""ptranking_amd — MI355X-native (gfx950 / CDNA4) implementation of wildltr/ptranking's ltr_adhoc loss + metric hot path.

    functional  fused HIP losses (autograd Functions) and device metrics on [B, L] tensors
    rankers     RankNet / LambdaRank / LambdaLoss / ApproxNDCG / ListNet / ListMLE / ... / WassRank with the reference's plugin surface
    host        LABEL_TYPE, DeviceEvaluator, DeviceTrainLoop, the stand-alone pointsf base ranker
    scorer      the pointsf MLP scorer on fused fp32-MFMA kernels (FusedPointScorer) + FlatAdam
    batching    PaddedQueryBatches: device-resident padded query batches (+ lens) replacing the reference's loader stack
    diversity   the diversification frame: DALETOR (alpha-DCG loss kernel), DivProbRanker (Gaussian pairwise-rank loss kernel),
                alpha-nDCG / ERR-IA / nERR-IA on the device, DivQueryBatches
    tree        the tree frame's custom LightGBM objectives (RankNet / LambdaRank / ListNet gradient + Hessian over ragged groups):
                TreeObjective, the six drop-in functions, install_tree(): the hook for a LightGBM booster
    gbdt        a native LambdaMART: GBDT (a histogram gradient-boosted tree trainer on the device, leaf-wise growth on fixed-point
                integer histograms) and LambdaMART (the tree objectives above + GBDT, scores and gradients never leave the device)
    adversarial the adversarial frame's IRGAN point and pair machines (IRGAN_Point, IRGAN_Pair): device sampling of the documents both
                players train on and the two players' fused losses; install_adversarial() rebinds them in the reference's driver module;
                IRFGAN_Point, IRFGAN_Pair (EXTRA_AD_RANKER_NAMES, install_adversarial(extras=True)): the same players under eight
                f-divergences, the pair machine's n x n Bernoulli sampler recomputed on the device and never stored;
                IRGAN_List, IRFGAN_List (LIST_AD_RANKER_NAMES, install_adversarial_list()): the players on whole rankings — one launch
                samples the standard and the generated rankings, one fused launch per player gives the ranking-probability loss
    dp          data-parallel gradient exchange (one RCCL all-reduce per step)
    install()   rebinds the ranker names of RANKER_NAMES (RankNet, LambdaRank, LambdaLoss, ApproxNDCG, ListNet, ListMLE, STListNet,
                RankCosine, RankMSE, SoftRank, WassRank) inside an installed ptranking so LTREvaluator uses them unchanged; a WassRank
                configured with mode='EntropicOT' (or smooth_type='NG') now raises NotImplementedError instead of running the reference's
                torch code; install(names=RANKER_NAMES + METRIC_RANKER_NAMES) adds SmoothMetric (P / AP / nERR / nDCG on smooth ranks as the
                training objective), which the reference has no class for; install(names=RANKER_NAMES + PROB_RANKER_NAMES) adds
                ProbSmoothMetric (the same four objectives on Gaussian expected ranks, a mean and a variance per document)

The only compute implementation is the HIP library ptranking_amd/libptranking_amd.so (C ABI: include/ptranking_amd.h);
there is no CPU fallback.  Build it with `python -m ptranking_amd.build`.
"""
from . import _lib, adversarial, batching, diversity, dp, functional, gbdt, host, rankers, scorer, tree   # noqa: F401
from .gbdt import GBDT, LambdaMART                  # noqa: F401
from .batching import PaddedQueryBatches            # noqa: F401
from . import letor                                   # noqa: F401
from .host import LABEL_TYPE, DeviceEvaluator       # noqa: F401
from .install import install, install_adversarial, install_adversarial_list, install_diversification, install_tree, uninstall   # noqa: F401
from .adversarial import (AD_RANKER_NAMES, EXTRA_AD_RANKER_NAMES, LIST_AD_RANKER_NAMES, IRFGAN_List, IRFGAN_Pair, IRFGAN_Point, IRGAN_List,   # noqa: F401
                          IRGAN_Pair, IRGAN_Point)
from .tree import TreeObjective                     # noqa: F401
from .diversity import DALETOR, DIV_RANKER_NAMES, EXTRA_DIV_RANKER_NAMES, DivProbRanker, DivQueryBatches     # noqa: F401
from .rankers import (ApproxNDCG, LambdaLoss, LambdaRank, ListMLE, ListNet, RankNet, STListNet, RankCosine, RankMSE, SoftRank, WassRank, DASALC, MDPRank,  # noqa: F401
                      SmoothMetric, ProbSmoothMetric, DEFAULT_PARAS, EXTRA_RANKER_NAMES, METRIC_RANKER_NAMES, PROB_RANKER_NAMES, RANKER_NAMES,
                      make_ranker_classes)

__version__ = "0.1.0"
