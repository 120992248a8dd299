"""mirror_amd — MI355X-native (gfx950) implementation of the MIRROR pre-training hot path.

Host side mirrors the reference's Python surface (`models.mirror`, `losses.MIRRORLoss`,
`losses.InfoNCE`; the survival losses and metric of train_survival.py in `losses` and `survival`, with the Cox
partial-likelihood loss and the log-rank test beside them; the subtyping losses
and metrics of train_subtyping.py in `losses` and `metrics`; the zero-shot retrieval metrics and top-k
neighbours of the alignment heads in `retrieval`; the kNN probe of frozen embeddings in `knn`, the few-shot prototype probe in
`fewshot`, the label-free cluster probe (k-means scored with NMI, ARI and purity) in `cluster`, the cross-validated linear
probe (softmax regression over folds and L2 strengths) in `linprobe` and its survival counterpart (hazard regression scored with the
censored concordance index) in `survprobe`, with the cross-validated ridge Cox probe on the follow-up time itself in `coxprobe`;
the upstream choice of transcripts, cross-validated recursive gene elimination (RFECV over squared-hinge machines), in `geneselect`);
all arithmetic runs in hand-written HIP kernels behind the C ABI of `include/mirror_hip.h` (`mirror_amd/lib/libmirror_hip.so`).  There is no CPU fallback.
"""
from ._lib import MirrorHipError, LIB_PATH  # noqa: F401

__version__ = "0.1.0"

__all__ = ["MirrorHipError", "LIB_PATH", "FewShotProbe", "ClusterProbe", "LinearProbe", "SurvivalProbe", "CoxProbe", "GeneSelect", "install_aliases"]


def __getattr__(name: str):
    # `mirror_amd.FewShotProbe` / `from mirror_amd import FewShotProbe`: resolved on first use, so importing the package stays free of torch
    if name == "FewShotProbe":
        from .fewshot import FewShotProbe
        return FewShotProbe
    if name == "ClusterProbe":
        from .cluster import ClusterProbe
        return ClusterProbe
    if name == "LinearProbe":
        from .linprobe import LinearProbe
        return LinearProbe
    if name == "SurvivalProbe":
        from .survprobe import SurvivalProbe
        return SurvivalProbe
    if name == "CoxProbe":
        from .coxprobe import CoxProbe
        return CoxProbe
    if name == "GeneSelect":
        from .geneselect import GeneSelect
        return GeneSelect
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def install_aliases() -> None:
    """Make the reference trainers' own imports resolve to this build: `import models`
    (train_mirror.py:43), `from losses import MIRRORLoss` (:889-891), `from losses import InfoNCE`
    (train_pretrain.py:43), `from losses import CrossEntropySurvLoss, NLLSurvLoss` (train_survival.py:47) and the sub-module paths
    `models.mirror`, `losses.mirror_loss`, `losses.info_nce`, `losses.nll_surv`, `losses.cross_entropy_surv`;
    `from losses import CoxSurvLoss` and `losses.cox_surv` resolve too.
    Call it before the trainer's imports run (sitecustomize.py or the first lines of the script)."""
    import importlib
    import sys
    from . import losses, models
    # by module path: `models.mirror` the attribute is the registry function (models/__init__.py:1), not the module
    mirror_mod = importlib.import_module(__name__ + ".models.mirror")
    mirror_loss = importlib.import_module(__name__ + ".losses.mirror_loss")
    info_nce = importlib.import_module(__name__ + ".losses.info_nce")
    nll_surv = importlib.import_module(__name__ + ".losses.nll_surv")
    ce_surv = importlib.import_module(__name__ + ".losses.cross_entropy_surv")
    cox_surv = importlib.import_module(__name__ + ".losses.cox_surv")
    sys.modules["models"] = models
    sys.modules["models.mirror"] = mirror_mod
    sys.modules["losses"] = losses
    sys.modules["losses.mirror_loss"] = mirror_loss
    sys.modules["losses.info_nce"] = info_nce
    sys.modules["losses.nll_surv"] = nll_surv
    sys.modules["losses.cross_entropy_surv"] = ce_surv
    sys.modules["losses.cox_surv"] = cox_surv
