"""Drop-in for the reference's `losses` package (losses/__init__.py:1-12): the pre-training losses (`MIRRORLoss`, `InfoNCE`) and
the downstream survival losses of train_survival.py (`NLLSurvLoss`, `CrossEntropySurvLoss`)."""
from .cross_entropy_surv import CrossEntropySurvLoss
from .info_nce import InfoNCE
from .mirror_loss import ClipLoss, MIRRORLoss
from .nll_surv import NLLSurvLoss

__all__ = ["CrossEntropySurvLoss", "InfoNCE", "MIRRORLoss", "NLLSurvLoss"]
