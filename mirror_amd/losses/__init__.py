"""Drop-in for the reference's `losses` package (losses/__init__.py:1-12): the pre-training losses (`MIRRORLoss`, `InfoNCE`) and
the downstream survival losses of train_survival.py (`NLLSurvLoss`, `CrossEntropySurvLoss`).

The classification losses of train_subtyping.py (`LabelSmoothingCrossEntropy` for timm's, `CrossEntropyLoss` for nn's) are
exported here too but stay out of `__all__`, which lists the reference package's names: the trainer imports them from timm and
torch, and a user swaps those imports.  `CoxSurvLoss` (the continuous-time Cox partial likelihood, which the
reference package does not have) is exported the same way."""
from .cox_surv import CoxSurvLoss
from .cross_entropy import CrossEntropyLoss
from .cross_entropy_surv import CrossEntropySurvLoss
from .info_nce import InfoNCE
from .label_smoothing import LabelSmoothingCrossEntropy
from .mirror_loss import ClipLoss, MIRRORLoss
from .nll_surv import NLLSurvLoss

__all__ = ["CrossEntropySurvLoss", "InfoNCE", "MIRRORLoss", "NLLSurvLoss"]
