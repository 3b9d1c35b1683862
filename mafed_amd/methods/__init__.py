"""CL-method registry of the path (reference: mafed/methods/__init__.py:6-11).

``ewc`` is a different method from MAFED; it is built as the first "next" row.  ``lwf`` has no reference
implementation (only the checkpoint suffix, mafed/utils/eval_utils.py:23): its arithmetic is DESIGN.md section 4h, and it is an
extension of the registry, not one of the reference's entries.  ``AGEM`` has no reference implementation either; it is
exported here and constructed directly -- it is not in the registry yet.  The same holds for ``SI``, ``MAS`` (section 4k), ``PackNet`` (section 4l), ``DER`` (section 4n), ``TaskMerging`` (section 4p) and ``GEM`` (section 4q: A-GEM's parent method, one constraint per finished task).
How ``ER``, ``DER``, ``AGEM``, ``GEM`` and ``FeatureDistillation`` fill their replay memory is their ``memory_selection`` argument (``mafed_amd.selection``, section 4m).
"""
from mafed_amd.methods.agem import AGEM
from mafed_amd.methods.base import CLStrategy, Naive
from mafed_amd.methods.der import DER
from mafed_amd.methods.distillation import FeatureDistillation
from mafed_amd.methods.distillation_loss_weights import DistillationWeights
from mafed_amd.methods.ewc import EWC
from mafed_amd.methods.gem import GEM
from mafed_amd.methods.lwf import LwF
from mafed_amd.methods.mas import MAS
from mafed_amd.methods.memory import HBMReplayBuffer
from mafed_amd.methods.merging import TaskMerging
from mafed_amd.methods.packnet import PackNet
from mafed_amd.methods.replay import ER
from mafed_amd.methods.si import SI


class MethodRegistry(dict):
    """``CLMethod``: the reference's registry, which is what iterating it, ``len`` and ``keys()`` give (its four entries: the names the
    reference's command line and checkpoint layout know) -- plus ``extensions``, methods of this project without a reference entry.  An
    extension is constructed like any other entry, ``CLMethod["lwf"](...)``, and ``"lwf" in CLMethod`` holds; ``names()`` lists both."""

    def __init__(self, reference, extensions):
        super().__init__(reference)
        self.extensions = dict(extensions)

    def __missing__(self, key):
        return self.extensions[key]

    def __contains__(self, key):
        return super().__contains__(key) or key in self.extensions

    def get(self, key, default=None):
        return self[key] if key in self else default

    def names(self):
        return list(self) + list(self.extensions)


CLMethod = MethodRegistry({
    "naive": Naive,
    "ewc": EWC,
    "replay": ER,
    "featdistill": FeatureDistillation,
}, extensions={"lwf": LwF})
