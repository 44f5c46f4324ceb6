from .infonce import INFONCEHook, SelfPacedINFONCEHook, PScheduler, get_n_point_coordinate  # noqa: F401
from .creator import create_infonce_hooks, create_sp_infonce_hooks, feature_until_from_hooks  # noqa: F401
from .creator import (create_consistency_hook, create_cross_pseudo_hook, create_discrete_mi_consistency_hook,  # noqa: F401
                      create_discrete_mi_hooks, create_entropy_min_hook, create_mean_teacher_hook,
                      create_iic_estimator_hooks, create_midl_hook, create_mine_hooks, create_pica_consistency_hook, create_pica_hooks,
                      create_pixel_contrast_hook, create_pseudo_label_hook, create_strong_view_hook,
                      create_uc_mean_teacher_hook)
from .consistency import ConsistencyTrainerHook  # noqa: F401
from .cps import CrossPseudoTrainerHook  # noqa: F401
from .discretemi import DiscreteMITrainHook  # noqa: F401
from .entmin import EntropyMinTrainerHook  # noqa: F401
from .iic_estimator import IICEstimatorTrainHook  # noqa: F401
from .midl import MIDLPaperTrainerHook  # noqa: F401
from .mine import MineTrainHook  # noqa: F401
from .mt import MeanTeacherTrainerHook  # noqa: F401
from .pica import PICATrainHook  # noqa: F401
from .pixelcontrast import PixelContrastTrainerHook  # noqa: F401
from .pseudolabel import PseudoLabelTrainerHook  # noqa: F401
from .mixup import MixUpHook  # noqa: F401
from .strongview import StrongViewTrainerHook  # noqa: F401
from .ucmt import UCMeanTeacherTrainerHook  # noqa: F401
