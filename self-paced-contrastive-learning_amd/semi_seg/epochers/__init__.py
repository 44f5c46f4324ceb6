from .pretrain import PretrainDecoderEpocher, PretrainEncoderEpocher, unzip_twice_transformed  # noqa: F401
from .finetune import EvalEpocher, FineTuneEpocher, InferenceEpocher  # noqa: F401
from .legacy import ContrastiveProjectorWrapper, InfoNCEPretrainEpocher  # noqa: F401
from .semi import SemiSupervisedEpocher  # noqa: F401
from .adversarial import AdversarialEpocher  # noqa: F401
from .monitor import EmbeddingMonitor, parse_monitor  # noqa: F401
from .dense_monitor import DenseEmbeddingMonitor, parse_dense_monitor  # noqa: F401
