"""Mirror of the factories in ``semi_seg/hooks/creator.py``: ``feature_until_from_hooks`` (:23-29),
``create_infonce_hooks`` (:69-99) and ``create_sp_infonce_hooks`` (:102-124) -- one hook per (feature, weight,
contrast_on) triple combined into one TrainerHook -- and the UDA-IIC factories ``create_consistency_hook`` (:32-33),
``create_discrete_mi_hooks`` (:36-47) and ``create_discrete_mi_consistency_hook`` (:50-66).  ``create_mean_teacher_hook`` and
``create_entropy_min_hook`` have no counterpart there: the reference builds those two baselines in their trainers
(semi_seg/trainers/trainer.py:227-271, from ``EntropyMinParameters`` / ``MeanTeacherParameters``); the hook names are its
trainer-registry keys (semi_seg/trainers/__init__.py:11-12).  ``create_uc_mean_teacher_hook`` likewise stands for
``UCMeanTeacherTrainer`` (trainer.py:274-290, registry key ``ucmeanteacher``) and ``create_midl_hook`` for ``MIDLTrainer``
(trainer.py:39-60, registry key ``midl``) and ``create_mine_hooks`` for ``MineTrainer`` (trainer.py:98-107, registry key
``mine``).  ``create_pica_hooks`` / ``create_pica_consistency_hook`` are the two discrete-MI factories with the PICA criteria
(contrastyou/losses/pica_loss.py; the reference pairs them with the cluster heads in ``PICALossWrapper``,
semi_seg/utils.py:242-263, and has no factory of its own for them).  ``create_pseudo_label_hook`` builds the pseudo-labelling
baseline (FixMatch / FreeMatch thresholds) and ``create_pixel_contrast_hook`` the label-guided pixel contrast on a decoder
feature; ``create_cross_pseudo_hook`` builds cross pseudo supervision with a peer network; ``create_strong_view_hook`` makes the
unlabelled pair's second view a strong intensity view; the reference lacks all four altogether."""
from typing import List, Union

from ...contrastyou.hooks.base import CombineTrainerHook
from ..arch.unet import sort_arch
from .consistency import ConsistencyTrainerHook
from .cps import CrossPseudoTrainerHook
from .discretemi import DiscreteMITrainHook
from .entmin import EntropyMinTrainerHook
from .iic_estimator import IICEstimatorTrainHook
from .infonce import INFONCEHook, SelfPacedINFONCEHook, decoder_names
from .midl import MIDLPaperTrainerHook
from .mine import MineTrainHook
from .mt import MeanTeacherTrainerHook
from .pica import PICATrainHook
from .pixelcontrast import PixelContrastTrainerHook
from .pseudolabel import PseudoLabelTrainerHook
from .strongview import StrongViewTrainerHook
from .ucmt import UCMeanTeacherTrainerHook


def _listify(v, n):
    return list(v) if isinstance(v, (list, tuple)) else [v] * n


def feature_until_from_hooks(*hooks) -> Union[str, None]:
    names = []
    for h in hooks:
        for sub in (h._hooks if isinstance(h, CombineTrainerHook) else [h]):
            if hasattr(sub, "_feature_name"):
                names.append(sub._feature_name)
    return sort_arch(names)[-1] if names else None


def create_infonce_hooks(*, model, feature_names: Union[str, List[str]], weights, contrast_ons, data_name="acdc",
                         **kw):
    feature_names = _listify(feature_names, 1)
    n = len(feature_names)
    hooks = [INFONCEHook(name=f"infonce_{f.lower()}_{c}", model=model, feature_name=f, weight=w, data_name=data_name,
                         contrast_on=c, **kw)
             for f, w, c in zip(feature_names, _listify(weights, n), _listify(contrast_ons, n))]
    return CombineTrainerHook(*hooks)


def create_sp_infonce_hooks(*, model, feature_names: Union[str, List[str]], weights, contrast_ons, begin_values,
                            end_values, mode: str, max_epoch: int, p=0.5, correct_grad=False, data_name="acdc", **kw):
    feature_names = _listify(feature_names, 1)
    n = len(feature_names)
    corr = _listify(correct_grad, n)
    hooks = [SelfPacedINFONCEHook(name=f"spinfonce_{f.lower()}_{c}", model=model, feature_name=f, weight=w,
                                  data_name=data_name, contrast_on=c, mode=mode, p=p, begin_value=b, end_value=e,
                                  correct_grad=cg, max_epoch=max_epoch, **kw)
             for f, w, c, b, e, cg in zip(feature_names, _listify(weights, n), _listify(contrast_ons, n),
                                          _listify(begin_values, n), _listify(end_values, n), corr)]
    return CombineTrainerHook(*hooks)


def ntuple(n):
    """contrastyou/utils/utils.py:176-192: a scalar or a one-element list repeated n times; a list of another length
    raises RuntimeError"""
    from itertools import repeat

    def parse(x):
        if isinstance(x, str):
            return tuple(repeat(x, n))
        if isinstance(x, (list, tuple)):
            x = list(x)
            if len(x) == 1:
                return tuple(repeat(x[0], n))
            if len(x) != n:
                raise RuntimeError(f"inconsistent shape between {x} and {n}")
            return x
        return tuple(repeat(x, n))

    return parse


def create_consistency_hook(weight: float):
    return ConsistencyTrainerHook(name="consistency", weight=weight)


def create_discrete_mi_hooks(*, feature_names: List[str], weights: List[float], paddings: List[int], model):
    assert len(feature_names) == len(weights), (feature_names, weights)
    decoder_features = [f for f in feature_names if f in decoder_names]
    assert len(paddings) == len(decoder_features), (decoder_features, paddings)
    _pad_gen = iter(paddings)
    paddings_ = [next(_pad_gen) if f in decoder_features else None for f in feature_names]
    hooks = [DiscreteMITrainHook(name=f"discreteMI/{f.lower()}", model=model, feature_name=f, weight=w, padding=p)
             for f, w, p in zip(feature_names, weights, paddings_)]
    return CombineTrainerHook(*hooks)


def create_discrete_mi_consistency_hook(*, model, feature_names: Union[str, List[str]],
                                        mi_weights: Union[float, List[float]], dense_paddings: List[int] = None,
                                        consistency_weight: float):
    n_features = 1 if isinstance(feature_names, str) else len(feature_names)
    pair_generator = ntuple(n_features)
    feature_names = pair_generator(feature_names)
    mi_weights = pair_generator(mi_weights)
    n_dense_features = len([f for f in feature_names if f in decoder_names])
    dense_paddings = ntuple(n_dense_features)(dense_paddings)
    discrete_mi_hook = create_discrete_mi_hooks(feature_names=feature_names, weights=mi_weights, paddings=dense_paddings,
                                                model=model)
    consistency_hook = create_consistency_hook(weight=consistency_weight)
    return CombineTrainerHook(discrete_mi_hook, consistency_hook)


def create_pica_hooks(*, feature_names: List[str], weights: List[float], paddings: List[int], model, lamda: float = 2.0):
    """``create_discrete_mi_hooks`` with the PICA criteria: one hook ``pica/<feature>`` per feature, ``paddings`` for the
    decoder features in their order"""
    assert len(feature_names) == len(weights), (feature_names, weights)
    decoder_features = [f for f in feature_names if f in decoder_names]
    assert len(paddings) == len(decoder_features), (decoder_features, paddings)
    _pad_gen = iter(paddings)
    paddings_ = [next(_pad_gen) if f in decoder_features else None for f in feature_names]
    hooks = [PICATrainHook(name=f"pica/{f.lower()}", model=model, feature_name=f, weight=w, padding=p, lamda=lamda)
             for f, w, p in zip(feature_names, weights, paddings_)]
    return CombineTrainerHook(*hooks)


def create_pica_consistency_hook(*, model, feature_names: Union[str, List[str]], pica_weights: Union[float, List[float]],
                                 dense_paddings: List[int] = None, consistency_weight: float, lamda: float = 2.0):
    """``PICAConsistencyParams``: ``create_discrete_mi_consistency_hook`` with the PICA criteria (and their ``lamda``)"""
    n_features = 1 if isinstance(feature_names, str) else len(feature_names)
    pair_generator = ntuple(n_features)
    feature_names = pair_generator(feature_names)
    pica_weights = pair_generator(pica_weights)
    n_dense_features = len([f for f in feature_names if f in decoder_names])
    dense_paddings = ntuple(n_dense_features)(dense_paddings)
    pica_hook = create_pica_hooks(feature_names=feature_names, weights=pica_weights, paddings=dense_paddings, model=model,
                                  lamda=lamda)
    return CombineTrainerHook(pica_hook, create_consistency_hook(weight=consistency_weight))


def create_mean_teacher_hook(*, model, weight: float, alpha: float = 0.999, weight_decay: float = 1e-5, name: str = "mse"):
    """``MeanTeacherParameters`` of config/specific/mt.yaml: ``name`` is the teacher criterion (only ``mse`` is mirrored)"""
    if name != "mse":
        raise NotImplementedError(f"mean teacher criterion {name!r}: only 'mse' is mirrored")
    return MeanTeacherTrainerHook(name="meanteacher", weight=weight, model=model, alpha=alpha, weight_decay=weight_decay)


def create_uc_mean_teacher_hook(*, model, weight: float, max_epoch: int, alpha: float = 0.999, weight_decay: float = 1e-5,
                                name: str = "mse", **uc):
    """``UCMeanTeacherParameters``: the keys of ``MeanTeacherParameters`` plus the hook's own (``num_samples``, ``noise_std``,
    ``threshold``, ``cumulative_noise``); ``name`` is the teacher criterion (only ``mse`` is mirrored)"""
    if name != "mse":
        raise NotImplementedError(f"uncertainty-aware mean teacher criterion {name!r}: only 'mse' is mirrored")
    return UCMeanTeacherTrainerHook(name="ucmeanteacher", weight=weight, model=model, max_epoch=max_epoch, alpha=alpha,
                                    weight_decay=weight_decay, **uc)


def create_pseudo_label_hook(*, model, weight: float, threshold=0.95, adaptive: bool = False, momentum: float = 0.999,
                             teacher: str = "self", alpha: float = 0.999, weight_decay: float = 1e-5):
    """``PseudoLabelParameters``: confidence-thresholded self-training on the unlabelled batch (semi_seg/hooks/pseudolabel.py);
    ``alpha`` and ``weight_decay`` are the mean teacher's and matter with ``teacher="ema"`` only"""
    return PseudoLabelTrainerHook(name="pseudolabel", weight=weight, model=model, threshold=threshold, adaptive=adaptive,
                                  momentum=momentum, teacher=teacher, alpha=alpha, weight_decay=weight_decay)


def create_pixel_contrast_hook(*, model, weight: float, feature_name: str = "Up_conv3", samples_per_class: int = 256,
                               temperature: float = 0.1, hidden_dim: int = 128, output_dim: int = 64, head_type: str = "mlp",
                               unlabeled_threshold=None, seed: int = 0):
    """``PixelContrastParameters``: a class-balanced sample of the hooked feature's cells, chosen on the device by the label
    maps, under a supervised-contrastive criterion (semi_seg/hooks/pixelcontrast.py)"""
    return PixelContrastTrainerHook(name="pixelcontrast", model=model, feature_name=feature_name, weight=weight,
                                    samples_per_class=samples_per_class, temperature=temperature, hidden_dim=hidden_dim,
                                    output_dim=output_dim, head_type=head_type, unlabeled_threshold=unlabeled_threshold,
                                    seed=seed)


def create_cross_pseudo_hook(*, model, weight: float, threshold=0.0, peer_seed: int = 1,
                             on=("labeled", "unlabeled", "unlabeled_tf"), cutmix=None):
    """``CrossPseudoParameters``: cross pseudo supervision with a peer network of the model's class, initialised under
    ``peer_seed`` (semi_seg/hooks/cps.py); ``threshold`` 0 is plain CPS, ``on`` names the class maps the cross term covers.
    ``"cutmix"`` in ``on`` adds the CutMix term (``on: [cutmix]`` alone is the official CPS + CutMix); ``cutmix`` = {"prop_range":
    [lo, hi], "seed": s} sets its box-area range and first seed word (defaults [0.25, 0.5] and 0)"""
    return CrossPseudoTrainerHook(name="cps", weight=weight, model=model, threshold=threshold, peer_seed=peer_seed, on=on,
                                  cutmix=cutmix)


def create_strong_view_hook(*, seed: int = 0, **ops):
    """``StrongViewParameters``: the unlabelled pair's second view becomes a strong intensity view (semi_seg/hooks/strongview.py).
    ``seed`` is the first seed word; ``gamma``, ``contrast``, ``brightness``, ``blur`` and ``noise`` are sections ``{p, range:
    [lo, hi]}`` (defaults: functional.STRONG_VIEW_DEFAULTS); any other key is refused by name.  The hook adds no loss."""
    return StrongViewTrainerHook(name="strongview", seed=seed, **ops)


def create_entropy_min_hook(*, weight: float):
    return EntropyMinTrainerHook(name="entropy", weight=weight)


def create_midl_hook(*, consistency_weight: float, iic_weight: float = 0.1, padding: int = 1, patch_size: int = 1024,
                     name: str = "mse"):
    """``MIDLPaperParameters``: the keys of config/specific/midl.yaml plus ``consistency_weight`` and ``name``, which the
    reference's ``MIDLTrainer`` reads from ``UDARegCriterion`` (``weight`` and ``name``: trainer.py:24-26,42); ``name`` is the
    consistency criterion (only ``mse`` is mirrored).  The sum is comparable.py:224: ``uda_loss * consistency_weight +
    iic_loss * iic_weight``."""
    if name != "mse":
        raise NotImplementedError(f"MIDL consistency criterion {name!r}: only 'mse' is mirrored")
    return CombineTrainerHook(ConsistencyTrainerHook(name="consistency", weight=consistency_weight),
                              MIDLPaperTrainerHook(name="midl", weight=iic_weight, padding=padding, patch_size=patch_size))


def create_mine_hooks(*, model, feature_names: Union[str, List[str]], weights: Union[float, List[float]]):
    """``MineParameters``: one MINE hook ``mine/<feature>`` per feature, each with a statistics network of its own
    (mineestimator.py:39-50).  The reference multiplies the ``feature_importance``-weighted average of the per-feature losses
    by ``IICRegParameters.weight`` (_mixins.py:93, trainer.py:98-107): ``weights[i] = weight * imp_i / sum(imp)`` is that sum."""
    feature_names = _listify(feature_names, 1)
    weights = ntuple(len(feature_names))(weights)
    hooks = [MineTrainHook(name=f"mine/{f.lower()}", model=model, feature_name=f, weight=w)
             for f, w in zip(feature_names, weights)]
    return CombineTrainerHook(*hooks)


def create_iic_estimator_hooks(*, model, feature_names: Union[str, List[str]], feature_importance=1.0, weight: float,
                               EncoderParams: dict, DecoderParams: dict, LossParams: dict, enforce_matching: bool = False):
    """``IICRegParameters`` (config/specific/iic.yaml, with the ``feature_names`` / ``feature_importance`` the old API read
    from ``FeatureExtractor``): an ``IICEstimatorArray`` built as ``IICTrainer._init`` builds it (trainer.py:64-76) and one
    hook ``iic/<feature>`` per estimator.  The reference multiplies the ``feature_importance``-weighted average of the
    per-feature losses by ``weight`` (_mixins.py:93): hook weights ``weight * imp_i / sum(imp)`` are that sum.
    ``LossParams.paddings`` lists one value per DECODER feature.  ``enforce_matching`` is read and, as in the reference, never
    used."""
    from ..mi_estimator.discrete_mi_estimator import IICEstimatorArray
    feature_names = _listify(feature_names, 1)
    importance = [float(v) for v in ntuple(len(feature_names))(feature_importance)]
    array = IICEstimatorArray()
    array.add_encoder_interface(feature_names=feature_names, model=model, **EncoderParams)
    array.add_decoder_interface(feature_names=feature_names, model=model, **DecoderParams, **LossParams)
    total = sum(importance)
    hooks = [IICEstimatorTrainHook(name=f"iic/{f.lower()}", model=model, feature_name=f, estimator=array[f],
                                   weight=float(weight) * imp / total)
             for f, imp in zip(feature_names, importance)]
    return CombineTrainerHook(*hooks)
