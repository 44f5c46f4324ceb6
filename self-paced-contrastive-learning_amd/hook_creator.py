"""Mirror of the reference's repo-root ``hook_creator.py``: which sections of the merged config turn into TrainerHooks.

Contract (hook_creator.py:10-28): ``InfonceParams`` builds plain InfoNCE hooks, ``SPInfonceParams`` the self-paced ones
(they also get the trainer's ``max_epoch`` for their age-parameter schedule); both receive ``Data.name``.
``DiscreteMIConsistencyParams`` (the UDA-IIC baseline) builds the discrete-MI + consistency hooks
(``create_discrete_mi_consistency_hook``) outside pre-training; during pre-training the reference raises RuntimeError for
it and so does this mirror.  ``MeanTeacherParameters`` (keys of config/specific/mt.yaml) and ``EntropyMinParameters``
(``weight``) build the mean-teacher and entropy-minimisation hooks under the same rule: the reference's
``create_hook_from_config`` notes that pre-training accepts no mean teacher (hook_creator.py:6).
``UCMeanTeacherParameters`` builds the uncertainty-aware mean teacher (``create_uc_mean_teacher_hook``): the keys of
``MeanTeacherParameters`` plus the hook's own (``num_samples``, ``noise_std``, ``cumulative_noise``), and the trainer's
``max_epoch`` for the threshold's ramp.  The reference's hook_creator has no such section -- its old-API
``UCMeanTeacherTrainer`` reads ``MeanTeacherParameters`` (semi_seg/trainers/trainer.py:252,274-279); a section of its own
lets one config hold either baseline.  Refused during pre-training like the other two.
``MIDLPaperParameters`` builds the MIDL baseline (``create_midl_hook``: the consistency hook plus the patch-wise IIC
segmentation criterion): the keys of config/specific/midl.yaml (``iic_weight``, ``padding``, ``patch_size``) plus
``consistency_weight`` and ``name``, which the reference's old-API ``MIDLTrainer`` reads from ``UDARegCriterion``
(semi_seg/trainers/trainer.py:24-26,42) -- a section of its own for the same reason.  Refused during pre-training too.
``MineParameters`` builds the MINE baseline (``create_mine_hooks``: one statistics network per feature): ``feature_names``
and ``weights``, where the reference's old-API ``MineTrainer`` (trainer.py:98-107) reads ``IICRegParameters.weight`` and
``FeatureExtractor.feature_names`` / ``feature_importance`` -- ``weights[i] = weight * imp_i / sum(imp)``.  Refused during
pre-training as well.
``PICAConsistencyParams`` builds the PICA baseline (``create_pica_consistency_hook``: the hooks of
``DiscreteMIConsistencyParams`` with ``PUILoss`` / ``PUISegLoss`` of contrastyou/losses/pica_loss.py as their criteria):
``feature_names``, ``pica_weights``, ``dense_paddings``, ``consistency_weight`` and ``lamda``.  The reference has the two
criteria and pairs them with the cluster heads (``PICALossWrapper``, semi_seg/utils.py:242-263) but has no section for them;
this one follows ``DiscreteMIConsistencyParams`` key for key.  Refused during pre-training like it.
``IICRegParameters`` builds the IIC-estimator baseline (``create_iic_estimator_hooks``: an ``IICEstimatorArray`` over the
encoder and decoder features, one hook per estimator): the keys of config/specific/iic.yaml (``EncoderParams``,
``DecoderParams``, ``LossParams``, ``weight``, ``enforce_matching``) plus ``feature_names`` and ``feature_importance``, which
the reference's old-API ``IICTrainer`` (trainer.py:64-95) reads from ``FeatureExtractor``.  Refused during pre-training.
``PseudoLabelParameters`` builds the pseudo-labelling baseline (``create_pseudo_label_hook``: FixMatch's confidence-thresholded
self-training, optionally with FreeMatch's self-adaptive thresholds): ``weight``, ``threshold``, ``adaptive``, ``momentum``,
``teacher`` and, for ``teacher: ema``, ``alpha`` / ``weight_decay``.  Not in the reference.  Refused during pre-training.
``PixelContrastParameters`` builds the label-guided pixel contrast (``create_pixel_contrast_hook``: a class-balanced sample of
a decoder feature's cells under a supervised-contrastive criterion): ``weight``, ``feature_name``, ``samples_per_class``,
``temperature``, ``hidden_dim``, ``output_dim``, ``head_type``, ``unlabeled_threshold`` and ``seed``.  Not in the reference.
Refused during pre-training (it needs the labelled batch's label maps).
``CrossPseudoParameters`` builds cross pseudo supervision (``create_cross_pseudo_hook``, hook name ``cps``: a peer network of
the model's class, each trained towards the other's arg-max prediction): ``weight``, ``threshold``, ``peer_seed``, ``on`` and
``cutmix`` (``{prop_range, seed}``; with ``"cutmix"`` in ``on`` the hook adds the CutMix term on a box-mixed unlabelled batch).
Not in the reference.  Refused during pre-training (the peer's own objective is the supervised loss).
``StrongViewParameters`` builds the strong intensity view of the unlabelled pair (``create_strong_view_hook``, hook name
``strongview``: the second view is the flip with gamma, contrast, brightness, blur and noise applied on the way): ``seed`` and
one section ``{p, range}`` per op.  It adds no loss; every hook that reads ``unlabeled_tf_logits`` trains on it.  Not in the
reference.  Refused during pre-training (the pre-train epocher has its own augmentation recipe)."""
from .semi_seg import hooks as _hooks

# config section -> (factory in semi_seg.hooks, does the factory take max_epoch?)
_SECTIONS = (
    ("InfonceParams", "create_infonce_hooks", False),
    ("SPInfonceParams", "create_sp_infonce_hooks", True),
)
_BASELINE_SECTION = "DiscreteMIConsistencyParams"
# semi-supervised baselines: section -> (factory, does the factory take the model?, ... the trainer's max_epoch?)
_SEMI_SECTIONS = (
    ("MeanTeacherParameters", "create_mean_teacher_hook", True, False),
    ("EntropyMinParameters", "create_entropy_min_hook", False, False),
    ("UCMeanTeacherParameters", "create_uc_mean_teacher_hook", True, True),
    ("MIDLPaperParameters", "create_midl_hook", False, False),
    ("MineParameters", "create_mine_hooks", True, False),
    ("PICAConsistencyParams", "create_pica_consistency_hook", True, False),
    ("IICRegParameters", "create_iic_estimator_hooks", True, False),
    ("PseudoLabelParameters", "create_pseudo_label_hook", True, False),
    ("PixelContrastParameters", "create_pixel_contrast_hook", True, False),
    ("CrossPseudoParameters", "create_cross_pseudo_hook", True, False),
    ("StrongViewParameters", "create_strong_view_hook", False, False),
)


def create_hook_from_config(model, config, is_pretrain=False):
    common = {"model": model, "data_name": config["Data"]["name"]}
    built = []
    for section, factory, wants_epochs in _SECTIONS:
        params = config.get(section)
        if params is None:
            continue
        extra = {"max_epoch": config["Trainer"]["max_epoch"]} if wants_epochs else {}
        built.append(getattr(_hooks, factory)(**common, **extra, **params))
    if _BASELINE_SECTION in config:
        if is_pretrain:
            raise RuntimeError(f"{_BASELINE_SECTION} are not supported for pretrain stage")
        built.append(_hooks.create_discrete_mi_consistency_hook(model=model, **config[_BASELINE_SECTION]))
    for section, factory, wants_model, wants_epochs in _SEMI_SECTIONS:
        if section in config:
            if is_pretrain:
                raise RuntimeError(f"{section} are not supported for pretrain stage")
            extra = {"model": model} if wants_model else {}
            if wants_epochs:
                extra["max_epoch"] = config["Trainer"]["max_epoch"]
            built.append(getattr(_hooks, factory)(**extra, **config[section]))
    return built
