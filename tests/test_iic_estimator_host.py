"""CPU-only: the IIC estimators' host side -- ``create_hook_from_config`` builds the hooks from ``IICRegParameters`` (refused
during pre-training), the per-feature weights follow the importance rule, the array's interfaces broadcast as ``_nlist`` does,
the state dict has the reference's ``nn.Sequential`` keys, a CPU tensor raises, the reference's import name resolves after
``install()``, and the new C entry points are declared in the header and ``native.py`` at ABI 26 and answer bad arguments
with an error code and a message, without a launch."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("spcl_iic_patch_heads_plan", "spcl_iic_patch_heads_forward", "spcl_iic_patch_heads_backward",
               "spcl_group_l2norm_temp_forward", "spcl_group_l2norm_temp_backward")
PARAMS = {"feature_names": ["Conv5", "Up_conv3", "Up_conv2"], "feature_importance": [1, 2, 5], "weight": 0.1,
          "EncoderParams": {"num_clusters": 20, "num_subheads": 5, "head_types": "linear", "normalize": False,
                            "temperature": 1.0},
          "DecoderParams": {"num_clusters": [20, 10], "num_subheads": 5, "head_types": "linear", "normalize": [False, True],
                            "temperature": 0.5},
          "LossParams": {"paddings": [1, 3], "patch_sizes": 1024}, "enforce_matching": False}


def _model():
    from spcl_amd.semi_seg.arch import UNet
    return UNet(input_dim=1, num_classes=4, max_channel=128)


def test_hooks_build_from_the_config_section_with_importance_weights():
    from spcl_amd.contrastyou.hooks.base import CombineTrainerHook
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.hooks import IICEstimatorTrainHook, create_iic_estimator_hooks, feature_until_from_hooks
    model = _model()
    base = {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2}}
    (hook,) = create_hook_from_config(model, dict(base, IICRegParameters=PARAMS))
    assert isinstance(hook, CombineTrainerHook) and all(isinstance(h, IICEstimatorTrainHook) for h in hook._hooks)
    assert [h._hook_name for h in hook._hooks] == ["iic/conv5", "iic/up_conv3", "iic/up_conv2"]
    assert [h._weight for h in hook._hooks] == pytest.approx([0.1 * 1 / 8, 0.1 * 2 / 8, 0.1 * 5 / 8], rel=1e-12)
    assert feature_until_from_hooks(hook) == "Up_conv2"
    ests = [h._estimator for h in hook._hooks]
    assert [e._input_dim for e in ests] == [model.get_channel_dim(f) for f in PARAMS["feature_names"]]
    assert [e.is_encoder for e in ests] == [True, False, False]
    assert [(e._num_clusters, e._normalize, e._t) for e in ests] == [(20, False, 1.0), (20, False, 0.5), (10, True, 0.5)]
    assert [e._criterion.padding for e in ests[1:]] == [1, 3]
    assert [e._criterion._patch_size for e in ests[1:]] == [(1024, 1024)] * 2
    assert all(h.learnable_modules == [h._estimator] for h in hook._hooks)
    n_est = sum(p.numel() for e in ests for p in e.parameters())
    assert sum(p.numel() for p in hook.parameters()) == n_est > 0
    with pytest.raises(RuntimeError, match="IICRegParameters are not supported for pretrain stage"):
        create_hook_from_config(model, dict(base, IICRegParameters=PARAMS), is_pretrain=True)
    one = create_iic_estimator_hooks(model=model, feature_names="Conv5", weight=0.5, EncoderParams={}, DecoderParams={},
                                     LossParams={})
    assert len(one._hooks) == 1 and one._hooks[0]._weight == 0.5


def test_array_interfaces_broadcast_and_keep_the_references_keys():
    from spcl_amd.semi_seg.mi_estimator import IICEstimator, IICEstimatorArray
    model = _model()
    arr = IICEstimatorArray()
    arr.add_encoder_interface(["Conv4", "Conv5", "Up_conv3"], num_subheads=[2, 3], num_clusters=7, model=model)
    arr.add_decoder_interface(["Conv5", "Up_conv3", "Up_conv2"], num_subheads=2, num_clusters=[4, 6], paddings=[0, 2],
                              patch_sizes=[16, 32], model=model)
    assert len(arr) == 4 and [e._layer_name for e in arr] == ["Conv4", "Conv5", "Up_conv3", "Up_conv2"]
    assert [(e._num_subhead, e._num_clusters) for e in arr] == [(2, 7), (3, 7), (2, 4), (2, 6)]
    assert isinstance(arr["Up_conv2"], IICEstimator) and arr["Up_conv2"]._criterion.padding == 2
    assert list(arr["Conv5"].state_dict()) == [f"_projector._headers.{s}.2.{n}" for s in range(3) for n in ("weight", "bias")]
    assert list(arr["Up_conv3"].state_dict()) == [f"_projector._headers.{s}.0.{n}" for s in range(2) for n in ("weight", "bias")]
    with pytest.raises(AssertionError):
        arr.add_encoder_interface(["Conv3", "Conv2"], num_subheads=[1, 2, 3], model=model)  # a list of another length
    with pytest.raises(AssertionError):
        arr.add(name="Conv5", input_dim=8, projector_params={}, criterion_params={"padding": 0, "patch_size": 0})
    # one seed draws the weights the reference's construction order draws
    from torch import nn
    torch.manual_seed(5)
    est = IICEstimator()
    est.init_projector(layer_name="Up_conv3", input_dim=8, num_subhead=2, num_cluster=4)
    torch.manual_seed(5)
    ref = [nn.Conv2d(8, 4, 1, 1, 0) for _ in range(2)]
    for s, m in enumerate(ref):
        assert torch.equal(est.state_dict()[f"_projector._headers.{s}.0.weight"], m.weight)
    with pytest.raises(ValueError, match="num_cluster"):
        IICEstimator().init_projector(layer_name="Conv5", input_dim=8, num_cluster=33)


def test_a_cpu_tensor_is_refused():
    from spcl_amd.semi_seg.mi_estimator import IICEstimator
    for layer in ("Conv5", "Up_conv3"):
        est = IICEstimator()
        est.init_projector(layer_name=layer, input_dim=8)
        est.init_criterion(padding=1, patch_size=8)
        with pytest.raises(RuntimeError, match="MI355X"):
            est.from_feature(torch.rand(4, 8, 6, 6))
        with pytest.raises(RuntimeError, match="MI355X"):
            est(torch.rand(2, 8, 6, 6), torch.rand(2, 8, 6, 6))
    with pytest.raises(RuntimeError, match="initialize"):
        IICEstimator().from_feature(torch.rand(4, 8, 6, 6))


def test_reference_import_name_resolves_after_install():
    import spcl_amd
    done = spcl_amd.install()
    assert "semi_seg.mi_estimator.discrete_mi_estimator" in done
    from semi_seg.mi_estimator.discrete_mi_estimator import IICEstimatorArray, IICEstimator  # noqa: F401
    from spcl_amd.semi_seg.mi_estimator import discrete_mi_estimator as mine
    assert IICEstimatorArray is mine.IICEstimatorArray


def test_new_entry_points_are_declared_and_check_their_arguments():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    hdr = open(os.path.join(REPO, "include", "spcl_hip.h")).read()
    assert int(re.search(r"#define\s+SPCL_ABI_VERSION\s+(\d+)", hdr).group(1)) == native.ABI_VERSION >= 26
    L = native.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in native._SIGNATURES and hasattr(L, name), name
    one = ctypes.c_void_p(64)  # never dereferenced: every call below is refused on the host

    def err():
        return L.spcl_last_error().decode()

    nP, ws, dj = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    out = (ctypes.byref(nP), ctypes.byref(ws), ctypes.byref(dj))
    assert L.spcl_iic_patch_heads_plan(2, 5, 20, 100, 56, 56, 1, 32, *out) == 0
    assert nP.value == 9 and dj.value == 5 * 9 * 9 * 20 * 20 and ws.value == 5 * 9 * 9 * 400 * 8 + 5 * 9 * 8 + 64
    assert L.spcl_iic_patch_heads_plan(2, 2, 17, 34, 9, 7, 2, 16, *out) == 0 and nP.value == 1 and dj.value == 2 * 25 * 400
    assert L.spcl_iic_patch_heads_plan(2, 5, 33, 200, 8, 8, 1, 8, *out) == -1 and "K = 33" in err()
    assert L.spcl_iic_patch_heads_plan(2, 5, 20, 100, 8, 8, 8, 8, *out) == -1 and "padding 8" in err()
    assert L.spcl_iic_patch_heads_plan(2, 5, 20, 100, 8, 8, 1, 1, *out) == -1 and "patch size 1" in err()
    assert L.spcl_iic_patch_heads_plan(2, 5, 20, 99, 8, 8, 1, 8, *out) == -1 and "ld = 99" in err()
    assert L.spcl_iic_patch_heads_plan(0, 5, 20, 100, 8, 8, 1, 8, *out) == -1 and "empty" in err()

    def fwd(lx=one, K=20, ws_bytes=1 << 30):
        return L.spcl_iic_patch_heads_forward(lx, one, 100, 2, 8, 8, 5, K, 1, 8, None, ctypes.c_float(1.0), one, None, one, one, one,
                                              ctypes.c_size_t(ws_bytes), None)

    assert fwd(lx=None) == -1 and "null" in err()
    assert fwd(K=1) == -1 and "K = 1" in err()
    assert fwd(ws_bytes=8) == -1 and "workspace" in err()
    assert L.spcl_iic_patch_heads_backward(one, one, 100, 2, 8, 8, 5, 20, 1, 8, None, None, None, one, None, None) == -1
    assert "null" in err()
    assert L.spcl_iic_patch_heads_backward(one, one, 64, 2, 8, 8, 5, 20, 1, 8, None, one, None, one, None, None) == -1
    assert "ld = 64" in err()
    f = ctypes.c_float
    assert L.spcl_group_l2norm_temp_forward(None, 4, 15, 3, 5, 1, f(1.0), one, None) == -1 and "null" in err()
    assert L.spcl_group_l2norm_temp_forward(one, 4, 14, 3, 5, 1, f(1.0), one, None) == -1 and "ld = 14" in err()
    assert L.spcl_group_l2norm_temp_forward(one, 0, 15, 3, 5, 1, f(1.0), one, None) == -1 and "empty" in err()
    assert L.spcl_group_l2norm_temp_forward(one, 4, 15, 3, 5, 1, f(0.0), one, None) == -1 and "temperature" in err()
    assert L.spcl_group_l2norm_temp_forward(one, 4, 15, 3, 5, 0, f(1.0), one, None) == 0  # the identity in place: no launch
    assert L.spcl_group_l2norm_temp_backward(one, None, 4, 15, 3, 5, 1, f(1.0), one, None) == -1 and "null" in err()
    assert L.spcl_group_l2norm_temp_backward(one, one, 4, 15, 3, 5, 1, f(-1.0), one, None) == -1 and "temperature" in err()


GOLDEN = os.path.join(REPO, "tests", "golden", "g15_iic_estimator.npz")
RTOL, ATOL = 1e-4, 1e-6


def _close(got, want, what):
    assert torch.allclose(got.float(), want.float(), rtol=RTOL, atol=ATOL), \
        (what, float((got.float() - want.float()).abs().max()))


def test_oracle_reproduces_the_references_recorded_results():
    """the float32 restatements of tests/_iic_estimator_oracle.py against what the reference's own classes computed"""
    from tests import _iic_estimator_oracle as E
    from tests import _iic_oracle as R
    heads, ests, z = E.load_golden(GOLDEN)
    assert len(heads) == 16 and len(ests) == 8
    S, K = 3, 5
    for key in heads:
        dense, ht, nz, T = E.parse_case(key)
        idx = (0, 2) if dense else (2, 4)
        assert z[key + "/keys"] == [f"_headers.{s}.{i}.{n}" for s in range(S) for i in idx[:2 if ht == "mlp" else 1]
                                   for n in ("weight", "bias")], key
        x = z[key + "/feat"].clone().requires_grad_(True)
        probs = E.head_probs(x, E.golden_state(z, key), dense, S, K, ht, nz, T)
        _close(probs.reshape(z[key + "/probs"].shape), z[key + "/probs"], key + " probs")
        (probs.reshape(z[key + "/up"].shape) * z[key + "/up"]).sum().backward()
        _close(x.grad, z[key + "/dfeat"], key + " dfeat")
    for key in ests:
        layer, ht, nz, T = E.parse_case(key)
        flags = [int(f) for f in z[key + "/flags"]]
        sd = {k[len("_projector."):]: v.clone().requires_grad_(True) for k, v in E.golden_state(z, key).items()}
        a = z[key + "/feat"].clone().requires_grad_(True)
        b = z[key + "/feat_tf"].clone().requires_grad_(True)
        loss = E.estimator_forward(b, R.flip(a, flags), sd, layer != "Conv5", S, K, ht, nz, T, 1, 8)
        loss.backward()
        _close(loss.detach(), z[key + "/loss"], key + " loss")
        _close(a.grad, z[key + "/dfeat"], key + " dfeat")
        _close(b.grad, z[key + "/dfeat_tf"], key + " dfeat_tf")
        for k, v in sd.items():
            _close(v.grad, z[f"{key}/grad/_projector.{k}"], key + " grad " + k)
