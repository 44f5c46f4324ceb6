"""CPU-only: the MINE baseline's host side -- the restatement of tests/_mine_oracle.py reproduces the reference's recorded
results (tests/golden/g12_mine.npz, written by tools/gen_golden_mine.py), ``create_mine_hooks`` and
``create_hook_from_config`` build the hooks from ``MineParameters`` (refused during pre-training, nothing without the
section), the estimator's ``state_dict`` is a stock ``nn.Sequential``'s and one seed draws the same initial weights, a CPU
tensor raises, the reference's import name resolves after ``install()``, and the four C entry points answer bad arguments with
an error code and a message."""
import ctypes
import os

import pytest
import torch

from tests import _mine_oracle as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_mine.npz")
RTOL, ATOL = 1e-4, 1e-6


def _close(got, want, what):
    assert torch.allclose(got.float(), want.float(), rtol=RTOL, atol=ATOL), \
        (what, float((got.float() - want.float()).abs().max()))


def test_oracle_reproduces_the_references_recorded_results():
    cases, z = M.load_golden(GOLDEN)
    assert cases == [f"n{n}_c{C}_h{H}_w{W}" for n, C, H, W in M.SHAPES]
    for key in cases:
        feat, flags = z[key + "/feat"], [int(f) for f in z[key + "/flags"]]
        sd0 = {k[len(key + "/init/"):]: v for k, v in z.items() if k.startswith(key + "/init/")}
        got = M.run(feat, flags, sd0, torch.float32)
        _close(got["loss"], z[key + "/loss"], key + " loss")
        _close(got["dfeat"], z[key + "/dfeat"], key + " dfeat")
        for k, g in got["grads"].items():
            _close(g, z[key + "/grad/" + k], key + " grad " + k)
        for k, v in got["state"].items():
            if "running" in k:
                _close(v, z[key + "/after/" + k], key + " " + k)
            elif "num_batches" in k:
                assert int(v) == int(z[key + "/after/" + k]) == 2, k


def _model():
    from spcl_amd.semi_seg.arch import UNet
    return UNet(input_dim=1, num_classes=4, max_channel=128)


def test_hooks_build_from_the_config_section():
    from spcl_amd.contrastyou.hooks.base import CombineTrainerHook
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.hooks import MineTrainHook, create_mine_hooks, feature_until_from_hooks
    model = _model()
    base = {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2}}
    assert create_hook_from_config(model, base) == []
    cfg = dict(base, MineParameters={"feature_names": ["Conv5", "Up_conv3"], "weights": [0.1, 0.05]})
    (hook,) = create_hook_from_config(model, cfg)
    assert isinstance(hook, CombineTrainerHook) and len(hook._hooks) == 2
    assert [h._hook_name for h in hook._hooks] == ["mine/conv5", "mine/up_conv3"]
    assert all(isinstance(h, MineTrainHook) for h in hook._hooks)
    assert [h._weight for h in hook._hooks] == [0.1, 0.05]
    assert [h._estimator._input_dim for h in hook._hooks] == [model.get_channel_dim("Conv5"), model.get_channel_dim("Up_conv3")]
    assert feature_until_from_hooks(hook) == "Up_conv3"
    n_est = sum(p.numel() for h in hook._hooks for p in h._estimator.parameters())
    assert sum(p.numel() for p in hook.parameters()) == n_est > 0
    with pytest.raises(RuntimeError, match="pretrain"):
        create_hook_from_config(model, cfg, is_pretrain=True)
    one = create_mine_hooks(model=model, feature_names="Conv5", weights=0.5)
    assert len(one._hooks) == 1 and one._hooks[0]._weight == 0.5 and feature_until_from_hooks(one) == "Conv5"


def test_state_dict_is_a_stock_sequentials_and_one_seed_draws_the_same_weights():
    from spcl_amd.semi_seg.mi_estimator import MineEstimator, MineEstimatorArray
    torch.manual_seed(7)
    est = MineEstimator(layer_name="Conv5", input_dim=16)
    torch.manual_seed(7)
    ref = M.projector(16)
    sd, rsd = est.state_dict(), ref.state_dict()
    assert list(sd) == ["_projector." + k for k in rsd]
    for k, v in rsd.items():
        assert torch.equal(sd["_projector." + k], v), k
    assert tuple(sd["_projector.0.weight"].shape) == (16, 32, 3, 3) and tuple(sd["_projector.0.bias"].shape) == (16,)
    assert tuple(sd["_projector.3.weight"].shape) == (8, 16, 3, 3) and tuple(sd["_projector.8.weight"].shape) == (1, 8)
    est.load_state_dict({"_projector." + k: v for k, v in M.init_state(16, 3).items()}, strict=True)
    assert est.eval()._projector[1].training is False and est.train()._projector[4].training is True
    with pytest.raises(RuntimeError, match="MI355X"):
        est(torch.rand(2, 16, 5, 7), torch.rand(2, 16, 5, 7))
    with pytest.raises(RuntimeError, match="MI355X"):
        est.from_feature(torch.rand(4, 16, 5, 7))
    assert int(est._projector[1].num_batches_tracked) == 0  # a refused call counted nothing
    for bad in (15, 1024):
        with pytest.raises(ValueError, match="input_dim"):
            MineEstimator(layer_name="Conv5", input_dim=bad)
    arr = MineEstimatorArray()
    arr.add_interface(["Conv5", "Up_conv3"], model=_model())
    arr.add("Up_conv2", input_dim=8)
    assert len(arr) == 3 and [e._layer_name for e in arr] == ["Conv5", "Up_conv3", "Up_conv2"]


def test_reference_import_name_resolves_after_install():
    import spcl_amd
    done = spcl_amd.install()
    assert "semi_seg.mi_estimator.mineestimator" in done and "semi_seg.hooks.mine" in done
    from semi_seg.mi_estimator.mineestimator import MineEstimator, MineEstimatorArray  # noqa: F401
    from semi_seg.hooks import create_mine_hooks  # noqa: F401


def test_c_entry_points_answer_bad_arguments_with_codes():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    assert native.ABI_VERSION >= 21
    names = ("spcl_mine_pairs_forward", "spcl_mine_pairs_backward", "spcl_mine_head_forward", "spcl_mine_head_backward")
    assert all(n in native._SIGNATURES for n in names) and "spcl_mine_head_workspace_bytes" in native._SIGNATURES
    L = native.lib()
    assert all(hasattr(L, n) for n in names)
    one = ctypes.c_void_p(64)  # never dereferenced: every call below is refused on the host

    def err():
        return L.spcl_last_error().decode()

    ws_bytes = L.spcl_mine_head_workspace_bytes
    assert ws_bytes(3, 5, 7, 16) == 64 + 2 * 3 * 1 * 8 * 8 and ws_bytes(3, 56, 56, 64) == 64 + 2 * 3 * 13 * 32 * 8
    assert ws_bytes(0, 5, 7, 16) == 0 and ws_bytes(3, 5, 7, 15) == 0 and ws_bytes(3, 5, 7, 514) == 0
    assert L.spcl_mine_pairs_forward(None, None, 0, 2, 5, 7, 16, one, one, None) == -1 and "null" in err()
    assert L.spcl_mine_pairs_forward(one, None, 0, 0, 5, 7, 16, one, one, None) == -1 and "n, H, W, C > 0" in err()
    assert L.spcl_mine_pairs_forward(one, None, 2, 2, 5, 7, 16, one, one, None) == -1 and "dtype" in err()
    assert L.spcl_mine_pairs_backward(one, None, None, 0, 2, 5, 7, 16, one, None) == -1 and "null" in err()
    assert L.spcl_mine_pairs_backward(one, one, None, 1, -1, 5, 7, 16, one, None) == -1 and "n, H, W, C > 0" in err()

    def fwd(act=one, n=2, C=16, ws=one, ws_bytes=64 + 2 * 2 * 8 * 8):
        return L.spcl_mine_head_forward(act, one, 0, n, 5, 7, C, one, one, one, one, one, one, ws, ctypes.c_size_t(ws_bytes), None)

    assert fwd(act=None) == -1 and "null" in err()
    assert fwd(n=0) == -1 and "n, H, W > 0" in err()
    assert fwd(C=15) == -1 and "even" in err()
    assert fwd(C=514) == -1 and "256" in err()
    assert fwd(ws_bytes=64) == -1 and "workspace" in err()
    assert fwd(ws=None) == -1 and "null" in err()

    def bwd(t=one, n=2, C=16):
        return L.spcl_mine_head_backward(t, one, one, one, None, 1, n, 5, 7, C, one, one, None, None, None)

    assert bwd(t=None) == -1 and "null" in err()
    assert bwd(n=0) == -1 and "n, H, W > 0" in err()
    assert bwd(C=7) == -1 and "even" in err()
    assert bwd(C=1024) == -1 and "256" in err()
