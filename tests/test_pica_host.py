"""CPU-only: the PICA baseline's host side -- the float64 restatement of tests/_pica_oracle.py reproduces the reference's
recorded results (tests/golden/g13_pica.npz, written by tools/gen_golden_pica.py) within the gaps the reference itself shows
between float32 and float64; the dense balance term is the constant ``log M - (M / K) log K``; the C ABI carries the new
entries; the reference's import names resolve after ``install()``; ``PICALossWrapper`` holds the two criteria; the hooks build
from ``PICAConsistencyParams`` (refused during pre-training) under the names ``pica/<feature>``."""
import math
import os
import re

import pytest
import torch

from tests import _pica_oracle as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "g13_pica.npz")
HEADER = os.path.join(REPO, "include", "spcl_hip.h")
F32 = 2.0 ** -23


def test_oracle_reproduces_the_references_recorded_results():
    cases, z = P.load_golden(GOLDEN)
    assert cases == [P.case_key(*c) for c in P.GOLDEN_CASES]
    for case in P.GOLDEN_CASES:
        kind, N, K, H, W, pad, lamda = case
        key = P.case_key(*case)
        loss, ce, gx, gy = P.run_case(z[key + "/x"], z[key + "/y"], kind, pad, lamda, torch.float64)
        gap_loss, gap_gy = float(z[key + "/gap_loss"]), float(z[key + "/gap_gy"])
        # the recorded values are float32 results: they miss float64 by the recorded gap (and by one rounding of the result)
        got_l, got_g = P.rel(z[key + "/loss"], loss), P.rel_l2(z[key + "/gy"], gy)
        print(f"{key}: loss {got_l:.2e} (gap {gap_loss:.2e}), gy {got_g:.2e} (gap {gap_gy:.2e})")
        assert got_l <= gap_loss + F32, (key, got_l, gap_loss)
        assert got_g <= gap_gy + F32, (key, got_g, gap_gy)


@pytest.mark.parametrize("N,K,H,W,pad", [(2, 20, 9, 11, 1), (1, 10, 13, 7, 3), (3, 2, 5, 6, 0), (5, 20, 28, 28, 1)])
def test_dense_balance_term_is_a_constant_of_the_shape(N, K, H, W, pad):
    x, y = P.make_probabilities(N, K, H, W, seed=7)
    x = x.double()
    x = x / x.sum(1, keepdim=True)
    _, _, ne = P.pui_seg_loss(x, y.double(), pad)
    want = P.balance_constant(N * H * W, K)
    assert want == math.log(N * H * W) - (N * H * W / K) * math.log(K)
    assert abs(float(ne) - want) <= 1e-12 * abs(want), (float(ne), want)
    from spcl_amd import functional as F_hip
    assert F_hip.pica_balance_constant(N * H * W, K) == want


def test_abi_carries_the_new_entries():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    assert native.ABI_VERSION >= 22
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("spcl_pica_workspace_bytes", "spcl_pica_seg_loss", "spcl_pica_global_loss"):
        assert name in native._SIGNATURES, name
        args = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(native._SIGNATURES[name][1]) == len(args.split(",")), name
        assert hasattr(native.lib(), name)
    L = native.lib()
    assert native.call("spcl_pica_workspace_bytes", 5) == 5 * 2 * 8 + 64 and native.call("spcl_pica_workspace_bytes", 0) == 0
    import ctypes
    one = ctypes.c_void_p(64)  # never dereferenced: every call below is refused on the host
    seg = L.spcl_pica_seg_loss
    assert seg(one, one, 1, 20, 3, ctypes.c_double(0), ctypes.c_float(1), None, one, one, one, one, ctypes.c_size_t(80),
               None) == -1 and "exactly one" in L.spcl_last_error().decode()
    assert seg(None, one, 1, 33, 3, ctypes.c_double(0), ctypes.c_float(1), None, one, one, one, one, ctypes.c_size_t(80),
               None) == -1 and "bad shape" in L.spcl_last_error().decode()
    assert seg(None, one, 1, 20, 4, ctypes.c_double(0), ctypes.c_float(1), None, one, one, one, one, ctypes.c_size_t(80),
               None) == -1 and "bad shape" in L.spcl_last_error().decode()
    assert seg(None, one, 1, 20, 3, ctypes.c_double(0), ctypes.c_float(1), None, one, one, one, one, ctypes.c_size_t(8),
               None) == -1 and "missing buffer" in L.spcl_last_error().decode()
    glob = L.spcl_pica_global_loss

    def g(lx=one, ld=20, N=3, K=20, ws=80):
        return glob(lx, one, ctypes.c_long(ld), N, 1, K, ctypes.c_float(2), ctypes.c_float(1), None, one, one, one, one, one,
                    ctypes.c_size_t(ws), None)

    assert g(lx=None) == -1 and "null" in L.spcl_last_error().decode()
    assert g(N=0) == -1 and "bad shape" in L.spcl_last_error().decode()
    assert g(K=1) == -1 and "bad shape" in L.spcl_last_error().decode()
    assert g(ld=19) == -1 and "row pitch" in L.spcl_last_error().decode()
    assert g(ws=8) == -1 and "workspace" in L.spcl_last_error().decode()


def test_reference_import_names_resolve_after_install():
    import spcl_amd
    done = spcl_amd.install()
    for name in ("contrastyou.losses.pica_loss", "contrastyou.losses.wrappers", "semi_seg.utils", "semi_seg.hooks.pica"):
        assert name in done, name
    from contrastyou.losses.pica_loss import PUILoss, PUISegLoss  # noqa: F401
    from contrastyou.losses.wrappers import LossWrapperBase  # noqa: F401
    from semi_seg.utils import IICLossWrapper, PICALossWrapper, _filter_decodernames, _filter_encodernames, _nlist  # noqa: F401
    from semi_seg.hooks import create_pica_consistency_hook, create_pica_hooks  # noqa: F401


def test_loss_wrappers_hold_the_criteria():
    from spcl_amd.contrastyou.losses.iic_loss import IIDLoss, IIDSegmentationSmallPathLoss
    from spcl_amd.contrastyou.losses.pica_loss import PUILoss, PUISegLoss
    from spcl_amd.contrastyou.losses.wrappers import LossWrapperBase
    from spcl_amd.semi_seg.utils import IICLossWrapper, PICALossWrapper, _nlist
    w = PICALossWrapper(["Conv5", "Up_conv3"], paddings=1)
    assert isinstance(w, LossWrapperBase) and w.feature_names == ["Conv5", "Up_conv3"]
    assert isinstance(w["Conv5"], PUILoss) and w["Conv5"].lamda == 2.0
    assert isinstance(w["Up_conv3"], PUISegLoss) and w["Up_conv3"].padding == 1
    assert [type(c) for c in w] == [PUILoss, PUISegLoss] and [k for k, _ in w.items()] == ["Conv5", "Up_conv3"]
    with pytest.raises(IndexError):
        w["Conv1"]
    w2 = PICALossWrapper(["Up_conv3", "Conv5", "Up_conv2"], paddings=[1, 3])  # encoder features first, as the reference
    assert w2.feature_names == ["Conv5", "Up_conv3", "Up_conv2"] and w2["Up_conv2"].padding == 3
    with pytest.raises(AssertionError):
        PICALossWrapper(["Up_conv3", "Up_conv2"], paddings=[1, 2, 3])
    iic = IICLossWrapper(["Conv5", "Up_conv2"], paddings=1, patch_sizes=32)
    assert isinstance(iic["Conv5"], IIDLoss) and isinstance(iic["Up_conv2"], IIDSegmentationSmallPathLoss)
    assert iic["Up_conv2"].padding == 1 and iic["Up_conv2"]._patch_size == (32, 32)
    assert _nlist(3)(1) == [1, 1, 1] and _nlist(2)("ab") == ["ab", "ab"] and _nlist(2)([4, 5]) == [4, 5]
    # the classes keep the reference's assert message and refuse a CPU tensor (no eager fall-back)
    with pytest.raises(AssertionError, match="same shape"):
        PUILoss()(torch.rand(3, 4), torch.rand(3, 5))
    with pytest.raises(AssertionError, match="same shape"):
        PUISegLoss()(torch.rand(1, 4, 5, 5), torch.rand(1, 4, 5, 6))
    with pytest.raises(RuntimeError, match="MI355X"):
        PUILoss()(torch.rand(3, 4).softmax(1), torch.rand(3, 4).softmax(1))
    with pytest.raises(AssertionError):
        PUISegLoss(check_inputs=True)(torch.rand(1, 4, 5, 5), torch.rand(1, 4, 5, 5))


def test_hooks_build_from_the_config_section():
    from spcl_amd.contrastyou.hooks.base import CombineTrainerHook
    from spcl_amd.contrastyou.losses.pica_loss import PUILoss, PUISegLoss
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.hooks import (ConsistencyTrainerHook, DiscreteMITrainHook, PICATrainHook, create_pica_hooks,
                                         feature_until_from_hooks)
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    base = {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2}}
    cfg = dict(base, PICAConsistencyParams={"feature_names": ["Conv5", "Up_conv3", "Up_conv2"], "pica_weights": [0.1, 0.05, 0.05],
                                            "dense_paddings": [1, 3], "consistency_weight": 1, "lamda": 1.5})
    (hook,) = create_hook_from_config(model, cfg)
    assert isinstance(hook, CombineTrainerHook) and len(hook._hooks) == 2
    pica, cons = hook._hooks
    assert isinstance(cons, ConsistencyTrainerHook)
    assert [h._hook_name for h in pica._hooks] == ["pica/conv5", "pica/up_conv3", "pica/up_conv2"]
    assert all(isinstance(h, PICATrainHook) and isinstance(h, DiscreteMITrainHook) for h in pica._hooks)
    assert [type(h._criterion) for h in pica._hooks] == [PUILoss, PUISegLoss, PUISegLoss]
    assert [h._criterion.lamda for h in pica._hooks] == [1.5] * 3
    assert [h._criterion.padding for h in pica._hooks[1:]] == [1, 3]
    assert [h._weight for h in pica._hooks] == [0.1, 0.05, 0.05]
    assert all(h.learnable_modules == [h._projector] for h in pica._hooks)
    assert feature_until_from_hooks(pica) == "Up_conv2"
    with pytest.raises(RuntimeError, match="pretrain"):
        create_hook_from_config(model, cfg, is_pretrain=True)
    assert create_hook_from_config(model, base) == []
    one = create_pica_hooks(model=model, feature_names=["Conv5"], weights=[0.5], paddings=[])
    assert len(one._hooks) == 1 and one._hooks[0]._criterion.lamda == 2.0
