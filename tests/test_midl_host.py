"""CPU: the MIDL baseline is wired in -- ``iic_patch_starts`` follows ``patch_generator``'s rule, the factory and
``create_hook_from_config`` build consistency + patch-wise IIC from ``MIDLPaperParameters`` (refused during pre-training),
only the ``mse`` consistency criterion is mirrored, the reference-style imports resolve after ``install()``, ``mask`` and
``lamda != 1`` are refused, ``patch_generator`` slices what the reference slices, and the native table lists the new entry
points, whose argument checks answer on the host with an error code and a message."""
import ctypes

import pytest
import torch

MIDL = {"iic_weight": 0.1, "padding": 1, "patch_size": 16, "consistency_weight": 5.0, "name": "mse"}


def _config(**sections):
    return dict({"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 30}}, **sections)


@pytest.mark.parametrize("h,patch,want", [(20, 8, [0, 4, 8, 12]), (21, 8, [0, 4, 8, 12, 13]), (27, 8, [0, 4, 8, 12, 16, 19]),
                                          (9, 16, [0]), (16, 16, [0]), (21, 7, [0, 3, 6, 9, 12, 14]), (224, 1024, [0])])
def test_patch_starts(h, patch, want):
    from spcl_amd.functional import iic_patch_starts
    from tests._midl_oracle import starts
    assert iic_patch_starts(h, patch) == want == starts(h, patch)


def test_patch_starts_of_the_workload_and_refusals():
    from spcl_amd.functional import iic_patch_starts
    s = iic_patch_starts(224, 32)
    assert len(s) == 13 and s[-1] == 192 and s[:3] == [0, 16, 32]
    with pytest.raises(ValueError):
        iic_patch_starts(224, 1)
    from spcl_amd.contrastyou.losses.iic_loss import IIDSegmentationSmallPathLoss
    with pytest.raises(ValueError):
        IIDSegmentationSmallPathLoss(patch_size=1)


def test_library_counts_the_same_patches():
    from spcl_amd import native
    from spcl_amd.functional import iic_patch_starts
    n, ws, dj = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    for H, W, patch, pad, C in ((21, 27, 8, 1, 4), (21, 27, 7, 1, 4), (9, 7, 16, 1, 2), (224, 224, 32, 1, 4),
                                (224, 224, 1024, 1, 4), (19, 33, 10, 2, 5), (5, 224, 2, 7, 16)):
        native.call("spcl_iic_patch_plan", 2, C, H, W, pad, patch, ctypes.byref(n), ctypes.byref(ws), ctypes.byref(dj))
        nP, T, CP = len(iic_patch_starts(H, patch)) * len(iic_patch_starts(W, patch)), 2 * pad + 1, (C + 3) // 4 * 4
        assert n.value == nP
        assert dj.value == nP * T * T * CP * CP
        assert ws.value >= nP * T * T * C * C * 8 + nP * 8 + 4


def test_factory_and_config_section_build_the_hooks():
    from spcl_amd.contrastyou.hooks.base import CombineTrainerHook
    from spcl_amd.contrastyou.losses.iic_loss import IIDSegmentationSmallPathLoss
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.hooks import ConsistencyTrainerHook, MIDLPaperTrainerHook, create_midl_hook
    (hook,) = create_hook_from_config(None, _config(MIDLPaperParameters=MIDL))
    assert isinstance(hook, CombineTrainerHook)
    consistency, midl = hook._hooks
    assert isinstance(consistency, ConsistencyTrainerHook) and consistency._weight == 5.0
    assert isinstance(midl, MIDLPaperTrainerHook) and midl._weight == 0.1
    assert isinstance(midl._criterion, IIDSegmentationSmallPathLoss)
    assert midl._criterion.padding == 1 and midl._criterion._patch_size == (16, 16) and midl._criterion._step_size == (8, 8)
    assert repr(midl._criterion) == "IIDSegmentationSmallPathLoss with patch_size=(16, 16) and padding=1."
    assert list(hook.parameters()) == []
    with pytest.raises(RuntimeError):
        create_hook_from_config(None, _config(MIDLPaperParameters=MIDL), is_pretrain=True)
    assert create_hook_from_config(None, _config()) == []
    # the defaults are those of config/specific/midl.yaml
    default = create_midl_hook(consistency_weight=1.0)._hooks[1]
    assert default._weight == 0.1 and default._criterion.padding == 1 and default._criterion._patch_size == (1024, 1024)
    eh = hook()
    assert [type(h).__name__ for h in eh._epocher_hook] == ["_ConsistencyEpocherHook", "_MIDLPaperEpocherHook"]
    assert eh.graph_key() is None


def test_only_the_mse_consistency_criterion_is_mirrored():
    from spcl_amd.semi_seg.hooks import create_midl_hook
    with pytest.raises(NotImplementedError):
        create_midl_hook(consistency_weight=1.0, name="kl")


def test_install_resolves_the_reference_style_imports():
    import spcl_amd
    done = spcl_amd.install()
    assert "semi_seg.hooks.midl" in done
    from contrastyou.losses.iic_loss import IIDSegmentationSmallPathLoss, patch_generator
    from semi_seg.hooks import create_midl_hook
    from semi_seg.hooks.midl import MIDLPaperTrainerHook
    from spcl_amd.contrastyou.losses import iic_loss
    from spcl_amd.semi_seg.hooks import creator
    assert IIDSegmentationSmallPathLoss is iic_loss.IIDSegmentationSmallPathLoss
    assert patch_generator is iic_loss.patch_generator
    assert create_midl_hook is creator.create_midl_hook and MIDLPaperTrainerHook is creator.MIDLPaperTrainerHook


def test_mask_and_lamda_are_refused():
    from spcl_amd.contrastyou.losses.iic_loss import IIDSegmentationSmallPathLoss
    p = torch.full((1, 4, 8, 8), 0.25)
    with pytest.raises(NotImplementedError):
        IIDSegmentationSmallPathLoss(padding=1, patch_size=4)(p, p, mask=torch.ones(1, 1, 8, 8))
    with pytest.raises(NotImplementedError):
        IIDSegmentationSmallPathLoss(lamda=2)
    with pytest.raises(NotImplementedError):
        IIDSegmentationSmallPathLoss(patch_size=(8, 16))


def test_patch_generator_slices_in_row_major_order():
    from spcl_amd.contrastyou.losses.iic_loss import patch_generator
    from tests._midl_oracle import starts
    x = torch.arange(2 * 3 * 21 * 27, dtype=torch.float32).view(2, 3, 21, 27)
    got = list(patch_generator(x, (8, 8), (4, 4)))
    want = [x[:, :, a:a + 8, b:b + 8] for a in starts(21, 8) for b in starts(27, 8)]
    assert len(got) == len(want) == 30 and all(torch.equal(g, w) for g, w in zip(got, want))
    (one,) = list(patch_generator(x, (1024, 1024), (512, 512)))
    assert torch.equal(one, x)


def test_native_table_lists_the_entry_points_and_their_argument_checks_report():
    """every refusal below happens on the host, before any device call"""
    from spcl_amd import native
    for name in ("spcl_iic_patch_plan", "spcl_iic_patch_forward", "spcl_iic_patch_backward"):
        assert name in native._SIGNATURES
    assert native.ABI_VERSION >= 14
    L = native.lib()
    f = ctypes.c_float
    fake = ctypes.c_void_p(4096)  # never dereferenced: each call below is refused before a launch

    def forward(C=4, pad=1, patch=8, lx=fake, loss=fake, flag=fake, dj=fake, ws=fake, ws_bytes=1 << 24):
        return L.spcl_iic_patch_forward(lx, fake, 2, C, 21, 27, pad, patch, None, f(1.0), loss, None, flag, dj, ws, ws_bytes,
                                        None)

    for kwargs, word in (({"C": 17}, b"C = 17"), ({"C": 1}, b"C = 1"), ({"pad": 8}, b"padding 8"), ({"pad": -1}, b"padding -1"),
                         ({"patch": 1}, b"patch size 1"), ({"lx": None}, b"null"), ({"loss": None}, b"null"),
                         ({"flag": None}, b"null"), ({"dj": None}, b"null"), ({"ws": None}, b"null"),
                         ({"ws_bytes": 64}, b"workspace")):
        assert forward(**kwargs) == -1, kwargs
        assert word in L.spcl_last_error(), (kwargs, L.spcl_last_error())
    assert L.spcl_iic_patch_backward(fake, fake, 2, 4, 21, 27, 1, 1, None, fake, None, fake, None, None) == -1
    assert b"patch size 1" in L.spcl_last_error()
    assert L.spcl_iic_patch_backward(fake, fake, 2, 4, 21, 27, 1, 8, None, fake, None, None, None, None) == -1
    assert b"null" in L.spcl_last_error()
