"""CPU-only side of test-time augmentation: the C ABI's two entry points (header, signature table, version), the view table
and the oracle of tests/_tta_oracle.py on known answers, the host-side refusals of ``functional.tta_views`` / ``tta_merge`` and
``InferenceEpocher(tta=...)``, and the top-two gap of every seeded input of tests/test_gpu_tta_kernels.py -- asserted here so
that the GPU tests compare the arg-max at EVERY pixel."""
import inspect
import os
import re

import pytest
import torch

from tests import _tta_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "spcl_hip.h")


# ---- the C ABI
def test_header_and_native_agree_on_the_entries():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    hdr = open(HEADER).read()
    assert int(re.search(r"#define\s+SPCL_ABI_VERSION\s+(\d+)", hdr).group(1)) == native.ABI_VERSION >= 28
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "size_t spcl_tta_merge_workspace_bytes(int N, int H, int W);" in flat
    assert ("int spcl_tta_merge(const float* const* views, const uint8_t* ops, int V, int N, int C, int H, int W, float eps, "
            "float* prob, int64_t* pred, float* entropy, float* mean_entropy, void* ws, size_t ws_bytes, void* stream);") in flat
    assert "comparable.py:94-98" in hdr
    assert len(native._SIGNATURES["spcl_tta_merge"][1]) == 15
    assert len(native._SIGNATURES["spcl_tta_merge_workspace_bytes"][1]) == 3


# ---- the view table
def test_modes_are_ops_0_to_3_and_0_to_7():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    assert tuple(F_hip.TTA_MODES["flips"]) == O.MODES["flips"] == (0, 1, 2, 3)
    assert tuple(F_hip.TTA_MODES["dihedral"]) == O.MODES["dihedral"] == (0, 1, 2, 3, 4, 5, 6, 7)
    assert [op for _, op in O.views(torch.zeros(1, 1, 4, 4), "dihedral")] == list(range(8))


@pytest.mark.parametrize("mode,hw", [("flips", (6, 10)), ("dihedral", (7, 7))])
def test_oracle_inverse_map_restores_the_image(mode, hw):
    image = torch.arange(2 * hw[0] * hw[1], dtype=torch.float32).view(2, 1, *hw)
    vs = O.views(image, mode)
    assert vs[0][1] == 0 and torch.equal(vs[0][0], image)
    for v, op in vs:
        assert torch.equal(O.unview(v, op), image), op
    # the definition, spelled out for one pixel of every op: view[a][b] = image[u'][v'] read at (a, b) = (u, v), swapped: (v, u)
    H, W = hw
    u, v = 1, 2
    for x, op in vs:
        uu, vv = (H - 1 - u if op & 1 else u), (W - 1 - v if op & 2 else v)
        assert x[0, 0, v, u] == image[0, 0, uu, vv] if op & 4 else x[0, 0, u, v] == image[0, 0, uu, vv], op


def test_dihedral_views_of_an_asymmetric_image_are_pairwise_different():
    image = torch.arange(25, dtype=torch.float32).view(1, 1, 5, 5)
    vs = [v for v, _ in O.views(image, "dihedral")]
    for i in range(8):
        for j in range(i + 1, 8):
            assert not torch.equal(vs[i], vs[j]), (i, j)


@pytest.mark.parametrize("mode,shape", [("flips", (2, 4, 6, 10)), ("dihedral", (2, 5, 12, 12))])
def test_oracle_on_exact_copies_is_the_softmax_of_the_map(mode, shape):
    L = 3 * torch.randn(shape, generator=torch.Generator().manual_seed(7))
    ops = O.MODES[mode]
    prob, pred, entropy, mean_entropy, _ = O.merge([O.view(L, op) for op in ops], ops)
    want = torch.softmax(L.double(), dim=1)
    assert float((prob - want).abs().max()) <= 1e-12
    assert torch.equal(pred, want.argmax(1))
    assert abs(mean_entropy - float(entropy.mean())) <= 1e-15 and 0 < mean_entropy < 1


# ---- host refusals
def test_inference_epocher_refuses_an_unknown_tta():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.epochers import InferenceEpocher
    from spcl_amd.semi_seg.trainers import FineTuneTrainer

    class _M(torch.nn.Module):
        num_classes = 4

    assert InferenceEpocher.TTA == (None, "flips", "dihedral")
    for bad in ("rot90", "Flips", True, 4):
        with pytest.raises(ValueError, match="tta"):
            InferenceEpocher(model=_M(), loader=[], sup_criterion=KL_div(verbose=False), device="cpu", tta=bad)

    def names(**kw):
        ep = InferenceEpocher(model=_M(), loader=[], sup_criterion=KL_div(verbose=False), device="cpu", **kw)
        return list(ep.meters._groups["eval"])

    assert names() == names(tta=None) == ["loss", "dice", "hd"]
    assert names(tta="flips") == ["loss", "dice", "hd", "loss_tta", "dice_tta", "hd_tta", "tta_entropy", "tta_changed"]
    plain = names(volumetric=True, postprocess="largest_component")
    full = names(volumetric=True, postprocess="largest_component", tta="dihedral")
    assert full[:len(plain)] == plain  # the key list without _tta is unchanged, and comes first
    assert full[len(plain):] == ["loss_tta", "dice_tta", "hd_tta", "hd3d_tta", "mhd3d_tta", "asd3d_tta", "dice_tta_lcc",
                                 "hd_tta_lcc", "hd3d_tta_lcc", "mhd3d_tta_lcc", "asd3d_tta_lcc", "lcc_removed_tta", "tta_entropy",
                                 "tta_changed"]
    sig = inspect.signature(InferenceEpocher.__init__).parameters
    assert sig["tta"].default is None and sig["tta"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(FineTuneTrainer.inference).parameters
    assert sig["tta"].default is None and sig["tta"].kind is inspect.Parameter.KEYWORD_ONLY


def test_views_and_merge_refuse_on_the_host():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    with pytest.raises(ValueError, match="square"):
        F_hip.tta_views(torch.zeros(2, 1, 6, 10), "dihedral")  # (a CPU tensor: refused before any device work)
    with pytest.raises(ValueError, match="tta mode"):
        F_hip.tta_views(torch.zeros(2, 1, 6, 6), "rot90")
    with pytest.raises(ValueError, match="square"):
        O.views(torch.zeros(2, 1, 6, 10), "dihedral")
    m = torch.zeros(1, 4, 6, 10)
    with pytest.raises(ValueError, match="1, 2, 4 or 8"):
        F_hip.tta_merge([m, m, m], [0, 1, 2])
    with pytest.raises(ValueError, match="1, 2, 4 or 8"):
        F_hip.tta_merge([], [])
    with pytest.raises(ValueError, match="2 views and 1 ops"):
        F_hip.tta_merge([m, m], [0])
    with pytest.raises(ValueError, match="differ"):
        F_hip.tta_merge([m, torch.zeros(1, 4, 10, 6)], [0, 1])
    with pytest.raises(ValueError, match=r"\[0, 8\)"):
        F_hip.tta_merge([m, m], [0, 8])


# ---- the GPU kernel tests' inputs
@pytest.mark.parametrize("case", O.CASES, ids=[c[0] for c in O.CASES])
def test_gpu_inputs_keep_a_top_two_gap_at_every_pixel(case):
    gap = O.merge(O.case_logits(case), case[2])[4]
    print(f"{case[0]}: smallest top-two gap {gap:.3e}")
    assert gap >= O.GAP
