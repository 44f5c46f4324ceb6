"""CPU-only side of the largest-connected-component step: the oracle of tests/_lcc_oracle.py on hand-made known answers, the C
ABI's two entry points (header, signature table, argument checks: nothing is launched), and the host-side refusals of the
binding and of ``InferenceEpocher(postprocess=...)``."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _lcc_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "spcl_hip.h")


def _map(rows):
    return np.array([[int(ch) for ch in r] for r in rows], np.int64)


# ---- the oracle
def test_oracle_diagonal_contact_does_not_connect():
    m = _map(["1100000",
              "1100000",
              "0011100",
              "0011100",
              "0000000"])
    out, kept, ncomp = O.largest_components(m[None], 2)
    assert ncomp.tolist() == [[2]] and kept.tolist() == [[6]]
    assert np.array_equal(out[0], _map(["0000000", "0000000", "0011100", "0011100", "0000000"]))


def test_oracle_tie_keeps_the_blob_that_starts_first_in_raster_order():
    m = _map(["0000110",
              "0000110",
              "1100000",
              "1100000",
              "0000000"])
    out, kept, ncomp = O.largest_components(m[None], 2)
    assert ncomp.tolist() == [[2]] and kept.tolist() == [[4]]
    assert np.array_equal(out[0], _map(["0000110", "0000110", "0000000", "0000000", "0000000"]))
    # the one that starts first by (y, x), not by x: the left blob begins in a later row
    assert out[0][2, 0] == 0


def test_oracle_z_only_bridge_joins_two_slices():
    v = np.zeros((2, 4, 6), np.int64)
    v[0, 0:2, 0:2] = 1  # 4 voxels
    v[1, 1:4, 1:5] = 1  # 12 voxels; (0, 1, 1) and (1, 1, 1) touch along z only
    v[0, 3, 5] = 1      # an island
    out, kept, ncomp = O.largest_components(v, 2, volumetric=True)
    assert kept.tolist() == [[16]] and ncomp.tolist() == [[2]] and out[0, 3, 5] == 0 and out.sum() == 16
    out, kept, ncomp = O.largest_components(v, 2, volumetric=False)  # each slice on its own
    assert kept.tolist() == [[4], [12]] and ncomp.tolist() == [[2], [1]] and out.sum() == 16 and out[0, 3, 5] == 0
    # other classes and unlisted labels are left alone
    v[1, 0, 5] = 3
    out, kept, ncomp = O.largest_components(v, 4, classes=[1], volumetric=True)
    assert out[1, 0, 5] == 3 and kept.tolist() == [[16]]
    assert O.removed_fraction(v, out) == 1 / 18


def test_oracle_serpentine_is_one_long_and_one_short_snake():
    m = O.serpentine(33, 65)
    out, kept, ncomp = O.largest_components(m, 2)
    assert ncomp.tolist() == [[2]] and m.shape == (1, 1, 33, 65)
    assert kept[0, 0] > (m != 0).sum() // 2 and (out != 0).sum() == kept[0, 0] and out[0, 0, 0, 0] == 0 and out[0, 0, 32, 64] == 1


# ---- the C ABI
def test_header_and_native_agree_on_the_entry():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    hdr = open(HEADER).read()
    assert int(re.search(r"#define\s+SPCL_ABI_VERSION\s+(\d+)", hdr).group(1)) == native.ABI_VERSION >= 27
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "size_t spcl_largest_component_workspace_bytes(int V, int D, int H, int W, int n_classes);" in flat
    assert ("int spcl_largest_component(const int64_t* labels, int V, int D, int H, int W, int C, const int* classes, "
            "int n_classes, int64_t* out, int64_t* kept_size, int32_t* n_components, void* ws, size_t ws_bytes, "
            "void* stream);") in flat
    res, args = native._SIGNATURES["spcl_largest_component_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_int] * 5
    res, args = native._SIGNATURES["spcl_largest_component"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert res is I and args == [P, I, I, I, I, I, P, I, P, P, P, P, ctypes.c_size_t, P]
    assert all(hasattr(native.lib(), n) for n in ("spcl_largest_component_workspace_bytes", "spcl_largest_component"))
    assert native.call("spcl_abi_version") >= 27


def test_argument_checks_report_minus_one_and_launch_nothing():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    L = native.lib()
    ws_bytes = L.spcl_largest_component_workspace_bytes
    n = 10 * 224 * 224
    assert ws_bytes(1, 10, 224, 224, 3) >= 4 * n  # at least the parent array
    assert ws_bytes(1, 2048, 1024, 1024, 1) == 0 and ws_bytes(1, 8, 8, 8, 0) == 0 and ws_bytes(1, 8, 8, 8, 16) == 0
    assert ws_bytes(0, 8, 8, 8, 1) == 0 and ws_bytes(1, 8, 0, 8, 1) == 0

    def rc(V, D, H, W, C, classes, labels=None, out=None, rest=None, ws=None, nbytes=0):
        arr = (ctypes.c_int * max(len(classes), 1))(*classes) if classes is not None else None
        code = L.spcl_largest_component(labels, V, D, H, W, C, arr, len(classes) if classes is not None else 1, out, rest, rest,
                                        ws, nbytes, None)
        return code, L.spcl_last_error().decode()

    for shape in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 0)):
        code, msg = rc(*shape, 4, [1])
        assert code == -1 and "bad shape" in msg, shape
    code, msg = rc(1, 2048, 1024, 1024, 4, [1])  # D H W = 2^31
    assert code == -1 and "2^31" in msg
    code, msg = rc(1, 8, 8, 8, 1, [1])
    assert code == -1 and "two classes" in msg
    code, msg = rc(1, 8, 8, 8, 4, [])
    assert code == -1 and "listed classes" in msg
    code, msg = rc(1, 8, 8, 8, 20, list(range(1, 17)))
    assert code == -1 and "listed classes" in msg
    code, msg = rc(1, 8, 8, 8, 4, None)
    assert code == -1 and "listed classes" in msg
    code, msg = rc(1, 8, 8, 8, 4, [0])
    assert code == -1 and "class 0 is not in [1, 4)" in msg
    code, msg = rc(1, 8, 8, 8, 4, [1, 4])
    assert code == -1 and "class 4 is not in [1, 4)" in msg
    code, msg = rc(1, 8, 8, 8, 4, [2, 1, 2])
    assert code == -1 and "class 2 is listed twice" in msg
    code, msg = rc(1, 8, 8, 8, 4, [1, 2, 3])  # every value check passed: only the pointers are missing
    assert code == -1 and "null pointer" in msg
    # host buffers stand in for device memory: every one of these calls is refused before a launch
    n = 8 * 8 * 8
    lab, out = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
    rest, ws = (ctypes.c_int64 * 8)(), ctypes.create_string_buffer(1 << 16)
    p = lambda b: ctypes.cast(b, ctypes.c_void_p)  # noqa: E731
    code, msg = rc(1, 8, 8, 8, 4, [1], p(lab), p(lab), p(rest), p(ws), 1 << 16)
    assert code == -1 and "alias" in msg
    half = ctypes.c_void_p(ctypes.addressof(lab) + 8 * (n // 2))  # overlaps the second half of `labels`
    code, msg = rc(1, 8, 8, 8, 4, [1], p(lab), half, p(rest), p(ws), 1 << 16)
    assert code == -1 and "alias" in msg
    need = ws_bytes(1, 8, 8, 8, 1)
    code, msg = rc(1, 8, 8, 8, 4, [1], p(lab), p(out), p(rest), p(ws), need - 1)
    assert code == -1 and "workspace" in msg and str(need) in msg


# ---- the binding and the epocher
def test_binding_refuses_on_the_host():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    vol = torch.zeros(3, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.largest_components(vol, 4)
    with pytest.raises(TypeError, match="class-coded integer"):
        F_hip.largest_components(vol.float(), 4)
    with pytest.raises(TypeError, match="class-coded integer"):
        F_hip.largest_components(vol[0], 4)
    sig = inspect.signature(F_hip.largest_components).parameters
    assert list(sig) == ["labels", "num_classes", "classes", "volumetric", "out"]
    assert sig["classes"].default is None and sig["volumetric"].default is True and sig["out"].default is None


def test_inference_epocher_postprocess_argument():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.contrastyou.meters import AverageValueMeter, SurfaceMeter, UniversalDice, VolumeSurfaceMeter
    from spcl_amd.semi_seg.epochers import InferenceEpocher
    from spcl_amd.semi_seg.epochers.helper import write_predict
    from spcl_amd.semi_seg.trainers import FineTuneTrainer

    class _Net(torch.nn.Module):
        num_classes = 4

    def build(**kw):
        ep = InferenceEpocher(model=_Net(), loader=[], sup_criterion=KL_div(verbose=False), device="cpu", **kw)
        return ep, list(ep.meters._groups["eval"])

    for bad in ("x", "largest", True, 1):
        with pytest.raises(ValueError, match="postprocess"):
            build(postprocess=bad)
    assert build()[1] == build(postprocess=None)[1] == ["loss", "dice", "hd"]
    ep, names = build(postprocess="largest_component")
    assert names == ["loss", "dice", "hd", "dice_lcc", "hd_lcc", "lcc_removed"]
    with ep.meters.focus_on("eval"):
        assert [type(ep.meters[k]) for k in names[3:]] == [UniversalDice, SurfaceMeter, AverageValueMeter]
        assert ep.meters["dice_lcc"]._report_axis == [1, 2, 3] and ep.meters["hd_lcc"]._report_axis == [1, 2, 3]
    ep, names = build(postprocess="largest_component", volumetric=True)
    assert names == ["loss", "dice", "hd", "hd3d", "mhd3d", "asd3d", "dice_lcc", "hd_lcc", "hd3d_lcc", "mhd3d_lcc", "asd3d_lcc",
                     "lcc_removed"]
    with ep.meters.focus_on("eval"):
        assert [type(ep.meters[k]) for k in names[8:11]] == [VolumeSurfaceMeter] * 3
    sig = inspect.signature(FineTuneTrainer.inference).parameters
    assert sig["postprocess"].default is None and sig["postprocess"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(write_predict).parameters["folder"].default == "pred"
