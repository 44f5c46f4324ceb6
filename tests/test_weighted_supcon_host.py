"""CPU-only: the float64 (P, E) restatement of SupConLoss2 / 3 / 4 (tests/_weighted_supcon_oracle.py) against the reference's
recorded results (tests/golden/g11_weighted_supcon.npz); the host side of the mirror ``contrastyou/losses/contrast_loss.py``
-- the reference's refusals with their types, the install alias, no CPU fallback -- and the four native entry points."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _weighted_supcon_oracle as O

SHAPES = [(3, 5), (6, 32), (33, 128)]


def _inputs(g, n, d):
    return {k: torch.tensor(g[f"n{n}_d{d}/{k}"]) for k in ("z1", "z2", "target", "mask", "pos_weight", "w11", "w22", "w12")}


def test_fixture_holds_the_issue_cases_and_the_seeded_inputs(golden):
    g = golden("g11_weighted_supcon.npz")
    want = [f"n{n}_d{d}/{s}/{m}" for n, d in SHAPES for s in O.SOURCES for m in ("out", "in")]
    assert sorted(g["cases"].tolist()) == sorted(want)
    for n, d in SHAPES:
        inp, fresh = _inputs(g, n, d), O.make_inputs(n, d)
        for k, v in inp.items():
            assert torch.equal(v, fresh[k]), k  # (the GPU tests regenerate inputs of other shapes the same way)
        m = inp["mask"].repeat(2, 2)
        m.fill_diagonal_(0)
        assert set(inp["mask"].unique().tolist()) <= {0.0, 0.5, 1.0} and bool(((m == 1).sum(1) >= 1).all())
        for k in ("pos_weight", "w11", "w22", "w12"):
            assert not torch.equal(inp[k], inp[k].t())


@pytest.mark.parametrize("n,d", SHAPES)
def test_restatement_matches_the_reference(golden, n, d):
    """the project's f32 bars (the recorded numbers are the reference's own float32): loss rtol 1e-4 / atol 1e-5, gradients
    rtol 1e-3 / atol 1e-5"""
    g = golden("g11_weighted_supcon.npz")
    inp = _inputs(g, n, d)
    for source in O.SOURCES:
        P, E = O.pe_of(source, inp)
        for out_mode in (True, False):
            key = f"n{n}_d{d}/{source}/{'out' if out_mode else 'in'}"
            loss, dz1, dz2 = O.loss_and_grads(inp["z1"], inp["z2"], P, E, out_mode=out_mode)
            np.testing.assert_allclose(float(loss), float(g[key + "/loss"]), rtol=1e-4, atol=1e-5, err_msg=key)
            np.testing.assert_allclose(dz1.numpy(), g[key + "/dz1"], rtol=1e-3, atol=1e-5, err_msg=key)
            np.testing.assert_allclose(dz2.numpy(), g[key + "/dz2"], rtol=1e-3, atol=1e-5, err_msg=key)


def test_single_pair_closed_forms():
    """n = 1: out mode is exactly 0; in mode is -mean_i(log(w_i) / w_i), w_i the row's single off-diagonal weight"""
    inp = O.make_inputs(1, 4)
    P, E = O.pe_blocks(1, inp["w11"], inp["w22"], inp["w12"])
    assert abs(float(O.criterion(inp["z1"], inp["z2"], P, E, out_mode=True))) < 1e-12
    w = inp["w12"].double().reshape(())
    np.testing.assert_allclose(float(O.criterion(inp["z1"], inp["z2"], P, E, out_mode=False)), float(-torch.log(w) / w),
                               rtol=1e-12)


def _unit(n, d):
    return torch.nn.functional.normalize(torch.randn(n, d), dim=1)


def test_host_side_refusals_keep_the_reference_types():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.contrast_loss import SupConLoss2, SupConLoss3, SupConLoss4
    z, w = _unit(4, 8), torch.rand(4, 4)
    with pytest.raises(RuntimeError, match="same time"):
        SupConLoss2()(z, z, target=[0, 1, 0, 1], mask=w)
    with pytest.raises(AssertionError):
        SupConLoss2()(z, _unit(5, 8))
    with pytest.raises(AssertionError):
        SupConLoss2()(z, z, mask=torch.rand(3, 4))
    with pytest.raises(AssertionError):
        SupConLoss3()(z, z)
    with pytest.raises(AssertionError):
        SupConLoss3()(z, z, pos_weight=torch.rand(4, 3))
    with pytest.raises(AssertionError):
        SupConLoss4()(proj_feat1=z, proj_feat2=z, one2one_weight=None, two2two_weight=None, one2two_weight=None)
    with pytest.raises(TypeError):
        SupConLoss4()(proj_feat1=z, proj_feat2=z, one2one_weight=None, two2two_weight=w, one2two_weight=w)
    with pytest.raises(TypeError):
        SupConLoss4()(z, z, two2two_weight=w)  # keyword-only, as the reference's signature


def test_product_path_has_no_cpu_fallback():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.contrast_loss import SupConLoss2, SupConLoss3, SupConLoss4
    z, w = _unit(4, 8), torch.rand(4, 4)
    for call in (lambda: SupConLoss2()(z, z, target=[0, 1, 0, 1]), lambda: SupConLoss2(out_mode=False)(z, z),
                 lambda: SupConLoss2()(z, z, mask=(w > 0.5).float()), lambda: SupConLoss3()(z, z, pos_weight=w),
                 lambda: SupConLoss4()(proj_feat1=z, proj_feat2=z, one2one_weight=w, two2two_weight=w, one2two_weight=w)):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()


def test_install_resolves_the_reference_style_import():
    import spcl_amd
    assert "contrastyou.losses.contrast_loss" in spcl_amd.install()
    from contrastyou.losses.contrast_loss import SupConLoss2 as SupConLoss1
    from contrastyou.losses.contrast_loss import SupConLoss3, SupConLoss4, exp_sim_temperature, is_normalized  # noqa: F401
    from spcl_amd.contrastyou.losses import contrast_loss
    assert SupConLoss1 is contrast_loss.SupConLoss2
    assert is_normalized(_unit(3, 5)) and not is_normalized(2 * _unit(3, 5))
    with SupConLoss3().register_writer(None, epoch=3, extra_tag="x"):  # yields, writes nothing
        pass


def test_native_table_lists_the_weighted_entry_points():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    assert native.ABI_VERSION >= 20
    names = ("spcl_supcon_weighted_workspace_bytes", "spcl_supcon_weighted_forward", "spcl_supcon_weighted_backward",
             "spcl_supcon_weighted_materialize")
    for name in names:
        assert name in native._SIGNATURES and hasattr(native.lib(), name)
    assert native._SIGNATURES[names[0]][0] is ctypes.c_size_t
    assert [len(native._SIGNATURES[k][1]) for k in names] == [2, 15, 10, 17]
    wb = lambda n, d: native.call(names[0], n, d)  # noqa: E731
    assert wb(32, 256) == (64 * 256 + 64) * 4          # one workgroup: the unit-gradient block + the taps' scratch
    # above: [2n, 2n] + six statistics rows + the backward's partial sums (the contraction in 2 parts / 1 part) + the taps' scratch
    assert wb(33, 128) == (66 * 66 + 7 * 66 + 2 * 66 * 128) * 4
    assert wb(32, 257) == (64 * 64 + 7 * 64 + 64 * 257) * 4
    assert wb(4096, 4096) > 0 and wb(4097, 8) == 0 and wb(8, 4097) == 0 and wb(0, 8) == 0


def test_argument_checks_report_minus_one_and_launch_nothing():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    L = native.lib()
    one = ctypes.c_void_p(16)  # (never dereferenced: every call below is refused before a launch)
    t = ctypes.c_float(0.07)

    def fwd(z1=one, labels=None, w11=None, blocks=0, n=4, d=8, temp=t):
        return L.spcl_supcon_weighted_forward(z1, one, labels, w11, None, None, blocks, 0, 0, n, d, temp, one, one, None)

    assert fwd(z1=None) == -1 and b"null" in L.spcl_last_error()
    assert fwd(n=5000) == -1 and b"n=5000" in L.spcl_last_error()
    assert fwd(temp=ctypes.c_float(0.0)) == -1
    assert fwd(blocks=1) == -1 and b"null block" in L.spcl_last_error()
    assert fwd(blocks=8) == -1
    assert fwd(labels=one, w11=one, blocks=1) == -1 and b"together" in L.spcl_last_error()
    assert L.spcl_supcon_weighted_backward(one, one, 4, 8, t, one, None, one, one, None) == -1
    assert L.spcl_supcon_weighted_materialize(one, one, None, None, None, None, 2, 0, 4, 8, t, one, None, None, None, None,
                                              None) == -1
