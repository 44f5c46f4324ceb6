"""Self-paced SupCon on HIP against the oracle in FLOAT64 (same float32 inputs cast up, the oracle's own autograd) where
test_gpu_loss.py cannot see an error: age parameters that put the weights on both sides of their threshold at every
schedule, the padded rows of the fused large-batch sweeps, temperatures other than 0.07, labels=None and an explicit mask
at 2n >= 1024, d % 4 != 0 / d % 8 != 0 in the large-batch prep kernel, and the lazily materialised taps at size.

Inputs, age parameters and the schedule each shape is meant to hit: tests/_supcon_cases.py; that they qualify (weights on
both sides, no pair within twice the kernels' worst-case error of the hard threshold): tests/test_supcon_cases_host.py.

Tolerances (the project's, test_gpu_loss.py): loss rtol 1e-4 / atol 1e-5; gradients rtol 2e-3 / atol 2e-4 max|grad| -- one
wrongly weighted pair moves a gradient row by the order of max|grad| itself; rho in hard mode to 1e-6 relative (sum of
weights and number of positives are integers below 2^24, exact in float32: only the division rounds, a flipped pair is
>= 1 / 3840 relative); rho in soft mode rtol 1e-4."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _supcon_cases as C


def _crit(mode, gamma, t):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.contrast_loss3 import SupConLoss1, SelfPacedSupConLoss
    if mode == "supcon1":
        return SupConLoss1(temperature=t)
    soft = mode in ("soft", "soft_12_cg")
    c = SelfPacedSupConLoss(temperature=t, weight_update="soft" if soft else "hard", correct_grad=soft)
    c.set_gamma(gamma)
    return c


def _run(z1, z2, t, mode, gamma, labels=None, mask=None, gradient=None):
    """-> dict(loss, dz1, dz2, rho, crit) of one forward + backward on the GPU"""
    x, y = z1.cuda().requires_grad_(True), z2.cuda().requires_grad_(True)
    crit = _crit(mode, gamma, t)
    loss = crit(x, y, target=None if labels is None else list(labels), mask=None if mask is None else mask.cuda())
    assert loss.dim() == 0
    loss.backward() if gradient is None else loss.backward(gradient=torch.full((), gradient, device="cuda"))
    return {"loss": loss.item(), "dz1": x.grad.cpu(), "dz2": y.grad.cpu(), "crit": crit,
            "rho": None if mode == "supcon1" else crit.downgrade_ratio}


def _compare(got, ref, mode, tag):
    """the comparisons of section a; every figure is printed before it is asserted (pytest -s)"""
    scale = float(np.abs(ref["dz1"]).max())
    e1 = float(np.abs(got["dz1"].numpy() - ref["dz1"]).max()) / scale
    e2 = float(np.abs(got["dz2"].numpy() - ref["dz2"]).max()) / scale
    rho_err = 0.0 if got["rho"] is None else abs(got["rho"] - ref["rho"]) / ref["rho"]
    print(f"\n[supcon parity] {tag} {mode}: loss {got['loss']:.7f} ref {ref['loss']:.7f} rel {abs(got['loss'] - ref['loss']) / abs(ref['loss']):.2e}"
          f" | grad err / max|grad| {max(e1, e2):.2e} | rho {got['rho']} ref {ref['rho']} rel {rho_err:.2e}")
    assert torch.isfinite(got["dz1"]).all() and torch.isfinite(got["dz2"]).all(), tag
    np.testing.assert_allclose(got["loss"], ref["loss"], rtol=1e-4, atol=1e-5, err_msg=tag)
    if mode == "hard":
        assert rho_err <= 1e-6, (tag, got["rho"], ref["rho"])
    elif mode != "supcon1":
        np.testing.assert_allclose(got["rho"], ref["rho"], rtol=1e-4, err_msg=tag)
    np.testing.assert_allclose(got["dz1"].numpy(), ref["dz1"], rtol=2e-3, atol=2e-4 * scale, err_msg=tag)
    np.testing.assert_allclose(got["dz2"].numpy(), ref["dz2"], rtol=2e-3, atol=2e-4 * scale, err_msg=tag)


# ------------------------------------------------------------------------------------------ a. thresholds on both sides
@pytest.mark.parametrize("mode", ["hard", "soft"])
@pytest.mark.parametrize("t", C.TEMPERATURES)
@pytest.mark.parametrize("n,d", C.CASES)
def test_thresholds_on_both_sides(n, d, t, mode):
    """every schedule, clustered inputs, hard rule at the mid-gap age parameter (rho 0.3 .. 0.7: the kept set must be the
    oracle's, pair for pair) and soft rule at the median (half of the positives at the clip), correct_grad"""
    z1, z2, labels = C.clustered(n, d)
    ref, gamma, _ = C.reference("clustered", n, d, t, mode)
    got = _run(z1, z2, t, mode, gamma, labels)
    _compare(got, ref, mode, f"({n}, {d}) t={t} [{C.SCHEDULES[(n, d)]}]")


@pytest.mark.parametrize("n,d", [(577, 128), (520, 64)])  # fused sweeps / materialised logits
def test_half_upstream_gradient_is_exactly_half(n, d):
    z1, z2, labels = C.clustered(n, d)
    gamma = C.gammas("clustered", n, d, 0.07)[0]
    full = _run(z1, z2, 0.07, "hard", gamma, labels)
    half = _run(z1, z2, 0.07, "hard", gamma, labels, gradient=0.5)
    assert full["loss"] == half["loss"]
    assert torch.equal(half["dz1"], full["dz1"] * 0.5) and torch.equal(half["dz2"], full["dz2"] * 0.5)


# --------------------------------------------------------------------------------------- b. padding of the fused sweeps
@pytest.mark.parametrize("mode", ["supcon1", "soft_12_cg"])
@pytest.mark.parametrize("t", C.TEMPERATURES)
@pytest.mark.parametrize("n,d", [(576, 128), (577, 128), (608, 64), (639, 100)])
def test_padded_rows_of_the_fused_sweeps(n, d, t, mode):
    """isotropic rows keep D_i small: 126 padded columns counted by mistake move it by ~8 % at t = 0.07 and by far more at
    t = 0.5.  (576, 128) is the unpadded neighbour (2n = 1152: logits materialised) -- both sides of the switch on record."""
    z1, z2 = C.isotropic(n, d)
    labels = tuple(i % 5 for i in range(n))
    ref, gamma, _ = C.reference("isotropic", n, d, t, mode, nlab_iso=5)
    got = _run(z1, z2, t, mode, gamma, labels)
    _compare(got, ref, mode, f"isotropic ({n}, {d}) t={t}")


# -------------------------------------------------------------------------------------- c. labels=None at large sizes
@pytest.mark.parametrize("t", C.TEMPERATURES)
@pytest.mark.parametrize("kind", ["isotropic", "paired"])
@pytest.mark.parametrize("n,d", C.LABEL_FREE_SHAPES)
def test_simclr_positives_at_large_sizes(n, d, kind, t):
    z1, z2, _ = C.inputs(kind, n, d)
    ref, _, _ = C.reference(kind, n, d, t, "supcon1", labelled=False)
    _compare(_run(z1, z2, t, "supcon1", None), ref, "supcon1", f"labels=None {kind} ({n}, {d}) t={t}")


@pytest.mark.parametrize("kind,n,d,t", C.LABEL_FREE_HARD)
def test_simclr_positives_hard_rule(kind, n, d, t):
    z1, z2, _ = C.inputs(kind, n, d)
    ref, gamma, _ = C.reference(kind, n, d, t, "hard", labelled=False)
    _compare(_run(z1, z2, t, "hard", gamma), ref, "hard", f"labels=None {kind} ({n}, {d}) t={t}")


# ------------------------------------------------------------------------------------------------- d. explicit mask
@pytest.mark.parametrize("mode", ["hard", "soft"])
@pytest.mark.parametrize("t", C.TEMPERATURES)
@pytest.mark.parametrize("n,d", [(520, 64), (33, 100)])
def test_explicit_mask(n, d, t, mode):
    """mask = the label-equality matrix: at 2n = 1040 the exact-f32 sweeps with 128-row padding, while the same positives
    given as labels take the split-bf16 schedule -- both against the float64 oracle, and against each other"""
    z1, z2, labels = C.clustered(n, d)
    mask = C.label_mask(labels)
    ref, gamma, _ = C.reference("clustered", n, d, t, mode, use_mask=True)
    assert gamma == C.reference("clustered", n, d, t, mode)[1]  # (the same positives: the same age parameter)
    by_mask = _run(z1, z2, t, mode, gamma, mask=mask)
    _compare(by_mask, ref, mode, f"mask ({n}, {d}) t={t}")
    by_labels = _run(z1, z2, t, mode, gamma, labels)
    as_ref = {"loss": by_labels["loss"], "rho": by_labels["rho"], "dz1": by_labels["dz1"].numpy(),
              "dz2": by_labels["dz2"].numpy()}
    _compare(by_mask, as_ref, mode, f"mask against labels ({n}, {d}) t={t}")


# ---------------------------------------------------------------------------- e. temperature on the remaining schedules
@pytest.mark.parametrize("n,d", [(17, 40), (33, 100), (40, 300), (513, 128), (520, 64), (520, 200), (639, 100)])
def test_temperature_one(n, d):
    """t = 1.0 (the IIC configs of the reference), SupConLoss1, one shape per schedule"""
    z1, z2, labels = C.clustered(n, d)
    ref, _, _ = C.reference("clustered", n, d, 1.0, "supcon1")
    _compare(_run(z1, z2, 1.0, "supcon1", None, labels), ref, "supcon1", f"({n}, {d}) t=1.0 [{C.SCHEDULES[(n, d)]}]")


def test_temperature_one_simclr_fused():
    """the fused path's counterpart of the small-batch KAT (orthonormal rows do not fit n = 640): SimCLR positives on
    paired clusters, d = 64, t = 1.0, against float64"""
    z1, z2, _ = C.inputs("paired", 640, 64)
    ref, _, _ = C.reference("paired", 640, 64, 1.0, "supcon1", labelled=False)
    _compare(_run(z1, z2, 1.0, "supcon1", None), ref, "supcon1", "labels=None paired (640, 64) t=1.0")


# ---------------------------------------------------------------------------------------------------- f. taps at size
def test_taps_at_size():
    """(577, 128), hard rule: the tap kernel computes in exact f32, the forward ran split-bf16 -- the gap around the age
    parameter (test_supcon_cases_host.py) is what makes their weights agree pair for pair"""
    n, d, t = 577, 128, 0.07
    z1, z2, labels = C.clustered(n, d)
    ref, gamma, _ = C.reference("clustered", n, d, t, "hard")
    crit = _run(z1, z2, t, "hard", gamma, labels)["crit"]
    pos = ref["pos"] > 0
    sp_mask = crit.sp_mask.cpu().numpy()
    assert sp_mask.shape == (2 * n, 2 * n)
    np.testing.assert_array_equal(crit.pos_mask.cpu().numpy(), ref["pos"])
    np.testing.assert_array_equal(sp_mask[pos], ref["w"][pos])
    err = float(np.abs(crit.sim_logits.cpu().numpy() - ref["sim_logits"]).max())
    print(f"\n[supcon parity] taps ({n}, {d}): max |sim_logits - float64| {err:.2e}")
    assert err <= 2e-5
    rho_tap = float(sp_mask[pos].astype(np.float64).mean())
    assert abs(rho_tap - crit.downgrade_ratio) <= 1e-6 * rho_tap, (rho_tap, crit.downgrade_ratio)
