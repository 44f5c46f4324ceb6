"""The inputs of tests/test_gpu_supcon_structured.py qualify (CPU, float64 oracle alone; no kernel runs here): the age
parameters derived from them put the self-paced weights on BOTH sides of their threshold, and no positive pair lies closer to
the hard threshold than twice the kernels' worst-case error of ell.  A new shape or seed in tests/_supcon_cases.py that does
not qualify fails here -- change the case, not these conditions."""
import numpy as np
import pytest

from tests import _supcon_cases as C

# (kind, n, d, labelled, t): the table's cases on clustered inputs, and the label-free ones of the GPU file
INPUTS = [("clustered", n, d, True, t) for n, d in C.CASES for t in C.TEMPERATURES] + \
         [(kind, n, d, False, t) for kind, n, d, t in C.LABEL_FREE_HARD]


def test_the_table_names_the_schedule_the_dispatch_takes():
    """supcon_layout / supcon_use_small / _big / _fused of csrc/supcon.hip, restated: which rows are padded, which path"""
    for (n, d), name in C.SCHEDULES.items():
        n2 = 2 * n
        wide, big = d > 256, 2 * n >= 1024 and d <= 256
        n2p = -(-n2 // (128 if big else 64)) * (128 if big else 64)
        dp = 64 if d <= 64 else 128 if d <= 128 else 256 if d <= 256 else -(-d // 256) * 256
        if wide:
            got = "wide"
        elif not big:
            got = "one-workgroup" if n2p == 64 else "exact sweeps"
        elif dp <= 128 and n2p % 256 == 0:
            got = "fused"
        else:
            got = ("DP = 256" if dp == 256 else "logits v1") + (" + vector row pass" if n % 4 == 0 else " + scalar row pass")
        assert name.startswith(got), ((n, d), name, got)
        assert C.split_bf16(n, d) == big
    pad = {nd: -(-2 * nd[0] // 128) * 128 - 2 * nd[0] for nd in ((577, 128), (608, 64), (639, 100), (640, 37))}
    assert pad == {(577, 128): 126, (608, 64): 64, (639, 100): 2, (640, 37): 0}


@pytest.mark.parametrize("kind,n,d,labelled,t", INPUTS)
def test_thresholds_split_the_positives_with_a_margin(kind, n, d, labelled, t):
    z1, z2, labels = C.inputs(kind, n, d)
    l = C.neg_ell64(z1, z2, labels if labelled else None, t=t)  # (asserts that every row has a positive)
    assert np.isfinite(l).all() and l.size >= 2 * n
    g_hard, half, g_soft = C.gammas(kind, n, d, t, labelled)
    bound = C.ell_bound(t, split_bf16=True)
    print(f"{kind} ({n}, {d}) t={t}: half-gap {half:.3e} = {half / bound:.1f} x bound, gamma hard {g_hard:.4f} soft {g_soft:.4f}")
    assert half >= 2 * bound, (half, bound)
    assert np.abs(l - g_hard).min() >= 2 * bound
    hard, _, _ = C.reference(kind, n, d, t, "hard", labelled)
    assert 0.2 < hard["rho"] < 0.8, hard["rho"]
    assert hard["rho"] == pytest.approx(float((l <= g_hard).mean()), abs=1e-12)
    soft, _, _ = C.reference(kind, n, d, t, "soft", labelled)
    pos = soft["pos"] > 0
    zero = float((soft["w"][pos] == 0).mean())
    assert 0.2 < zero < 0.8, zero
    assert (soft["pos"].sum(1) >= 1).all()


def test_helpers():
    l = np.array([0.0, 1.0, 2.0, 3.0, 3.5, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0])
    g, half = C.hard_gamma(l)  # quantile range = indices 3 .. 7: the widest gap there is 3.5 -> 6
    assert (g, half) == (4.75, 1.25)
    assert C.soft_gamma(l) == 6.0
    assert C.ell_bound(0.07, True) == 6 * 2.0 ** -18 / 0.07 and C.ell_bound(0.5, False) == 6 * 2.0 ** -22 / 0.5
    z1, z2, labels = C.clustered(17, 40)
    assert z1.dtype.is_floating_point and z1.shape == (17, 40) and labels == tuple(i % 9 for i in range(17))
    np.testing.assert_allclose(z1.norm(dim=1).numpy(), 1.0, atol=1e-6)
    assert C.clustered(17, 40, nlab=17)[2] == tuple(range(17))
    a, b = C.isotropic(17, 40)
    np.testing.assert_allclose(b.norm(dim=1).numpy(), 1.0, atol=1e-6)
