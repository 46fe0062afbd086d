"""The dedrift stage without a GPU: the literal restatement (tests/dedrift_literal.py) is established as a yardstick -- known answers for the warp,
the correction, the distortion maps and the statistics -- and the new bindings are checked to exist.  Bounds are the issue's: 1e-12 absolute for the
identity and the common-drift cases (measured 4.3e-14 .. 7.5e-14 on the radius-100 sphere), a mean angle below 0.02 degrees for the invariance to a
common drift at ico5 (measured 0.0019 degrees)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import dedrift_literal as L

NEW_SYMBOLS = ["msm_dedrift_create", "msm_dedrift_destroy", "msm_dedrift_reset", "msm_dedrift_accumulate", "msm_dedrift_finish", "msm_dedrift_correct",
               "msm_dedrift_set_map", "msm_dedrift_group_stats"]


def run_literal(template, subjects, data, **kw):
    from newmsm_amd import dedrift

    return dedrift.dedrift_group(L.LiteralOps(), template, subjects, data, **kw)


def test_bindings_exist(built):
    import newmsm_amd as M
    from newmsm_amd import _lib, dedrift

    lib = M.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.msm_abi_version() == 12
    for name in ("dedrift_group", "pairwise_stats", "ProductOps", "Dedrift", "format_stats", "distortion_summary"):
        assert hasattr(dedrift, name), name


def test_identity(built):
    xyz, tri = O.icosphere(3)
    S = 3
    subjects = [(xyz, xyz, tri)] * S
    data = [L.smooth_data(xyz, 2, s) for s in range(S)]
    got = run_literal((xyz, tri), subjects, data)
    errW = float(np.abs(got["W"] - xyz).max())
    errC = max(float(np.abs(c - xyz).max()) for c in got["corrected"])
    errJ = max(float(np.abs(d[0]).max()) for d in got["distortion"])
    errR = max(float(np.abs(d[1]).max()) for d in got["distortion"])
    print("identity: max|W - T| %.3g, max|corrected - R| %.3g, max|log2 J| %.3g, max|log2 R| %.3g" % (errW, errC, errJ, errR))
    assert errW <= 1e-12 and errC <= 1e-12 and errJ <= 1e-12
    # R = (I + sqrt(I^2 - 4)) / 2 at I = 2 + e is 1 + sqrt(e): corrected_s equals M_s to some 1e-16 relative, which leaves e at a few tens of ulps
    # (1e-14) and log2 R at sqrt(1e-14) / ln 2 = 1.5e-7 at most.  "Zero to rounding" for this row is therefore 1e-6, not 1e-12.
    assert errR <= 1e-6
    for s in range(S):  # a mesh resampled onto itself
        assert np.allclose(got["resampled"][s], data[s], rtol=0, atol=1e-12)


@pytest.mark.parametrize("order", [3, 4])
def test_common_drift_is_removed(built, order):
    xyz, tri = O.icosphere(order)
    S = 4
    reg = xyz @ L.Q_COMMON.T  # R_s = Q M_s for every subject, M_s = T
    subjects = [(xyz, reg, tri)] * S
    data = [L.smooth_data(xyz, 1, s) for s in range(S)]
    got = run_literal((xyz, tri), subjects, data)
    errW = float(np.abs(got["W"] - xyz @ L.Q_COMMON).max())  # Q^T T
    errC = max(float(np.abs(c - xyz).max()) for c in got["corrected"])
    print("common drift, ico%d: max|W - Q^T T| %.3g, max|corrected - M| %.3g" % (order, errW, errC))
    assert errW <= 1e-12 and errC <= 1e-12


def test_invariance_to_a_common_drift(built):
    """what dedrifting exists for: composing one rotation onto every registered sphere changes the corrected spheres only by interpolation error"""
    xyz, tri = O.icosphere(5)
    S = 4
    regs = [L.smooth_warp(xyz, s) for s in range(S)]
    data = [L.smooth_data(xyz, 1, s) for s in range(S)]
    a = run_literal((xyz, tri), [(xyz, r, tri) for r in regs], data)
    b = run_literal((xyz, tri), [(xyz, r @ L.Q_COMMON.T, tri) for r in regs], data)
    drift_deg = L.mean_angle_deg(a["drift"], xyz)[0]
    angles = [L.mean_angle_deg(ca, cb) for ca, cb in zip(a["corrected"], b["corrected"])]
    mean_deg, max_deg = float(np.mean([m for m, _ in angles])), max(m for _, m in angles)
    print("invariance, ico5: group drift %.3f deg; mean angle between the two runs %.5f deg, max %.5f deg" % (drift_deg, mean_deg, max_deg))
    assert mean_deg < 0.02


def test_distortion_of_one_triangle():
    o = np.array([[[10.0, 0.0, 99.0], [12.0, 1.0, 99.0], [10.5, 3.0, 99.0]]])
    d = np.array([0.6, 0.8, 0.0])  # a unit vector in the triangle's plane
    for k in (1.3, 2.0, 0.8):
        f = o + (k - 1.0) * (o @ d)[..., None] * d
        J, R = L.triangle_JR(o, f)
        assert J[0] == pytest.approx(k, rel=1e-12)
        assert R[0] == pytest.approx(max(k, 1.0 / k), rel=1e-9)  # R is the root of a difference of squares: half the digits near 1
    # a rigid motion: J = R = 1
    J, R = L.triangle_JR(o, o @ L.Q_COMMON.T)
    assert J[0] == pytest.approx(1.0, rel=1e-12) and R[0] == pytest.approx(1.0, abs=1e-6)


def test_distortion_of_a_uniform_scaling(built):
    xyz, tri = O.icosphere(2)
    k = 1.25
    dist = L.vertex_distortion(xyz, k * xyz, tri)
    assert np.allclose(dist[0], 2.0 * np.log2(k), rtol=0, atol=1e-12)
    assert np.allclose(dist[1], 0.0, rtol=0, atol=1e-6)


def test_statistics_against_numpy():
    rng = np.random.default_rng(5)
    S, D, V = 5, 2, 642
    base = rng.standard_normal((D, V))
    maps = [base + 0.5 * rng.standard_normal((D, V)) for _ in range(S)]
    mean, sd = L.moments(maps)
    assert np.allclose(mean, np.mean(maps, axis=0), rtol=1e-13, atol=0)
    assert np.allclose(sd, np.std(np.array(maps), axis=0, ddof=0), rtol=1e-12, atol=0)
    cc, dice = L.pair_matrices(maps, 75)
    for d in range(D):
        full = np.corrcoef(np.array([m[d] for m in maps]))
        assert np.allclose(cc[d], full, rtol=0, atol=1e-13)
        for i in range(S):
            for j in range(S):
                a, b = maps[i][d] > np.percentile(maps[i][d], 75), maps[j][d] > np.percentile(maps[j][d], 75)
                assert dice[d, i, j] == 2 * np.sum(a & b) / (np.sum(a) + np.sum(b))
    assert L.threshold_gaps(maps) > 0

    from newmsm_amd import dedrift

    want = [np.mean([cc[d][i, j] for i in range(S) for j in range(i + 1, S)]) for d in range(D)]
    assert np.allclose(dedrift.pair_means(cc), want, rtol=1e-14)
    dist = [rng.standard_normal((2, 100)) for _ in range(S)]
    summ = dedrift.distortion_summary(dist)
    areal = np.abs(np.concatenate([x[0] for x in dist]))
    assert summ["areal_95"] == np.percentile(areal, 95) and summ["areal_max"] == areal.max()
    text = dedrift.format_stats("g", ["Sulc", "Curv"], dedrift.pair_means(cc), dedrift.pair_means(dice), summ)
    assert "CC similarity: {:.4}; Dice overlap: {:.4}".format(float(dedrift.pair_means(cc)[0]), float(dedrift.pair_means(dice)[0])) in text
    assert "Areal mean: {:.4};".format(summ["areal_mean"]) in text
