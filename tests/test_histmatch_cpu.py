"""--IN / --INc (histogram matching) without a GPU: properties of the literal restatement (tests/histmatch_literal.py), the two configuration front
ends, and the level loops of newmsm_amd/registration.py / group_registration.py driven by the oracle's ops with the literal as their matching.
tests/test_gpu_histmatch.py holds the MI355X path against the same literal."""
import json
import os
import subprocess

import numpy as np
import pytest

import histmatch_literal as HL
import trans_excl_cases as C
from newmsm_amd import config, group_registration, registration
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "histmatch_config.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "histmatch_config")
LIBDIR = os.path.join(ROOT, "newmsm_amd")
BASE = "--opt=DISCRETE,DISCRETE\n--lambda=0.1,0.2\n--regoption=3\n--sigma_in=3,1\n--dopt=HOCR\n"


# ---------------------------------------------------------------- the literal
def _rows(seed=0, n=3000):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=n)
    y = rng.gamma(2.0, 1.5, size=n // 2) + 3.0
    return x, y


def _match_with_mask(seed, n_src, n_ref):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=n_src)
    y = rng.gamma(2.0, 1.5, size=n_ref) + 3.0
    mx = (rng.random(x.size) > 0.3).astype(float)
    x[5], x[6], mx[7] = np.nan, np.inf, 0.0
    out, t = HL.match_row(x, mx, y, np.ones(y.size))
    return x, y, np.isfinite(x) & (mx > 0), out, t


def test_rank_preserving_bounded_and_at_most_256_values():
    """A target whose top bin holds no larger share of its values than the source's top bin (one value of 6 000 against one of about 1 000): the case
    in which the definition keeps the ranks of all counted values -- see the next test for the other case"""
    x, y, counted, out, t = _match_with_mask(0, 1500, 6000)
    assert t is not None and np.all(np.diff(t[:-1]) >= 0)
    order = np.argsort(x[counted], kind="stable")
    assert np.all(np.diff(out[counted][order]) >= 0)                       # ranks are kept over the counted values
    assert np.array_equal(out[~counted], x[~counted], equal_nan=True)      # uncounted and non-finite values untouched
    assert not np.array_equal(out[counted], x[counted])
    assert len(np.unique(out[counted])) <= HL.B
    assert out[counted].min() >= y.min() and out[counted].max() <= y.max()


def test_the_top_bin_is_the_one_exception_to_rank_preservation():
    """Step 4 gives source bin B the bottom of target bin B (newbin = B, dist = 0: lo_y + (B - 1) w_y), whatever the CDFs say; a lower source bin whose
    CDF value lies inside target bin B lands above that.  It happens when the target's top bin holds a larger share of its values than the source's
    (here one of 1 500 against one of 2 087; measured: t[B - 1] lies 0.016 above t[B], 0.28 of the target's bin width).  The definition is the
    contract and is pinned as it stands: ranks are kept over bins 1 .. B - 1 always, and over all bins in the case of the test above."""
    x, y, counted, out, t = _match_with_mask(0, 3000, 1500)
    w_y = (y.max() - y.min()) / HL.B
    assert np.all(np.diff(t[:-1]) >= 0) and t[-1] == y.min() + (HL.B - 1) * w_y
    assert 0.0 < t[-2] - t[-1] < w_y                                       # the exception, bounded by one target bin
    below_top = counted & (x < x[counted].max())
    order = np.argsort(x[below_top], kind="stable")
    assert np.all(np.diff(out[below_top][order]) >= 0)
    assert len(np.unique(out[counted])) <= HL.B and out[counted].min() >= y.min() and out[counted].max() <= y.max()


def test_rows_that_are_left_unchanged():
    x, y = _rows(2)
    ones_x, ones_y = np.ones(x.size), np.ones(y.size)
    for xs, mxs, ys, mys in ((np.full(x.size, 2.5), ones_x, y, ones_y),    # constant row
                             (x, np.zeros(x.size), y, ones_y),             # all masked
                             (x, ones_x, y, np.zeros(y.size)),             # the target all masked
                             (x, ones_x, np.full(y.size, -1.0), ones_y),   # constant target row
                             (np.full(x.size, np.nan), ones_x, y, ones_y)):
        out, t = HL.match_row(xs, mxs, ys, mys)
        assert t is None and np.array_equal(out, xs, equal_nan=True)


def test_mask_rows_follow_the_feature_row_when_there_are_enough():
    rng = np.random.default_rng(3)
    src, ref = rng.normal(size=(3, 500)), rng.normal(size=(3, 400)) * 2.0 + 1.0
    m3, m1 = (rng.random((3, 500)) > 0.4).astype(float), (rng.random(500) > 0.4).astype(float)
    a, b = HL.histogram_match(src, ref, m3), HL.histogram_match(src, ref, m1)
    for d in range(3):
        assert np.array_equal(a[d], HL.match_row(src[d], m3[d], ref[d], np.ones(400))[0])
        assert np.array_equal(b[d], HL.match_row(src[d], m1, ref[d], np.ones(400))[0])
    two = HL.histogram_match(src, ref, m3[:2])  # two rows for three features: the third falls back to row 0 (M/reg_tools.cpp:764-767)
    assert np.array_equal(two[2], HL.match_row(src[2], m3[0], ref[2], np.ones(400))[0])


@pytest.mark.parametrize("n_src,n_ref,seed", [(2562, 2562, 11), (642, 10242, 12)])
def test_percentiles_land_within_three_target_bins(n_src, n_ref, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=n_src)
    y = rng.gamma(2.0, 2.0, size=n_ref) - 1.5
    out = HL.histogram_match(x[None], y[None])[0]
    w_y = (y.max() - y.min()) / HL.B
    q = [5, 25, 50, 75, 95]
    worst = np.abs(np.percentile(out, q) - np.percentile(y, q)).max() / w_y
    print("worst percentile distance: %.2f target bin widths" % worst)
    assert worst <= 3.0


# ---------------------------------------------------------------- front ends
@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as g

    g.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE, "-L", LIBDIR, "-lmsmhip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def cpp(exe, tmp_path, text, optin, groupwise=False):
    path = tmp_path / "conf"
    path.write_text(text)
    out = subprocess.run([exe, str(path), "2", "1" if optin else "0"] + (["groupwise"] if groupwise else []), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("groupwise", [False, True])
@pytest.mark.parametrize("flags,intensity,cut,excl", [("--IN\n", True, False, False), ("--INc\n", True, True, False), ("--excl\n--IN\n", True, False, True),
                                                      ("--IN\n--INc\n--VN\n", True, True, False), ("", False, False, False)])
def test_opt_in_carries_intensity_and_cut_in_python_and_cpp(exe, tmp_path, flags, intensity, cut, excl, groupwise):
    cfg = config.parse_config(BASE + flags)
    levels, run_kw, _ = config.levels_from_config(cfg, 2, groupwise=groupwise, histmatch=True)
    assert run_kw == dict(varnorm="--VN" in flags, intensity=intensity, cut=cut) and config.run_options(cfg)["excl"] == excl
    got = cpp(exe, tmp_path, BASE + flags, True, groupwise)
    assert got == dict(levels=len(levels), varnorm="--VN" in flags, intensity=intensity, cut=cut, excl=excl)


@pytest.mark.parametrize("flags", ["--IN\n", "--INc\n", "--excl\n--IN\n"])
def test_without_the_opt_in_the_refusal_stands(exe, tmp_path, flags):
    for groupwise in (False, True):
        with pytest.raises(config.ConfigError, match="--IN / --INc .* is not available"):
            config.levels_from_config(config.parse_config(BASE + flags), 2, groupwise=groupwise)
        assert "--IN / --INc" in cpp(exe, tmp_path, BASE + flags, False, groupwise)["error"]
    assert config.levels_from_config(config.parse_config(BASE), 2)[1] == dict(varnorm=False)  # and nothing new is returned without it


# ---------------------------------------------------------------- the level loops over the oracle's ops, with the literal as their matching
class Captured(Exception):
    """the features a level hands to its model: the loop is stopped there"""

    def __init__(self, feats):
        self.feats = feats


class _StubGroup:
    def __init__(self, S):
        self.S, self.feats = S, {}

    def set_template(self, *a):
        pass

    def initialize(self, *a):
        pass

    def set_subject(self, s, mesh, feat):
        self.feats[s] = np.array(feat)
        if len(self.feats) == self.S:
            raise Captured([self.feats[k] for k in range(self.S)])


class RecordingOps(HL.LiteralMatchMixin, C.MaskOracleOps):
    """the oracle's ops + the literal's matching; logs the feature-preparation calls and stops a level where its model takes the features"""

    def __init__(self):
        import newmsm_amd as M

        super().__init__(M.mcmc_optimise)
        self.log = []

    def create_exclusion(self, *a):
        self.log.append("create_exclusion")
        return super().create_exclusion(*a)

    def metric_resample(self, *a, **k):
        self.log.append("metric_resample" + ("+mask" if k.get("excl") is not None else ""))
        return super().metric_resample(*a, **k)

    def smooth_data(self, *a, **k):
        self.log.append("smooth_data" + ("+mask" if k.get("excl") is not None else ""))
        return super().smooth_data(*a, **k)

    def histogram_match(self, *a, **k):
        self.log.append("histogram_match")
        return super().histogram_match(*a, **k)

    def variance_normalise(self, *a, **k):
        self.log.append("variance_normalise" + ("+mask" if k.get("excl") is not None else ""))
        return super().variance_normalise(*a, **k)

    def cost(self, kind, simmeasure, rmode, params, target, source, cpgrid, src_feat):
        raise Captured([np.array(src_feat), np.array(target.feat)])

    def rigid_level(self, target_xyz, target_tri, ref_feat, source_xyz, source_tri, src_feat, *a):
        raise Captured([np.array(src_feat), np.array(ref_feat)])

    def group(self, S, *a, **k):
        return _StubGroup(S)


LEVEL = dict(data_order=2, cp_order=1, sigma_in=20.0, sigma_ref=15.0, iters=1, mciters=10)
RIGID = dict(method="RIGID", data_order=2, sigma_in=20.0, sigma_ref=15.0, iters=1, simmeasure=1, stepsize=C.F32_001, gradsampling=0.5)


@pytest.fixture(scope="module")
def case():
    return C.pairwise_case(order=3, D=2, cap=True)  # an irregular ico3 sphere, both data sets exactly 0 on a cap


def prepared(native, data, ico, sigma, masked):
    """one data set resampled and smoothed by the oracle, call by call"""
    if not masked:
        f = O.metric_resample(native, data, ico)
        return (O.smooth_data(ico, f, ico, sigma) if sigma > 0.0 else f), None
    mask = O.create_exclusion(data, *C.CUTTHR)
    f, mask = O.metric_resample_excl(native, data, ico, mask)
    if sigma > 0.0:
        f, mask = O.smooth_data(ico, f, ico, sigma, excl=mask)
    return f, mask


def normalised(f, m):
    return O.variance_normalise(f) if m is None else O.variance_normalise(f, excl=m)


def first_level_features(ops, case, lv, **kw):
    with pytest.raises(Captured) as e:
        C.run(ops, case, [lv], **kw)
    return e.value.feats


@pytest.mark.parametrize("lv", [LEVEL, RIGID], ids=["discrete", "rigid"])
@pytest.mark.parametrize("excl,cut", [(False, False), (True, False), (False, True)], ids=["IN", "excl_IN", "INc"])
def test_pairwise_level_matches_reference_to_input_between_smoothing_and_normalising(case, lv, excl, cut):
    xyz, tri, src, ref, _ = case
    ops = RecordingOps()
    got = first_level_features(ops, case, lv, excl=excl, cutthr=C.CUTTHR, intensity=True, cut=cut)
    masked = excl or cut  # M/featurespace.cpp:61: --INc alone creates the masks
    native, ico = O.Mesh(xyz, tri), O.Mesh(*O.icosphere(lv["data_order"]))
    (f_in, m_in), (f_ref, m_ref) = prepared(native, src, ico, lv["sigma_in"], masked), prepared(native, ref, ico, lv["sigma_ref"], masked)
    one = ["create_exclusion", "metric_resample+mask", "smooth_data+mask"] if masked else ["metric_resample", "smooth_data"]
    vn = "variance_normalise" + ("+mask" if masked else "")
    assert ops.log == one + one + ["histogram_match", vn, vn]               # resample -> smooth, both data sets; then match; then normalise
    (srcs, target, src_masks, ref_mask), = ops.match_calls
    assert len(srcs) == 1 and np.array_equal(srcs[0], f_ref) and np.array_equal(target, f_in)  # the quirk: the REFERENCE data is matched to the INPUT data
    if masked:
        assert np.array_equal(src_masks[0], m_ref) and np.array_equal(ref_mask, m_in) and 0 < (m_in > 0).sum() < m_in.size
    else:
        assert src_masks is None and ref_mask is None
    matched = HL.histogram_match(f_ref, f_in, m_ref, m_in)
    assert not np.allclose(matched, f_ref, atol=1e-3)
    assert np.array_equal(got[0], normalised(f_in, m_in)) and np.array_equal(got[1], normalised(matched, m_ref))


def test_with_the_option_off_the_ops_are_called_as_before(case):
    for excl in (False, True):
        ops = RecordingOps()
        first_level_features(ops, case, LEVEL, excl=excl, cutthr=C.CUTTHR)
        one = ["create_exclusion", "metric_resample+mask", "smooth_data+mask", "variance_normalise+mask"] if excl else ["metric_resample", "smooth_data", "variance_normalise"]
        assert ops.log == one + one and not hasattr(ops, "match_calls")


def test_cut_without_intensity_only_creates_the_masks(case):
    """_cut is set by --INc, which sets _IN too; the loop still keeps the two apart as featurespace::initialise does"""
    ops = RecordingOps()
    first_level_features(ops, case, LEVEL, cut=True, cutthr=C.CUTTHR)
    one = ["create_exclusion", "metric_resample+mask", "smooth_data+mask"]
    assert ops.log == one + one + ["variance_normalise+mask"] * 2


@pytest.mark.parametrize("cut", [False, True], ids=["IN", "INc"])
def test_groupwise_level_matches_every_later_subject_to_subject_0(cut):
    import newmsm_amd as M
    from newmsm_amd import synthetic

    S, D = 4, 2
    xyz, tri = M.make_mesh_from_icosa(3)
    meshes = [(synthetic.known_warp(xyz, seed=40 + s, rot_deg=0.0, amp=1.0), tri) for s in range(S)]
    datas = [synthetic.features(synthetic.known_warp(meshes[s][0], seed=90 + s, rot_deg=3.0, amp=2.0), D, seed=5) * (1.0 + s) + s for s in range(S)]
    for s in range(S):
        datas[s][:, meshes[s][0][:, 2] > C.CAP_Z] = 0.0
    lv = dict(data_order=2, cp_order=1, sg_order=3, iters=1, simmeasure=2, cost_params=dict(lambda_=1e-3), sigma_in=20.0)
    ops = RecordingOps()
    with pytest.raises(Captured) as e:
        group_registration.run_group_multiresolution(ops, meshes, datas, xyz, tri, [lv], varnorm=True, fixnan=True, intensity=True, cut=cut, cutthr=C.CUTTHR)
    ico = O.Mesh(*O.icosphere(2))
    prep = [prepared(O.Mesh(*meshes[s]), datas[s], ico, 20.0, cut) for s in range(S)]
    one = ["create_exclusion", "metric_resample+mask", "smooth_data+mask"] if cut else ["metric_resample", "smooth_data"]
    assert ops.log == one * S + ["histogram_match"] + ["variance_normalise" + ("+mask" if cut else "")] * S
    (srcs, target, src_masks, ref_mask), = ops.match_calls  # one call: (S - 1) D rows against one target
    assert len(srcs) == S - 1 and np.array_equal(target, prep[0][0]) and all(np.array_equal(srcs[s - 1], prep[s][0]) for s in range(1, S))
    assert (src_masks is None and ref_mask is None) if not cut else (np.array_equal(ref_mask, prep[0][1]) and all(np.array_equal(src_masks[s - 1], prep[s][1]) for s in range(1, S)))
    assert np.array_equal(e.value.feats[0], normalised(*prep[0]))
    for s in range(1, S):
        assert np.array_equal(e.value.feats[s], normalised(HL.histogram_match(prep[s][0], prep[0][0], prep[s][1], prep[0][1]), prep[s][1]))


@pytest.mark.parametrize("excl", [False, True], ids=["IN", "excl_IN"])
def test_final_resampling_matches_input_to_reference(case, excl):
    """save_transformed_data (M/mesh_registration.cpp:371-383): the native input data matched to the native reference data -- the other way round than in
    the levels --, masks under --excl only, then metric_resample"""
    xyz, tri, src, ref, _ = case
    ops = RecordingOps()
    from newmsm_amd import synthetic

    moved = ops.mesh(synthetic.known_warp(xyz, seed=8, rot_deg=2.0, amp=1.0), tri)
    target = ops.mesh(*O.icosphere(3))
    ref_data = O.metric_resample(O.Mesh(xyz, tri), ref, target) * 3.0 + 1.0  # the reference's data on its own sphere, another range
    got = registration.transformed_data(ops, moved, src, target, ref_data, excl=excl, cutthr=C.CUTTHR, intensity=True)
    assert ops.log == (["create_exclusion", "create_exclusion", "histogram_match", "metric_resample+mask"] if excl else ["histogram_match", "metric_resample"])
    (srcs, tgt, src_masks, ref_mask), = ops.match_calls
    assert np.array_equal(srcs[0], src) and np.array_equal(tgt, ref_data)
    if excl:
        m_in, m_ref = O.create_exclusion(src, *C.CUTTHR), O.create_exclusion(ref_data, *C.CUTTHR)
        assert np.array_equal(src_masks[0], m_in) and np.array_equal(ref_mask, m_ref)
        want = O.metric_resample_excl(moved, HL.histogram_match(src, ref_data, m_in, m_ref), target, m_in)[0]
    else:
        assert src_masks is None and ref_mask is None
        want = O.metric_resample(moved, HL.histogram_match(src, ref_data), target)
    assert np.array_equal(got, want)
    plain = RecordingOps()  # without the option: exactly the calls of before
    registration.transformed_data(plain, moved, src, target, excl=excl, cutthr=C.CUTTHR)
    assert plain.log == (["create_exclusion", "metric_resample+mask"] if excl else ["metric_resample"])
