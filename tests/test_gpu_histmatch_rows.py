"""msm_histogram_match on rows longer than one workgroup's chunk (kHistChunk = 4096 values), where a row's range, counts and application are joined
across workgroups: the cases of tests/histmatch_row_cases.py (tests/test_histmatch_rows_cpu.py shows on the CPU that each reaches what it is named
for) against the literal restatement bit for bit, the context's scratch across calls of different sizes, msm_level_features matching in place on an
ico5 grid, and the final matching of run_multiresolution (native input data to native reference data, Vs != Vt) through ProductOps.  No tolerance
anywhere: integer counts, one rounding per operation (the library is built with -ffp-contract=off)."""
import time

import numpy as np
import pytest

import histmatch_literal as HL
import histmatch_row_cases as C
import newmsm_amd as M
import trans_excl_cases as T
from newmsm_amd import api, registration
from test_gpu_level_features import check, native, same_bytes

pytestmark = pytest.mark.gpu


def assert_same(got, want, what):
    assert got.shape == want.shape
    same = (got == want) | (np.isnan(got) & np.isnan(want))  # == on the doubles; a NaN that was left in place is a NaN
    assert same.all(), "%s: %d of %d values differ, first at %s" % (what, (~same).sum(), same.size, np.argwhere(~same)[0])


def assert_properties(got, src, ref, se, re_, what):
    """what holds for any correct matching, from the inputs alone: uncounted values keep their bytes, the counted values of a matched row lie inside
    the target row's finite range and take at most 256 values (one per bin), an unmatched row keeps its bytes"""
    n, D, Vs = src.shape
    for s in range(n):
        for d in range(D):
            x, y, out = src[s, d], ref[d], got[s, d]
            mx, my = C.row_masks(se, re_, s, d, Vs, ref.shape[1])
            c = C.counted(x, mx)
            assert out[~c].tobytes() == x[~c].tobytes(), "%s: an uncounted value of source %d row %d changed" % (what, s, d)
            if not C.is_matched(x, mx, y, my):
                assert out.tobytes() == x.tobytes(), "%s: source %d row %d has no table and changed" % (what, s, d)
                continue
            fy = y[np.isfinite(y)]
            assert fy.min() <= out[c].min() and out[c].max() <= fy.max(), "%s: source %d row %d left the target's range" % (what, s, d)
            assert len(np.unique(out[c])) <= HL.B, "%s: source %d row %d takes more than 256 values" % (what, s, d)


def run_case(ctx, inputs, want, what):
    src, ref, se, re_ = inputs
    got = M.histogram_match(ctx, src, ref, se, re_)
    assert_same(got, want, what)
    assert_properties(got, src, ref, se, re_, what)
    return got


@pytest.mark.parametrize("name", C.CASES)
def test_rows_equal_the_literal_bit_for_bit(ctx, name):
    inputs = C.case(name)
    got = run_case(ctx, inputs, C.literal(*inputs), name)
    again = M.histogram_match(ctx, *inputs)
    assert again.tobytes() == got.tobytes()  # two calls on the same input give the same bits


def test_scratch_reused_across_sizes(ctx):
    """the range words and the counters share one buffer of the context, grown on demand and zeroed per call for the call's rows: a long call, a
    small one with more rows, one chunk against two, and the long one again -- nothing of an earlier call is left in a later one's words"""
    small = C.random_inputs((1, 3, 642, 642), 500)
    calls = [("native", C.case("native")), ("small", small), ("below_above", C.case("below_above")), ("native again", C.case("native"))]
    got = [run_case(ctx, inputs, C.literal(*inputs), what) for what, inputs in calls]
    assert got[0].tobytes() == got[3].tobytes()


@pytest.mark.parametrize("exclude", [True, False], ids=["exclude", "no_masks"])
def test_level_features_matches_on_an_ico5_grid(ctx, exclude):
    """hist_match_dev as msm_level_features calls it: in place on the feature block behind data set 0's, N = 10 242 values a row (three chunks),
    the masks one row per data set.  Three data sets on warped natives of ico4, ico5 and ico4, D = 2, no smoothing, --IN --VN; the bytes of the
    composition of the entry points, the oracle composition (the literal for the matching) within helpers.ulp_close; the matching changed data sets 1
    and 2 and left data set 0's bytes alone.  Measured on an MI355X: 0.30 s with masks, 0.19 s without, oracle leg included (0.55 s / 0.36 s of it on
    a slower CPU), against 1.4 s for the slowest test of tests/test_gpu_level_features.py in the same run -- so the oracle leg stays"""
    nats = [native(4, 61, 2), native(5, 62, 2), native(4, 63, 2)]
    sigmas = [0.0, 0.0, 0.0]
    t0 = time.perf_counter()
    f, m = check(ctx, 5, nats, sigmas, exclude=exclude, intensity=True, varnorm=True)
    print("ico5 level features, exclude=%s: %.2f s" % (exclude, time.perf_counter() - t0))
    assert f.shape == (3, 2, 10242) and C.chunks(f.shape[2]) == 3
    grid = M.Mesh(ctx, *M.make_mesh_from_icosa(5))
    plain, _ = api.level_features(grid, [M.Mesh(ctx, x, t) for x, t, _ in nats], [d for _, _, d in nats], sigmas, exclude=exclude, intensity=False, varnorm=True,
                                  cutthr=T.CUTTHR)
    assert same_bytes(f[0], plain[0])
    assert not np.allclose(f[1], plain[1], atol=1e-3) and not np.allclose(f[2], plain[2], atol=1e-3)


def test_final_matching_shape_through_product_ops(ctx):
    """the call of registration.transformed_data: the native input data (32 492 values a row, 8 chunks) matched to the native reference data (40 962,
    11 chunks), D = 2, V-vector masks that keep about 75 % as create_exclusion returns them; then without masks"""
    rng = np.random.default_rng(600)
    D, Vs, Vt = 2, 32492, 40962
    in_data = rng.normal(size=(D, Vs)) * rng.uniform(0.5, 3.0, size=(D, 1))
    ref_data = rng.gamma(2.0, 2.0, size=(D, Vt)) - 1.5
    in_mask, ref_mask = (rng.random(Vs) > 0.25).astype(np.float64), (rng.random(Vt) > 0.25).astype(np.float64)
    assert (C.chunks(Vs), C.chunks(Vt)) == (8, 11) and 0.7 < in_mask.mean() < 0.8 and 0.7 < ref_mask.mean() < 0.8
    ops = registration.ProductOps(ctx)
    for se, re_ in ((in_mask, ref_mask), (None, None)):
        got = ops.histogram_match([in_data], ref_data, None if se is None else [se], re_)[0]
        assert_same(got, HL.histogram_match(in_data, ref_data, se, re_), "masks" if se is not None else "no masks")
        assert_properties(got[None], in_data[None], ref_data, None if se is None else se[None, None], re_, "final matching")
        assert (got != in_data).sum() == (D * Vs if se is None else D * int(in_mask.sum()))
