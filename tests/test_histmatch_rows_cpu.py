"""The long-row cases of tests/histmatch_row_cases.py on their inputs and the literal alone, no GPU: each case must reach what it is named for -- the
chunk counts, the chunks that hold the extremes, the chunks without a counted value, n = 1, a table or none, the number of values the matching
changes -- so that tests/test_gpu_histmatch_rows.py cannot pass by accident.  Every number asserted here follows from the case's construction (the
docstrings say how); the rest of what the literal gives is quoted as observed.  "Row 0" is feature row 0 of source 0 against row 0 of the target."""
import numpy as np
import pytest

import histmatch_literal as HL
import histmatch_row_cases as C


def row0(name):
    """(x, mask of x, y, mask of y, the literal's matched x, its table or None) of row 0, and the whole case"""
    src, ref, se, re_ = C.case(name)
    x, y = src[0, 0], ref[0]
    mx, my = C.row_masks(se, re_, 0, 0, len(x), len(y))
    out, table = HL.match_row(x, mx, y, my)
    return x, mx, y, my, out, table, (src, ref, se, re_)


def changed(out, x):
    return ~((out == x) | (np.isnan(out) & np.isnan(x)))


def extreme_chunks(v):
    """(chunk of the only minimum, chunk of the only maximum) over the finite values"""
    f = np.where(np.isfinite(v), v, 0.0)
    lo, hi = v[np.isfinite(v)].min(), v[np.isfinite(v)].max()
    assert (v == lo).sum() == 1 and (v == hi).sum() == 1
    return C.chunk_of(np.argmin(f)), C.chunk_of(np.argmax(f))


def test_chunk_is_the_kernels():
    """importing the cases has compared CHUNK with kHistChunk of histmatch.hpp; the sizes below are cut around it"""
    assert C.CHUNK == 4096 and C.TAIL == 2050 and C.chunks(4096) == 1 and C.chunks(4097) == 2 and C.chunks(10242) == 3
    assert len(C.CASES) == len(set(C.CASES)) == 18


# name -> (chunks of Vs, chunks of Vt, mask rows of the sources, of the target, values in the last chunk of x, of y)
SHAPES = {
    "at_chunk": (1, 1, None, None, 4096, 4096),
    "below_above": (1, 2, 1, 1, 4095, 1),
    "above_below": (2, 1, 2, 2, 1, 4095),
    "two_full": (2, 3, None, None, 4096, 1),
    "ico5": (3, 3, 1, 1, 2050, 2050),
    "long_source": (3, 1, 2, 2, 2050, 642),
    "long_target": (1, 3, None, None, 642, 2050),
    "native": (8, 11, 1, 1, 3820, 2),
    "mask_rows_short": (3, 3, 2, 1, 2050, 2050),
}


@pytest.mark.parametrize("name", list(C.SHAPE_CASES))
def test_shape_cases(name):
    """Random rows, so every chunk of both rows holds counted values (a mask keeps about 75 %; where the last chunk holds one or two values the seed
    is one that keeps them: below_above's target 3 060 + 1, above_below's source 3 112 + 1, two_full's target 4 096 + 4 096 + 1, native's target
    ten chunks of about 3 080 and then 2), every row yields a table, and the literal changes every counted value of every row and no other (a
    continuous value does not sit on one of 256 table entries): row 0 changes 4 096, 3 027, 3 113, 8 192, 7 616, 7 721, 642, 24 414 and 7 679 values
    in the order of the table above.  The masks cycle: none, one row, D rows."""
    cs, ct, src_rows, ref_rows, last_x, last_y = SHAPES[name]
    x, mx, y, my, out, table, (src, ref, se, re_) = row0(name)
    (n, D, Vs, Vt), _ = C.SHAPE_CASES[name]
    assert src.shape == (n, D, Vs) and ref.shape == (D, Vt)
    assert (C.chunks(Vs), C.chunks(Vt)) == (cs, ct)
    assert (None if se is None else se.shape) == (None if src_rows is None else (n, src_rows, Vs))
    assert (None if re_ is None else re_.shape) == (None if ref_rows is None else (ref_rows, Vt))
    assert Vs - (cs - 1) * C.CHUNK == last_x and Vt - (ct - 1) * C.CHUNK == last_y
    assert table is not None
    want = C.literal(src, ref, se, re_)
    for s in range(n):
        for d in range(D):
            xs, ys = src[s, d], ref[d]
            ms, mt = C.row_masks(se, re_, s, d, Vs, Vt)
            assert min(C.counted_per_chunk(xs, ms)) >= 1 and min(C.counted_per_chunk(ys, mt)) >= 1  # no chunk is idle, the ragged last one included
            assert C.is_matched(xs, ms, ys, mt)
            assert np.array_equal(changed(want[s, d], xs), C.counted(xs, ms))
    assert np.array_equal(want[0, 0], out)


def test_ico5_has_rows_and_sources_beyond_the_first():
    """yrow = n_src * D + row % D: with n_src = 3 and D = 2 a row's target is neither `row` nor `row % n_src`; the two target rows differ, so another
    target row gives another table (source 1, row 1 matched to target row 0 differs from the literal at every one of its 7 684 counted values but
    those that fall in the same place by chance)"""
    src, ref, se, re_ = C.case("ico5")
    assert src.shape[:2] == (3, 2) and not np.array_equal(ref[0], ref[1])
    mx, my = C.row_masks(se, re_, 1, 1, 10242, 10242)
    right, wrong = HL.match_row(src[1, 1], mx, ref[1], my)[0], HL.match_row(src[1, 1], mx, ref[0], my)[0]
    assert (right != wrong).sum() > 0.9 * C.counted(src[1, 1], mx).sum()


def test_long_rows_beside_short_rows():
    """long_source: the grid of the range and count kernels has three chunks for every row, the target rows (642 values) end inside the first: their
    workgroups y = 1, 2 begin beyond the row.  long_target: the same for the source rows, and the apply grid (source rows only) has one chunk"""
    for name, long_is_source in (("long_source", True), ("long_target", False)):
        (n, D, Vs, Vt), _ = C.SHAPE_CASES[name]
        short, long_ = (Vt, Vs) if long_is_source else (Vs, Vt)
        assert short <= C.CHUNK and C.chunks(long_) == 3 and C.chunks(max(Vs, Vt)) == 3 and C.chunks(Vs) == (3 if long_is_source else 1)


def test_mask_rows_short_falls_back_to_mask_row_0():
    """D = 3 with two source mask rows and one target mask row: feature row 2 is served by mask row 0 on both sides (M/reg_tools.cpp:764-767), feature
    row 1 by source mask row 1 and target mask row 0.  The two source mask rows differ (they agree at about 5/8 of the places), so the fallback
    shows: row 2 of source 0 counts 7 679 values, as row 0 does, where mask row 1 keeps 7 725"""
    src, ref, se, re_ = C.case("mask_rows_short")
    assert se.shape == (2, 2, 10242) and re_.shape == (1, 10242) and src.shape[1] == 3
    for s in range(2):
        assert np.array_equal(C.row_masks(se, re_, s, 2, 10242, 10242)[0], se[s, 0]) and np.array_equal(C.row_masks(se, re_, s, 1, 10242, 10242)[0], se[s, 1])
        assert 0.5 < (se[s, 0] == se[s, 1]).mean() < 0.75
    assert np.array_equal(C.row_masks(se, re_, 0, 2, 10242, 10242)[1], re_[0])
    assert C.counted(src[0, 2], se[0, 0]).sum() != C.counted(src[0, 2], se[0, 1]).sum()


# ---------------------------------------------------------------- the placement cases
def test_extremes_apart():
    """No masks.  The source row's only minimum (-7) lies in chunk 0 and its only maximum (9) in chunk 2, the target's in chunks 2 and 0; every
    other value lies in [-2, 2] (the target's in [-1.5, 2]: the gamma fill ends at -1.5), so the range of any one chunk, and of any two, is not
    the row's.  The literal changes every value but the minimum: bin 1 of the source holds the -7 alone, the target's bin 1 holds its -7, so
    t[1] = lo_y = -7 -- 10 241 of 10 242 changed."""
    x, mx, y, my, out, table, (src, ref, se, re_) = row0("extremes_apart")
    assert se is None and re_ is None and len(x) == len(y) == 10242
    assert extreme_chunks(x) == (0, 2) and extreme_chunks(y) == (2, 0)
    for v in (x, y):
        inner = np.sort(v)[1:-1]
        assert (v.min(), v.max()) == (-7.0, 9.0) and -2.0 <= inner[0] and inner[-1] <= 2.0
        for k in range(3):
            part = v[k * C.CHUNK:(k + 1) * C.CHUNK]
            assert (part.min(), part.max()) != (-7.0, 9.0)
    assert table is not None and table[0] == -7.0
    assert changed(out, x).sum() == 10241 and not changed(out, x)[np.argmin(x)]


def test_nan_chunk_masked_chunk_and_last_chunk_only():
    """nan_chunk_masked_chunk: chunk 0 is masked (finite: it still sets the range -- minimum and maximum both lie in it), chunk 1 is NaN, mask 1 on
    the tail.  last_chunk_only: chunks 0 and 1 masked and finite (minimum in chunk 0, maximum in chunk 1).  Both count the 2 050 values of the ragged
    last chunk and no other, and the literal changes exactly those"""
    for name in ("nan_chunk_masked_chunk", "last_chunk_only"):
        x, mx, y, my, out, table, _ = row0(name)
        assert C.counted_per_chunk(x, mx) == [0, 0, C.TAIL] and min(C.counted_per_chunk(y, my)) > 1000
        tail = x[2 * C.CHUNK:]
        fin = x[np.isfinite(x)]
        assert fin.min() < tail.min() and fin.max() > tail.max()  # the range comes from uncounted values
        assert C.chunk_of(np.nanargmin(x)) < 2 and C.chunk_of(np.nanargmax(x)) < 2
        assert table is not None and changed(out, x).sum() == C.TAIL and changed(out, x)[2 * C.CHUNK:].all()
        if name == "nan_chunk_masked_chunk":
            assert np.isnan(x[C.CHUNK:2 * C.CHUNK]).all() and np.isfinite(x[:C.CHUNK]).all() and np.isnan(out[C.CHUNK:2 * C.CHUNK]).all()
        else:
            assert np.isfinite(x).all() and extreme_chunks(x) == (0, 1)


def test_one_counted_value():
    """4 097 values, the source mask 1 at index 4 096 alone: nx = 1, counted by the one active lane of the second chunk's workgroup, while the range
    comes from all 4 097.  cdf_x is a step from 0 to 1 at that value's bin, so the table has at most three values -- lo_y below the step, the
    upper edge of the last target bin that holds a counted value (clipped to hi_y) from the step on, and the fixed last entry lo_y + 255 w_y -- and
    the value, which is not in the last source bin, takes the second: exactly one value changes, to no less than the largest counted target value"""
    x, mx, y, my, out, table, _ = row0("one_counted_value")
    assert len(x) == len(y) == C.CHUNK + 1 and C.counted_per_chunk(x, mx) == [0, 1] and mx[C.CHUNK] == 1.0 and mx.sum() == 1.0
    assert C.counted(y, my).sum() > 1000 and C.counted_per_chunk(y, my)[1] == 1
    b = int(HL.bins_of(x[C.CHUNK:], x.min(), (x.max() - x.min()) / HL.B)[0])
    assert table is not None and len(set(table)) <= 3 and b < HL.B and (table[:b - 1] == y.min()).all() and (table[b - 1:-1] == table[b - 1]).all()
    ch = changed(out, x)
    assert ch.sum() == 1 and ch[C.CHUNK] and out[C.CHUNK] == table[b - 1] and y[C.counted(y, my)].max() <= out[C.CHUNK] <= y.max()


def test_one_counted_target_value():
    """the target mask 1 at index 4 096 alone: ny = 1 and cdf_y is a step from 0 to 1 at that value's bin k (k = 9 with this seed: k > 1, so the table's
    division runs), so every source bin b < 256 that holds or follows a counted value moves into bin k: t[b] = lo_y + (k - 1) w_y + cdf_x[b] w_y
    (t[256] is lo_y + 255 w_y whatever the counts).  The source row counts 3 063 + 1 values (one-row mask) and all 3 064 change"""
    x, mx, y, my, out, table, _ = row0("one_counted_target_value")
    assert C.counted_per_chunk(y, my) == [0, 1] and my.sum() == 1.0 and C.counted_per_chunk(x, mx)[1] == 1
    lo, w = y.min(), (y.max() - y.min()) / HL.B
    k = int(HL.bins_of(y[C.CHUNK:], lo, w)[0])
    assert 1 < k < HL.B
    c = C.counted(x, mx)
    inner = c & (HL.bins_of(np.where(c, x, 0.0), x.min(), (x.max() - x.min()) / HL.B) < HL.B)
    assert table is not None and inner.sum() >= c.sum() - 1 and out[inner].min() >= lo + (k - 1) * w - 1e-9 and out[inner].max() <= lo + k * w + 1e-9
    assert np.array_equal(changed(out, x), c) and c.sum() > 3000


def test_range_from_masked():
    """-50 at index 0 and +50 at index V - 1, both masked: the range [-50, 50] is set by two values that are never counted and lie in chunks 0 and 2;
    every counted value lies within 5 standard deviations of at most 3, well inside it.  All 7 652 counted values change"""
    x, mx, y, my, out, table, _ = row0("range_from_masked")
    assert extreme_chunks(x) == (0, 2) and (x[0], x[-1]) == (-50.0, 50.0) and mx[0] == 0.0 and mx[-1] == 0.0
    c = C.counted(x, mx)
    assert np.abs(x[c]).max() < 15.0 and min(C.counted_per_chunk(x, mx)) > 1000
    assert table is not None and np.array_equal(changed(out, x), c)


def test_dominant_bin_across_chunks():
    """No masks.  Source indices 3 000 to 6 999 are exactly 0.0 -- 1 096 values at the end of chunk 0 and 2 904 at the start of chunk 1, whole
    wavefronts of one bin in two workgroups -- and target indices 7 000 to 9 999 likewise over chunks 1 and 2 (1 192 and 1 808).  The zero bin
    holds at least those 4 000 values (4 068 observed) of 10 242."""
    x, mx, y, my, out, table, (src, ref, se, re_) = row0("dominant_bin_across_chunks")
    assert se is None and re_ is None
    for v, a, b in ((x, 3000, 7000), (y, 7000, 10000)):
        assert (v[a:b] == 0.0).all() and C.chunk_of(a) + 1 == C.chunk_of(b - 1) and (v == 0.0).sum() == b - a
        border = C.chunk_of(b - 1) * C.CHUNK
        assert (border - a) // C.WAVE >= 16 and (b - border) // C.WAVE >= 16  # at least 16 whole wavefronts on either side of the border
        lo, w = v.min(), (v.max() - v.min()) / HL.B
        h = np.bincount(HL.bins_of(v, lo, w), minlength=HL.B + 1)
        assert h.max() >= b - a and h.argmax() == HL.bins_of(np.zeros(1), lo, w)[0]
    assert table is not None and changed(out, x).all()


def test_wave_patterns():
    """From index CHUNK on (lane 0 of wavefront 0 in the second chunk's first sweep) five runs of 64 values, each one wavefront's lanes: one value
    (1 bin, 64 counted), two alternating values (2 bins, 64), four cycling values (4 bins, 64: two are left after the two leader rounds), a NaN
    in the leader lane before 63 equal values (1 bin, 63), random values with every other lane masked, the leader lane among them (32 counted, 28
    bins observed).  The bin width is (hi - lo) / 256 < 24 / 256 < 0.5 = half the least distance between two of the values, so different values
    never share a bin (0.019 observed).  Row 0 counts 4 096 + 4 063 + 2 050 values and all of them change"""
    x, mx, y, my, out, table, _ = row0("wave_patterns")
    fin = x[np.isfinite(x)]
    lo, w = fin.min(), (fin.max() - fin.min()) / HL.B
    assert w < 0.5 * np.diff(C.WAVE_VALUES).min()
    want = dict(one_value=(64, 1), two_values=(64, 2), four_values=(64, 4), nan_leader=(63, 1), every_other_masked=(32, None))
    for k, name in enumerate(C.WAVE_RUNS):
        begin = C.CHUNK + k * C.WAVE
        assert begin % C.WAVE == 0 and C.chunk_of(begin) == C.chunk_of(begin + C.WAVE - 1) == 1
        xs, ms = x[begin:begin + C.WAVE], mx[begin:begin + C.WAVE]
        c = C.counted(xs, ms)
        bins = len(np.unique(HL.bins_of(xs[c], lo, w)))
        assert c.sum() == want[name][0]
        assert bins == want[name][1] if want[name][1] else bins >= 3
        if name == "nan_leader":
            assert np.isnan(xs[0]) and c[1:].all()
        if name == "every_other_masked":
            assert not c[0::2].any() and c[1::2].all()
    assert C.counted_per_chunk(x, mx) == [C.CHUNK, C.CHUNK - 33, C.TAIL]
    assert table is not None and np.array_equal(changed(out, x), C.counted(x, mx))


def test_row_unchanged_long():
    """Row 0 of source 0 is 1.25 in all three chunks (hi == lo: no table) and target row 1 is constant, so feature row 1 of both sources is left
    unchanged as well; row 0 of source 1 is matched and all its counted values change (10 242: this seed's masks are none).  Every apply
    workgroup of an unchanged row must take the same decision"""
    x, mx, y, my, out, table, (src, ref, se, re_) = row0("row_unchanged_long")
    assert (x == 1.25).all() and C.chunks(len(x)) == 3 and table is None and np.array_equal(out, x)
    assert (ref[1] == ref[1, 0]).all() and not (ref[0] == ref[0, 0]).all()
    want = C.literal(src, ref, se, re_)
    ch = changed(want, src).sum(axis=2)
    m10 = C.row_masks(se, re_, 1, 0, 10242, 10242)[0]
    assert ch[0, 0] == 0 and ch[0, 1] == 0 and ch[1, 1] == 0 and ch[1, 0] == C.counted(src[1, 0], m10).sum() > 7000
    assert [[C.is_matched(src[s, d], *C.row_masks(se, re_, s, d, 10242, 10242)[:1], ref[d], C.row_masks(se, re_, s, d, 10242, 10242)[1]) for d in range(2)]
            for s in range(2)] == [[False, False], [True, False]]


@pytest.mark.parametrize("name", [n for n in C.PLACEMENT_CASES if n not in ("row_unchanged_long", "one_counted_value", "one_counted_target_value")])
def test_other_rows_of_the_placement_cases_stay_random(name):
    """(2, 2, 10 242, 10 242): rows (0, 1), (1, 0) and (1, 1) are matched, with every chunk counted, whatever row 0 of source 0 is shaped into"""
    src, ref, se, re_ = C.case(name)
    assert src.shape == (2, 2, 10242) and ref.shape == (2, 10242)
    for s, d in ((0, 1), (1, 0), (1, 1)):
        ms, mt = C.row_masks(se, re_, s, d, 10242, 10242)
        assert C.is_matched(src[s, d], ms, ref[d], mt) and min(C.counted_per_chunk(src[s, d], ms)) > 1000 and min(C.counted_per_chunk(ref[d], mt)) > 1000
