"""Shared by tests/test_histmatch_rows_cpu.py (the inputs and tests/histmatch_literal.py alone: does each case reach what it is named for?) and
tests/test_gpu_histmatch_rows.py (msm_histogram_match against the literal, bit for bit): feature rows longer than one workgroup's chunk.  The range,
count and apply kernels of histmatch_kernels.hip give every (row, chunk of kHistChunk values) a workgroup, and a row's result is joined across its
workgroups in three places -- the two atomicMax range words, the 256 atomicAdd counters, the chunk by chunk apply with its ragged last sweep -- none
of which a row of at most one chunk exercises.  No mesh, no oracle: the matrices are seeded random fill (sources normal, targets gamma, as make_inputs
of tests/test_gpu_histmatch.py), and a placement case then shapes row 0 of source 0 (and row 0 of the target where it says so)."""
import os
import re

import numpy as np

import histmatch_literal as HL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4096  # histmatch.hpp: kHistChunk
WAVE = 64     # lanes of a wavefront: 64 consecutive values of a sweep, from a multiple of 64 on
with open(os.path.join(ROOT, "newmsm_amd", "csrc", "histmatch.hpp")) as _f:
    assert int(re.search(r"constexpr int kHistChunk = (\d+);", _f.read()).group(1)) == CHUNK, "kHistChunk changed: the cases below are cut for 4096"

LONG = (2, 2, 10242, 10242)  # n_src, D, Vs, Vt of the placement cases: three chunks, the last of 2 050 values
TAIL = 10242 - 2 * CHUNK

# name -> ((n_src, D, Vs, Vt), seed); seed % 3 picks the masks: none, one row, D rows
SHAPE_CASES = {
    "at_chunk": ((1, 1, 4096, 4096), 300),        # exactly one full chunk
    "below_above": ((1, 2, 4095, 4097), 301),     # one chunk against two, the second holding one value
    "above_below": ((1, 2, 4097, 4095), 302),     # the same, the other way round
    "two_full": ((1, 1, 8192, 8193), 303),        # a full last chunk against a ragged one
    "ico5": ((3, 2, 10242, 10242), 304),          # three chunks; yrow = n_src * D + row % D with both factors > 1
    "long_source": ((2, 2, 10242, 642), 305),     # target rows: workgroups y = 1, 2 start beyond the row
    "long_target": ((2, 2, 642, 10242), 306),     # source rows likewise; the apply grid has one chunk, the range and count grids three
    "native": ((1, 1, 32492, 40962), 307),        # 8 against 11 chunks, the final matching's shape
    "mask_rows_short": ((2, 3, 10242, 10242), 308),  # source mask with 2 rows, target mask with 1: the row-0 fallback of row_view beyond one chunk
}
PLACEMENT_CASES = ("extremes_apart", "nan_chunk_masked_chunk", "last_chunk_only", "one_counted_value", "one_counted_target_value", "range_from_masked",
                   "dominant_bin_across_chunks", "wave_patterns", "row_unchanged_long")
CASES = tuple(SHAPE_CASES) + PLACEMENT_CASES

# wave_patterns: the 64-value runs from index CHUNK on, in this order
WAVE_RUNS = ("one_value", "two_values", "four_values", "nan_leader", "every_other_masked")
WAVE_VALUES = (-1.5, -0.5, 0.5, 1.5)


def random_inputs(shape, seed, src_rows="cycle", ref_rows="cycle"):
    """n_src x D x Vs sources (normal, a scale per row), a D x Vt target (gamma) and their masks (about 75 % kept); mask rows: a number, None, or
    "cycle" -- none, one row or D rows with seed % 3"""
    n, D, Vs, Vt = shape
    rng = np.random.default_rng(seed)
    src = rng.normal(size=(n, D, Vs)) * rng.uniform(0.5, 3.0, size=(n, D, 1))
    ref = rng.gamma(2.0, 2.0, size=(D, Vt)) - 1.5
    cyc = (None, 1, D)[seed % 3]
    src_rows, ref_rows = (cyc if r == "cycle" else r for r in (src_rows, ref_rows))
    src_excl = None if src_rows is None else (rng.random((n, src_rows, Vs)) > 0.25).astype(np.float64)
    ref_excl = None if ref_rows is None else (rng.random((ref_rows, Vt)) > 0.25).astype(np.float64)
    return src, ref, src_excl, ref_excl


def case(name):
    """(src n x D x Vs, ref D x Vt, src_excl n x rows x Vs or None, ref_excl rows x Vt or None) of a named case"""
    if name in SHAPE_CASES:
        shape, seed = SHAPE_CASES[name]
        if name == "mask_rows_short":
            return random_inputs(shape, seed, 2, 1)
        return random_inputs(shape, seed)
    seed = 400 + PLACEMENT_CASES.index(name)
    if name == "extremes_apart":
        # all values inside [-2, 2] but one minimum and one maximum, which lie two chunks apart (and the other way round on the target)
        src, ref, se, re_ = random_inputs(LONG, seed, None, None)
        x, y = src[0, 0], ref[0]
        np.clip(x, -2.0, 2.0, out=x)
        np.clip(y, -2.0, 2.0, out=y)
        x[100], x[2 * CHUNK + 808] = -7.0, 9.0
        y[2 * CHUNK + 1308], y[50] = -7.0, 9.0
    elif name == "nan_chunk_masked_chunk":
        src, ref, se, re_ = random_inputs(LONG, seed, 2, 2)
        src[0, 0, CHUNK:2 * CHUNK] = np.nan
        se[0, 0] = 1.0
        se[0, 0, :CHUNK] = 0.0
    elif name == "last_chunk_only":
        src, ref, se, re_ = random_inputs(LONG, seed, 2, 2)
        se[0, 0] = 1.0
        se[0, 0, :2 * CHUNK] = 0.0
    elif name == "one_counted_value":
        src, ref, se, re_ = random_inputs((1, 1, CHUNK + 1, CHUNK + 1), seed, 1, 1)
        se[0, 0] = 0.0
        se[0, 0, CHUNK] = 1.0
    elif name == "one_counted_target_value":
        src, ref, se, re_ = random_inputs((1, 1, CHUNK + 1, CHUNK + 1), seed, 1, 1)
        re_[0] = 0.0
        re_[0, CHUNK] = 1.0
    elif name == "range_from_masked":
        src, ref, se, re_ = random_inputs(LONG, seed, 2, 2)
        src[0, 0, 0], src[0, 0, -1] = -50.0, 50.0
        se[0, 0, 0] = se[0, 0, -1] = 0.0
    elif name == "dominant_bin_across_chunks":
        src, ref, se, re_ = random_inputs(LONG, seed, None, None)
        src[0, 0, 3000:7000] = 0.0
        ref[0, 7000:10000] = 0.0
    elif name == "wave_patterns":
        src, ref, se, re_ = random_inputs(LONG, seed, 2, 2)
        x, m = src[0, 0], se[0, 0]
        m[:] = 1.0
        a, b, c, d = WAVE_VALUES
        run = lambda k: slice(CHUNK + k * WAVE, CHUNK + (k + 1) * WAVE)  # noqa: E731
        x[run(0)] = c
        x[run(1)] = np.tile([c, b], WAVE // 2)
        x[run(2)] = np.tile([a, b, c, d], WAVE // 4)  # beyond the two leader rounds of k_hist_counts: the last two values add for themselves
        x[run(3)] = c
        x[CHUNK + 3 * WAVE] = np.nan                  # the leader lane is uncounted
        m[run(4)] = np.tile([0.0, 1.0], WAVE // 2)    # (the values stay random: the leader lane and every other lane masked)
    elif name == "row_unchanged_long":
        src, ref, se, re_ = random_inputs(LONG, seed)
        src[0, 0] = 1.25
        ref[1] = -2.0
    else:
        raise ValueError(name)
    return src, ref, se, re_


def chunks(V):
    return (V + CHUNK - 1) // CHUNK


def chunk_of(i):
    return int(i) // CHUNK


def row_masks(src_excl, ref_excl, s, d, Vs, Vt):
    """the masks that serve feature row d of source s and of the target (all ones without a mask)"""
    return HL.mask_row(None if src_excl is None else src_excl[s], d, Vs), HL.mask_row(ref_excl, d, Vt)


def counted(x, m):
    """finite and mask > 0"""
    return np.isfinite(x) & (m > 0)


def counted_per_chunk(x, m):
    c = counted(x, m)
    return [int(c[k * CHUNK:(k + 1) * CHUNK].sum()) for k in range(chunks(len(x)))]


def is_matched(x, mx, y, my):
    """step 1 of DESIGN.md section 5.11 from the inputs alone: both rows have a counted value and a range of more than one value"""
    fx, fy = x[np.isfinite(x)], y[np.isfinite(y)]
    return bool(counted(x, mx).any() and counted(y, my).any() and fx.min() != fx.max() and fy.min() != fy.max())


def literal(src, ref, src_excl, ref_excl):
    return np.stack([HL.histogram_match(src[s], ref, None if src_excl is None else src_excl[s], ref_excl) for s in range(src.shape[0])])
