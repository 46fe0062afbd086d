"""The shapes of tests/unary_rows_cases.py on the oracle alone: the patch sizes that its table states -- which are what makes each shape exercise what
tests/test_gpu_unary_rows.py says it does -- and tables that are finite in every entry and, but for the one-point patches, not constant, so that a
comparison of every entry means something and a constant table cannot pass."""
import numpy as np
import pytest

import unary_rows_cases as R


@pytest.mark.parametrize("name", list(R.CASES))
def test_shapes(name):
    _, _, _, _, L, N, pmin, pmax = R.CASES[name]
    ptr, idx = R.oracle(name).patches()
    sizes = np.diff(ptr)
    print(name, "patches", sizes.min(), "..", sizes.max(), "sizes", sorted(set(sizes.tolist())))
    assert len(sizes) == N and sizes.min() == pmin and sizes.max() == pmax
    assert R.form_of(name) == ("staged" if name == "over" else "rows")
    for sim in R.SIMS:
        U = R.oracle_table(name, sim)
        assert U.shape == (L, N) and np.isfinite(U).all()
        print(name, "sim", sim, "spread", np.ptp(U))
        if name == "one" and sim == 2:  # a single point has no variance: 0.5 AbsoluteWeights, and the weights are 1 to the last bit or two
            assert np.ptp(U) < 1e-15 and abs(U[0, 0] - 0.5) < 1e-15
        else:
            assert np.ptp(U) > 0.05


def test_what_the_shapes_cover():
    sizes = {name: np.diff(R.oracle(name).patches()[0]) for name in R.CASES}
    assert sizes["few"].max() < 8                                   # lanes of a group without a point
    assert 8 < sizes["slot2"].min() and sizes["slot2"].max() < 24   # second slot everywhere, third partly
    assert sizes["wave"].max() < 64                                 # one round of the 64-lane statistics
    assert (sizes["wave2"] > 64).any() and (sizes["wave2"] < 64).any()
    assert (R.CASES["wave2"][4] * R.CASES["wave2"][5]) % 32 != 0    # the last workgroup of the row kernel is partly filled
    assert sizes["full"].max() > 88 and sizes["full"].max() <= R.ROWS_PMAX < sizes["over"].max()  # the twelfth slot; the threshold from both sides
    assert R.CASES["many"][4] > 32


def test_weight_rows():
    """the weight row changes the tables, and the zeros of `few` cover whole patches and nothing of any other patch (sw == 0 there, sw > 0 elsewhere)"""
    ptr, idx = R.oracle("few").patches()
    assert len(set(idx.tolist())) == len(idx)  # disjoint patches
    w = R.weights("few", "zero")[0]
    sw = np.array([w[idx[ptr[k]:ptr[k + 1]]].sum() for k in range(len(ptr) - 1)])
    assert sorted(np.flatnonzero(sw == 0).tolist()) == list(R.ZEROED) and (np.delete(sw, R.ZEROED) > 1.0).all()
    for sim in R.SIMS:
        Uz, Uw, U = R.oracle_table("few", sim, "zero"), R.oracle_table("few", sim, "row"), R.oracle_table("few", sim)
        assert np.isfinite(Uz).all() and np.isfinite(Uw).all()
        assert not np.allclose(Uw, U, rtol=1e-3, atol=0)
        zeroed = Uz[:, list(R.ZEROED)]
        print("sim", sim, "zeroed columns:", zeroed[0])
        # without weight nothing correlates (r = 0: half the control point's AbsoluteWeights, which stay above zero) and nothing differs (SSD: 0)
        assert np.ptp(zeroed, axis=0).max() < 1e-15 and ((zeroed > 0.1).all() if sim == 2 else (zeroed == 0).all())
