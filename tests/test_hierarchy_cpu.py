"""The hierarchy stage without a GPU: the clustering and path files of tools/hierarchy_files.py and its refusals, the new bindings, and
hierarchy.merge_groups over the literal restatement alone (tests/hierarchy_literal.py) on a case with a known answer: with identity child
registrations (R_g = T) the merge changes nothing -- W = T, C_g = T, composed_s = corrected_s to 1e-12 of the radius (the identity bar of
tests/test_dedrift_cpu.py), and every child's figures in the parent's frame equal the ones it had in its own."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import dedrift_literal as L
from tests import hierarchy_literal as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAD = 100.0


@pytest.fixture(scope="module")
def tool(built):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import hierarchy_files
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return hierarchy_files


def write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def tool_args(tmp_path, clusters, path_rows):
    d = str(tmp_path) + os.sep
    write(d + "clusters.csv", clusters)
    write(d + "path.csv", path_rows)
    write(d + "names.txt", "s0\ns1\ns2\ns3\n")
    write(d + "meshes.txt", d + "sphere.surf.gii\n")
    write(d + "data.txt", "".join(d + "data%d.func.gii\n" % s for s in range(4)))
    return ["--clusters=" + d + "clusters.csv", "--path=" + d + "path.csv", "--subjects=" + d + "names.txt", "--meshes=" + d + "meshes.txt",
            "--data=" + d + "data.txt", "--template=" + d + "template.surf.gii", "--conf=" + d + "conf", "--dir=" + d + "out" + os.sep]


def test_bindings_exist(built):
    import newmsm_amd as M
    from newmsm_amd import _lib, dedrift, hierarchy

    lib = M.lib()
    for name in ("msm_dedrift_set_warp", "msm_dedrift_group_stats_select"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.msm_abi_version() == 12
    for name in ("set_warp", "group_stats_select"):
        assert hasattr(dedrift.Dedrift, name) and hasattr(dedrift.ProductOps, name), name
    assert hasattr(hierarchy, "merge_groups")


def test_clusters_and_path_parsing(tool, tmp_path):
    c = write(tmp_path / "c.csv", "1,bob,G2\n0,al,G2\n0,cy,G1\n\n1, di ,G1\n")
    assert tool.read_clusters(c) == {"G2": ["al", "bob"], "G1": ["cy", "di"]}  # `line` orders a group, not the file
    p = write(tmp_path / "p.csv", "G1,G2,R1\nR1,G3,R2\n")
    assert tool.read_path(p) == [("G1", "G2", "R1"), ("R1", "G3", "R2")]
    with pytest.raises(SystemExit) as e:
        tool.read_clusters(write(tmp_path / "bad.csv", "0,al,G1\n2,bob,G1\n"))
    assert "G1" in str(e.value)
    with pytest.raises(SystemExit):
        tool.read_path(write(tmp_path / "badp.csv", "G1,G2\n"))
    table = tool.subject_table(["a", "b"], ["one.surf.gii"], ["da", "db"])  # one mesh line serves every subject
    assert table == {"a": ("one.surf.gii", "da"), "b": ("one.surf.gii", "db")}
    with pytest.raises(SystemExit) as e:
        tool.subject_table(["a", "b"], ["m0", "m1", "m2"], ["da", "db"])
    assert "2 subject names, 3 meshes, 2 data files" in str(e.value)


def test_an_unknown_child_is_named(tool, tmp_path):
    argv = tool_args(tmp_path, "0,s0,G1\n1,s1,G1\n0,s2,G2\n1,s3,G2\n", "G1,G9,R1\n")
    os.makedirs(str(tmp_path / "out"))
    for s in range(2):
        write(tmp_path / "out" / ("G1.sphere-%d.reg.corrected.surf.gii" % s), "")
    write(tmp_path / "out" / "G1.mean.func.gii", "")
    with pytest.raises(SystemExit) as e:
        tool.main(argv)
    assert "G9" in str(e.value) and "row 1" in str(e.value)


def test_a_missing_leaf_prints_the_two_commands(tool, tmp_path):
    argv = tool_args(tmp_path, "0,s0,G1\n1,s1,G1\n0,s2,G2\n1,s3,G2\n", "G1,G2,R1\n")
    with pytest.raises(SystemExit) as e:
        tool.main(argv)
    text = str(e.value)
    assert "leaf group G1" in text and "G1.mean" in text
    assert "register_files.py --groupwise" in text and "dedrift_files.py" in text
    assert text.index("register_files.py --groupwise") < text.index("dedrift_files.py")
    assert "--out=" + str(tmp_path / "out") + os.sep + "G1." in text


def test_identity_child_registrations_change_nothing(built):
    from newmsm_amd import dedrift, hierarchy

    txyz, ttri = O.icosphere(3)
    children, own = [], []
    seed = 0
    for orders in ([3, 2], [2, 3, 2]):
        subjects, data = [], []
        for order in orders:
            xyz, tri = O.icosphere(order)
            reg = L.smooth_warp(xyz, seed)
            subjects.append((xyz, reg, tri))
            data.append(L.group_data(reg, 2, seed))
            seed += 1
        leaf = dedrift.dedrift_group(L.LiteralOps(), (txyz, ttri), subjects, data)  # the child as the existing stage leaves it
        own.append(leaf)
        children.append(dict(reg=txyz, mean=leaf["mean"], subjects=[(m, c, t) for (m, _, t), c in zip(subjects, leaf["corrected"])], data=data))
    got = hierarchy.merge_groups(H.LiteralOps(), (txyz, ttri), children)
    assert got["order"] == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]
    assert np.abs(got["W"] - txyz).max() <= 1e-12 * RAD
    slot = 0
    for g, leaf in enumerate(own):
        assert np.abs(got["child_corrected"][g] - txyz).max() <= 1e-12 * RAD
        assert np.allclose(got["child_mean"][g], leaf["mean"], rtol=0, atol=1e-12)  # a map resampled onto its own mesh
        n = len(leaf["corrected"])
        for s in range(n):
            err = float(np.abs(got["composed"][slot + s] - leaf["corrected"][s]).max())
            assert err <= 1e-12 * RAD, (g, s, err)
            assert np.allclose(got["resampled"][slot + s], leaf["resampled"][s], rtol=1e-12, atol=1e-12)
        cs = got["children_stats"][g]
        assert np.allclose(cs["mean"], leaf["mean"], rtol=1e-12, atol=1e-12) and np.allclose(cs["stdev"], leaf["stdev"], rtol=1e-12, atol=1e-12)
        assert np.abs(cs["cc"] - leaf["cc"]).max() <= 1e-9 and np.array_equal(cs["dice"], leaf["dice"])
        assert np.allclose(cs["cc_mean"], leaf["cc_mean"], rtol=0, atol=1e-9) and np.allclose(cs["dice_mean"], leaf["dice_mean"], rtol=1e-12, atol=0)
        # and the parent's matrices hold the child's block
        assert np.array_equal(got["cc"][:, slot:slot + n, slot:slot + n], cs["cc"]) and np.array_equal(got["dice"][:, slot:slot + n, slot:slot + n], cs["dice"])
        slot += n
    assert got["cc"].shape == (2, 5, 5) and got["mean"].shape == (2, len(txyz))
