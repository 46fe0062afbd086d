"""The C++ mirror of the dedrift stage (include/msmhip_dedrift.hpp) driven by a compiled program (tests/cpp/dedrift_client.cpp) with no Python in the
loop: the same library calls in the same order as newmsm_amd/dedrift.py, so W and a subject's outputs are the Python call's bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from newmsm_amd.bag import read_bag, write_bag
from tests.test_cpp_host import build_cpp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dedrift_client.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "dedrift_client")


def test_dedrift_header_compiles_without_gpu(built):
    build_cpp(SRC, EXE)  # -Wall -Wextra -Werror, no HIP headers


@pytest.mark.gpu
def test_cpp_dedrift_equals_python_call(built, ctx, tmp_path):
    """case (a) of tests/test_gpu_dedrift.py: ico4 template, five subjects on meshes of three sizes, D = 2"""
    from newmsm_amd import dedrift
    from tests.test_gpu_dedrift import case_a

    build_cpp(SRC, EXE)
    (txyz, ttri), subjects, data = case_a()
    S, D, pick = len(subjects), data[0].shape[0], 2
    arrays = dict(template_xyz=txyz, template_tri=ttri, sizes=np.array([S, D, pick]), percentile=np.array([75.0]))
    for s, (orig, reg, tri) in enumerate(subjects):
        arrays.update({"orig%d" % s: orig, "reg%d" % s: reg, "tri%d" % s: tri, "data%d" % s: data[s]})
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_bag(fin, **arrays)
    run = subprocess.run([EXE, fin, fout], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    got = read_bag(fout)
    want = dedrift.dedrift_group(ctx, (txyz, ttri), subjects, data, percentile=75)
    assert np.array_equal(got["W"].reshape(-1, 3), want["W"]) and np.array_equal(got["drift"].reshape(-1, 3), want["drift"])
    assert np.array_equal(got["corrected"].reshape(-1, 3), want["corrected"][pick])
    assert np.array_equal(got["resampled"].reshape(D, -1), want["resampled"][pick])
    assert np.array_equal(got["distortion"].reshape(2, -1), want["distortion"][pick])
    for k in ("mean", "stdev", "cc", "dice"):
        assert np.array_equal(got[k], want[k].ravel()), k
    s = want["summary"]
    figures = np.concatenate([want["cc_mean"], want["dice_mean"], [s["areal_mean"], s["areal_max"], s["areal_95"], s["areal_98"], s["shape_mean"], s["shape_max"]]])
    # the pair means are the same additions in the same order; numpy's mean of the distortion summary is a pairwise sum, the client's a serial one
    assert np.array_equal(got["figures"][:2 * D], figures[:2 * D])
    assert np.allclose(got["figures"], figures, rtol=1e-12, atol=0)
