"""msmhip::ResamplePlan (include/msmhip.hpp) driven by a compiled program (tests/cpp/resample_plan_client.cpp) with no Python in the loop: the same
library calls as newmsm_amd.ResamplePlan, so its arrays are the Python call's bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from newmsm_amd.bag import read_bag, write_bag
from tests.test_cpp_host import build_cpp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "resample_plan_client.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "resample_plan_client")


def test_resample_plan_header_compiles_without_gpu(built):
    build_cpp(SRC, EXE)  # -Wall -Wextra -Werror, no HIP headers


@pytest.mark.gpu
def test_cpp_resample_plan_equals_python_call(built, ctx, tmp_path):
    """case E's meshes and mask (tests/test_resample_plan_cpu.py: warped ico3 -> ico2), D = 3 maps and two rows of keys"""
    import newmsm_amd as M
    from newmsm_amd import synthetic
    from tests.test_resample_plan_cpu import case, tie_keys

    build_cpp(SRC, EXE)
    xin, tin, xnew, tnew, excl = case("E")
    data = synthetic.features(xin, 3, seed=5)
    keys = np.stack([tie_keys(xin), np.arange(len(xin)) % 7]).astype(np.int32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_bag(fin, in_xyz=xin, in_tri=tin, new_xyz=xnew, new_tri=tnew, data=data, excl=excl, keys=keys)
    run = subprocess.run([EXE, fin, fout], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr + run.stdout
    got = read_bag(fout)
    min_, mnew = M.Mesh(ctx, xin, tin), M.Mesh(ctx, xnew, tnew)
    plan = M.ResamplePlan(min_, mnew)
    rp, col, val = plan.weights()
    assert tuple(got["sizes"]) == plan.sizes()
    assert np.array_equal(got["row_ptr"], rp) and np.array_equal(got["col"], col) and np.array_equal(got["val"], val)
    assert np.array_equal(got["out64"].reshape(3, -1), plan.apply(data))
    assert np.array_equal(got["out32"].reshape(3, -1).astype(np.float32), plan.apply(data.astype(np.float32)))
    assert np.array_equal(got["out32"], got["out32"].astype(np.float32))  # float32 values, widened by the container
    assert np.array_equal(got["labels"].reshape(2, -1), plan.apply_labels(keys, unassigned=-1))
    masked, mask = M.ResamplePlan(min_, mnew, excl=excl).apply(data)
    assert np.array_equal(got["masked"].reshape(3, -1), masked) and np.array_equal(got["mask"], mask)
    assert np.array_equal(got["nearest"].reshape(3, -1), M.ResamplePlan(min_, mnew, method="nearest").apply(data))
    assert np.array_equal(got["bary"].reshape(3, -1), M.ResamplePlan(min_, mnew, method="barycentric").apply(np.ascontiguousarray(xin.T)))
