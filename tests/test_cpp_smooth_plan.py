"""msmhip::ResamplePlan::smoothing (include/msmhip.hpp) driven by a compiled program (tests/cpp/smooth_plan_client.cpp) with no Python in the loop: the
same library calls as newmsm_amd.ResamplePlan.smoothing, so its arrays are the Python call's bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from newmsm_amd.bag import read_bag, write_bag
from tests.test_cpp_host import build_cpp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "smooth_plan_client.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "smooth_plan_client")


def test_smooth_plan_header_compiles_without_gpu(built):
    build_cpp(SRC, EXE)  # -Wall -Wextra -Werror, no HIP headers


@pytest.mark.gpu
def test_cpp_smooth_plan_equals_python_call(built, ctx, tmp_path):
    """case PE (tests/test_smooth_plan_cpu.py: a warped ico3 sphere, sigma 10, the three-valued mask), D = 3 maps"""
    import newmsm_amd as M
    from tests.test_smooth_plan_cpu import reference

    build_cpp(SRC, EXE)
    r = reference("PE")
    data = np.ascontiguousarray(r["data"][:3])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_bag(fin, xyz=r["xorig"], tri=r["tri"], data=data, excl=r["excl"], sigma=np.array([r["sigma"]]))
    run = subprocess.run([EXE, fin, fout], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr + run.stdout
    got = read_bag(fout)
    sphere = M.Mesh(ctx, r["xorig"], r["tri"])
    plan = M.ResamplePlan.smoothing(sphere, sphere, r["sigma"], r["excl"])
    rp, col, val = plan.weights()
    assert tuple(got["sizes"]) == plan.sizes()
    assert np.array_equal(got["row_ptr"], rp) and np.array_equal(got["col"], col) and np.array_equal(got["val"], val)
    assert np.array_equal(got["div"], plan.divisors())
    out, mask = plan.apply(data)
    assert np.array_equal(got["out64"].reshape(3, -1), out) and np.array_equal(got["mask"], mask)
    assert np.array_equal(got["out32"].reshape(3, -1).astype(np.float32), plan.apply(data.astype(np.float32))[0])
    assert np.array_equal(got["out32"], got["out32"].astype(np.float32))  # float32 values, widened by the container
    assert np.array_equal(got["plain"].reshape(3, -1), M.ResamplePlan.smoothing(sphere, sphere, r["sigma"]).apply(data))
