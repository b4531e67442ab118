"""The host side of the ODE forward solve, what needs no GPU: csrc/rnde_fwd_plan.h by a stand-alone program (tests/save_host/fwd_plan_check.cpp)
compiled with the address and undefined-behaviour sanitizers -- the saving callback's value for every kind (zero and NaN estimates, the values at
init), the eigen_est cotangent coefficients against fp64 central differences of that same rule, the saved values and the step ends of
written-down attempt logs, and the sizing rules (attempt limit, speculative records, chunks, retry window, NFE, saveat validation) at their
corners."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forward_plan_by_a_sanitized_host_program(tmp_path):
    exe = os.path.join(str(tmp_path), "fwd_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "regneuralde.jl_amd", "csrc"), os.path.join(ROOT, "tests", "save_host", "fwd_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "forward plan checks passed" in r.stdout
