"""The host side of a launch that carries several TrackedFFJORD batches, what needs no GPU: csrc/rnde_group_plan.h by a stand-alone program
(tests/group_host/group_plan_check.cpp) compiled with the address and undefined-behaviour sanitizers -- the group table (columns to tiles,
first tile and caller column of each group, the padded stride) against tables written out by hand at B = 1, 15, 16, 17, for unequal groups
and for more than 32 tiles, and every refusal string of rnde_ffjord_reserve_groups / rnde_ffjord_forward_groups for every limit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_plan_by_a_sanitized_host_program(tmp_path):
    exe = os.path.join(str(tmp_path), "group_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "regneuralde.jl_amd", "csrc"), os.path.join(ROOT, "tests", "group_host", "group_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "group plan checks passed" in r.stdout
