"""The host part of csrc/rnde_meet.h (the workgroup meeting every one-launch solve and sweep rests on): the verdict over the check
words, the tag formula and the epoch bump, checked by a stand-alone program (tests/meet_host/meet_host_check.cpp) compiled with the address and undefined-behaviour sanitizers.  No GPU is touched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_meet_verdict_tags_and_epoch_bump(tmp_path):
    exe = os.path.join(str(tmp_path), "meet_host_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "regneuralde.jl_amd", "csrc"), os.path.join(ROOT, "tests", "meet_host", "meet_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "meet host checks passed" in r.stdout
