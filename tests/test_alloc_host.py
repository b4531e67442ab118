"""The owning buffer of csrc/rnde_alloc.h (Buf: every device, pinned and event resource of a handle rests on it) over a host allocator policy
with a live count and a request that fails on demand, checked by a stand-alone program (tests/alloc_host/alloc_host_check.cpp) compiled with
the address and undefined-behaviour sanitizers; the leak check at exit is part of it.  No GPU is touched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_releases_exactly_what_it_holds(tmp_path):
    exe = os.path.join(str(tmp_path), "alloc_host_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "regneuralde.jl_amd", "csrc"), os.path.join(ROOT, "tests", "alloc_host", "alloc_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "alloc host checks passed" in r.stdout
