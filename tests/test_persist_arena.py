"""The hand-off arena of the persistent decode (nanollama_amd/csrc/nl_persist.h: pd_arena) checked on the CPU: a stand-alone host
program (tests/host/pd_arena_check.hip) that walks every granule each phase of the kernel stores or polls -- x, the q | k | v rows
per unit, o per head, x', h through pd_h_row, the helpers' records, the 256 argmax granules, the token word -- for both
instantiated shape classes, their kv-head counts and 1 .. 16 layers: 16-byte aligned areas, no two areas overlapping, the largest
offset plus its width inside the total.  Built with hipcc and run once plain and once under the address and undefined-behaviour
sanitizers.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "pd_arena_check.hip")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("san", [(), ("-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all")],
                         ids=["plain", "asan_ubsan"])
def test_arena_areas_are_aligned_disjoint_and_inside_the_total(tmp_path, san):
    if not os.path.exists(HIPCC):
        pytest.fail(f"{HIPCC} is missing: the host check is built with the compiler the library is built with")
    exe = tmp_path / "pd_arena_check"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *san,
                           "-I", os.path.join(ROOT, "nanollama_amd", "csrc"), "-o", str(exe), SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pd_arena_check: ok" in r.stdout, r.stdout + r.stderr
