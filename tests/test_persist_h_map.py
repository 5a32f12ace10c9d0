"""The h granule layout of the persistent decode (nanollama_amd/csrc/nl_persist.h: pd_h_vpg, pd_h_row) checked on the CPU: a
stand-alone host program (tests/host/pd_h_map_check.hip) that walks the map for both instantiated shapes, built with hipcc and
run once plain and once under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "pd_h_map_check.hip")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("san", [(), ("-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all")],
                         ids=["plain", "asan_ubsan"])
def test_h_granule_ownership_map(tmp_path, san):
    if not os.path.exists(HIPCC):
        pytest.fail(f"{HIPCC} is missing: the host check is built with the compiler the library is built with")
    exe = tmp_path / "pd_h_map_check"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", *san,
                           "-I", os.path.join(ROOT, "nanollama_amd", "csrc"), "-o", str(exe), SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "pd_h_map_check: ok" in r.stdout, r.stdout + r.stderr
