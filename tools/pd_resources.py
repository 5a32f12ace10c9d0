"""Register and scratch figures of every pd_decode_kernel instantiation (nanollama_amd/csrc/nl_persist.h), read from the code
object metadata of a device-only compile: nl_engine.hip with the Makefile's flags plus -S --cuda-device-only.  No GPU needed.
The kernel has no register headroom (144 of 256 VGPRs hold weights): a change must leave 0 spilled vector registers and 0 bytes
of scratch on all of them.  Exit status 1 if one does not.
usage: python tools/pd_resources.py [--keep-asm FILE] [extra compiler flags, e.g. -DNL_PD_STAMPS]"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nanollama_amd", "csrc")
FIELDS = (".vgpr_count", ".vgpr_spill_count", ".sgpr_count", ".sgpr_spill_count", ".private_segment_fixed_size")


def makefile_flags():
    """HIPCC and CXXFLAGS as csrc/Makefile has them (the -D lines that carry hashes do not change code)"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1)
    arch = os.environ.get("ARCH") or re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    return hipcc, flags


def compile_asm(out, extra=()):
    hipcc, flags = makefile_flags()
    cmd = [hipcc] + flags + ['-DNL_SRC_SHA="x"', '-DNL_GIT_HEAD="x"', "-S", "--cuda-device-only", "-o", out, "nl_engine.hip"] + list(extra)
    subprocess.check_call(cmd, cwd=CSRC)


def kernel_resources(asm_path, needle="pd_decode_kernel"):
    """{mangled name: {field: int}} of the kernels whose name holds `needle`, from the amdhsa.kernels metadata"""
    out, cur = {}, None
    in_meta = False
    for line in open(asm_path):
        if line.startswith("amdhsa.kernels:"):
            in_meta = True
            continue
        if not in_meta:
            continue
        m = re.match(r"\s+(?:- )?(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip()
        if line.lstrip().startswith("- ") and line.startswith("  - "):
            cur = {}                       # a new kernel entry: its name follows among the keys
            cur["_first"] = (key, val)
        if cur is None:
            continue
        if key in FIELDS:
            cur[key] = int(val)
        if key == ".name" and needle in val:
            out[val] = cur
    for v in out.values():
        v.pop("_first", None)
    return out


def main():
    args = sys.argv[1:]
    keep = None
    if args[:1] == ["--keep-asm"]:
        keep, args = args[1], args[2:]
    with tempfile.TemporaryDirectory() as tmp:
        asm = keep or os.path.join(tmp, "nl_engine.s")
        compile_asm(asm, args)
        res = kernel_resources(asm)
    if not res:
        raise SystemExit("no pd_decode_kernel instantiation in the metadata")
    bad = 0
    print(f"{'kernel':58s} vgpr vgpr_spill sgpr sgpr_spill scratch_bytes")
    for name in sorted(res):
        r = res[name]
        short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
        short = re.sub(r"^void nl::|\(nl::PdParams\)$", "", short)
        print(f"{short:58s} {r['.vgpr_count']:4d} {r['.vgpr_spill_count']:10d} {r['.sgpr_count']:4d} {r['.sgpr_spill_count']:10d} {r['.private_segment_fixed_size']:13d}")
        bad += r[".vgpr_spill_count"] != 0 or r[".private_segment_fixed_size"] != 0
    if bad:
        raise SystemExit(f"{bad} instantiation(s) spill vector registers or use scratch")


if __name__ == "__main__":
    main()
