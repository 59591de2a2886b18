"""textparse.hip (the delimited-text parser) is part of the product build, compiles for gfx950 with the product build's
flags, holds each of its four kernels once, and none of them uses private-memory scratch: the decode kernel walks the
fields in a wave-uniform loop, so a field's kind and output pointer are scalar loads from the kernel argument instead
of a run-time indexed private array, and its 16-byte window is shifted, never indexed. Read from the code object's
metadata notes on the CPU (hipcc cross-compiles without a GPU), in the manner of test_string_order_build.py."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "netsdb_amd", "csrc", "kernels")
KERNELS = ("tp_count_kernel", "tp_scan_kernel", "tp_rows_kernel", "tp_decode_kernel")


def _setup_module():
    spec = importlib.util.spec_from_file_location("nsdb_setup_for_test", os.path.join(ROOT, "setup.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_textparse_kernels_compile_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(hipcc) or not os.path.exists(readelf):
        pytest.skip("hipcc / llvm-readelf not available")
    st = _setup_module()
    assert "textparse.hip" in st.HIP_SOURCES and "textparse_bind.cpp" in st.HIP_SOURCES
    flags = st.PER_FILE_FLAGS.get("textparse.hip", [])
    assert not any("fast-math" in f and "no-" not in f for f in flags)      # a float is one IEEE division
    inc, defs, _ = st._torch_flags()
    obj = str(tmp_path / "textparse.hsaco")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-fno-gpu-rdc", "-munsafe-fp-atomics", "-O3", "-std=c++17",
           "-fPIC"] + defs + inc + flags + [
        "--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(KDIR, "textparse.hip"), "-o", obj]
    p = subprocess.run(cmd, cwd=KDIR, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    notes = subprocess.run([readelf, "--notes", obj], capture_output=True, text=True, timeout=120).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    assert len(names) == len(scratch) == len(KERNELS), notes[-2000:]
    for k in KERNELS:
        assert sum(k in nm for nm in names) == 1, (k, names)
    assert all(x == 0 for x in scratch), list(zip(names, scratch))
