"""sort.hip (the ORDER BY kernels) compiles for gfx950 with the product build's flags and none of its kernels uses
private-memory scratch: the scatter keeps 16 rows' words, ids and ranks in registers, and a spill or a run-time indexed
copy of the key table would put every row behind scratch loads. Read from the code object's metadata notes on the CPU
(hipcc cross-compiles without a GPU), in the manner of test_order_limit_build.py."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "netsdb_amd", "csrc", "kernels")
KERNELS = ("os_hist_kernel", "os_plan_kernel", "os_load_kernel", "os_count_kernel", "os_scan_kernel",
           "os_scatter_kernel", "os_out_kernel")


def _setup_module():
    spec = importlib.util.spec_from_file_location("nsdb_setup_for_test", os.path.join(ROOT, "setup.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sort_is_part_of_the_product_build():
    assert "sort.hip" in _setup_module().HIP_SOURCES


def test_sort_kernels_compile_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(hipcc) or not os.path.exists(readelf):
        pytest.skip("hipcc / llvm-readelf not available")
    st = _setup_module()
    inc, defs, _ = st._torch_flags()
    obj = str(tmp_path / "sort.hsaco")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-fno-gpu-rdc", "-munsafe-fp-atomics", "-O3", "-std=c++17",
           "-fPIC"] + defs + inc + st.PER_FILE_FLAGS.get("sort.hip", []) + [
        "--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(KDIR, "sort.hip"), "-o", obj]
    p = subprocess.run(cmd, cwd=KDIR, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    notes = subprocess.run([readelf, "--notes", obj], capture_output=True, text=True, timeout=120).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    assert len(names) == len(scratch) == len(lds) >= len(KERNELS), notes[-2000:]
    for k in KERNELS:
        assert any(k in nm for nm in names), (k, names)
    # the word-width templates: a 32-bit and a 64-bit form of every kernel that touches the words
    for k in ("os_load_kernel", "os_count_kernel", "os_scatter_kernel"):
        assert sum(k in nm for nm in names) == 2, (k, names)
    assert all(x == 0 for x in scratch), list(zip(names, scratch))
    assert all(x < 64 * 1024 for x in lds), list(zip(names, lds))
