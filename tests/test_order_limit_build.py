"""topk.hip (the ORDER BY ... LIMIT k kernels) compiles for gfx950 with the product build's flags and none of its
kernels uses private-memory scratch: a run-time indexed copy of the key table or a spilled sort comparator would put
every row's digit extraction behind scratch loads. Read from the code object's metadata notes on the CPU (hipcc
cross-compiles without a GPU), in the manner of test_kernel_resources.py."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "netsdb_amd", "csrc", "kernels")
KERNELS = ("ol_diff_kernel", "ol_hist0_kernel", "ol_pass_kernel", "ol_sort_kernel")


def _setup_module():
    spec = importlib.util.spec_from_file_location("nsdb_setup_for_test", os.path.join(ROOT, "setup.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_topk_is_part_of_the_product_build():
    assert "topk.hip" in _setup_module().HIP_SOURCES


def test_topk_kernels_compile_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(hipcc) or not os.path.exists(readelf):
        pytest.skip("hipcc / llvm-readelf not available")
    st = _setup_module()
    inc, defs, _ = st._torch_flags()
    obj = str(tmp_path / "topk.hsaco")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-fno-gpu-rdc", "-munsafe-fp-atomics", "-O3", "-std=c++17",
           "-fPIC"] + defs + inc + st.PER_FILE_FLAGS.get("topk.hip", []) + [
        "--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(KDIR, "topk.hip"), "-o", obj]
    p = subprocess.run(cmd, cwd=KDIR, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    notes = subprocess.run([readelf, "--notes", obj], capture_output=True, text=True, timeout=120).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    assert len(names) == len(scratch) >= len(KERNELS), notes[-2000:]
    for k in KERNELS:
        assert any(k in nm for nm in names), (k, names)
    assert all(x == 0 for x in scratch), list(zip(names, scratch))
