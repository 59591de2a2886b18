"""strings.hip (the string-column kernels, with the ORDER BY pair str_order_words_kernel / str_cmp_pairs_kernel) compiles
for gfx950 with the product build's flags and none of its kernels uses private-memory scratch: the order-words kernel
writes its up to four chunk words straight to their columns (a run-time indexed register array would live in scratch),
and one lane per row leaves no room for spills in a kernel that is a few loads per row. Read from the code object's
metadata notes on the CPU (hipcc cross-compiles without a GPU), in the manner of test_order_by_build.py."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "netsdb_amd", "csrc", "kernels")
ORDER_KERNELS = ("str_order_words_kernel", "str_cmp_pairs_kernel")
KERNELS = ORDER_KERNELS + ("str_hash_kernel", "str_like_kernel", "like_occ_kernel", "like_rows_kernel",
                           "str_gather_kernel", "str_slice_kernel", "str_pack_kernel", "str_eq_pairs_kernel")


def _setup_module():
    spec = importlib.util.spec_from_file_location("nsdb_setup_for_test", os.path.join(ROOT, "setup.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_string_kernels_compile_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(hipcc) or not os.path.exists(readelf):
        pytest.skip("hipcc / llvm-readelf not available")
    st = _setup_module()
    assert "strings.hip" in st.HIP_SOURCES                  # the file is part of the product build
    inc, defs, _ = st._torch_flags()
    obj = str(tmp_path / "strings.hsaco")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-fno-gpu-rdc", "-munsafe-fp-atomics", "-O3", "-std=c++17",
           "-fPIC"] + defs + inc + st.PER_FILE_FLAGS.get("strings.hip", []) + [
        "--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(KDIR, "strings.hip"), "-o", obj]
    p = subprocess.run(cmd, cwd=KDIR, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    notes = subprocess.run([readelf, "--notes", obj], capture_output=True, text=True, timeout=120).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    assert len(names) == len(scratch) >= len(KERNELS), notes[-2000:]
    for k in KERNELS:
        assert sum(k in nm for nm in names) == 1, (k, names)
    assert all(x == 0 for x in scratch), list(zip(names, scratch))
