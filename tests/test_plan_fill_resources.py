"""Resource budget of the plan fill (plan_fill_kernel<NBITS>, NBITS = 0..6 panel bits), read from the code object
metadata hipcc emits for gfx950.  Four 512-thread workgroups per CU need 8 wavefronts per SIMD, i.e. at most 64
VGPRs, and at most 40 KiB of LDS each; a spill would put scratch traffic into a kernel that is one pass over A.
Metadata only: no assertion on instruction patterns."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "matrixextra_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    asm = tmp_path_factory.mktemp("fill") / "spmm_plan.s"
    flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=on".split()          # as in csrc/Makefile
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "spmm_plan.hip"), "-o", str(asm)],
                   check=True, capture_output=True, timeout=600)
    text = asm.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for block in re.split(r"\n  - (?=\.agpr_count)", meta)[1:]:
        fields = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", block, flags=re.M))
        out[fields["name"]] = fields
    return out


def test_every_fill_instantiation_fits_four_workgroups_per_cu(kernel_metadata):
    fills = {k: f for k, f in kernel_metadata.items() if "plan_fill_kernel" in k}
    # plan_fill_kernel<NBITS>: Itanium mangling of the template argument
    assert sorted(re.search(r"plan_fill_kernelILi(\d+)E", k).group(1) for k in fills) == [str(b) for b in range(7)], sorted(fills)
    for name, f in fills.items():
        assert int(f["vgpr_count"]) <= 64, name
        assert int(f["agpr_count"]) == 0, name
        assert int(f["group_segment_fixed_size"]) <= 40960, name
        assert int(f["private_segment_fixed_size"]) == 0, name
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, name
