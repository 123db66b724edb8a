"""Resource budget of the planned sweep (spmm_plan_kernel), read from the code object metadata hipcc emits for
gfx950.  One 1024-thread workgroup per CU needs 16 wavefronts per CU, i.e. at most 128 VGPRs; the accumulators of
1024 rows must fit the CU's 160 KiB of LDS; a spill would put scratch traffic into the B-line pipeline.
Metadata only: no assertion on instruction patterns."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "matrixextra_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

# spmm_plan_kernel<real_t, COLMAJOR, 16>: Itanium mangling of the template arguments
HEADLINE = {"f64 colmajor": "IdLb1ELi16EE", "f64 rowmajor": "IdLb0ELi16EE",
            "f32 colmajor": "IfLb1ELi16EE", "f32 rowmajor": "IfLb0ELi16EE"}


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    asm = tmp_path_factory.mktemp("sweep") / "spmm.s"
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


@pytest.mark.parametrize("which", sorted(HEADLINE))
def test_sixteen_wave_sweep_fits_one_workgroup_per_cu(kernel_metadata, which):
    names = [k for k in kernel_metadata if "spmm_plan_kernel" + HEADLINE[which] in k]
    assert len(names) == 1, names
    f = kernel_metadata[names[0]]
    assert int(f["vgpr_count"]) <= 128
    assert int(f["agpr_count"]) == 0
    assert int(f["group_segment_fixed_size"]) <= 163840
    assert int(f["private_segment_fixed_size"]) == 0
    assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0
