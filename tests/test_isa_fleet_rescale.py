"""fleet_rescale_kernel (csrc/fleet_rescale_kernels.hpp) runs the row bodies of row_op_kernel and scale_csr_kernel and the
element bodies of the resc_* kernels on an argument block read from a table in device memory, step after step in one
workgroup.  It must be in the gfx950 code object, and neither the table nor running every step in one kernel may cost
scratch: its private segment is no larger than the largest among row_op_kernel's instantiations and scale_csr_kernel in
the same dump.  Reads the code object's metadata only (hipcc cross-compiles without a GPU), in the style of
tests/test_isa_fleet_checks.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if not hipcc:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_fleet_rescale") / "pdhg.s"
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", "-o", str(out), os.path.join(ROOT, "firstorderlp.jl_amd", "csrc", "pdhg_hip.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def _scratch(isa, kernel):
    """{mangled name: private_segment_fixed_size} of the kernels named `kernel` (`<length><kernel>E`, or `...I` for the
    instantiations of a template)."""
    tags = (f"{len(kernel)}{kernel}E", f"{len(kernel)}{kernel}I")
    names = sorted({n for n in re.findall(r"\.name:\s+(_ZN\S+)", isa) if any(t in n for t in tags) and not n.endswith(".kd")})
    found = {}
    for name in names:
        meta = isa[isa.index(".name:           " + name):]
        meta = meta[:meta.index("\n  - ", 1) if "\n  - " in meta[1:] else len(meta)]
        found[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    return found


def test_the_kernel_is_in_the_code_object(isa):
    assert len(_scratch(isa, "fleet_rescale_kernel")) == 1


def test_the_kernel_spills_no_more_than_the_kernels_whose_bodies_it_runs(isa):
    fleet = _scratch(isa, "fleet_rescale_kernel")
    parts = {**_scratch(isa, "row_op_kernel"), **_scratch(isa, "scale_csr_kernel")}
    assert len(fleet) == 1 and len(parts) == 4, (fleet, parts)       # three statistics, one scaling kernel
    (size,) = fleet.values()
    assert size <= max(parts.values()), f"fleet_rescale_kernel: {size} bytes of scratch per lane, its parts have {parts}"
