"""The many-LP launch (csrc/small_lp_kernel.hpp: small_lp_fleet_kernel) runs the solo small-LP kernel's body on an
argument block it reads from a table in device memory instead of its kernel arguments.  Both instantiations must be in
the gfx950 code object, and reading the block from memory must not cost them scratch: each one's private segment is no
larger than that of the solo kernel with the same thread count, in the same dump.  Compiles the device code (hipcc
cross-compiles without a GPU), in the style of tests/test_isa_waits.py."""
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
    out = tmp_path_factory.mktemp("isa_fleet") / "pdhg.s"
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", "-o", str(out), os.path.join(ROOT, "firstorderlp.jl_amd", "csrc", "pdhg_hip.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def _scratch(isa, kernel, threads):
    """private_segment_fixed_size of the one kernel whose mangled name holds `<kernel>ILi<threads>E`."""
    names = [n for n in re.findall(r"\.name:\s+(_ZN\S+)", isa) if f"{kernel}ILi{threads}E" in n and not n.endswith(".kd")]
    assert len(set(names)) == 1, (kernel, threads, names)
    meta = isa[isa.index(".name:           " + names[0]):]
    meta = meta[:meta.index("\n  - ", 1) if "\n  - " in meta[1:] else len(meta)]
    return int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))


@pytest.mark.parametrize("threads", [256, 1024])
def test_fleet_kernel_is_there_and_spills_no_more_than_the_solo_kernel(isa, threads):
    assert re.search(r"\n_ZN[^\n:]*small_lp_fleet_kernelILi%dE[^\n:]*:" % threads, isa), f"no small_lp_fleet_kernel<{threads}> in the ISA"
    fleet = _scratch(isa, "small_lp_fleet_kernel", threads)
    solo = _scratch(isa, "small_lp_steps_kernel", threads)
    assert fleet <= solo, f"small_lp_fleet_kernel<{threads}>: {fleet} bytes of scratch per lane, the solo kernel has {solo}"
