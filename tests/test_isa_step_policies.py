"""The constant and the Malitsky-Pock policy run the small-LP kernel's body (csrc/small_lp_kernel.hpp) behind kernels of
their own names, solo and as a fleet's shared launch.  All eight instantiations must be in the gfx950 code object, and
none may cost more scratch than the adaptive solo kernel with the same thread count, in the same dump.  Names and that
one metadata field only.  Compiles the device code (hipcc cross-compiles without a GPU), in the style of
tests/test_isa_fleet.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KERNELS = ("small_lp_constant_kernel", "small_lp_malitsky_pock_kernel", "small_fleet_constant_kernel",
               "small_fleet_malitsky_pock_kernel")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if not hipcc:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_step_policies") / "pdhg.s"
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
@pytest.mark.parametrize("kernel", NEW_KERNELS)
def test_policy_kernel_is_there_and_spills_no_more_than_the_adaptive_solo_kernel(isa, kernel, threads):
    assert re.search(r"\n_ZN[^\n:]*%sILi%dE[^\n:]*:" % (kernel, threads), isa), f"no {kernel}<{threads}> in the ISA"
    # (the names by which tests/test_isa_fleet.py finds the adaptive kernels must not match the new ones)
    assert "small_lp_steps_kernelILi" not in kernel + "ILi" and "small_lp_fleet_kernelILi" not in kernel + "ILi"
    mine = _scratch(isa, kernel, threads)
    solo = _scratch(isa, "small_lp_steps_kernel", threads)
    assert mine <= solo, f"{kernel}<{threads}>: {mine} bytes of scratch per lane, the adaptive solo kernel has {solo}"
