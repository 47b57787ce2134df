"""Small QPs run the small-LP kernel's body in its QP form (csrc/small_lp_kernel.hpp) behind kernels of their own names,
solo and as a fleet's shared launch, for the adaptive and the constant policy.  All eight instantiations must be in the
gfx950 code object, none may use scratch, and reading the argument block from a table in device memory must not cost
the fleet forms more of it than the solo forms have.  Names and that one metadata field only.  Compiles the device code
(hipcc cross-compiles without a GPU), in the style of tests/test_isa_fleet.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("small_qp_steps_kernel", "small_qp_fleet_kernel"), ("small_qp_constant_kernel", "small_qp_fleet_constant_kernel"))


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if not hipcc:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_small_qp") / "pdhg.s"
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
@pytest.mark.parametrize("solo,fleet", PAIRS)
def test_qp_kernels_are_there_and_use_no_scratch(isa, solo, fleet, threads):
    for kernel in (solo, fleet):
        assert re.search(r"\n_ZN[^\n:]*%sILi%dE[^\n:]*:" % (kernel, threads), isa), f"no {kernel}<{threads}> in the ISA"
    mine, theirs = _scratch(isa, fleet, threads), _scratch(isa, solo, threads)
    assert mine <= theirs, f"{fleet}<{threads}>: {mine} bytes of scratch per lane, {solo} has {theirs}"
    assert theirs == 0 and mine == 0, f"scratch per lane: {solo}<{threads}> {theirs}, {fleet}<{threads}> {mine}"
