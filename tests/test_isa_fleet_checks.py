"""The check kernels of a fleet (csrc/fleet_check_kernels.hpp) run the per-member kernels' bodies on an argument block
read from a table in device memory: fleet_tr_kernel the body of tr_small_kernel, fleet_eval_kernel those of
eval_rows_kernel, eval_cols_kernel, dist2_kernel and multi_final_kernel one after the other.  All three must be in the
gfx950 code object, and neither the table nor running several bodies in one kernel may cost scratch: each one's private
segment is no larger than that of the kernels it is made of, in the same dump.  Reads the code object's metadata only
(hipcc cross-compiles without a GPU), in the style of tests/test_isa_fleet.py."""
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
    out = tmp_path_factory.mktemp("isa_fleet_checks") / "pdhg.s"
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", "-o", str(out), os.path.join(ROOT, "firstorderlp.jl_amd", "csrc", "pdhg_hip.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def _scratch(isa, kernel):
    """private_segment_fixed_size of the one kernel whose mangled name holds `<length><kernel>E`."""
    tag = f"{len(kernel)}{kernel}E"
    names = [n for n in re.findall(r"\.name:\s+(_ZN\S+)", isa) if tag in n and not n.endswith(".kd")]
    assert len(set(names)) == 1, (kernel, names)
    meta = isa[isa.index(".name:           " + names[0]):]
    meta = meta[:meta.index("\n  - ", 1) if "\n  - " in meta[1:] else len(meta)]
    return int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))


def test_the_trust_region_kernel_spills_no_more_than_the_solo_kernel(isa):
    fleet, solo = _scratch(isa, "fleet_tr_kernel"), _scratch(isa, "tr_small_kernel")
    assert fleet <= solo, f"fleet_tr_kernel: {fleet} bytes of scratch per lane, tr_small_kernel has {solo}"


def test_the_evaluation_kernel_spills_no_more_than_its_parts(isa):
    parts = {k: _scratch(isa, k) for k in ("eval_rows_kernel", "eval_cols_kernel", "dist2_kernel", "multi_final_kernel")}
    fleet = _scratch(isa, "fleet_eval_kernel")
    assert fleet <= max(parts.values()), f"fleet_eval_kernel: {fleet} bytes of scratch per lane, its parts have {parts}"


def test_the_point_products_kernel_is_there_without_scratch(isa):
    assert _scratch(isa, "fleet_point_products_kernel") == 0
