"""The QP forms of a fleet's check kernels (csrc/fleet_check_kernels.hpp: fleet_qp_point_products_kernel, fleet_qp_eval_kernel)
are kernels of their own names in the gfx950 code object -- not instantiations of the LP kernels' names, which
tests/test_isa_fleet_checks.py finds by a unique mangled name -- and cost no scratch beyond the kernels they are made of.
Reads the code object's metadata only (hipcc cross-compiles without a GPU), in the style of tests/test_isa_fleet_checks.py."""
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
    out = tmp_path_factory.mktemp("isa_fleet_qp_checks") / "pdhg.s"
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


def test_the_qp_point_products_kernel_is_there_without_scratch(isa):
    assert _scratch(isa, "fleet_qp_point_products_kernel") == 0


def test_the_qp_evaluation_kernel_spills_no_more_than_its_parts(isa):
    parts = {k: _scratch(isa, k) for k in ("eval_rows_kernel", "eval_cols_kernel", "dist2_kernel", "multi_final_kernel")}
    fleet = _scratch(isa, "fleet_qp_eval_kernel")
    assert fleet <= max(parts.values()), f"fleet_qp_eval_kernel: {fleet} bytes of scratch per lane, its parts have {parts}"


def test_the_lp_kernels_keep_their_names_to_themselves(isa):
    for kernel in ("fleet_point_products_kernel", "fleet_eval_kernel", "fleet_tr_kernel"):
        _scratch(isa, kernel)             # (asserts that exactly one kernel carries the name)
