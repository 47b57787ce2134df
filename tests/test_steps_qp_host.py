"""The QP form of the multi-step persistent kernel (csrc/trial_kernel.hpp) arrives as two more instantiations of
steps_kernel behind the existing PDHG_DEVICE_LOOP; the two LP instantiations, which sit at their register limit, must
stay the kernels they were.  Host side: the header's row of the variable, the four instantiations in the gfx950 code
object, and the LP forms' register and scratch figures against those of the parent commit.  Names and metadata fields
only.  Compiles the device code (hipcc cross-compiles without a GPU), in the style of tests/test_isa_small_qp.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (LOCAL, QP) -> VGPRs, spilled SGPRs, scratch bytes per lane of the LP forms, from a cross-compilation of commit
# 97ecc1cf0dc64966db22d0f4e2a17ce531298ce0 (the parent of the QP form) with the flags below; there the kernels were
# steps_kernel<false> and steps_kernel<true>
PARENT_LP = {(0, 0): (128, 188, 32), (1, 0): (128, 250, 36)}


def test_the_header_row_names_qps_and_keeps_its_format():
    with open(os.path.join(ROOT, "include", "pdhg_hip.h")) as f:
        head = f.read()
    row = re.search(r"^ \*   PDHG_DEVICE_LOOP\s+1 \| 0\s+(.*(?:\n \*\s{20,}\S.*)*)", head, flags=re.M)
    assert row, "no PDHG_DEVICE_LOOP row of the form `1 | 0`"
    text = row.group(1)
    assert "QP" in text and "several take_steps per launch of the persistent kernel" in text
    assert re.search(r"[Uu]nset: LPs", text) and "launch by launch" in text


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if not hipcc:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_steps_qp") / "pdhg.s"
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", "-o", str(out), os.path.join(ROOT, "firstorderlp.jl_amd", "csrc", "pdhg_hip.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def _steps_kernels(isa):
    """{(LOCAL, QP): metadata entry} of the steps_kernel instantiations (small_lp_steps_kernel and its kin have other names)."""
    out = {}
    for entry in isa[isa.index("amdhsa.kernels:"):].split("\n  - "):
        m = re.search(r"\.name:\s+_ZN\S*?\d+steps_kernelILb([01])ELb([01])EEEv\S*\n", entry)
        if m:
            key = (int(m.group(1)), int(m.group(2)))
            assert key not in out, key
            out[key] = entry
    return out


def _field(entry, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, entry).group(1))


def test_four_instantiations(isa):
    assert sorted(_steps_kernels(isa)) == [(0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.mark.parametrize("local", [0, 1], ids=["all_xcd", "xcd_local"])
def test_the_lp_forms_keep_their_registers_and_scratch(isa, local):
    entry = _steps_kernels(isa)[(local, 0)]
    got = (_field(entry, "vgpr_count"), _field(entry, "sgpr_spill_count"), _field(entry, "private_segment_fixed_size"))
    assert got == PARENT_LP[(local, 0)], f"steps_kernel<{local}, 0>: (VGPRs, spilled SGPRs, scratch bytes) {got}, the parent had {PARENT_LP[(local, 0)]}"
