"""The batched product kernels (csrc/batch_kernels.hpp) must issue the gathers of one step -- BATCH_U = 8 entries
per lane -- back to back, with no `s_waitcnt vmcnt` between them: the gathers are what the member-interleaved layout
widens, and a wait between two of them would leave one in flight per lane.  Compiles the device code (hipcc
cross-compiles without a GPU) and reads the instruction stream, in the style of tests/test_isa_waits.py."""
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
    out = tmp_path_factory.mktemp("isa_batch") / "pdhg.s"
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", "-o", str(out), os.path.join(ROOT, "firstorderlp.jl_amd", "csrc", "pdhg_hip.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def _body(isa, key):
    m = re.search(r"\n(_ZN[^\n:]*" + re.escape(key) + r"[^\n:]*):[^\n]*\n(.*?)\n\s*s_endpgm", isa, re.S)
    assert m, key
    return m.group(2)


def _longest_gather_run(body):
    best = run = 0
    for line in body.split("\n"):
        t = line.strip()
        if t.startswith("global_load_dwordx2") and not t.endswith(" nt"):
            run += 1
            best = max(best, run)
        elif t.startswith("s_waitcnt") and "vmcnt" in t or t.startswith("s_barrier"):
            run = 0
    return best


@pytest.mark.parametrize("key", ["batch_spmv_kernelILi1E", "batch_spmv_kernelILi2E", "batch_long_partial_kernel"])
def test_batched_products_issue_a_step_of_gathers_back_to_back(isa, key):
    run = _longest_gather_run(_body(isa, key))
    assert run >= 8, f"{key}: {run} gathers in flight per lane (8 expected)"


def test_batched_kernels_do_not_spill(isa):
    for name in re.findall(r"\.name:\s+(_ZN12_GLOBAL__N_1\d+batch_\S*)", isa):
        meta = isa[isa.index(".name:           " + name):][:2000]
        size = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
        assert size == 0, f"{name}: {size} bytes of scratch per lane"
