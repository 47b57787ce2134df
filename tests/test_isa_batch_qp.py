"""The kernels a QP batch adds (csrc/batch_kernels.hpp: the pack kernel, the QP primal kernel, the two Q products'
instantiations of batch_spmv_kernel / batch_long_final_kernel, the five-sum final kernel) use no scratch, and the two Q
products keep the BATCH_U = 8 gathers of a step back to back like the products of A.  The method of
tests/test_isa_batch.py: compile the device code (hipcc cross-compiles without a GPU) and read the instruction stream."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mangled-name fragments: MODE_PLAIN = 0 (Q X), BATCH_MODE_QDX = 3 (Q' DX); the QP forms carry one more argument pack
QP_KERNELS = ["batch_pack_kernel", "batch_primal_qp_kernel", "batch_spmv_kernelILi0E", "batch_spmv_kernelILi3E",
              "batch_long_final_kernelILi0E", "batch_long_final_kernelILi3E", "batch_final_kernelIJPKdiEE"]


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if not hipcc:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_batch_qp") / "pdhg.s"
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


@pytest.mark.parametrize("key", ["batch_spmv_kernelILi0E", "batch_spmv_kernelILi3E"])
def test_q_products_issue_a_step_of_gathers_back_to_back(isa, key):
    run = _longest_gather_run(_body(isa, key))
    assert run >= 8, f"{key}: {run} gathers in flight per lane (8 expected)"


@pytest.mark.parametrize("key", QP_KERNELS)
def test_qp_kernels_do_not_spill(isa, key):
    names = [n for n in re.findall(r"\.name:\s+(_ZN12_GLOBAL__N_1\d+batch_\S*)", isa) if key in n]
    assert len(names) == 1, (key, names)
    meta = isa[isa.index(".name:           " + names[0]):][:2000]
    size = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    assert size == 0, f"{names[0]}: {size} bytes of scratch per lane"


def test_qp_kernels_address_global_memory(isa):
    """The members' pointers come out of device memory (BatchMemberDev, the qx table); the kernels must still address them
    as global memory, not through flat instructions (which wait on two counters and cannot be told from LDS traffic)."""
    for key in ("batch_spmv_kernelILi0E", "batch_spmv_kernelILi3E"):
        body = _body(isa, key)
        flat = [t for t in (line.strip() for line in body.split("\n")) if t.startswith("flat_load")]
        assert not flat, f"{key}: {len(flat)} flat loads"
