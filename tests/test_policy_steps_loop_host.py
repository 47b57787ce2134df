"""The constant and the Malitsky-Pock policy in the persistent multi-step kernel (csrc/trial_kernel.hpp:
policy_steps_kernel<LOCAL, POLICY, QP>, behind PDHG_DEVICE_LOOP=1): what can be checked without a GPU.  The six
instantiations are in the gfx950 code object, steps_kernel keeps exactly its four, the header's row of the variable keeps
its format and names the two policies, and the two calls' argument checks still return before any device work.  Names
and metadata fields only; the device code is cross-compiled as tests/test_steps_qp_host.py does."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from firstorderlp_jl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTANT, MALITSKY_POCK = 1, 2      # enum SmallPolicy, csrc/common.hpp


def test_the_header_row_keeps_its_format_and_names_the_two_policies():
    with open(os.path.join(ROOT, "include", "pdhg_hip.h")) as f:
        head = f.read()
    row = re.search(r"^ \*   PDHG_DEVICE_LOOP\s+1 \| 0\s+(.*(?:\n \*\s{20,}\S.*)*)", head, flags=re.M)
    assert row, "no PDHG_DEVICE_LOOP row of the form `1 | 0`"
    text = " ".join(re.sub(r"^ \*\s+", "", line) for line in row.group(1).split("\n"))
    assert "QP" in text and "several take_steps per launch of the persistent kernel" in text
    assert re.search(r"[Uu]nset: LPs", text) and "launch by launch" in text
    assert "constant" in text and "Malitsky-Pock" in text
    assert "pdhg_take_steps_constant" in text and "pdhg_take_steps_malitsky_pock" in text


def test_the_policy_enum_is_what_the_kernel_names_are_read_with():
    with open(os.path.join(ROOT, "firstorderlp.jl_amd", "csrc", "common.hpp")) as f:
        m = re.search(r"enum SmallPolicy \{ SMALL_ADAPTIVE = (\d), SMALL_CONSTANT = (\d), SMALL_MALITSKY_POCK = (\d) \};", f.read())
    assert m and tuple(int(v) for v in m.groups()) == (0, CONSTANT, MALITSKY_POCK)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel name: metadata entry} of the gfx950 code object."""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if not hipcc:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_policy_steps") / "pdhg.s"
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", "-o", str(out), os.path.join(ROOT, "firstorderlp.jl_amd", "csrc", "pdhg_hip.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = out.read_text()
    found = {}
    for entry in isa[isa.index("amdhsa.kernels:"):].split("\n  - "):
        m = re.search(r"\.name:\s+(\S+)\n", entry)
        if m:
            found[m.group(1)] = entry
    return found


def test_the_six_instantiations_of_the_new_kernel(kernels):
    got = set()
    for name in kernels:
        m = re.search(r"\d+policy_steps_kernelILb([01])ELi(\d+)ELb([01])EEEv", name)
        if m:
            key = tuple(int(v) for v in m.groups())
            assert key not in got, key
            got.add(key)
    want = {(local, policy, qp) for local in (0, 1) for policy, qp in ((CONSTANT, 0), (CONSTANT, 1), (MALITSKY_POCK, 0))}
    assert got == want, sorted(got)


def test_steps_kernel_keeps_exactly_its_four(kernels):
    got = sorted(tuple(int(v) for v in m.groups()) for m in
                 (re.search(r"_ZN\S*?\d+steps_kernelILb([01])ELb([01])EEEv", name) for name in kernels) if m)
    assert got == [(0, 0), (0, 1), (1, 0), (1, 1)]
    # the new kernel's name puts no digit directly in front of `steps_kernel`: the pattern above does not see it
    assert not any(re.search(r"\d+steps_kernelI\S*PolicyStepsArgs", name) for name in kernels)


def test_the_new_forms_need_no_more_scratch_than_their_adaptive_counterparts(kernels):
    def scratch(pattern):
        (entry,) = [e for name, e in kernels.items() if re.search(pattern, name)]
        return int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1))
    for local in (0, 1):
        for policy, qp in ((CONSTANT, 0), (CONSTANT, 1), (MALITSKY_POCK, 0)):
            new = scratch(r"\d+policy_steps_kernelILb%dELi%dELb%dEEEv" % (local, policy, qp))
            old = scratch(r"_ZN\S*?\d+steps_kernelILb%dELb%dEEEv" % (local, qp))
            assert new <= old, (local, policy, qp, new, old)


def test_argument_checks_return_what_they_returned_before(monkeypatch):
    L = _lib.lib()
    d, i64, i32 = ctypes.c_double, ctypes.c_int64, ctypes.c_int
    ref = ctypes.byref
    fake = ctypes.c_void_p(8)       # never looked at: the checks below return first
    for setting in (None, "0", "1"):
        monkeypatch.delenv("PDHG_DEVICE_LOOP", raising=False)
        if setting is not None:
            monkeypatch.setenv("PDHG_DEVICE_LOOP", setting)
        ss, ratio, kkt, it, err, done = d(1.0), d(1.0), d(0.0), i64(0), i32(0), i64(7)
        assert L.pdhg_take_steps_constant(None, 3, 1.0, 1.0, ref(kkt), ref(done)) == -1
        assert done.value == 0 and kkt.value == 0.0
        done = i64(7)
        assert L.pdhg_take_steps_malitsky_pock(None, 3, 0.7, 0.99, 1.0, ref(ss), ref(ratio), 1.0, ref(it), ref(kkt), ref(err),
                                               ref(done)) == -1
        assert (ss.value, ratio.value, it.value, kkt.value, done.value) == (1.0, 1.0, 0, 0.0, 0)
        assert L.pdhg_take_steps_constant(fake, -1, 1.0, 1.0, ref(kkt), ref(done)) == -2
        assert L.pdhg_take_steps_malitsky_pock(fake, -1, 0.7, 0.99, 1.0, ref(ss), ref(ratio), 1.0, ref(it), ref(kkt), ref(err),
                                               ref(done)) == -2
        assert b"n_steps < 0" in L.pdhg_last_error()
        assert L.pdhg_take_steps_constant(fake, 3, 1.0, 1.0, ref(kkt), None) == -1
        assert (ss.value, ratio.value, it.value, kkt.value) == (1.0, 1.0, 0, 0.0)
