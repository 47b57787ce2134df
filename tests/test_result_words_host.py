"""The result words of the one-launch kernels (csrc/grid_sync.hpp): k values, a checksum and a sequence number that a
kernel writes into pinned memory WITHOUT a fence, so the host may see any mixture of this launch's and the last one's
words and must accept nothing but the whole of this launch's.  No GPU: tests/result_words_driver.hip is compiled for the
host against the header's own publish_words / words_checksum / words_ready and run on ordinary memory.  For every case
and two consecutive sequence numbers: a published buffer is accepted and returns the bits it was given (NaN, -0.0 and
all-ones among them); the zeroed buffer of the allocation is refused for every sequence number, 0 included; a buffer in
which one value word, the checksum word or the sequence word is still the last launch's is refused; so is a reader that
asks for k - 1 or k + 1 words.  Skips without hipcc, like the ISA tests."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHECKS = ["payloads_differ_from_previous_launch", "published_accepted_bitwise", "previous_launch_refused_for_seq",
          "published_refused_for_other_seq", "zero_buffer_refused", "stale_value_word_refused", "stale_checksum_refused",
          "stale_sequence_refused", "other_count_refused"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if not hipcc:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("result_words") / "driver"
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "firstorderlp.jl_amd", "csrc"), "-o", str(exe),
                        os.path.join(ROOT, "tests", "result_words_driver.hip")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(exe)


def _check(driver, cap, k, seq):
    r = subprocess.run([driver, "check", str(cap), str(k), str(seq)], capture_output=True, text=True, timeout=60)
    lines = r.stdout.split("\n")
    assert r.returncode == 0, r.stdout + r.stderr
    want = CHECKS + (["payloads_hold_nan_negzero_allones"] if k >= 13 else [])
    for s in (seq, seq + 1):          # every property was looked at, for both launches, and held
        for name in want:
            assert f"PASS seq{s} {name}" in lines, (name, s, r.stdout)
    assert not [ln for ln in lines if ln.startswith("FAIL")], r.stdout


def _library_pairs(driver):
    r = subprocess.run([driver, "pairs"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    pairs = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in r.stdout.strip().split("\n")}
    assert sorted(pairs) == ["ev_host", "res_host", "steps_res"], pairs
    return pairs


@pytest.mark.parametrize("seq", [1, 2 ** 40 + 7])
@pytest.mark.parametrize("k", [1, 6, 13, 32])
def test_words_of_k_values(driver, k, seq):
    cap = _library_pairs(driver)["ev_host"][0]       # the buffer whose count varies by call
    assert cap >= 32
    _check(driver, cap, k, seq)


@pytest.mark.parametrize("seq", [1, 2 ** 40 + 7])
@pytest.mark.parametrize("buffer", ["res_host", "steps_res", "ev_host"])
def test_the_librarys_buffers(driver, buffer, seq):
    cap, k = _library_pairs(driver)[buffer]          # the header's constants
    _check(driver, cap, k, seq)
