"""PDHG_SMALL_QP (small QPs in the one-workgroup LDS kernel, csrc/small_lp_kernel.hpp) is a documented run-time variable:
tabled in include/pdhg_hip.h, named in the README's list, and the two counts say so."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_table():
    header = open(os.path.join(ROOT, "include", "pdhg_hip.h")).read()
    head = header[:header.index("#ifndef PDHG_HIP_H_")]
    return head, re.findall(r"^ \*   (PDHG_[A-Z0-9_]+) ", head, flags=re.M)


def test_small_qp_is_tabled_in_the_header():
    head, names = _header_table()
    assert "PDHG_SMALL_QP" in names and names.index("PDHG_SMALL_QP") == names.index("PDHG_SMALL_LP") + 1
    assert len(names) == len(set(names)) == 28
    assert re.search(r"These 28 are the\s*\n? \* library's run-time knobs", head)
    row = re.search(r"^ \*   PDHG_SMALL_QP\s+0 \| 1\s", head, flags=re.M)      # the default first: off
    assert row, "PDHG_SMALL_QP's row must give its values, the default (0) first"


def test_small_qp_is_named_in_the_readme():
    readme = open(os.path.join(ROOT, "README.md")).read()
    part = readme[readme.index("## Environment switches"):]
    listed = re.findall(r"`(PDHG_[A-Z0-9_]+)`", part[:part.index("Every other `PDHG_*` name")])
    _, names = _header_table()
    assert "PDHG_SMALL_QP" in listed and listed == names
    assert "**28 documented run-time variables**" in part


def test_the_library_reads_it_with_plain_getenv():
    src = open(os.path.join(ROOT, "firstorderlp.jl_amd", "csrc", "host_small_lp.hpp")).read()
    assert 'getenv("PDHG_SMALL_QP")' in src and 'dev_env("PDHG_SMALL_QP")' not in src
