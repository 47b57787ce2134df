"""Small QPs in a fleet's shared check launches, on the host: PDHG_SMALL_QP's row in include/pdhg_hip.h says that the switch
covers the checks too and keeps the table's format, the check calls read it with plain getenv at every call, and the
feature adds no export and leaves the ABI version alone."""
import os
import re

import folp_loader

folp_loader.load()
from firstorderlp_jl_amd import _lib  # noqa: E402
from tests import test_small_qp_host as SQ  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "firstorderlp.jl_amd", "csrc")


def _small_qp_row():
    head, _ = SQ._header_table()
    rows = re.split(r"^ \*   (?=PDHG_[A-Z0-9_]+ )", head, flags=re.M)
    (row,) = [r for r in rows if r.startswith("PDHG_SMALL_QP ")]
    return row


def test_the_header_row_mentions_the_checks_and_keeps_its_format():
    row = _small_qp_row()
    assert "check" in row and "pdhg_fleet_eval_points" in row and "pdhg_fleet_trust_region_bounds" in row, row
    assert re.match(r"PDHG_SMALL_QP\s+0 \| 1\s", row), row
    SQ.test_small_qp_is_tabled_in_the_header()
    SQ.test_small_qp_is_named_in_the_readme()


def test_the_check_calls_read_the_switch_with_plain_getenv_per_call():
    src = open(os.path.join(CSRC, "abi_fleet_checks.hpp")).read()
    body = src[src.index("static bool fleet_check_eligible"):]
    body = body[:body.index("\n}\n")]
    assert 'getenv("PDHG_SMALL_QP")' in body and 'dev_env("PDHG_SMALL_QP")' not in src
    assert "static const" not in body                 # nothing cached across calls


def test_no_new_export_and_the_same_abi_version():
    header = open(os.path.join(ROOT, "include", "pdhg_hip.h")).read()
    declared = set(re.findall(r"\b(pdhg_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_lib.EXPORTS) and len(_lib.EXPORTS) == len(declared) == 69      # as before the QP forms of the check kernels
    assert _lib.lib().pdhg_abi_version() == _lib.ABI_VERSION == 11
