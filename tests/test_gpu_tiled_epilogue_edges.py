"""The sweep's row epilogue (spmv_tiled_kernel, after the tile loop) walks a wave's rows 64 at a time.  Rows per wave around
every boundary of that loop and of a batch of four of its iterations -- fewer rows than lanes, exactly one iteration, one
more, four iterations (256 rows), one row less and one more, a partial second batch, and the benchmark's 1 221 -- with
the row count chosen so that the launch holds one full workgroup, one full wave, a wave of a single row and dead waves:
m = 8 R + R + 1.  Both products: the matrix as it is (the rows of A: MODE_DUAL, with and without the deferred sum_y
update) and with m and n swapped (the rows of A': MODE_ATY); MODE_PLAIN through spmv / spmv_t.  Everything bitwise
against the oracle: every lane adds its rows to the partial sums in ascending order.

(Written with a form of the loop that requests the operands of four iterations at once.  That form computed these bits
and made both product kernels of the 10M LP slower, 749 -> 797 us and 739 -> 795 us -- NOTEBOOK section 11 -- so the
loop is row by row again; the cases stay for whoever reorders it next.)

One exception, which is the relaxed row order's own contract and not the epilogue's: where a row has more than 8 entries
inside ONE tile, the relaxed order reduces that chunk by a tree (tiled_chunk_relaxed), within 1e-13 * sum |a x| of the
sequential sum.  At R = 1 with m and n swapped A' is 10 x 500 with ~50 entries per row and tile; that case then takes
the helpers' relaxed bars with the forced sweep's limit of 8 entries (helpers.assert_products_match_oracle) -- in strict
order it is bitwise like every other."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import HipPdhgEngine
from firstorderlp_jl_amd.generators import random_lp
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROWS_PER_WAVE = [1, 63, 64, 65, 255, 256, 257, 300, 1221]


TILE_COLS = 97


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _longest_run_in_a_tile(M):
    """The most entries a row of M holds inside one tile of TILE_COLS columns."""
    M = sp.csr_matrix(M)
    if M.nnz == 0:
        return 0
    rows = np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr))
    ntile = M.shape[1] // TILE_COLS + 1
    return int(np.unique(rows * ntile + M.indices // TILE_COLS, return_counts=True)[1].max())


@pytest.mark.parametrize("swap", [False, True], ids=["rows_of_A", "rows_of_At"])
@pytest.mark.parametrize("R", ROWS_PER_WAVE)
def test_batched_row_epilogue_at_its_edges(gpu_required, monkeypatch, R, swap):
    monkeypatch.setenv("PDHG_SPMV", "tiled")
    monkeypatch.setenv("PDHG_TILE_COLS", str(TILE_COLS))
    monkeypatch.setenv("PDHG_TW_ROWS", str(R))
    long_side, short_side = 8 * R + R + 1, 500
    m, n = (short_side, long_side) if swap else (long_side, short_side)
    p = random_lp(m, n, 5, seed=R)
    A = p.constraint_matrix
    eng = HipPdhgEngine.from_problem(p)
    info = eng.layout_info()
    assert info["A_tiled_waves"] > 0 and info["At_tiled_waves"] > 0
    # eight waves of R rows, one more of R rows, one of a single row (the second workgroup's other six are dead)
    assert info["At_tiled_waves" if swap else "A_tiled_waves"] == 10, info
    label = f"R = {R}, {'A transposed' if swap else 'A'}"
    bitwise = os.environ.get("PDHG_ROW_ORDER") == "strict" or max(_longest_run_in_a_tile(A), _longest_run_in_a_tile(A.T)) <= 8
    assert bitwise or (R == 1 and swap), label          # the one case the docstring names
    if not bitwise:
        monkeypatch.setattr(H, "bitexact_row_limit", lambda: 8)
    st = H.oracle_from_problem(p)
    step, pw = H.initial_step_and_weight(p)
    raw = eng.trial_step(step, pw, 1.0)
    H.assert_trial_matches_oracle(raw, eng.get_trial(), st, step, pw, A, label=label + ", first trial")
    # accept, then a second trial: its dual epilogue carries the deferred sum_y update (the third load of MODE_DUAL)
    eng.accept(step)
    st.step_size = step
    st.accept(st.x_next, st.y_next, st.aty_next)
    if not bitwise:                                     # the second trial starts from the device's own iterate
        st.x, st.y = eng.get_current()
        st.aty = eng.get_dual_product()
    raw = eng.trial_step(0.9 * step, pw, 1.0)
    H.assert_trial_matches_oracle(raw, eng.get_trial(), st, 0.9 * step, pw, A, label=label + ", second trial")
    xa, ya = eng.get_average()
    wxa, wya = st.compute_average()
    if bitwise:
        assert np.array_equal(_bits(xa), _bits(wxa)) and np.array_equal(_bits(ya), _bits(wya)), label + ": average"
    else:
        np.testing.assert_allclose(xa, wxa, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(ya, wya, rtol=1e-9, atol=1e-12)
    rng = np.random.default_rng(R + 1)
    H.assert_products_match_oracle(eng, A, rng.standard_normal(n), rng.standard_normal(m), forced_sweep=True, label=label)
    eng.close()
    st.close()
