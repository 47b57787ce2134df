"""The device layout builders (csrc/device_layout.hpp) at their scan, sort and tile edges: the smallest shapes that reach
every branch of the tiled exclusive scan, the 8-bit LSD radix sort, the ballot-based peer ranks, the per-wave counting
sort of the sweep's tile-major copy, the slab count / fill and the CSC ingest -- with PDHG_DEVICE_LAYOUT=1, which forces
the path that pdhg_create takes by itself from 8 M nonzeros on.

Every case goes through assert_device_layout():
  1. the device build against the host build: layout_info(), all 32 checksums and both products, bitwise;
  2. both builds against a reference from OUTSIDE the library: checksum_kernel's sum restated in numpy over the words of
     scipy's CSR of A (slots 0, 1, 2) and of A' (slots 16, 17, 18);
  3. the device build's products against the CPU oracle (helpers.assert_products_match_oracle);
  4. the branch the case is there for, computed from m and nnz with the code's own formulas (digit passes, scan depth,
     sort workgroups) or read from layout_info() (tiles, slabs, long rows), so that no case passes by missing its branch.

Matrices are built once per module (every GPU test runs in both row orders) and never changed."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from firstorderlp_jl_amd import HipPdhgEngine, _lib
from oracle import oracle as orc
from tests import helpers as H

gpu = pytest.mark.gpu

# csrc/device_layout.hpp / common.hpp
SCAN_TILE = 2048        # elements per workgroup of scan_tiles_kernel; device_exclusive_scan recurses on the tile sums
RS_TILE = 4096          # entries per workgroup of rs_hist_kernel / rs_scatter_kernel (4 waves x 16 chunks x 64 lanes)
RS_BITS = 8             # bits per digit pass of device_radix_sort
BLOCK_NNZ = 2048        # rows beyond it go to the long-row tables (the default long-row threshold)
GOLDEN = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int64)


# ---------------------------------------------------------------- the code's formulas, restated

def digit_passes(rows):
    """host_shards.hpp, ingest_on_device: key_bits from the row count; device_radix_sort: one pass per RS_BITS of them."""
    key_bits = 1
    while (1 << key_bits) < rows:
        key_bits += 1
    return -(-key_bits // RS_BITS)


def scan_depth(n):
    """Levels of device_exclusive_scan over n elements: one, plus the scan of the tile sums while there are several."""
    depth, tiles = 1, -(-n // SCAN_TILE)
    while tiles > 1:
        depth, tiles = depth + 1, -(-tiles // SCAN_TILE)
    return depth


def sort_workgroups(nnz):
    return -(-nnz // RS_TILE)


# ---------------------------------------------------------------- the reference checksum

def words_checksum(a):
    """checksum_kernel in numpy: sum over the 4-byte words w[i] of a of (w[i] + GOLDEN) * (2 i + 1), modulo 2^64
    (uint64 arrays wrap)."""
    w = np.ascontiguousarray(a).view(np.uint32).astype(np.uint64)
    i = np.arange(len(w), dtype=np.uint64)
    return int(((w + np.uint64(GOLDEN)) * (np.uint64(2) * i + np.uint64(1))).sum(dtype=np.uint64))


def test_numpy_checksum_against_a_hand_worked_example():
    """Ten words; term i is (w[i] + GOLDEN) * (2 i + 1) mod 2^64, G = GOLDEN = 0x9E3779B97F4A7C15:
         i  w[i]         term
         0  0            G                                  = 0x9E3779B97F4A7C15
         1  1            3 (G + 1)        = 3 G + 3         = 0xDAA66D2C7DDF7442
         2  2            5 (G + 2)        = 5 G + 10        = 0x1715609F7C746C73 (the low 64 bits)
         3  0xFFFFFFFF   7 (G + 2^32 - 1) = 7 G + 7 2^32 - 7
         4  0x80000000   9 (G + 2^31)     = 9 G + 9 2^31
         5  7            11 (G + 7)       = 11 G + 77
         6  0            13 G
         7  0x12345678   15 (G + 0x12345678)
         8  3            17 (G + 3)       = 17 G + 51
         9  0xDEADBEEF   19 (G + 0xDEADBEEF)
       The multipliers sum to 100 (ten odd numbers), so the total is
         100 G + 3 + 10 + 7 (2^32 - 1) + 9 2^31 + 77 + 15 * 0x12345678 + 51 + 19 * 0xDEADBEEF   (mod 2^64)
       = 100 G + 124 956 065 099, and 100 G mod 2^64 = 0xCDAB8C75B9187834, which gives the constant below.  The same sum
       is taken once more with Python's unbounded integers."""
    w = [0, 1, 2, 0xFFFFFFFF, 0x80000000, 7, 0, 0x12345678, 3, 0xDEADBEEF]
    small = 3 + 10 + 7 * (2 ** 32 - 1) + 9 * 2 ** 31 + 77 + 15 * 0x12345678 + 51 + 19 * 0xDEADBEEF
    assert small == 124_956_065_099
    assert (100 * GOLDEN) & MASK64 == 0xCDAB8C75B9187834
    by_hand = (0xCDAB8C75B9187834 + 124_956_065_099) & MASK64
    assert by_hand == 0xCDAB8C92D10EB57F
    assert sum((v + GOLDEN) * (2 * i + 1) for i, v in enumerate(w)) & MASK64 == by_hand
    assert words_checksum(np.array(w, dtype=np.uint32)) == by_hand
    # an int32 array and a float64 array (two words each, low word first) are taken by their words
    assert words_checksum(np.array(w, dtype=np.uint32).view(np.int32)) == by_hand
    d = np.array(w, dtype=np.uint32).view(np.float64)
    assert len(d) == 5 and words_checksum(d) == by_hand
    assert words_checksum(np.zeros(0, dtype=np.int32)) == 0
    # order-sensitive: swapping two different words changes it
    w2 = list(w)
    w2[1], w2[2] = w2[2], w2[1]
    assert words_checksum(np.array(w2, dtype=np.uint32)) != by_hand


def test_formulas_of_the_digit_passes_and_the_scan_depth():
    assert [digit_passes(r) for r in (1, 2, 255, 256, 257, 65_535, 65_536, 65_537, 1 << 24, (1 << 24) + 1)] == \
        [1, 1, 1, 1, 2, 2, 2, 3, 3, 4]
    assert [scan_depth(n) for n in (1, 2047, 2048, 2049, 4096, 4097, 2048 ** 2, 2048 ** 2 + 1)] == [1, 1, 1, 2, 2, 2, 2, 3]
    assert [sort_workgroups(k) for k in (1, 4095, 4096, 4097, 8192, 8193)] == [1, 1, 1, 2, 2, 3]


def reference_checksums(A, caller_order=False):
    """{slot: checksum} for rowptr, col, val of CSR(A) (slots 0, 1, 2) and of CSR(A') (16, 17, 18), from scipy's
    conversions with sorted indices.  caller_order: the matrix holds unsorted or repeated entries, which the library keeps
    as the caller gave them -- CSR(A') is then the CSC input itself and CSR(A) a stable sort of its entries by row."""
    m, n = A.shape
    if caller_order:
        cols = np.repeat(np.arange(n), np.diff(A.indptr))
        order = np.argsort(A.indices, kind="stable")
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(A.indices, minlength=m))])
        csr = (rowptr, cols[order], A.data[order])
        csr_t = (A.indptr, A.indices, A.data)
    else:
        R, T = sp.csr_matrix(A), sp.csr_matrix(A.T)
        R.sort_indices()
        T.sort_indices()
        assert R.nnz == A.nnz and T.nnz == A.nnz and R.has_canonical_format and T.has_canonical_format
        csr, csr_t = (R.indptr, R.indices, R.data), (T.indptr, T.indices, T.data)
    out = {}
    for base, (rowptr, col, val) in ((0, csr), (16, csr_t)):
        out[base] = words_checksum(np.asarray(rowptr).astype(np.int32))
        out[base + 1] = words_checksum(np.asarray(col).astype(np.int32))
        out[base + 2] = words_checksum(np.asarray(val, dtype=np.float64))
    return out


# ---------------------------------------------------------------- cases

class Case:
    """A matrix in CSC form as the caller passes it, trivial-but-not-zero problem vectors, two vectors for the products
    and the reference checksums (computed once)."""

    def __init__(self, A, seed=0, caller_order=False):
        self.A = A if caller_order else sp.csc_matrix(A)
        if not caller_order:
            self.A.sort_indices()
        self.caller_order = caller_order
        m, n = self.A.shape
        rng = np.random.default_rng(1000 + seed)
        self.c, self.b = rng.standard_normal(n), rng.standard_normal(m)
        self.lb = np.where(rng.random(n) < 0.3, -np.inf, 0.0)
        self.ub = np.where(rng.random(n) < 0.5, np.inf, 2.0)
        self.ne = m // 3
        self.x, self.y = rng.standard_normal(n), rng.standard_normal(m)
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = reference_checksums(self.A, self.caller_order)
        return self._ref

    def engine(self, **kw):
        return HipPdhgEngine(self.A, self.c, self.b, self.lb, self.ub, self.ne, **kw)


def scattered_rows(m, n, per_row, seed, extra=0):
    """m x n CSR: row i holds per_row distinct columns (s_i + k * step_i) mod n, standard-normal values; the first
    `extra` rows hold one more."""
    rng = np.random.default_rng(seed)
    top = per_row + (1 if extra else 0)
    if n < top:
        per_row, top, extra = n, n, 0
    lens = np.full(m, per_row, dtype=np.int64)
    lens[:extra] += 1
    step = rng.integers(1, max(2, n // top), m) if n // top >= 2 else np.ones(m, dtype=np.int64)
    start = rng.integers(0, n, m)
    k = np.arange(top)
    cols = (start[:, None] + k[None, :] * step[:, None]) % n
    keep = k[None, :] < lens[:, None]
    indptr = np.concatenate([[0], np.cumsum(lens)])
    A = sp.csr_matrix((rng.standard_normal(int(lens.sum())), cols[keep], indptr), shape=(m, n))
    A.sort_indices()
    assert A.has_canonical_format and A.nnz == lens.sum()
    return A


def from_triplets(m, n, rows, cols, seed):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    pairs = np.unique(rows * n + cols)
    rng = np.random.default_rng(seed)
    A = sp.csc_matrix((rng.standard_normal(len(pairs)), (pairs // n, pairs % n)), shape=(m, n))
    A.sort_indices()
    assert A.nnz == len(pairs)
    return A


def tall_sparse(m, n, special_rows, random_rows, seed):
    """m x n with every column in each of a few rows: the special ones (first, last, tile boundaries of the scan) and
    `random_rows` more."""
    rng = np.random.default_rng(seed)
    rows = np.unique(np.concatenate([np.asarray([r for r in special_rows if 0 <= r < m], dtype=np.int64),
                                     rng.integers(0, m, random_rows)]))
    return from_triplets(m, n, np.repeat(rows, n), np.tile(np.arange(n), len(rows)), seed)


def alternating_digits(nnz, m=1000, n=700, seed=0, per_col=12):
    """Exactly nnz entries, no (row, column) twice.  Even columns draw their rows from 16 rows with FOUR distinct low
    digits (r mod 256 < 4), odd columns from all rows, per_col entries each: the input (column-major) order alternates
    between runs of few and of many distinct digits, so a 64-entry chunk of rs_scatter_kernel holds large and small peer
    groups side by side."""
    rng = np.random.default_rng(seed)
    few = np.array([d + 256 * h for h in range(4) for d in range(4) if d + 256 * h < m])
    rows, cols, left, j = [], [], nnz, 0
    while left > 0:
        assert j < n
        k = min(left, per_col)
        pick = rng.choice(few, k, replace=False) if j % 2 == 0 else rng.choice(m, k, replace=False)
        rows.append(np.sort(pick))
        cols.append(np.full(k, j))
        left -= k
        j += 1
    A = from_triplets(m, n, np.concatenate(rows), np.concatenate(cols), seed)
    assert A.nnz == nnz
    return A


def shuffled_within_columns(A, seed, repeats=0):
    """A's entries in the CALLER'S order: every column's entries permuted at random; `repeats` entries are given twice
    (a second value at the same row and column).  Built from the arrays: scipy does not canonicalise."""
    rng = np.random.default_rng(seed)
    C = sp.coo_matrix(A)
    rows, cols, vals = C.row.astype(np.int64), C.col.astype(np.int64), C.data.copy()
    if repeats:
        again = rng.choice(len(rows), repeats, replace=False)
        rows, cols = np.concatenate([rows, rows[again]]), np.concatenate([cols, cols[again]])
        vals = np.concatenate([vals, rng.standard_normal(repeats)])
    order = np.lexsort((rng.random(len(rows)), cols))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=A.shape[1]))])
    out = sp.csc_matrix((vals[order], rows[order], indptr), shape=A.shape)
    assert out.nnz == len(rows)
    return out


def sorted_with_repeats(A, seed, repeats):
    """Ascending rows inside a column, `repeats` entries given twice, side by side."""
    rng = np.random.default_rng(seed)
    C = sp.coo_matrix(A)
    again = rng.choice(C.nnz, repeats, replace=False)
    rows, cols = np.concatenate([C.row, C.row[again]]).astype(np.int64), np.concatenate([C.col, C.col[again]]).astype(np.int64)
    vals = np.concatenate([C.data, rng.standard_normal(repeats)])
    order = np.lexsort((np.arange(len(rows)), rows, cols))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=A.shape[1]))])
    out = sp.csc_matrix((vals[order], rows[order], indptr), shape=A.shape)
    assert out.nnz == C.nnz + repeats
    return out


def _one_row(m, n, row, length, seed):
    rng = np.random.default_rng(seed)
    return from_triplets(m, n, np.full(length, row), rng.choice(n, length, replace=False), seed)


def _distinct_digit_chunks(seed):
    """1000 x 700: column 0 holds rows 0 .. 63 (the first 64 input entries: 64 different digits of the first pass),
    column 1 rows 15 k (64 different low digits, four different high digits), column 2 rows 256 h + 3 (one low digit);
    scattered entries elsewhere."""
    rng = np.random.default_rng(seed)
    rows = [np.arange(64), 15 * np.arange(64), 256 * np.arange(4) + 3, rng.integers(0, 1000, 3000)]
    cols = [np.zeros(64), np.ones(64), np.full(4, 2), rng.integers(3, 700, 3000)]
    A = from_triplets(1000, 700, np.concatenate(rows), np.concatenate(cols), seed)
    assert np.array_equal(A.indices[:64], np.arange(64))
    return A


def _with_long_row(A, row, length, seed, allowed=None):
    """A with `row` replaced by one of `length` entries (columns drawn from `allowed`)."""
    rng = np.random.default_rng(seed)
    m, n = A.shape
    keep = sp.diags((np.arange(m) != row).astype(float)) @ A
    cols = rng.choice(n if allowed is None else allowed, length, replace=False)
    long = sp.csr_matrix((rng.standard_normal(length) + 3.0, (np.full(length, row), cols)), shape=(m, n))
    out = sp.csr_matrix(keep + long)
    out.eliminate_zeros()
    out.sort_indices()
    return out


def _slab_matrix(n, holes, seed):
    """120 000 rows, 1 050 000 scattered entries; holes: (first column, width) of a column range without entries, and
    then row 777 holds 2 500 entries (long in the full matrix)."""
    m = 120_000
    if not holes:
        return scattered_rows(m, n, 8, seed, extra=90_000)
    h0, hw = holes
    B = scattered_rows(m, n - hw, 8, seed, extra=90_000).tocsc()
    A = sp.hstack([B[:, :h0], sp.csc_matrix((m, hw)), B[:, h0:]]).tocsr()
    allowed = np.concatenate([np.arange(h0), np.arange(h0 + hw, n)])
    return _with_long_row(A, 777, 2500, seed, allowed)


def _edge_border(m, n, seed):
    """Entries only in the last row and the last column."""
    rows = np.concatenate([np.full(n, m - 1), np.arange(m - 1)])
    cols = np.concatenate([np.arange(n), np.full(m - 1, n - 1)])
    return from_triplets(m, n, rows, cols, seed)


def _empty_borders(seed):
    """500 x 400, about 6 per row, first / last row and first / last column empty."""
    A = sp.lil_matrix((500, 400))
    A[1:-1, 1:-1] = scattered_rows(498, 398, 6, seed)
    return sp.csc_matrix(A)


def _empty_row_block(seed):
    """5 000 x 300 whose rows 1 000 .. 3 999 are empty."""
    top, bottom = scattered_rows(1000, 300, 5, seed), scattered_rows(1000, 300, 5, seed + 1)
    return sp.vstack([top, sp.csr_matrix((3000, 300)), bottom])


TWO24 = 1 << 24
SCAN_EDGE_ROWS = [0, 1] + [2048 * k + d for k in (1, 2, 3, 1000, 2047, 2048) for d in (-2, -1, 0, 1)]

# name -> (maker, env, expectations)
MAKERS = {}
for _m in (1, 2, 255, 256, 257, 65_535, 65_536, 65_537):
    MAKERS[f"digits_m{_m}"] = (functools.partial(scattered_rows, _m, 300, 5, 10 + _m % 97), {}, {})
MAKERS["digits_m2p24_plus_1"] = (lambda: tall_sparse(TWO24 + 1, 3, list(range(10)) + [255, 256, 257, 65_535, 65_536, TWO24 - 1] +
                                                      list(range(TWO24 - 9, TWO24 + 1)) + SCAN_EDGE_ROWS, 2000, 3), {}, {})
for _m1 in (2047, 2048, 2049, 4096, 4097):
    MAKERS[f"scan_rows_plus_1_{_m1}"] = (functools.partial(scattered_rows, _m1 - 1, 300, 5, 20 + _m1 % 89), {}, {})
for _m1 in (2048 ** 2, 2048 ** 2 + 1):
    MAKERS[f"scan_rows_plus_1_{_m1}"] = (functools.partial(tall_sparse, _m1 - 1, 4, SCAN_EDGE_ROWS + [_m1 - 2, _m1 - 3], 1000, 5), {}, {})
SORT_NNZ = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193)
for _k in SORT_NNZ:
    MAKERS[f"sort_nnz{_k}"] = (functools.partial(alternating_digits, _k, seed=_k), {}, {"nnz": _k})
MAKERS["sort_one_row"] = (lambda: _one_row(1000, 3000, 517, 2500, 7), {}, {"A_long_rows": 1, "A_max_row_nnz": 2500})
MAKERS["sort_64_distinct_digits"] = (lambda: _distinct_digit_chunks(8), {}, {})
MAKERS["one_by_one"] = (lambda: sp.csc_matrix(np.array([[2.5]])), {}, {"nnz": 1})
MAKERS["dense_row"] = (lambda: sp.csc_matrix(np.random.default_rng(1).standard_normal((1, 130))), {}, {"nnz": 130})
MAKERS["dense_column"] = (lambda: sp.csc_matrix(np.random.default_rng(2).standard_normal((130, 1))), {}, {"nnz": 130})
MAKERS["empty_borders"] = (lambda: _empty_borders(3), {}, {})
MAKERS["empty_row_block"] = (lambda: _empty_row_block(4), {}, {})
MAKERS["last_row_and_column_only"] = (lambda: _edge_border(300, 260, 5), {}, {"nnz": 559})
SWEEP_ENV = {"PDHG_SPMV": "tiled", "PDHG_TILE_COLS": "64"}
for _n, _tiles in ((64 * 63, 63), (64 * 64, 64), (64 * 64 + 1, 65), (64 * 65, 65), (64 * 128 + 1, 129), (65_536, 1024), (65_537, 1025)):
    MAKERS[f"sweep_n{_n}"] = (functools.partial(scattered_rows, 3000, _n, 8, 30 + _n % 83), SWEEP_ENV, {"tiles": _tiles})
MAKERS["sweep_var_tiles"] = (functools.partial(scattered_rows, 3000, 64 * 65, 8, 41), dict(SWEEP_ENV, PDHG_VAR_TILES="1"), {"var_tiles": True})
MAKERS["sweep_long_row"] = (lambda: _with_long_row(scattered_rows(3000, 64 * 65, 8, 42), 1234, 2100, 42), SWEEP_ENV,
                            {"tiles": 65, "A_long_rows": 1})
SLAB_ENV = {"PDHG_SLAB_MB": "0.25", "PDHG_SLABS": "2"}
MAKERS["slabs_2"] = (lambda: _slab_matrix(50_000, None, 51), SLAB_ENV, {"A_slabs": 2, "At_slabs": 4, "nnz": 1_050_000})
MAKERS["slabs_4_empty_slab_long_row"] = (lambda: _slab_matrix(100_000, (50_000, 25_000), 52), SLAB_ENV,
                                         {"A_slabs": 4, "At_slabs": 4, "A_long_rows": 1})
_BASE_500 = functools.partial(scattered_rows, 500, 300, 6, 61)
MAKERS["caller_unsorted"] = (lambda: shuffled_within_columns(_BASE_500(), 62), {}, {"caller_order": True})
MAKERS["caller_repeats"] = (lambda: sorted_with_repeats(_BASE_500(), 63, 200), {}, {"caller_order": True, "nnz": 3200})
MAKERS["caller_unsorted_repeats"] = (lambda: shuffled_within_columns(_BASE_500(), 64, repeats=200), {},
                                     {"caller_order": True, "nnz": 3200})

_CASES = {}


def case(name):
    if name not in _CASES:
        maker, _, expect = MAKERS[name]
        _CASES[name] = Case(maker(), seed=len(_CASES), caller_order=expect.get("caller_order", False))
    return _CASES[name]


CHECKSUM_LABELS = ["rowptr", "col", "val", "blks", "long_row", "long_chunk_ptr", "chunk_row", "chunk_off", "pk", "tv",
                   "wave_rows", "wave_ent", "wave_step_off", "step_tile", "wg_step_off", "plan"]


def _slot(q):
    return ("A" if q < 16 else "At") + "." + CHECKSUM_LABELS[q % 16]


def assert_device_layout(cs, monkeypatch, env=None, label=""):
    """The check of every case (module docstring, 1 - 3).  Returns the device build's layout_info()."""
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    engines = {}
    try:
        for mode in ("0", "1"):
            monkeypatch.setenv("PDHG_DEVICE_LAYOUT", mode)
            engines[mode] = cs.engine()
        eng_h, eng_d = engines["0"], engines["1"]
        info_h, info_d = eng_h.layout_info(), eng_d.layout_info()
        assert info_h == info_d, (label, info_h, info_d)
        ck_h, ck_d = eng_h.layout_checksums(), eng_d.layout_checksums()
        bad = [_slot(q) for q in range(32) if ck_h[q] != ck_d[q]]
        assert not bad, f"{label}: device build differs from the host build in {bad}"
        for build, ck in (("host", ck_h), ("device", ck_d)):
            bad = [_slot(q) for q, want in cs.ref.items() if int(ck[q]) != want]
            assert not bad, f"{label}: {build} build differs from the numpy / scipy reference in {bad}"
        A, x, y = cs.A, cs.x, cs.y
        got_x, got_y = eng_d.spmv(x), eng_d.spmv_t(y)
        assert np.array_equal(got_x, eng_h.spmv(x)), label + ": A x differs between the builds"
        assert np.array_equal(got_y, eng_h.spmv_t(y)), label + ": A'y differs between the builds"
        if cs.caller_order:
            # the oracle's summation order for unsorted / repeated input is not part of its contract: 1e-13 * sum |a x|, every row
            m, n = A.shape
            absA = sp.csc_matrix((np.abs(A.data), A.indices, A.indptr), shape=A.shape)
            assert np.all(np.abs(got_x - orc.spmv(m, n, A.indptr, A.indices, A.data, x)) <= 1e-13 * (absA @ np.abs(x)) + 1e-300), label
            assert np.all(np.abs(got_y - orc.spmv_t(m, n, A.indptr, A.indices, A.data, y)) <= 1e-13 * (absA.T @ np.abs(y)) + 1e-300), label
        else:
            H.assert_products_match_oracle(eng_d, A, x, y, forced_sweep=env.get("PDHG_SPMV") == "tiled", label=label)
        return info_d
    finally:
        for e in engines.values():
            e.close()


def _assert_expectations(name, cs, info):
    expect = MAKERS[name][2]
    m, n = cs.A.shape
    if "nnz" in expect:
        assert cs.A.nnz == expect["nnz"]
    for key in ("A_slabs", "At_slabs", "A_max_row_nnz"):
        if key in expect:
            assert info[key] == expect[key], (name, key, info)
    if "A_long_rows" in expect:
        assert info["A_long_rows"] >= expect["A_long_rows"] and np.diff(sp.csr_matrix(cs.A).indptr).max() > BLOCK_NNZ, (name, info)
    if "tiles" in expect:
        assert info["A_tiled_waves"] > 0 and info["At_tiled_waves"] > 0 and info["A_tile_cols"] == 64, (name, info)
        assert -(-n // info["A_tile_cols"]) == expect["tiles"]
    if expect.get("var_tiles"):
        assert info["A_tiled_waves"] > 0 and info["var_tiles"] & 1, (name, info)


# ---------------------------------------------------------------- digit passes, the scratch swap, scan depth

@gpu
@pytest.mark.parametrize("m, passes", [(1, 1), (2, 1), (255, 1), (256, 1), (257, 2), (65_535, 2), (65_536, 2), (65_537, 3)])
def test_digit_passes_and_the_scratch_swap(gpu_required, monkeypatch, m, passes):
    """One, two and three passes, on both sides of 2^8 and 2^16 rows; an odd count leaves the result in the scratch
    triple (the in_scratch swap)."""
    name = f"digits_m{m}"
    cs = case(name)
    assert cs.A.shape == (m, 300) and cs.A.nnz == 5 * m
    assert digit_passes(m) == passes
    _assert_expectations(name, cs, assert_device_layout(cs, monkeypatch, label=name))


@gpu
def test_four_digit_passes_and_a_three_level_scan(gpu_required, monkeypatch):
    """2^24 + 1 rows: four passes (the result back in the caller's triple) and rows + 1 = 2^24 + 2 counts scanned in
    three levels (8 193 tiles, 5, 1).  Entries in the first, the last and some 2 000 middle rows."""
    name = "digits_m2p24_plus_1"
    cs = case(name)
    m, n = cs.A.shape
    rows = np.unique(cs.A.indices)
    assert (m, n) == (TWO24 + 1, 3) and 5000 <= cs.A.nnz <= 7000 and rows[0] == 0 and rows[-1] == m - 1
    assert digit_passes(m) == 4 and scan_depth(m + 1) == 3 and scan_depth(256 * sort_workgroups(cs.A.nnz)) == 1
    _assert_expectations(name, cs, assert_device_layout(cs, monkeypatch, label=name))


@gpu
@pytest.mark.parametrize("rows_plus_1, depth", [(2047, 1), (2048, 1), (2049, 2), (4096, 2), (4097, 2), (2048 ** 2, 2), (2048 ** 2 + 1, 3)])
def test_scan_boundaries_on_the_row_counts(gpu_required, monkeypatch, rows_plus_1, depth):
    """rows + 1 counts at a multiple of SCAN_TILE and one past it, and two levels against three (2048^2 and one more;
    entries in the last row and around rows 2048 k - 1)."""
    name = f"scan_rows_plus_1_{rows_plus_1}"
    cs = case(name)
    m = cs.A.shape[0]
    assert m + 1 == rows_plus_1 and scan_depth(m + 1) == depth
    if rows_plus_1 >= 2048 ** 2:
        rows = np.unique(cs.A.indices)
        assert rows[-1] == m - 1 and {2047, 2048, 4095, 2048 * 1000 - 1, 2048 * 2047 - 1} <= set(rows.tolist())
        assert digit_passes(m) == 3
    _assert_expectations(name, cs, assert_device_layout(cs, monkeypatch, label=name))


# ---------------------------------------------------------------- sort tiles and peer ranks

@gpu
@pytest.mark.parametrize("nnz", SORT_NNZ)
def test_sort_tiles(gpu_required, monkeypatch, nnz):
    """nnz at the 64-entry chunk, the 1024-entry wave share and the 4096-entry workgroup tile of rs_scatter_kernel, and
    one past each; two digit passes (1000 rows); runs of few and of many distinct digits alternate in the input."""
    name = f"sort_nnz{nnz}"
    cs = case(name)
    assert cs.A.shape == (1000, 700) and cs.A.nnz == nnz and digit_passes(1000) == 2
    assert sort_workgroups(nnz) == {1: 1, 63: 1, 64: 1, 65: 1, 1023: 1, 1024: 1, 1025: 1, 4095: 1, 4096: 1, 4097: 2, 8192: 2, 8193: 3}[nnz]
    if nnz >= 64:
        low = (cs.A.indices[:24] & 255)
        assert len(np.unique(low[:12])) <= 4 < len(np.unique(low[12:24]))        # few, then many
    _assert_expectations(name, cs, assert_device_layout(cs, monkeypatch, label=name))


@gpu
@pytest.mark.parametrize("name", ["sort_one_row", "sort_64_distinct_digits"])
def test_peer_groups_of_one_and_of_sixty_four(gpu_required, monkeypatch, name):
    """All entries in one row (every lane is every other's peer in both passes; the row is long, so the long-row tables
    are built too) and 64 consecutive entries with 64 different digits (every lane alone)."""
    cs = case(name)
    _assert_expectations(name, cs, assert_device_layout(cs, monkeypatch, label=name))


# ---------------------------------------------------------------- degenerate and structural

@gpu
@pytest.mark.parametrize("name", ["one_by_one", "dense_row", "dense_column", "empty_borders", "empty_row_block",
                                  "last_row_and_column_only"])
def test_degenerate_and_structural_shapes(gpu_required, monkeypatch, name):
    cs = case(name)
    A = sp.csr_matrix(cs.A)
    if name == "empty_borders":
        assert A[0].nnz == A[-1].nnz == cs.A[:, 0].nnz == cs.A[:, -1].nnz == 0 and A.nnz > 2000
    if name == "empty_row_block":
        assert np.all(np.diff(A.indptr)[1000:4000] == 0) and A.nnz == 10_000
    if name == "last_row_and_column_only":
        assert np.all(np.diff(A.indptr)[:-1] == 1) and np.diff(A.indptr)[-1] == A.shape[1]
    _assert_expectations(name, cs, assert_device_layout(cs, monkeypatch, label=name))


@gpu
@pytest.mark.parametrize("shape, nnz", [((40, 30), 0), ((0, 30), 0), ((40, 0), 0)], ids=["no_entries", "no_rows", "no_columns"])
def test_empty_matrices_take_the_host_path(gpu_required, monkeypatch, shape, nnz):
    """nnz = 0, m = 0, n = 0: build_layout_pair keeps the host builders whatever PDHG_DEVICE_LAYOUT says; create must
    succeed and the products are zeros (or empty)."""
    monkeypatch.setenv("PDHG_DEVICE_LAYOUT", "1")
    cs = Case(sp.csc_matrix(shape), seed=99)
    eng = cs.engine()
    try:
        ax, aty = eng.spmv(cs.x), eng.spmv_t(cs.y)
        assert ax.shape == (shape[0],) and aty.shape == (shape[1],) and not ax.any() and not aty.any()
    finally:
        eng.close()


# ---------------------------------------------------------------- caller's order

@gpu
@pytest.mark.parametrize("name", ["caller_unsorted", "caller_repeats", "caller_unsorted_repeats"])
def test_callers_order_is_kept(gpu_required, monkeypatch, name):
    """Unsorted row indices inside a column and repeated (row, column) entries: CSR(A') is the input as it is, CSR(A) a
    STABLE sort of it by row -- on the device as on the host."""
    cs = case(name)
    A = cs.A
    unsorted = any(np.any(np.diff(A.indices[A.indptr[j]:A.indptr[j + 1]]) < 0) for j in range(A.shape[1]))
    cols = np.repeat(np.arange(A.shape[1]), np.diff(A.indptr))
    repeated = len(np.unique(A.indices.astype(np.int64) * A.shape[1] + cols)) < A.nnz
    assert unsorted == ("unsorted" in name) and repeated == ("repeats" in name)
    _assert_expectations(name, cs, assert_device_layout(cs, monkeypatch, label=name))


# ---------------------------------------------------------------- the sweep's tables

@gpu
@pytest.mark.parametrize("n, tiles", [(64 * 63, 63), (64 * 64, 64), (64 * 64 + 1, 65), (64 * 65, 65), (64 * 128 + 1, 129),
                                      (65_536, 1024), (65_537, 1025)])
def test_sweep_tables_at_the_tile_counts(gpu_required, monkeypatch, n, tiles):
    """tw_fill_kernel's prefix over the tiles in blocks of 64 lanes (63, 64, 65, 129 tiles: none, one and two carries),
    peer_mask at a power of two of tiles and one past it, 1024 tiles (the most the device mode takes) and 1025 (handed
    back to the host builders, still bit-identical)."""
    name = f"sweep_n{n}"
    cs = case(name)
    assert cs.A.shape == (3000, n) and cs.A.nnz == 8 * 3000
    _assert_expectations(name, cs, assert_device_layout(cs, monkeypatch, MAKERS[name][1], label=name))


@gpu
@pytest.mark.parametrize("name", ["sweep_var_tiles", "sweep_long_row"])
def test_sweep_tables_with_unequal_tiles_and_a_skipped_row(gpu_required, monkeypatch, name):
    cs = case(name)
    _assert_expectations(name, cs, assert_device_layout(cs, monkeypatch, MAKERS[name][1], label=name))


# ---------------------------------------------------------------- slabs

@gpu
@pytest.mark.parametrize("name", ["slabs_2", "slabs_4_empty_slab_long_row"])
def test_slabs_built_on_the_device(gpu_required, monkeypatch, name):
    """slab_count_kernel / slab_fill_kernel: two slabs; four slabs of which one holds no entry, with a row that is long in
    the full matrix (both kernels skip it)."""
    cs = case(name)
    if name == "slabs_4_empty_slab_long_row":
        assert cs.A[:, 50_000:75_000].nnz == 0 and cs.A.nnz >= 1 << 20
    _assert_expectations(name, cs, assert_device_layout(cs, monkeypatch, MAKERS[name][1], label=name))


# ---------------------------------------------------------------- index_base = 1

def raw_create(cs, base, device_ids=None, A=None):
    """pdhg_create / pdhg_create_multi through ctypes with colptr + base, rowval + base: what julia/FirstOrderLpHIP.jl
    passes (base 1).  Returns an engine over the handle; raises PdhgHipError as the binding does."""
    L = _lib.lib()
    A = cs.A if A is None else A
    m, n = A.shape
    colptr = np.ascontiguousarray(A.indptr, dtype=np.int64) + base
    rowval = np.ascontiguousarray(A.indices, dtype=np.int64) + base
    nzval = np.ascontiguousarray(A.data, dtype=np.float64)
    return _raw_create_arrays(L, m, n, colptr, rowval, nzval, base, cs, device_ids)


def _raw_create_arrays(L, m, n, colptr, rowval, nzval, base, cs, device_ids=None):
    h = ctypes.c_void_p()
    common = (m, n, len(nzval), colptr.ctypes.data_as(_ip), rowval.ctypes.data_as(_ip), nzval.ctypes.data_as(_dp), base,
              cs.c.ctypes.data_as(_dp), cs.b.ctypes.data_as(_dp), cs.lb.ctypes.data_as(_dp), cs.ub.ctypes.data_as(_dp), cs.ne)
    if device_ids is None:
        _lib.check(L.pdhg_create(ctypes.byref(h), *common, -1, None))
    else:
        ids = (ctypes.c_int * len(device_ids))(*device_ids)
        _lib.check(L.pdhg_create_multi(ctypes.byref(h), *common, len(device_ids), ids))
    return HipPdhgEngine._wrap(L, h, m, n)


def _assert_group_products_match_oracle(eng, cs, label=""):
    """A row-partitioned group: a row is whole inside one shard, so A x is the oracle's bitwise (the rows of these cases
    hold at most 8 entries, within the bit-exact limit of every layout and row order); A'y is the sum over the shards, in
    rank order, of partial sums of the same products.  Any summation order of k products is within (k - 1) eps sum |a y|
    of any other to first order, and no column here holds 100 entries: (k - 1) eps < 100 * 1.2e-16 < 1e-13, the project's
    bar for a row summed in another order."""
    A = cs.A
    m, n = A.shape
    assert np.diff(sp.csr_matrix(A).indptr).max() <= 8 and np.diff(A.indptr).max() < 100
    assert np.array_equal(eng.spmv(cs.x), orc.spmv(m, n, A.indptr, A.indices, A.data, cs.x)), label + ": A x"
    err = np.abs(eng.spmv_t(cs.y) - orc.spmv_t(m, n, A.indptr, A.indices, A.data, cs.y))
    assert np.all(err <= 1e-13 * (abs(A).T @ np.abs(cs.y)) + 1e-300), label + ": A'y"


def _trial(eng, step=0.05, weight=1.3):
    raw = eng.trial_step(step, weight, 1.0)
    return [raw] + list(eng.get_trial())


@gpu
@pytest.mark.parametrize("device_ids", [None, [0, 0]], ids=["one_handle", "two_shards"])
@pytest.mark.parametrize("mode", ["0", "1"], ids=["host_layout", "device_layout"])
@pytest.mark.parametrize("name", ["digits_m257", "sweep_n4097", "empty_borders"])
def test_one_based_arrays_give_the_same_engine(gpu_required, monkeypatch, name, mode, device_ids):
    """index_base = 1 through pdhg_create and pdhg_create_multi: checksums, layout_info, both products and one trial are
    bitwise those of the base-0 engine of the same matrix, and the products match the oracle."""
    cs = case(name)
    env = MAKERS[name][1]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PDHG_DEVICE_LAYOUT", mode)
    zero = cs.engine() if device_ids is None else cs.engine(device_ids=device_ids)
    one = raw_create(cs, 1, device_ids)
    try:
        assert one.layout_info() == zero.layout_info()
        ck0, ck1 = zero.layout_checksums(), one.layout_checksums()
        assert np.array_equal(ck0, ck1), [_slot(q) for q in range(32) if ck0[q] != ck1[q]]
        if device_ids is None:
            assert not [_slot(q) for q, want in cs.ref.items() if int(ck1[q]) != want]
        assert np.array_equal(one.spmv(cs.x), zero.spmv(cs.x)) and np.array_equal(one.spmv_t(cs.y), zero.spmv_t(cs.y))
        if device_ids is None:
            H.assert_products_match_oracle(one, cs.A, cs.x, cs.y, forced_sweep=env.get("PDHG_SPMV") == "tiled", label=name)
        else:
            _assert_group_products_match_oracle(one, cs, label=name)
        for a, b in zip(_trial(one), _trial(zero)):
            assert np.array_equal(a, b)
    finally:
        one.close()
        zero.close()


def _qp_cases():
    from firstorderlp_jl_amd.generators import random_lp
    p = H.example_qp()
    yield "example_qp", p
    p = random_lp(1500, 1200, 6, seed=13)
    B = sp.random(1200, 1200, density=0.004, random_state=9, format="csc")
    p.objective_matrix = sp.csc_matrix(5.0 * (B.T @ B) + sp.diags(np.random.default_rng(1).uniform(0.0, 3.0, 1200)))
    yield "sparse_psd_1200", p


@gpu
@pytest.mark.parametrize("mode", ["0", "1"], ids=["host_layout", "device_layout"])
def test_one_based_objective_matrix(gpu_required, monkeypatch, mode):
    """pdhg_set_objective_matrix with base 1 (on an engine created with base 1): one trial bitwise the base-0 engine's."""
    monkeypatch.setenv("PDHG_DEVICE_LAYOUT", mode)
    for label, p in _qp_cases():
        zero = HipPdhgEngine.from_problem(p)
        cs = Case(p.constraint_matrix)
        cs.c, cs.b, cs.lb, cs.ub = (np.ascontiguousarray(v, dtype=np.float64) for v in (
            p.objective_vector, p.right_hand_side, p.variable_lower_bound, p.variable_upper_bound))
        cs.ne = int(p.num_equalities)
        one = raw_create(cs, 1, A=sp.csc_matrix(p.constraint_matrix))
        try:
            Q = sp.csc_matrix(p.objective_matrix)
            qc, qr = Q.indptr.astype(np.int64) + 1, Q.indices.astype(np.int64) + 1
            qv = np.ascontiguousarray(Q.data, dtype=np.float64)
            _lib.check(one._L.pdhg_set_objective_matrix(one._h, len(qv), qc.ctypes.data_as(_ip), qr.ctypes.data_as(_ip),
                                                        qv.ctypes.data_as(_dp), 1))
            got, want = _trial(one, 0.1, 0.8), _trial(zero, 0.1, 0.8)
            assert want[0][4] != 0.0, label + ": the trial did not see Q"
            for a, b in zip(got, want):
                assert np.array_equal(a, b), label
        finally:
            one.close()
            zero.close()


@gpu
@pytest.mark.parametrize("mode", ["0", "1"], ids=["host_layout", "device_layout"])
def test_one_based_arrays_are_validated(gpu_required, monkeypatch, mode):
    """Base 1: a row index 0 or m + 1 fails with "rowval", colptr[0] = 0 with "colptr"."""
    monkeypatch.setenv("PDHG_DEVICE_LAYOUT", mode)
    cs = case("digits_m257")
    A = cs.A
    m, n = A.shape
    L = _lib.lib()
    colptr, rowval = A.indptr.astype(np.int64) + 1, A.indices.astype(np.int64) + 1
    nzval = np.ascontiguousarray(A.data, dtype=np.float64)
    for k, bad_row in ((17, 0), (A.nnz - 1, m + 1), (0, 0)):
        rv = rowval.copy()
        rv[k] = bad_row
        with pytest.raises(_lib.PdhgHipError, match="rowval"):
            _raw_create_arrays(L, m, n, colptr, rv, nzval, 1, cs).close()
    cp = colptr.copy()
    cp[0] = 0
    with pytest.raises(_lib.PdhgHipError, match="colptr"):
        _raw_create_arrays(L, m, n, cp, rowval, nzval, 1, cs).close()
    # the arrays as they are pass
    _raw_create_arrays(L, m, n, colptr, rowval, nzval, 1, cs).close()


# ---------------------------------------------------------------- shards and one-sided builds

@functools.lru_cache(maxsize=None)
def _shard_case():
    """Rows of equal length, so that the library's nnz-balanced partition cuts 769 rows into shards of 256 and 257 rows
    (one and two digit passes side by side in one group).  The entries and the two vectors are small INTEGERS: every sum
    is then exact in any order, so A'y -- which a group adds up over its shards' partial sums -- can be held bitwise to
    the single handle and to the oracle, like A x; a misplaced or swapped entry still changes the result."""
    A = scattered_rows(769, 300, 5, 71)
    rng = np.random.default_rng(72)
    A.data = rng.choice(np.concatenate([np.arange(-9.0, 0.0), np.arange(1.0, 10.0)]), A.nnz)
    cs = Case(A, seed=71)
    cs.x, cs.y = rng.integers(-20, 21, 300).astype(np.float64), rng.integers(-20, 21, 769).astype(np.float64)
    return cs


def test_the_partition_of_the_shard_case():
    bounds = HipPdhgEngine.partition_rows(_shard_case().A, 3)
    assert sorted(np.diff(bounds).tolist()) == [256, 256, 257], bounds


@gpu
def test_shards_of_256_and_257_rows(gpu_required, monkeypatch):
    cs = _shard_case()
    assert sorted(np.diff(HipPdhgEngine.partition_rows(cs.A, 3)).tolist()) == [256, 256, 257]
    assert digit_passes(256) == 1 and digit_passes(257) == 2
    monkeypatch.setenv("PDHG_DEVICE_LAYOUT", "1")
    group, single = cs.engine(device_ids=[0, 0, 0]), cs.engine()
    try:
        assert group.dist_info()["world"] == 3
        assert np.array_equal(group.spmv(cs.x), single.spmv(cs.x)) and np.array_equal(group.spmv_t(cs.y), single.spmv_t(cs.y))
        H.assert_products_match_oracle(group, cs.A, cs.x, cs.y, label="three shards")
    finally:
        group.close()
        single.close()


@gpu
def test_segments_build_one_side_each(gpu_required, monkeypatch):
    """PDHG_MAX_SHARD_NNZ: the matrix is held as row segments, each ingested by build_layout_pair with the other side
    skipped -- on the device here."""
    cs = Case(scattered_rows(6000, 5000, 6, 81), seed=81)
    monkeypatch.setenv("PDHG_MAX_SHARD_NNZ", str(cs.A.nnz // 4))
    engines = {}
    try:
        for mode in ("0", "1"):
            monkeypatch.setenv("PDHG_DEVICE_LAYOUT", mode)
            engines[mode] = cs.engine()
        info = engines["1"].layout_info()
        assert info["A_segments"] >= 4 and info["At_segments"] >= 4 and info == engines["0"].layout_info(), info
        assert np.array_equal(engines["1"].spmv(cs.x), engines["0"].spmv(cs.x))
        assert np.array_equal(engines["1"].spmv_t(cs.y), engines["0"].spmv_t(cs.y))
        H.assert_products_match_oracle(engines["1"], cs.A, cs.x, cs.y, label="segments")
    finally:
        for e in engines.values():
            e.close()
