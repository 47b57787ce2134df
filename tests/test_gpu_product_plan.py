"""One enumeration of a fused product's kernel steps (csrc/host_product.hpp: product_steps) feeds the direct launches, the
trial graph's nodes, the re-parameterised dual nodes and the names pdhg_kernel_name returns.  For every form a layout can
take -- stream, pipelined, sliced jagged (narrow and wide), a column-slab chain of each of those three, the sweep, with and
without the long-row pair -- 30 adaptive take_steps as ONE GRAPH per trial (the step size changes on the way, so the dual
nodes get new parameters) and launch by launch must not differ by a bit, the products must be the oracle's, and the
names must be the strings recorded from the commit BEFORE the enumeration existed (tests/golden/product_kernel_names.json,
written by this file's recorder: `python -m tests.test_gpu_product_plan OUT.json` on a GPU with that commit's library).

Shapes: a few hundred rows and columns, once with two dense rows and two dense columns that PDHG_LONG_THR=16 sends to the
long-row kernels.  The slab chains need more: slab_count (csrc/layout.hpp) takes no slab below 0.25 MiB and no matrix below
2^20 nonzeros, so three slabs for A and for A' (the middle pass exists from three on) start at 65 537 rows and columns;
66 000 x 66 000 with 16 entries per row is the smallest round shape that gives them.  Its two dense rows and columns are
long rows at the default threshold: the chain and the long-row pair are the graph's parallel branches.

Which rows are the oracle's bits: those of at most H.bitexact_row_limit() entries that stay on the row-block path.  Rows
beyond the layout's long-row threshold are summed by the long-row kernels' fixed tree in either row order
(spmv_kernels.hpp: long_chunk_finish), and a sweep forced onto a small matrix tree-reduces same-row runs of more than 8
entries in relaxed order (helpers.assert_products_match_oracle: forced_sweep); those rows are held to 1e-13 * sum |a x|,
as everywhere in this suite."""
import json
import os
import sys

import numpy as np
import pytest

import folp_loader

folp_loader.load()       # (the recorder runs without pytest, whose conftest loads the package)

from firstorderlp_jl_amd import HipPdhgEngine  # noqa: E402
from firstorderlp_jl_amd.generators import random_lp  # noqa: E402
from firstorderlp_jl_amd.primal_dual_hybrid_gradient import AdaptiveStepsizeParams, PdhgSolverState, take_step  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import helpers as H  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "product_kernel_names.json")
K_SPMV_DUAL, K_SPMV_ATY = 1, 2

SHAPES = {"plain": lambda: random_lp(300, 260, 4, seed=11),
          "long": lambda: H.with_dense_rows_and_columns(300, 280, 4, seed=12),
          "slab": lambda: H.with_dense_rows_and_columns(66_000, 66_000, 16, seed=13)}
# form -> (the knobs that force it, the kernel family its names must show)
FORMS = {"stream": (dict(PDHG_SPMV="stream", PDHG_SJ="0", PDHG_STREAM_PIPE="0"), "spmv_stream_kernel<"),
         "pipe": (dict(PDHG_SPMV="stream", PDHG_SJ="0", PDHG_STREAM_PIPE="1"), "spmv_stream_pipe_kernel<"),
         "sj_narrow": (dict(PDHG_SPMV="stream", PDHG_SJ="1", PDHG_SJ_WIDE="0", PDHG_STREAM_PIPE="0"), "spmv_sj_kernel<"),
         "sj_wide": (dict(PDHG_SPMV="stream", PDHG_SJ="1", PDHG_SJ_WIDE="1", PDHG_STREAM_PIPE="0"), "spmv_sj_kernel<"),
         "sweep": (dict(PDHG_SPMV="tiled", PDHG_TILE_COLS="64", PDHG_GRAPH_TILED="1", PDHG_TUNE="0"), "spmv_tiled_kernel<")}
for _f in ("stream", "pipe", "sj_narrow"):
    FORMS["slabs_" + _f] = (dict(FORMS[_f][0], PDHG_SLABS="1", PDHG_SLAB_MB="0.25"), FORMS[_f][1])
CASES = [(f, s) for f in ("stream", "pipe", "sj_narrow", "sj_wide", "sweep") for s in ("plain", "long")] + \
        [(f, "slab") for f in ("slabs_stream", "slabs_pipe", "slabs_sj_narrow")]
KNOBS = ("PDHG_SPMV", "PDHG_SJ", "PDHG_SJ_WIDE", "PDHG_SJ_MAXLEN", "PDHG_STREAM_PIPE", "PDHG_SLABS", "PDHG_SLAB_MB",
         "PDHG_TILE_COLS", "PDHG_TILE_SHIFT", "PDHG_VAR_TILES", "PDHG_GRAPH_TILED", "PDHG_TUNE", "PDHG_LONG_THR", "PDHG_GRAPH")


def _environment(form, shape, graph):
    """Every knob a case depends on: the value to set, or None for "not set"."""
    env = dict.fromkeys(KNOBS)
    env.update(PDHG_SLABS="0", PDHG_COOP="0", PDHG_DEVICE_LOOP="0", PDHG_SMALL_LP="0", PDHG_GRAPH=graph)
    env.update(FORMS[form][0])
    if shape == "long":
        env["PDHG_LONG_THR"] = "16"
    return env


def _names(eng):
    return [eng.kernel_name(K_SPMV_DUAL), eng.kernel_name(K_SPMV_ATY)]


def _assert_form_was_built(eng, form, shape):
    info, names = eng.layout_info(), _names(eng)
    family = FORMS[form][1]
    for side, name in zip(("A", "At"), names):
        assert family in name, (form, side, name)
        assert (info[side + "_tiled_waves"] > 0) == (form == "sweep"), (form, info)
        assert info[side + "_pipe"] == int(form.endswith("pipe")) and info[side + "_sj"] == int("sj" in form), (form, info)
        if "sj" in form:
            assert info[side + "_sj_wide"] == int(form.endswith("wide")), (form, info)
        if form.startswith("slabs"):       # first pass, middle pass(es), the pass with the epilogue
            assert info[side + "_slabs"] >= 3 and name.count(family) == 3, (form, info, name)
        else:
            assert info[side + "_slabs"] == 0 and name.count(family) == 1, (form, info, name)
        has_long = shape != "plain"
        assert (info[side + "_long_rows"] >= 2) == has_long and ("spmv_long_final_kernel<" in name) == has_long, (form, info, name)


def _assert_products_are_the_oracles(eng, p, form):
    A = p.constraint_matrix
    m, n = A.shape
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(n), rng.standard_normal(m)
    relaxed = os.environ.get("PDHG_ROW_ORDER", "relaxed") == "relaxed"
    limit = min(H.bitexact_row_limit(), int(os.environ.get("PDHG_LONG_THR", "2048")), 8 if form == "sweep" and relaxed else 2048)
    absA = abs(A).tocsr()
    for got, want, nnz_per, scale, name in (
            (eng.spmv(x), orc.spmv(m, n, A.indptr, A.indices, A.data, x), np.diff(A.tocsr().indptr), absA @ np.abs(x), "A x"),
            (eng.spmv_t(y), orc.spmv_t(m, n, A.indptr, A.indices, A.data, y), np.diff(A.indptr), absA.T @ np.abs(y), "A'y")):
        short = nnz_per <= limit
        assert 2 * short.sum() > short.size, (form, name, limit)       # (most rows are held to the bits)
        assert np.array_equal(got[short], want[short]), f"{form} {name}: rows of <= {limit} entries differ from the oracle"
        assert np.all(np.abs(got - want) <= 1e-13 * scale + 1e-300), f"{form} {name}: beyond 1e-13 * sum |a x|"


def _take_steps(eng, p, steps=30):
    step, pw = H.initial_step_and_weight(p)
    st = PdhgSolverState(eng, step_size=step, primal_weight=pw)
    sizes = []
    for _ in range(steps):
        take_step(AdaptiveStepsizeParams(0.3, 0.6), st)
        sizes.append(st.step_size)
    return (*eng.get_current(), *eng.get_average(), eng.get_dual_product(), np.array(sizes), st.total_number_iterations)


_made = {}


def _problem(shape):      # built once, shared by the cases
    if shape not in _made:
        _made[shape] = SHAPES[shape]()
    return _made[shape]


@pytest.mark.parametrize("form,shape", CASES, ids=[f"{f}-{s}" for f, s in CASES])
def test_graph_and_plain_launches_run_the_same_steps(gpu_required, monkeypatch, row_order_mode, form, shape):
    p = _problem(shape)
    engines = {}
    for graph in ("1", "0"):
        for k, v in _environment(form, shape, graph).items():
            monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)
        engines[graph] = HipPdhgEngine.from_problem(p)
        engines[graph].layout_info()       # (a handle reads PDHG_GRAPH when it is first asked how its trials run)
    try:
        eng, plain = engines["1"], engines["0"]
        _assert_form_was_built(eng, form, shape)
        with open(GOLDEN) as f:
            assert _names(eng) == json.load(f)[f"{form}-{shape}-{row_order_mode}"]
        assert _names(plain) == _names(eng)
        _assert_products_are_the_oracles(eng, p, form)
        r_graph, r_plain = _take_steps(eng, p), _take_steps(plain, p)
        assert len(set(r_graph[5].tolist())) > 1, "the step size never changed: the dual nodes kept their parameters"
        for a, b in zip(r_graph, r_plain):
            assert np.array_equal(a, b)
        # the graph run took its trials as graph launches, the other one none (and neither a persistent kernel)
        assert eng.layout_info()["trial_graph"] == 1 and eng.steps_info()[:2] == [0, 0] and eng.host_issue_stats()[0] >= 30
        assert plain.layout_info()["trial_graph"] == 0 and plain.steps_info()[:2] == [0, 0] and plain.host_issue_stats()[0] == 0
    finally:
        for e in engines.values():
            e.close()


def record(path):
    """The names of every case in both row orders, from the library this process loads."""
    os.environ["PDHG_DEV"] = "1"
    out = {}
    for form, shape in CASES:
        p = _problem(shape)
        for order in ("relaxed", "strict"):
            for k, v in dict(_environment(form, shape, "1"), PDHG_ROW_ORDER=order).items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            eng = HipPdhgEngine.from_problem(p)
            _assert_form_was_built(eng, form, shape)
            out[f"{form}-{shape}-{order}"] = _names(eng)
            eng.close()
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    record(sys.argv[1])
