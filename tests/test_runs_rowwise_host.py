"""options["runs"] around a caller's row-wise device objective, host side (no GPU): the ``rowwise`` tag of factory.batched, the
C ABI of csrc/sx_runs_unfused.hip -- struct mirror, entry points, the host-only record count -- and the argument checks of
optimize.minimize(factory.batched(f, rowwise=True), ..., options={"runs": R}), all of which raise a ValueError that names
`runs` before a device is needed."""
import ctypes as C
import os
import re
import warnings

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sx_runs_rowwise_partials", "sx_runs_rowwise_init", "sx_runs_rowwise_start", "sx_runs_rowwise_de_propose",
           "sx_runs_rowwise_pso_move", "sx_runs_rowwise_select", "sx_runs_rowwise_finalize")


@pytest.fixture(scope="module")
def lib():
    from stochopy_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def sa(lib):
    import stochopy_amd

    return stochopy_amd


def quadratic(X):
    return (X * X).sum(dim=1)


# ---- the tag
def test_batched_is_not_rowwise_unless_declared(sa):
    assert sa.factory.batched(quadratic).rowwise is False
    assert "rowwise" not in repr(sa.factory.batched(quadratic))


def test_rowwise_is_stored_and_shown(sa):
    f = sa.factory.batched(quadratic, rowwise=True)
    assert f.rowwise is True and f.fun is quadratic
    assert "rowwise=True" in repr(f) and "quadratic" in repr(f)
    assert sa.factory.batched(quadratic, rowwise=False).rowwise is False


def test_rowwise_takes_a_bool_by_keyword_only(sa):
    import inspect

    assert sa.factory.batched(quadratic, rowwise=True).rowwise is True  # the keyword exists ...
    for bad in (1, 0, None, "yes"):                                     # ... and takes nothing but a bool
        with pytest.raises(TypeError, match=re.escape(f"rowwise={bad!r}: expected True or False")):
            sa.factory.batched(quadratic, rowwise=bad)
    assert inspect.signature(sa.factory.batched).parameters["rowwise"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(TypeError):
        sa.factory.batched(quadratic, True)


def test_the_promise_is_in_the_docstring(sa):
    doc = " ".join(sa.factory.batched.__doc__.split())
    assert "the value of a row depends on that row only, so rows of several independent runs may be handed over in one call" in doc


def test_external_carries_the_flag(sa):
    from stochopy_amd.optimize import _common

    assert _common.resolve_objective(sa.factory.batched(quadratic, rowwise=True), ()).rowwise is True
    assert _common.resolve_objective(sa.factory.batched(quadratic), ()).rowwise is False


# ---- ABI
def test_struct_mirror_matches_the_library(lib):
    from stochopy_amd import _lib

    assert C.sizeof(_lib.SxRunsRowwiseArgs) == lib.sx_struct_size(12)
    assert _lib.SxRunsRowwiseArgs.R.offset == 19 * 8
    assert _lib.SxRunsRowwiseArgs.ftol.offset == C.sizeof(_lib.SxRunsRowwiseArgs) - 8
    assert lib.sx_struct_size(11) == -1 == lib.sx_struct_size(13)  # (11 is left out: tests/test_vd_runs_host.py)


def test_entry_points_are_declared_exported_and_bound(lib):
    from stochopy_amd import _lib

    with open(os.path.join(ROOT, "include", "stochopy_hip.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert "typedef struct sx_runs_rowwise_args" in header


@pytest.mark.parametrize("n", [3, 64, 65, 128, 129, 2048])
def test_record_count_per_run(lib, n):
    from stochopy_amd import _lib

    assert _lib.PROTOTYPES["sx_runs_rowwise_partials"][0] is C.c_int64  # (bound: a 64-bit count)
    rows = lib.sx_rows_per_workgroup(n)
    for P in (2, rows, rows + 1):
        if P < 2:
            continue
        assert lib.sx_runs_rowwise_partials(P, n) == -(-P // rows) == lib.sx_num_partials(P, n)


def test_record_count_refuses_what_is_no_batch(lib):
    from stochopy_amd import _lib

    assert lib.sx_runs_rowwise_partials.restype is _lib.PROTOTYPES["sx_runs_rowwise_partials"][0]
    assert lib.sx_runs_rowwise_partials(1, 8) < 0 and lib.sx_runs_rowwise_partials(8, 0) < 0
    assert lib.sx_runs_rowwise_partials(8, lib.sx_wide_from() + 1) < 0


# ---- refusals
R, P, N = 3, 8, 5
BASE = {"runs": R, "popsize": P, "maxiter": 4, "seed": 0, "rng": "philox", "updating": "deferred"}


def _call(sa, method="de", fun=None, x0=None, callback=None, n=N, **changes):
    opts = dict(BASE, **changes)
    if method in ("cmaes", "vdcma", "na"):  # (these have no `updating`)
        del opts["updating"]
    fun = fun if fun is not None else sa.factory.batched(quadratic, rowwise=True)
    return sa.optimize.minimize(fun, [[-5.12, 5.12]] * n, x0=x0, method=method, options=opts, callback=callback)


BAD = {
    "cmaes": lambda sa: _call(sa, "cmaes"),
    "vdcma": lambda sa: _call(sa, "vdcma", n=8),
    "na": lambda sa: _call(sa, "na"),
    "cpso, default competitivity": lambda sa: _call(sa, "cpso"),
    "cpso, one run restarts": lambda sa: _call(sa, "cpso", competitivity=[0.0, 0.5, 0.0]),
    "de, numpy-legacy": lambda sa: _call(sa, "de", rng="numpy-legacy"),
    "pso, numpy-legacy": lambda sa: _call(sa, "pso", rng="numpy-legacy"),
    "de, workers=2": lambda sa: _call(sa, "de", workers=2),
    "pso, workers=2": lambda sa: _call(sa, "pso", workers=2),
    "de, callback": lambda sa: _call(sa, "de", callback=lambda X, res: None),
    "pso, callback": lambda sa: _call(sa, "pso", callback=lambda X, res: None),
    "de, return_all": lambda sa: _call(sa, "de", return_all=True),
    "pso, return_all": lambda sa: _call(sa, "pso", return_all=True),
    "de, n = 2049": lambda sa: _call(sa, "de", n=2049),
    "pso, n = 2049": lambda sa: _call(sa, "pso", n=2049),
    "de, no seed": lambda sa: _call(sa, "de", seed=None),
    "pso, no seed": lambda sa: _call(sa, "pso", seed=None),
    "de, strict immediate": lambda sa: _call(sa, "de", updating="immediate", strict_updating=True),
    "pso, strict immediate": lambda sa: _call(sa, "pso", updating="immediate", strict_updating=True),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_refusals_name_runs_and_need_no_device(sa, what):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="runs"):
            BAD[what](sa)


def test_the_rowwise_batch_keeps_its_tables_to_itself(sa):
    """The base class knows nothing of its subclass: the row-wise entries are real symbols, in RowwiseBatch's own table."""
    from stochopy_amd import _lib
    from stochopy_amd.optimize import _runs

    assert sorted(_runs.RowwiseBatch.SWEEP) == sorted(_runs.RowwiseBatch.KINDS) == ["sx_runs_rowwise_de_propose",
                                                                                    "sx_runs_rowwise_pso_move"]
    assert not any("rowwise" in entry for entry in _runs.Batch.SWEEP)
    assert all(entry in _lib.PROTOTYPES for entry in list(_runs.Batch.SWEEP) + list(_runs.RowwiseBatch.SWEEP))
    assert _runs.RowwiseBatch.launch is not _runs.Batch.launch


@pytest.mark.parametrize("changes", [{}, {"competitivity": [0.0, 0.5, 0.0]}])
def test_the_cpso_refusal_names_competitivity(sa, changes):
    with pytest.raises(ValueError, match="runs") as e:
        _call(sa, "cpso", **changes)
    assert "competitivity" in str(e.value)


@pytest.mark.parametrize("method", ["de", "pso"])
def test_an_undeclared_objective_is_refused_and_told_how(sa, method):
    with pytest.raises(ValueError, match="runs") as e:
        _call(sa, method, fun=sa.factory.batched(quadratic))
    assert "rowwise=True" in str(e.value)


def test_reference_checks_still_come_first(sa):
    with pytest.raises(ValueError) as e:
        _call(sa, "de", mutation=3.0)
    assert str(e.value) == ""  # the reference's bare ValueError
    with pytest.raises(KeyError):
        _call(sa, "de", strategy="rand3bin")
