"""sporco_amd.admm.tvl1.TVL1Deconv against fixtures of the unmodified reference (tests/golden/tvl1dcn_*_f64.npz,
tools/make_golden_tvdcn.py) and against the NumPy statement of tests/_tvdcn_numpy.py; the checks themselves are
in tests/_tvdcn_checks.py, shared with tests/test_tvl2dcn.py.

Tolerances.  float64: the project's 1e-9 relative l2 on iterates, traces and the final rho; XSlvRelRes (it sits
at 1e-16) to an absolute 1e-12.  float32 input against the float64 fixture: the project's 1e-4 on iterates and
1e-3 on traces, or four times what the NumPy statement run in float32 shows against the same fixtures, whichever
is larger (the margin of four covers the summation order and the transform's own rounding).

Measured (test_f32_measured_figures repeats the measurement on the CPU), worst case over the fixtures of the
NumPy statement in float32 against the float64 fixture:
  iterates X, Y, U, relative l2:   1.35e-6 (`vec`; `autorho` 8.7e-7, every other case <= 7.5e-7)
  traces and the final rho:        1.77e-6 (`relax1`; `vec` 1.0e-6, every other case <= 6.7e-7)
Four times either lies far below the project's 1e-4 / 1e-3, which therefore apply unchanged.
"""

import numpy as np
import pytest

import _tvdcn_checks as ck

KIND = 'l1'
F32_ITER_MEASURED = 1.4e-6
F32_TRACE_MEASURED = 1.8e-6
F32_TOLS = (max(4.0 * F32_ITER_MEASURED, 1e-4), max(4.0 * F32_TRACE_MEASURED, 1e-3))


# ---- the class against the fixtures of the unmodified reference ----------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', ck.CASES[KIND])
def test_against_reference_fixture(backend, case, dtype):
    ck.check_fixture(KIND, case, dtype, F32_TOLS)


def test_fixtures_hold_their_conditions():
    ck.check_fixture_conditions(KIND)


def test_f32_measured_figures():
    """The figures of the header, measured again; the statement in float64 reproduces every fixture to 1e-9."""
    wi, wt = ck.measured_figures(KIND)
    assert wi <= F32_ITER_MEASURED and wt <= F32_TRACE_MEASURED


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_one_step_from_recorded_state(backend, dtype):
    ck.check_one_step(KIND, dtype, F32_TOLS)


# ---- kernel edges against the NumPy statement, shapes from the plan ------------------------------------------
@pytest.mark.parametrize('idx', range(22))
def test_kernel_edges(backend, idx):
    shapes = ck.edge_shapes(KIND)
    assert len(shapes) == 22
    shape, caxis, aplanes, expect = shapes[idx]
    ck.check_edge(KIND, shape, caxis, aplanes, expect=expect)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,caxis', [((60, 131, 3), None), ((60, 131, 3), 2), ((40, 520, 8), None)])
def test_kernel_edges_gpu(gpu_backend, shape, caxis):
    ck.check_edge(KIND, shape, caxis)


@pytest.mark.gpu
def test_wide_rows_f32_gpu(gpu_backend):
    """(33, 1024) in float32: items of four elements, one 16-byte access each."""
    ck.check_edge(KIND, (33, 1024), dtype=np.float32, f32_tols=F32_TOLS, expect={'V': 4, 'strips': 1})


# ---- contract and refusals -----------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_bitwise_repeatable(backend, dtype):
    ck.check_bitwise_repeatable(KIND, dtype)


def test_solve_twice_equals_one_long_run(backend):
    ck.check_solve_twice(KIND)


def test_callback_and_fastsolve(backend):
    ck.check_callback_and_fastsolve(KIND)


def test_defaults_attributes_and_constraint(backend):
    ck.check_surface(KIND)


def test_refusals(backend):
    ck.check_refusals(KIND)


def test_device_input(backend):
    ck.check_device_input(KIND)


# ---- recovery: the reference's tests/admm/test_tvl1.py TestSet02.test_02 ------------------------------------------
def test_recovery(backend):
    ck.check_recovery(KIND)
