"""apply() / evolve() without a GPU: the stored-source Clenshaw recurrence restated in numpy against dense
V g(E) V†, the coefficient rules, the layouts and argument errors, and the register budget of the new kernels."""

import os
import shutil
import sys

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import apply as ap
from bodge_amd import chebyshev as cheb

import apply_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ algorithm
@pytest.mark.parametrize("name", ["disordered_real", "disordered_complex"])
def test_restatement_matches_dense_eigh(name):
    """Measured on the 9x8 lattices (a = 5.57, three random complex unit vectors, cut-off 1e-13): evolve 1e-15 at
    t = 0.5 (M = 19), 9e-15 at t = 10 (M = 93), 3e-14 at t = 100 (M = 635), 8e-14 at t = 400 (M = 2351); Fermi
    function at T = 0.05 3e-14 (M = 960); norm drift at most 2e-14.  Pinned at 1e-11 and 1e-12; the norm cannot
    drift by more than the error of the vector."""
    system = cases.SYSTEMS[name]()
    h = np.asarray(system.matrix("dense"))
    assert (np.abs(h.imag).max() == 0) == (name == "disordered_real")
    scale = cases.scale_of(system)
    x = cases.unit_vectors(system)
    for t in (0.5, 10.0, 100.0, 400.0):
        coef = ap.evolution_coefficients(scale, np.array([t]), 13.0)
        got = cases.stored_source_clenshaw(h, scale, coef, x)[:, 0]
        exact = cases.dense_function(system, lambda e: np.exp(-1j * e * t), x)
        error = np.abs(got - exact).max()
        drift = np.abs(np.linalg.norm(got, axis=1) - 1).max()
        print(name, "evolve", t, len(coef), error, drift)
        assert error < 1e-11 and drift < 1e-11
    coef = cases.fermi_coefficients(scale, 0.05)[:, None]
    got = cases.stored_source_clenshaw(h, scale, coef, x)[:, 0]
    exact = cases.dense_function(system, lambda e: cheb.fermi_function(e, 0.05), x)
    print(name, "fermi", len(coef), np.abs(got - exact).max())
    assert np.abs(got - exact).max() < 1e-12


def test_restatement_handles_several_functions_and_vectors():
    system = cases.SYSTEMS["disordered_complex"]()
    h = np.asarray(system.matrix("dense"))
    scale = cases.scale_of(system)
    x = cases.unit_vectors(system, 2)
    times = np.array([0.3, -2.0, 5.0])
    coef = ap.evolution_coefficients(scale, times, 13.0)
    got = cases.stored_source_clenshaw(h, scale, coef, x)
    exact = cases.dense_function(system, lambda e: np.exp(-1j * np.outer(times, e)), x)
    assert got.shape == exact.shape == (2, 3, h.shape[0])
    assert np.abs(got - exact).max() < 1e-11


# ------------------------------------------------------------------ coefficient rules
@pytest.mark.parametrize("reach", [0.0, 0.4, 7.0, 56.9, -56.9, 569.0])
def test_evolve_series_equals_the_chebyshev_gauss_coefficients(reach):
    coef = ap.evolution_coefficients(1.0, np.array([reach]), 13.0)[:, 0]
    gauss = cheb.chebyshev_coefficients_complex(lambda x: np.exp(-1j * reach * x), len(coef))
    assert np.abs(coef - gauss).max() < 1e-12
    # the cut-off: nothing of size 1e-13 is left out, and the last coefficient kept is above it
    longer = cheb.chebyshev_coefficients_complex(lambda x: np.exp(-1j * reach * x), len(coef) + 32)
    assert np.abs(longer[len(coef):]).max() < 1e-13 and (len(coef) == 1 or abs(coef[-1]) >= 1e-13)


def test_evolve_series_of_several_times_share_one_length():
    times = np.array([0.1, -3.0, 20.0])
    coef = ap.evolution_coefficients(5.7, times, 12.0)
    assert coef.shape[1] == 3 and coef.shape[0] == len(ap.evolution_coefficients(5.7, times[2:], 12.0))
    for f, t in enumerate(times):
        single = ap.evolution_coefficients(5.7, np.array([t]), 12.0)[:, 0]
        assert np.array_equal(coef[: len(single), f], single)
        assert np.abs(coef[len(single):, f]).max(initial=0.0) < 1e-12


def test_complex_coefficient_rule_keeps_the_real_one_bit_for_bit():
    real = cheb.chebyshev_coefficients(lambda x: cheb.fermi_function(5.7 * x, 0.05), 300)
    both = cheb.chebyshev_coefficients_complex(lambda x: cheb.fermi_function(5.7 * x, 0.05), 300)
    assert both.dtype == np.complex128 and np.array_equal(both.real, real) and not both.imag.any()
    mixed = cheb.chebyshev_coefficients_complex(lambda x: np.exp(x) + 1j * np.cos(3 * x), 40)
    assert np.array_equal(mixed.real, cheb.chebyshev_coefficients(np.exp, 40))
    assert np.array_equal(mixed.imag, cheb.chebyshev_coefficients(lambda x: np.cos(3 * x), 40))


@pytest.mark.parametrize("temperature", [0.02, 0.05, 0.2, 1.0])
def test_automatic_order_reproduces_the_fermi_rule(temperature):
    scale = 5.7
    coef = ap.series_coefficients(lambda e: cheb.fermi_function(e, temperature), scale, 12.0)
    rule = cheb.moments_for_fermi(scale, temperature, 12.0)
    print(temperature, len(coef), rule)
    assert rule / 2 <= len(coef) <= 2 * rule
    grid = np.linspace(-scale, scale, 4001)
    series = np.polynomial.chebyshev.chebval(grid / scale, coef)
    assert np.abs(series - cheb.fermi_function(grid, temperature)).max() < 1e-10


def test_a_step_function_is_refused():
    with pytest.raises(ValueError, match="not smooth"):
        ap.series_coefficients(lambda e: np.where(e > 0, 0.0, 1.0), 5.7, 12.0)


# ------------------------------------------------------------------ layouts and errors
class _RestatementSolver:
    """Stands in for the device mirror: the same call, summed by the numpy restatement."""

    def __init__(self, system):
        self.h = system.matrix("csr")
        self.calls = []

    def apply_series(self, scale, coef, x):
        self.calls.append((np.asarray(coef).shape, np.asarray(x).shape))
        return cases.stored_source_clenshaw(self.h, scale, coef, x)


@pytest.fixture
def host_system(monkeypatch):
    system = cases.uniform_swave((4, 3, 1))
    solver = _RestatementSolver(system)
    monkeypatch.setattr(system, "_solver", lambda *args, **kwargs: solver)
    return system, solver


def test_every_accepted_layout_round_trips(host_system):
    system, solver = host_system
    n = system.lattice.size
    rows = cases.unit_vectors(system, 3)
    layouts = {"(4N,)": rows[0], "(4N, R)": rows.T, "(N, 4)": rows[0].reshape(n, 4), "(R, N, 4)": rows.reshape(3, n, 4),
               "(4N, 1)": rows[:1].T, "(1, N, 4)": rows[:1].reshape(1, n, 4)}
    h = np.asarray(system.matrix("dense"))
    for label, given in layouts.items():
        same = system.apply(None, given, coefficients=[1.0])
        assert same.shape == given.shape and np.array_equal(same, given), label
        product = system.apply(lambda e: e, given, moments=2)
        expected = (rows[: 1 if "1" in label or label in ("(4N,)", "(N, 4)") else 3] @ h.T)
        got = product.T if label.startswith("(4N, ") else product
        assert np.allclose(got.reshape(-1, 4 * n), expected, rtol=0, atol=1e-13), label
    assert system.apply(None, rows[0].real, coefficients=[2.0]).dtype == np.complex128
    assert all(x_shape[1] == 4 * n for _, x_shape in solver.calls)


def test_function_and_time_axes_lead(host_system):
    system, _ = host_system
    n = system.lattice.size
    rows = cases.unit_vectors(system, 2)
    scale = cases.scale_of(system)
    coef = np.stack([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 2.0]], axis=1)  # 1, x, 2(2x²-1)-1: columns = functions
    h = np.asarray(system.matrix("dense")) / scale
    exact = [rows, rows @ h.T, 2 * (2 * rows @ h.T @ h.T - rows) - rows]
    for given, back in ((rows[0], lambda y: y[None]), (rows.T, lambda y: y.T), (rows[0].reshape(n, 4), lambda y: y.reshape(1, -1)),
                        (rows.reshape(2, n, 4), lambda y: y.reshape(2, -1))):
        out = system.apply(None, given, coefficients=coef)
        assert out.shape == (3,) + np.shape(given)
        for f in range(3):
            assert np.allclose(back(out[f]), exact[f][: back(out[f]).shape[0]], rtol=0, atol=1e-13)
        one = system.apply(None, given, coefficients=coef[:, :1])
        assert one.shape == (1,) + np.shape(given)  # a 2-D coefficient array always gives the axis
    x = rows.reshape(2, n, 4)
    times = np.array([0.0, 0.7, -0.7])
    moved = system.evolve(x, times)
    assert moved.shape == (3, 2, n, 4) and np.allclose(moved[0], x, rtol=0, atol=1e-13)
    assert system.evolve(x, 0.7).shape == x.shape and np.allclose(system.evolve(x, 0.7), moved[1], rtol=0, atol=1e-13)
    assert system.evolve(x, np.array([0.7])).shape == (1, 2, n, 4)
    exact = cases.dense_function(system, lambda e: np.exp(-1j * np.outer(times, e)), rows)  # (V, F, 4N)
    assert np.allclose(moved.reshape(3, 2, -1), np.moveaxis(exact, 1, 0), rtol=0, atol=1e-11)
    assert np.allclose(system.evolve(moved[1], -0.7), x, rtol=0, atol=1e-11)


def test_argument_errors(host_system):
    system, _ = host_system
    n = system.lattice.size
    x = cases.unit_vectors(system, 1)[0]
    for bad in (x[:-1], np.zeros((n, 3)), np.zeros((2, n + 1, 4)), np.zeros((4 * n, 0)), np.zeros((2, 2, n, 4)), 1.0):
        with pytest.raises(ValueError, match="vectors"):
            system.apply(None, bad, coefficients=[1.0])
        with pytest.raises(ValueError, match="vectors"):
            system.evolve(bad, 1.0)
    broken = x.copy()
    broken[3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        system.apply(np.exp, broken)
    with pytest.raises(ValueError, match="finite"):
        system.evolve(broken, 1.0)
    with pytest.raises(ValueError, match="empty"):
        system.evolve(x, [])
    for bad in (np.inf, [0.0, np.nan], 1j, [[1.0, 2.0]], "now"):
        with pytest.raises(ValueError, match="times"):
            system.evolve(x, bad)
    with pytest.raises(ValueError, match="either"):
        system.apply(None, x)
    with pytest.raises(ValueError, match="either"):
        system.apply(np.exp, x, coefficients=[1.0])
    with pytest.raises(ValueError, match="coefficients"):
        system.apply(None, x, coefficients=np.zeros((2, 2, 2)))
    with pytest.raises(ValueError, match="coefficients"):
        system.apply(None, x, coefficients=[])
    with pytest.raises(ValueError, match="finite"):
        system.apply(None, x, coefficients=[1.0, np.inf])
    with pytest.raises(ValueError, match="callable"):
        system.apply(3.0, x)
    with pytest.raises(ValueError, match="moments"):
        system.apply(np.exp, x, moments=0)
    with pytest.raises(ba.common.TypeCheckError):
        system.apply(np.exp, x, moments=2.5)
    for bad in ({"digits": "12"}, {"scale": "wide"}, {"digits": None}, {"scale": True}):
        with pytest.raises(ba.common.TypeCheckError):
            system.apply(np.exp, x, **bad)
        with pytest.raises(ba.common.TypeCheckError):
            system.evolve(x, 1.0, **bad)
    assert system.evolve(x, 1.0, digits=12, scale=6).shape == x.shape  # (whole numbers are numbers)
    with pytest.raises(ValueError, match="scale"):
        system.apply(np.exp, x, scale=-1.0)
    with pytest.raises(ValueError, match="not smooth"):
        system.apply(lambda e: np.sign(e), x)
    with pytest.raises(ValueError, match="finite"):
        with np.errstate(all="ignore"):
            system.apply(lambda e: 1.0 / (e - e), x, moments=8)


def test_entry_point_refuses_bad_arguments_without_a_gpu(hip_library):
    """bdg_apply_series checks its scalar arguments and pointers before it looks at the handle or a device, so each
    refusal is reachable here with buffers of one entry and no handle (the handle is the last thing it checks)."""
    import ctypes

    from bodge_amd import backend

    one = np.zeros(2)
    ptr = backend.as_f64p(one)
    call = hip_library.bdg_apply_series
    for args, message in (
        ((None, 1.0, 0, 1, ptr, 1, ptr, ptr), b"n_moments"),
        ((None, 1.0, 1, 0, ptr, 1, ptr, ptr), b"n_functions"),
        ((None, 1.0, 1, 1, ptr, 0, ptr, ptr), b"n_vectors"),
        ((None, 1.0, -3, 1, ptr, 1, ptr, ptr), b"n_moments"),
        ((None, 0.0, 1, 1, ptr, 1, ptr, ptr), b"scale"),
        ((None, float("nan"), 1, 1, ptr, 1, ptr, ptr), b"scale"),
        ((None, 1.0, 1, 1, None, 1, ptr, ptr), b"null argument"),
        ((None, 1.0, 1, 1, ptr, 1, None, ptr), b"null argument"),
        ((None, 1.0, 1, 1, ptr, 1, ptr, None), b"null argument"),
        ((None, 1.0, 1, 1, ptr, 1, ptr, ptr), b"null system handle"),
    ):
        assert call(*args) == -1 and message in hip_library.bdg_last_error(), (args[1:4], args[5], message)
    assert "bdg_apply_series" in backend.SIGNATURES and ("apply", ctypes.c_int32) in backend.Perf._fields_


def test_solver_binding_checks_shapes_before_the_library():
    """DeviceSolver.apply_series refuses wrong shapes itself: no library call is made (the object here has no handle)."""
    from bodge_amd.solver import DeviceSolver

    solver = object.__new__(DeviceSolver)
    solver.dim = 48
    x = np.zeros((2, 48), dtype=np.complex128)
    for coef, vectors in ((np.ones(3), x), (np.ones((0, 1)), x), (np.ones((3, 0)), x), (np.ones((3, 1)), x[0]),
                          (np.ones((3, 1)), x[:, :47]), (np.ones((3, 1)), x[:0])):
        with pytest.raises(ValueError, match="apply_series"):
            solver.apply_series(1.0, coef, vectors)


def test_product_path_fails_loudly_without_gpu(hip_library):
    """No CPU fallback: without a device apply() and evolve() raise, they do not compute."""
    from bodge_amd import backend

    if backend.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device behaviour cannot be exercised here")
    system = cases.uniform_swave((4, 3, 1))
    x = cases.unit_vectors(system, 1)[0]
    for call in (lambda: system.apply(np.exp, x), lambda: system.evolve(x, 1.0),
                 lambda: system.apply(None, x, coefficients=[1.0])):
        with pytest.raises(RuntimeError, match="GPU|HIP"):
            call()


# ------------------------------------------------------------------ kernels
@pytest.fixture(scope="module")
def resources():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    return kernel_resources.collect()


def _row(resources, name):
    # (c++filt prints the return type of template instances only)
    matches = [row for key, row in resources.items() if key.startswith((f"void bdg::{name}(", f"bdg::{name}("))]
    assert len(matches) == 1, (name, [k for k in resources if "apply" in k][:8])
    return matches[0]


@pytest.mark.timeout(900)
def test_stored_source_kernels_do_not_spill_and_keep_their_occupancy(resources):
    """The stored-source steps are the Clenshaw kernels with one more load per entry and a complex coefficient: the
    same register class (no scratch, at most 128 VGPRs, 4 waves per SIMD).  Every instance the compiler emitted is
    checked, and the list is the expected one: 20 generic (4 modes x 5 lane counts) and 54 dictionary instances
    (3 row widths x 4 lane counts in the real modes, x 5 in the complex ones)."""
    expected = set()
    for mode in ("RealPHMode", "ComplexPHMode", "RealMode", "ComplexMode"):
        for rl in (4, 8, 16, 32, 64):
            expected.add(f"void bdg::cheb_family<bdg::{mode}, {rl}, bdg::ApplyTail<false> >(bdg::ApplyTail<false>::Args)")
            if rl == 64 and mode.startswith("Real"):
                continue
            for maxb in (3, 5, 7):
                expected.add(f"void bdg::cheb_family_dict<bdg::{mode}, {rl}, {maxb}, bdg::ApplyTail<true> >(bdg::ApplyTail<true>::Args)")
    found = {key: row for key, row in resources.items() if "bdg::ApplyTail" in key}
    assert set(found) == expected and len(found) == 74, sorted(set(found) ^ expected)
    for key, row in found.items():
        assert row["scratch"] == 0 and row["vgpr"] <= 128 and row["occupancy"] >= 4, (key, row)
    for name in ("apply_scatter", "apply_gather"):
        assert _row(resources, name)["scratch"] == 0
