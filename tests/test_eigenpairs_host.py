"""eigenpairs() without a GPU: the filtered subspace iteration restated in numpy against dense eigh, the coefficient
rule, the argument errors, the refusals of the bdg_subspace_* entry points that need no device, and the register
budget of the new kernels."""

import os
import shutil
import sys

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import chebyshev as cheb
from bodge_amd import eigenpairs as ep

import eigenpairs_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The restatement against numpy.linalg.eigh, as measured at M = 256, tol = 1e-9 with the library's start vectors
# (seed 0): largest |E − E_ref| 2.9e-15, largest |V V† − 1| 3.6e-15 over the four systems.  Pinned at ten times that.
ENERGY_PIN = 3e-14
ORTHONORMALITY_PIN = 4e-14


# ------------------------------------------------------------------ algorithm
@pytest.mark.parametrize("name", sorted(cases.SYSTEMS))
def test_restatement_matches_dense_eigh(name):
    """ysr_real: 22 states, 19 iterations; ysr_complex: 16, 24; cube: 4, 7; periodic_degenerate: 32 in clusters of
    16, 8 and 8, 4 iterations.  The cap is twice the measured count: a filter or a criterion that got worse shows."""
    c = cases.case(name)
    energies, vectors, iterations, residuals, columns = cases.restated(name)
    print(name, "count", c.count, "iterations", iterations, "edge gap", c.edge_gap, "columns", columns)
    assert len(energies) == c.count and columns == int(np.ceil(1.25 * c.count)) + 8
    assert iterations <= 2 * cases.ITERATIONS[name]
    deviation = np.abs(energies - c.energies).max()
    orthonormality = cases.orthonormality(vectors)
    print(name, "dE", deviation, "orthonormality", orthonormality, "subspace", cases.subspace_deviation(c, vectors),
          "residual / a", residuals.max() / c.scale)
    assert deviation <= ENERGY_PIN and orthonormality <= ORTHONORMALITY_PIN
    assert residuals.max() <= cases.TOL * c.scale
    assert np.abs(c.dense.imag).max() > 0 if name == "ysr_complex" else np.abs(c.dense.imag).max() == 0


def test_the_cases_are_what_they_are_meant_to_be():
    counts = {name: cases.case(name).count for name in cases.SYSTEMS}
    assert counts == {"ysr_real": 22, "ysr_complex": 16, "cube": 4, "periodic_degenerate": 32}
    assert sorted(len(m) for m in cases.case("periodic_degenerate").clusters()) == [8, 8, 16]
    assert all(len(m) == 1 for m in cases.case("ysr_real").clusters())
    for name in cases.SYSTEMS:  # every edge sits in a gap: no level within 5e-3 of it
        assert cases.case(name).edge_gap > 5e-3


def test_start_vectors_are_rademacher_and_differ_by_id():
    block = cases.start_block(480, 0, 0, 6)
    assert block.dtype == np.complex128 and set(np.unique(block.real)) == {-1.0, 1.0} and not block.imag.any()
    assert np.abs(block @ block.T / 480 - np.eye(6)).max() < 0.2
    assert np.array_equal(cases.start_block(480, 0, 4, 2), block[4:])
    assert not np.array_equal(cases.start_vector(480, 1, 0), block[0])


# ------------------------------------------------------------------ coefficient rule
@pytest.mark.parametrize("window", [(0.0, 0.55), (-1.3, -0.2), (-0.4, 0.9), (6.0, 9.0), (-9.0, 9.0)])
def test_coefficients_equal_the_chebyshev_gauss_rule_of_the_damped_indicator(window):
    """The Gauss rule on N = 2^18 nodes sees the step aliased: c_k^N − c_k = Σ_j ±c_{2jN±k}, terms of size 2/(π·2jN)
    with alternating signs, so the difference stays below 4/(πN) = 5e-6 per edge; 2e-5 allows for both edges."""
    scale, moments = 7.5, 256
    lo, hi = window
    coef = ep.window_coefficients(scale, lo, hi, moments)
    gauss = cheb.chebyshev_coefficients(lambda x: ((scale * x >= lo) & (scale * x <= hi)).astype(float), moments,
                                        oversample=1024) * cheb.jackson_kernel(moments)
    print(window, np.abs(coef - gauss).max())
    assert np.abs(coef - gauss).max() < 2e-5
    assert np.array_equal(coef, cases.window_series(scale, lo, hi, moments))
    # what the series is for: 1 well inside, a half at an edge inside the band, small outside.  The Jackson kernel is
    # close to a Gaussian of width πa/M in energy, so two widths beyond an edge the step has fallen to about
    # Φ(−2) = 2.3e-2 (3e-2 allowed), and a window four widths wide reaches 1 − 2Φ(−2) at its centre.
    value = lambda e: np.polynomial.chebyshev.chebval(e / scale, coef)
    width = np.pi * scale / moments
    if hi - lo > 4 * width and hi < scale:
        assert abs(value(0.5 * (lo + hi)) - 1) < 5e-2 and abs(value(hi) - 0.5) < 2e-2
        assert abs(value(hi + 2 * width)) < 3e-2


def test_default_degree_follows_the_window_width():
    assert ep.default_moments(7.5, 0.0, 0.55) == int(np.ceil(8 * np.pi * 7.5 / 0.55))
    assert ep.default_moments(7.5, -7.0, 7.0) == ep.MOMENTS_MIN == 128
    assert ep.default_moments(7.5, 0.1, 0.101) == ep.MOMENTS_MAX == 4096
    assert ep.default_moments(7.5, 0.1, 0.1) == 4096
    assert ep.block_size(22) == 36 and ep.block_size(4) == 13 and ep.block_size(10.2, 1.0) == 24


def test_rayleigh_ritz_drops_dependent_directions():
    rng = np.random.default_rng(2)
    h = rng.standard_normal((30, 30))
    h = h + h.T
    x = rng.standard_normal((5, 30)) + 1j * rng.standard_normal((5, 30))
    x = np.vstack([x, x[0] + x[1]])  # six columns (as rows), rank five
    theta, q = ep.rayleigh_ritz(x.conj() @ x.T, x.conj() @ (h @ x.T))
    assert theta.shape == (5,) and q.shape == (6, 5)
    rotated = q.T @ x
    assert np.abs(rotated.conj() @ rotated.T - np.eye(5)).max() < 1e-12
    assert np.abs(rotated.conj() @ (h @ rotated.T) - np.diag(theta)).max() < 1e-12


# ------------------------------------------------------------------ argument errors
def test_argument_errors_need_no_device(monkeypatch):
    system = cases.case("cube").system
    monkeypatch.setattr(system, "_solver", lambda *a, **k: pytest.fail("a device call was made"))
    scale = cases.case("cube").scale
    for window, message in (((0.4, 0.1), "lo > hi"), ((0.0, np.inf), "finite"), ((np.nan, 1.0), "finite"),
                            ((scale + 0.1, scale + 1.0), "outside"), ((-20.0, -scale - 0.1), "outside"),
                            ((0.1,), "pair"), (0.3, "pair"), (("a", "b"), "pair")):
        for method in ("auto", "subspace"):
            with pytest.raises(ValueError, match=message):
                system.eigenpairs(window, method=method)
    with pytest.raises(ValueError, match="method"):
        system.eigenpairs((0.0, 0.4), method="lanczos")
    with pytest.raises(RuntimeError, match="format"):
        system.eigenpairs((0.0, 0.4), format="csr")
    for bad, message in (({"moments": 1}, "moments"), ({"tol": 0.0}, "tol"), ({"tol": np.nan}, "tol"),
                         ({"max_iter": 0}, "max_iter"), ({"max_states": 0}, "max_states")):
        with pytest.raises(ValueError, match=message):
            system.eigenpairs((0.0, 0.4), **bad)
    with pytest.raises(ValueError, match="512"):
        system.eigenpairs((0.0, 0.4), max_states=500, method="subspace")
    for bad in ({"moments": 2.5}, {"max_iter": "many"}, {"seed": 0.5}, {"tol": "fine"}):
        with pytest.raises(ba.common.TypeCheckError):
            system.eigenpairs((0.0, 0.4), **bad)


def test_entry_points_refuse_bad_arguments_without_a_gpu(hip_library):
    """Every bdg_subspace_* call checks its scalar arguments and pointers before the handle, and the handle before any
    device: reachable here without one."""
    from bodge_amd import backend

    one = np.zeros(2)
    ptr = backend.as_f64p(one)
    lib = hip_library
    for call, args, message in (
        (lib.bdg_subspace_begin, (None, 0, 0, 0), b"n_columns"),
        (lib.bdg_subspace_begin, (None, 5000, 0, 0), b"n_columns"),
        (lib.bdg_subspace_begin, (None, 4, 0, 0), b"null system handle"),
        (lib.bdg_subspace_end, (None,), b"null system handle"),
        (lib.bdg_subspace_filter, (None, 1.0, 0, ptr), b"n_moments"),
        (lib.bdg_subspace_filter, (None, 0.0, 2, ptr), b"scale"),
        (lib.bdg_subspace_filter, (None, 1.0, 2, None), b"null argument"),
        (lib.bdg_subspace_filter, (None, 1.0, 2, ptr), b"null system handle"),
        (lib.bdg_subspace_project, (None, None, ptr), b"null argument"),
        (lib.bdg_subspace_project, (None, ptr, ptr), b"null system handle"),
        (lib.bdg_subspace_rotate, (None, 1, ptr, None, ptr), b"null argument"),
        (lib.bdg_subspace_rotate, (None, 1, ptr, ptr, ptr), b"null system handle"),
        (lib.bdg_subspace_refill, (None, 0, 1, 0, 0), b"null system handle"),
        (lib.bdg_subspace_read, (None, 0, 1, None), b"null argument"),
        (lib.bdg_subspace_read, (None, 0, 1, ptr), b"null system handle"),
        (lib.bdg_subspace_write, (None, 0, 1, None), b"null argument"),
        (lib.bdg_subspace_write, (None, 0, 1, ptr), b"null system handle"),
    ):
        assert call(*args) == -1 and message in lib.bdg_last_error(), (call.__name__, message, lib.bdg_last_error())


def test_solver_binding_checks_shapes_before_the_library():
    """DeviceSolver.subspace_* refuse a missing block and wrong shapes themselves (the object here has no handle)."""
    from bodge_amd.solver import DeviceSolver

    solver = object.__new__(DeviceSolver)
    solver.dim = 48
    for call in (lambda: solver.subspace_filter(1.0, np.ones(4)), lambda: solver.subspace_project(),
                 lambda: solver.subspace_rotate(np.eye(3), np.zeros(3)), lambda: solver.subspace_refill(0, 1),
                 lambda: solver.subspace_read(0, 1), lambda: solver.subspace_write(0, np.zeros((1, 48)))):
        with pytest.raises(ValueError, match="subspace_begin"):
            call()
    solver._subspace_columns = 3
    for q, theta in ((np.eye(4), np.zeros(4)), (np.eye(3), np.zeros(2)), (np.zeros((3, 0)), np.zeros(0)), (np.ones(3), np.zeros(3))):
        with pytest.raises(ValueError, match="subspace_rotate"):
            solver.subspace_rotate(q, theta)
    with pytest.raises(ValueError, match="subspace_filter"):
        solver.subspace_filter(1.0, np.ones((2, 2)))
    for first, count in ((-1, 1), (0, 0), (2, 2)):
        with pytest.raises(ValueError, match="subspace_read"):
            solver.subspace_read(first, count)
    for first, x in ((0, np.zeros((1, 47))), (2, np.zeros((2, 48))), (0, np.zeros(48))):
        with pytest.raises(ValueError, match="subspace_write"):
            solver.subspace_write(first, x)


def test_product_path_fails_loudly_without_gpu(hip_library):
    """No CPU fallback: without a device eigenpairs() raises on both routes, it does not compute."""
    from bodge_amd import backend

    if backend.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device behaviour cannot be exercised here")
    system = cases.case("cube").system
    for method in ("auto", "subspace"):
        with pytest.raises(RuntimeError, match="GPU|HIP"):
            system.eigenpairs((0.0, 0.4), method=method, max_states=4)


# ------------------------------------------------------------------ kernels
@pytest.fixture(scope="module")
def resources():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    return kernel_resources.collect()


@pytest.mark.timeout(900)
def test_subspace_kernels_use_no_scratch(resources):
    """Every compiled instance of the rotation and residual kernels: no scratch (the rotation holds 64 accumulator
    registers and eight prefetched entries of X per lane), and the rotation keeps two workgroups per CU's LDS."""
    found = {key: row for key, row in resources.items() if "subspace_" in key}
    names = sorted(key.split("bdg::")[1].split("(")[0] for key in found)
    assert names == ["subspace_fill", "subspace_residual", "subspace_residual_reduce", "subspace_rotate"], names
    for key, row in found.items():
        print(key, row)
        assert row["scratch"] == 0, (key, row)
    rotate = next(row for key, row in found.items() if "subspace_rotate" in key)
    assert rotate["vgpr"] <= 128 and rotate["occupancy"] >= 2
