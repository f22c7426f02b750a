"""The dense-solver cases and their checker (tests/dense_cases.py) on the CPU: the truth is right, the similarities are
exact, numpy's own eigensolver leaves room under the bounds, and the checker rejects results the older pins
(eigenvalues 1e-10, residual and orthonormality 1e-9) accept.  DESIGN §19."""

import numpy as np
import pytest

import dense_cases as dc
from dense_cases import Case, EPS, LD


@pytest.mark.parametrize("n", [4, 12, 68, 260])
def test_bisection_reproduces_the_analytic_spectra(n):
    """Long-double Sturm bisection against 2 - 2 cos(kπ/(n+1)) and against ±(n-1), ±(n-3), ... (the Clement matrix with
    its off-diagonal SQUARES k(n-k) given exactly) to 1e-17 |A|; measured 1e-19 and 0."""
    d, e = dc.seed("toeplitz", n)
    exact = dc.analytic("toeplitz", n)
    assert np.abs(dc.bisect(d, e.astype(LD) ** 2) - exact).max() <= 1e-17 * exact.max()
    k = np.arange(1, n)
    exact = dc.analytic("clement", n)
    assert np.abs(dc.bisect(np.zeros(n), (k * (n - k)).astype(LD)) - exact).max() <= 1e-17 * exact.max()
    # the float64 seed rounds the square roots: its levels move by at most 2 max|δe| <= eps (n - 1) / 2
    d, e = dc.seed("clement", n)
    assert np.abs(dc.bisect(d, e.astype(LD) ** 2) - exact).max() <= EPS * (n - 1) / 2


@pytest.mark.parametrize("n", dc.ALL_SIZES + (1028,))
def test_the_reflector_similarity_is_exact(n):
    for family in dc.families_at(n):
        if dc.SIMILARITY[family] == "H":
            assert dc.reflector_is_exact(family, n), family


@pytest.mark.parametrize("n", [4, 12, 68, 100])
def test_apply_is_the_dense_matrix(n):
    """`apply` (the factors, long double) against the dense matrix times a vector in long double."""
    x = np.random.default_rng(n).standard_normal((n, 3)) + 1j * np.random.default_rng(n + 1).standard_normal((n, 3))
    for case in dc.cases_at(n):
        a = dc.matrix(case)
        assert np.array_equal(a, a.conj().T) and a.dtype == (np.complex128 if case.phases else np.float64)
        direct = a.astype(dc.CLD) @ x.astype(dc.CLD)
        norm = float(np.abs(dc.truth(case)).max())
        assert np.abs(dc.apply(case, x) - direct).max() <= 1e-17 * n * norm, case.id
        indptr, indices, data = dc.bsr_arrays(a)
        assert data.shape[1:] == (4, 4) and indptr[-1] == indices.size >= n // 4


@pytest.mark.parametrize("n", dc.ALL_SIZES)
def test_numpy_leaves_room_under_the_bounds(n):
    """numpy.linalg.eigh on every case: each of the three ratios of §2 at most 0.3 (measured 0.14 / 0.16 / 0.28), so a
    device result is not judged against a bound the reference itself only just meets."""
    for case in dc.cases_at(n):
        got = dc.reference_ratios(case)
        assert got.worst() <= 0.3, (case.id, str(got))


def _old_pins_accept(case, w, z):
    a = dc.matrix(case)
    return (np.abs(w - dc.truth(case).astype(np.float64)).max() <= 1e-10 and np.abs(a @ z - z * w).max() <= 1.001e-9
            and np.abs(z.conj().T @ z - np.eye(case.n)).max() <= 1.001e-9)


def test_the_checker_rejects_a_moved_eigenvalue():
    case = Case("toeplitz", 68)
    w, z = (v.copy() for v in dc.reference(case))
    w[-1] += 4 * 68 * EPS * float(dc.truth(case).max())
    assert _old_pins_accept(case, w, z)
    got = dc.ratios(case, w, z, gap_term=True)
    assert 3.5 <= got.eigenvalues <= 4.5 and got.residual > 1


@pytest.mark.parametrize("phases", [False, True])
def test_the_checker_rejects_a_rotated_wilkinson_pair(phases):
    case = Case("wilkinson", 68, phases)
    w, z = (v.copy() for v in dc.reference(case))
    assert w[-1] - w[-2] <= 4 * EPS * w[-1]  # the pair agrees to rounding
    z[:, -1] += 1e-10 * z[:, -2]
    assert _old_pins_accept(case, w, z)
    for gap_term in (False, True):
        got = dc.ratios(case, w, z, gap_term=gap_term)
        assert got.orthonormality > 1000 and got.residual <= 0.3 and got.eigenvalues <= 0.3


def test_the_checker_rejects_mixed_ladder_vectors():
    case = Case("ladder_above", 68)
    w, z = (v.copy() for v in dc.reference(case))
    z[:, 30] += 1e-9 * z[:, 31]
    assert _old_pins_accept(case, w, z)
    assert dc.ratios(case, w, z).orthonormality > 1000           # Jacobi's bound: m eps whatever the gap
    assert dc.ratios(case, w, z, gap_term=True).residual > 1     # 1e-9 x 2e-5 = 2e-14 > 68 eps |A|


def test_the_checker_rejects_levels_swapped_in_a_degenerate_matrix():
    case = Case("degenerate", 68)
    w, z = (v.copy() for v in dc.reference(case))
    w[[33, 34]] = w[[34, 33]]  # the last 1 and the first 2
    assert dc.ratios(case, w, z, gap_term=True).worst() == np.inf  # not ascending
    w, z = (v.copy() for v in dc.reference(case))
    z[:, [33, 34]] = z[:, [34, 33]]
    got = dc.ratios(case, w, z, gap_term=True)
    assert got.eigenvalues <= 0.3 and got.residual > 1e12 and got.orthonormality <= 0.3


def test_the_checker_on_partial_and_degenerate_input():
    """Vectors of w[first:] only; the zero matrix (bound 0: eigenvalues exact or rejected); non-finite vectors."""
    case = Case("glued", 68, True)
    w, z = dc.reference(case)
    assert dc.ratios(case, w, z[:, 41:], first=41, gap_term=True).worst() <= 0.3
    assert dc.ratios(case, w, z[:, 40:], first=41).worst() == np.inf  # one vector too many
    assert dc.ratios(case, w, z[:, :0], first=68).worst() <= 0.3
    zero = Case("zero", 8)
    assert dc.ratios(zero, np.zeros(8), np.eye(8)).worst() == 0
    assert dc.ratios(zero, np.full(8, 1e-300), np.eye(8)).eigenvalues == np.inf
    bad = np.eye(8)
    bad[3, 3] = np.nan
    assert dc.ratios(zero, np.zeros(8), bad).worst() == np.inf
