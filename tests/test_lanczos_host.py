"""The references of the Lanczos tests pinned to each other, and the two-pass front end run on them (no GPU).

tests/test_gpu_lanczos.py holds the device to 20 times the distances measured here, so this module asserts that
the numpy restatements of csrc/lanczos.hpp (tests/lanczos_cases.py) are what they claim to be:
* the float64 sparse process against the dense long-double one, over the 16 iterations a trajectory is compared;
* the relations every single iteration obeys, over 64 iterations, evaluated in long double;
* `observables.lowest_eigenvalues` / `lowest_eigenpairs` with the system's solver replaced by `NumpyLanczosSolver`,
  against numpy.linalg.eigh: the record / ghost / `_krylov_length` logic without a device;
* `ritz_pairs_reference` against the dense eigenprojectors.
Measured here (relative to ‖H‖², taken as the Gershgorin bound squared): float64 to long double 8.8e-16 .. 2.5e-15
over 16 iterations on the lattices and 3.0e-14 on random357 (whose Gershgorin bound is loose and whose β falls to
0.03 ‖H‖²); over 64 iterations local residual 4.0e-17 .. 9.3e-17, | ‖v‖ - 1 | 1.7e-16 .. 2.5e-16,
|α_j - ‖H v_j‖²| 2.7e-17 .. 1.4e-16, |v_j·v_{j+1}| 3.1e-15 .. 3.4e-14.
"""

import numpy as np
import pytest

import lanczos_cases as lc
from oracle import cheb_ref


@pytest.mark.parametrize("name", lc.SMALL)
def test_float64_restatement_stays_near_long_double(name):
    """α and β of the first 16 iterations: sparse float64 against dense long double, four seeds, Rademacher and Z4.
    The cap of 1e-13 catches a broken restatement; the measured distance is what the GPU tests multiply by 20."""
    scale2 = lc.norm_bound(name) ** 2
    for kind in (cheb_ref.VEC_RADEMACHER, cheb_ref.VEC_Z4):
        start = np.concatenate([lc.start_block(name, 1, seed, kind) for seed in range(4)], axis=1)
        _, beta, _ = lc.lanczos_reference(lc.sparse_long_double(name), start, lc.LOCAL_HORIZON, lc.LD)
        # a condition on the inputs: the process does not break down inside any horizon the tests use
        assert beta.min() > 1e-3 * scale2, (name, kind, float(beta.min() / scale2))
    distance = lc.reference_distance(name, dense=True)
    # (the GPU tests take the long-double side from the CSR product: the same number to a part in 10^3)
    assert abs(lc.reference_distance(name) - distance) <= 1e-3 * distance
    print(f"{name}: float64 to long double over {lc.HORIZON} iterations {distance:.2e} of |H|^2")
    assert 0.0 < distance <= 1e-13


def test_sparse_long_double_product_is_the_dense_one():
    """The CSR long-double product (local checks on many vectors) against the dense np.clongdouble matrix."""
    for name in ("plane9x13_flux", "random357"):
        x = lc.start_block(name, 3, 5, cheb_ref.VEC_Z4).astype(lc.CLD) / lc.LD(3)
        dense, sparse = lc.dense_long_double(name) @ x, lc.sparse_long_double(name) @ x
        assert np.abs(dense - sparse).max() <= 32 * np.finfo(lc.LD).eps * lc.norm_bound(name)


@pytest.mark.parametrize("name", lc.SMALL)
def test_local_relations_of_the_restatement(name):
    """Three-term residual, norms, neighbour overlaps and α_j = ‖H v_j‖² of the float64 restatement's own vectors,
    in long double, over 64 iterations (local relations hold where trajectories have long separated)."""
    for kind in (cheb_ref.VEC_RADEMACHER, cheb_ref.VEC_Z4):
        figures = lc.reference_local_figures(name, 4, 1, kind)
        print(f"{name} kind {kind}: " + ", ".join(f"{key} {value:.2e}" for key, value in figures.items()))
        # fixed caps that a broken restatement misses by ten orders; the measured figures are what the GPU tests use.
        # The overlap is the one figure that grows along the process (Paige: each step adds a few ε‖A‖/β_{j+1}, and
        # carries the earlier defect on); the others are a handful of roundings of one iteration.
        caps = dict(residual=1e-15, norm=1e-14, alpha=1e-14, overlap=1e-11)
        assert all(0.0 < figures[key] <= caps[key] for key in caps), figures


def test_accumulation_reference_is_the_plain_sum():
    rng = np.random.default_rng(3)
    vectors = rng.standard_normal((5, 12, 3)) + 1j * rng.standard_normal((5, 12, 3))
    coef = rng.standard_normal((4, 2, 3))
    got = lc.ritz_accumulate_reference(vectors, coef)
    assert got.shape == (2, 3, 12)
    assert np.allclose(got.astype(np.complex128), np.einsum("jlc,jnc->lcn", coef, vectors[:4]), rtol=1e-14, atol=1e-14)


# ------------------------------------------------------------------ front end on the numpy solver
def _patched(monkeypatch, name):
    system = lc.SYSTEMS[name]()
    solver = lc.NumpyLanczosSolver.from_hamiltonian(system)
    monkeypatch.setattr(system, "_solver", lambda *args, **kwargs: solver, raising=True)
    return system


def _two_pass(monkeypatch, name, vectors):
    """What the public two-pass logic hands to the second pass, on a system whose solver records it."""
    system = lc.SYSTEMS[name]()
    solver = lc.RecordingSolver.from_hamiltonian(system)
    monkeypatch.setattr(system, "_solver", lambda *args, **kwargs: solver, raising=True)
    return lc.two_pass(system, solver, vectors)


@pytest.mark.parametrize("name", ["square12", "plane10x12_flux", "swave20"])
def test_lowest_eigenvalues_front_end_on_the_numpy_solver(monkeypatch, recwarn, name):
    """(check_every=25: on matrices of a few hundred rows the window in which two successive checks agree, after the
    levels have converged and before plain Lanczos grows the first ghost copy, is some tens of iterations wide; the
    function is meant for matrices beyond dense reach, where it is thousands.  max_iter bounds a failure's run time.)"""
    system = _patched(monkeypatch, name)
    levels = lc.levels_of(name, 3)
    got = system.lowest_eigenvalues(3, tol=1e-9, check_every=25, max_iter=2000, method="lanczos")
    assert not [w for w in recwarn.list if issubclass(w.category, RuntimeWarning)]
    assert got.shape == (3,)
    assert np.allclose(got, [value for value, _, _ in levels], rtol=1e-8, atol=0)  # (tol = 1e-9 was asked for)


@pytest.mark.parametrize("rayleigh_ritz", ["device", "host"])
@pytest.mark.parametrize("name", ["square12", "plane10x12_flux", "swave20"])
def test_lowest_eigenpairs_front_end_on_the_numpy_solver(monkeypatch, recwarn, name, rayleigh_ritz):
    """Values with multiplicities, residual, orthonormality and both layouts, against numpy.linalg.eigh."""
    system = _patched(monkeypatch, name)
    matrix = lc.sparse_matrix(name)
    values = lc.dense_eigh(name)[0]
    k = 6
    expected = values[values > 0][:k]
    vals, raw = system.lowest_eigenpairs(k, format="raw", method="lanczos", rayleigh_ritz=rayleigh_ritz, max_iter=3000)
    assert not [w for w in recwarn.list if issubclass(w.category, RuntimeWarning)]
    assert vals.shape == (k,) and raw.shape == (matrix.shape[0], k)
    assert np.abs(vals - expected).max() <= 1e-10
    assert np.linalg.norm(matrix @ raw - raw * vals, axis=0).max() <= 1e-8
    assert np.abs(raw.conj().T @ raw - np.eye(k)).max() <= 1e-8
    vals2, shaped = system.lowest_eigenpairs(k, method="lanczos", rayleigh_ritz=rayleigh_ritz, max_iter=3000)
    assert shaped.shape == (k, matrix.shape[0] // 4, 4)
    assert np.array_equal(vals2, vals) and np.array_equal(shaped.reshape(k, -1).T, raw)


# ------------------------------------------------------------------ Rayleigh-Ritz reference
@pytest.mark.parametrize("vectors", [1, 2, 3, 4, 8, 16])
@pytest.mark.parametrize("name", ["square12", "plane10x12_flux"])
def test_ritz_pairs_reference_against_dense_eigenprojectors(monkeypatch, name, vectors):
    """Per level min(multiplicity, start vectors) states, and every one of them inside the level's dense eigenspace."""
    levels = lc.levels_of(name, 3)
    coef, eps, begin = _two_pass(monkeypatch, name, vectors)
    solver = lc.NumpyLanczosSolver(lc.sparse_matrix(name))
    solver.lanczos_begin(**begin)
    block = solver.lanczos_ritz_vectors(coef)
    values, states, found = lc.ritz_pairs_reference(lc.sparse_matrix(name), block, eps)
    assert list(found) == [min(multiplicity, vectors) for _, multiplicity, _ in levels]
    assert lc.states_per_level(values, levels) == list(found)
    projector = sum(p for _, _, p in levels)
    defect = np.abs(states.T - projector @ states.T).max()
    print(f"{name} {vectors} vectors: found {list(found)}, outside the dense eigenspaces {defect:.1e}")
    assert defect <= 1e-10
    ritz_projector = states.T @ states.conj()
    assert np.abs(ritz_projector @ projector - ritz_projector).max() <= 1e-10
    if vectors >= max(m for _, m, _ in levels):  # every level complete: the two projectors are the same matrix
        assert np.abs(ritz_projector - projector).max() <= 1e-10


def test_rank_tolerance_decides_how_many_states_a_level_keeps(monkeypatch):
    """The unit-diagonal Gram matrix of eight candidates in a four-fold level has four weights of order one: a cut
    at half the largest keeps fewer of them than the default 1e-4 does."""
    levels = lc.levels_of("square12", 3)
    coef, eps, begin = _two_pass(monkeypatch, "square12", 8)
    solver = lc.NumpyLanczosSolver(lc.sparse_matrix("square12"))
    solver.lanczos_begin(**begin)
    block = solver.lanczos_ritz_vectors(coef)
    loose = lc.ritz_pairs_reference(lc.sparse_matrix("square12"), block, eps, 1e-4)[2]
    tight = lc.ritz_pairs_reference(lc.sparse_matrix("square12"), block, eps, 0.5)[2]
    assert list(loose) == [m for _, m, _ in levels]
    assert all(1 <= t <= l for t, l in zip(tight, loose)) and tight[1] < loose[1]


def test_numpy_solver_refuses_what_the_library_refuses():
    solver = lc.NumpyLanczosSolver(lc.sparse_matrix("chain101"))
    for bad in (dict(n_vectors=0), dict(n_vectors=65), dict(n_vectors=2, max_iter=0), dict(n_vectors=2, kind=7)):
        with pytest.raises(ValueError):
            solver.lanczos_begin(**bad)
    with pytest.raises(ValueError):
        solver.lanczos_advance(1)
    solver.lanczos_begin(2, max_iter=8)
    with pytest.raises(ValueError):
        solver.lanczos_advance(9)
    with pytest.raises(ValueError):
        solver.lanczos_advance(0)
    first = solver.lanczos_advance(3)
    with pytest.raises(ValueError):
        solver.lanczos_ritz_vectors(np.ones((2, 1, 2)))  # the process has advanced
    solver.lanczos_begin(2, max_iter=8)
    with pytest.raises(ValueError):
        solver.lanczos_ritz_vectors(np.ones((9, 1, 2)))
    again = solver.lanczos_advance(3)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
