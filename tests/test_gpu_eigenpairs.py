"""eigenpairs() on the GPU: the bdg_subspace_* kernels through the ABI against numpy, the device filter against
apply() bit for bit, the whole iteration against dense eigh and the numpy restatement on the four systems, in every
arithmetic and kernel form, and the cases around it (empty window, a block that grows, too many states, a block ended
by a dense solve, the dense route)."""

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import backend
from bodge_amd import eigenpairs as ep

import eigenpairs_cases as cases
import lanczos_cases

pytestmark = pytest.mark.gpu

CLD = np.clongdouble


# ------------------------------------------------------------------ kernels through the ABI
@pytest.fixture(scope="module")
def kernel_systems():
    """nb = 1, 37, 1100: K = 4 nb = 4, 148 and 4400 (more than one 4096-entry slice of the Gram product)."""
    built = {}
    for nb, shape in ((1, (1, 1, 1)), (37, (37, 1, 1)), (1100, (44, 25, 1))):
        system = cases.swave_with_moments(shape, min(3, nb), ba.σ2, seed=1)
        h = system.matrix("csr")
        built[nb] = (system, h, lanczos_cases.SparseLongDouble(h))
    return built


def _tolerance(float64_value, long_double_value):
    """20 x the deviation of the numpy float64 evaluation from the long-double one, and no less
    than two spacings of the largest entry: a float64 sum that happens to round like the long-double one (K = 4)
    does not make the device's differently ordered sum wrong."""
    reference = np.asarray(long_double_value)
    deviation = float(np.abs(np.asarray(float64_value) - reference).max())
    return max(20 * deviation, 2 * float(np.spacing(float(np.abs(reference).max()))))


@pytest.mark.parametrize("nb", [1, 37, 1100])
@pytest.mark.parametrize("columns", [1, 5, 17, 65])
def test_project_rotate_and_residuals_match_numpy(kernel_systems, nb, columns):
    """S, G, X Q and the residuals against long-double numpy.  HX Q is not readable through the ABI: it is checked
    through the residuals, with a random θ and - a second rotation that only selects the live columns - with θ = 0,
    where the residual is |HX Q| itself."""
    system, h, h_long = kernel_systems[nb]
    solver = system._solver()
    dim = 4 * nb
    rng = np.random.default_rng(100 * nb + columns)
    x = rng.standard_normal((columns, dim)) + 1j * rng.standard_normal((columns, dim))
    solver.subspace_begin(columns, seed=3)
    try:
        assert np.array_equal(solver.subspace_read(0, columns), cases.start_block(dim, 3, 0, columns))
        solver.subspace_write(0, x)
        assert np.array_equal(solver.subspace_read(0, columns), x)
        s, g = solver.subspace_project()
        hx = (h @ x.T).T
        x_long, hx_long = x.astype(CLD), (h_long @ x.T.astype(CLD)).T
        for name, got, f64, ld in (("S", s, x.conj() @ x.T, x_long.conj() @ x_long.T),
                                   ("G", g, x.conj() @ hx.T, x_long.conj() @ hx_long.T)):
            tolerance = _tolerance(f64, ld)
            print(nb, columns, name, float(np.abs(got - ld).max()), tolerance)
            assert np.abs(got - ld).max() <= tolerance, name
        again = solver.subspace_project()
        assert np.array_equal(again[0], s) and np.array_equal(again[1], g)  # no atomics: the same bits

        n_out = max(1, columns - 2)
        q = rng.standard_normal((columns, n_out)) + 1j * rng.standard_normal((columns, n_out))
        theta = rng.standard_normal(n_out)
        residual = solver.subspace_rotate(q, theta)
        rotated = solver.subspace_read(0, n_out)
        q_long = q.astype(CLD)
        xq_long, hxq_long = q_long.T @ x_long, q_long.T @ hx_long
        tolerance = _tolerance(q.T @ x, xq_long)
        print(nb, columns, "XQ", float(np.abs(rotated - xq_long).max()), tolerance)
        assert np.abs(rotated - xq_long).max() <= tolerance
        expected = np.sqrt((np.abs(hxq_long - theta[:, None] * xq_long) ** 2).sum(axis=1))
        f64 = np.linalg.norm(q.T @ hx - theta[:, None] * (q.T @ x), axis=1)
        tolerance = _tolerance(f64, expected)
        print(nb, columns, "residual", float(np.abs(residual - expected).max()), tolerance)
        assert np.abs(residual - expected).max() <= tolerance

        select = np.eye(columns, n_out, dtype=np.complex128)
        norms = solver.subspace_rotate(select, np.zeros(n_out))
        expected = np.sqrt((np.abs(hxq_long) ** 2).sum(axis=1))
        tolerance = _tolerance(np.linalg.norm(q.T @ hx, axis=1), expected)
        print(nb, columns, "|HXQ|", float(np.abs(norms - expected).max()), tolerance)
        assert np.abs(norms - expected).max() <= tolerance
        assert np.array_equal(solver.subspace_read(0, n_out), rotated)  # a selection moves the entries as they are

        if columns > 1:
            solver.subspace_refill(1, columns - 1, seed=9, first_id=40)
            assert np.array_equal(solver.subspace_read(1, columns - 1), cases.start_block(dim, 9, 40, columns - 1))
            assert np.array_equal(solver.subspace_read(0, 1), rotated[:1])
        with pytest.raises(ValueError, match="not within the block"):  # (the library's own refusal)
            backend.check(solver._lib.bdg_subspace_read(solver._handle, columns, 1, backend.as_f64p(np.zeros(2 * dim))))
    finally:
        solver.subspace_end()


# ------------------------------------------------------------------ the filter against apply()
@pytest.mark.parametrize("name", ["ysr_real", "ysr_complex"])
def test_filter_equals_apply_bit_for_bit(name):
    """The same kernels, batches and coefficients: 20 columns in one batch of 32 lanes, and - with four lanes per
    row - in five batches, give the bits of apply() in one batch.  bdg_perf_query reports the filter like an apply."""
    c = cases.case(name)
    solver = c.system._solver()
    coef = ep.window_coefficients(c.scale, c.lo, c.hi, 64)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((20, c.dense.shape[0])) + 1j * rng.standard_normal((20, c.dense.shape[0]))
    expected = c.system.apply(None, x.T, coefficients=coef, scale=c.scale).T
    apply_perf = solver.perf()
    try:
        for lanes, batches in ((0, 1), (4, 5)):
            solver.set_lanes_per_row(lanes)
            solver.subspace_begin(20)
            solver.subspace_write(0, x)
            solver.subspace_filter(c.scale, coef)
            perf = solver.perf()
            assert np.array_equal(solver.subspace_read(0, 20), expected), lanes
            assert perf["apply"] == apply_perf["apply"] and perf["launches"] == 64 * batches
            assert perf["vector_steps"] == 64 * 20 and perf["lanes_per_row"] == (lanes or 32)
            s, _ = solver.subspace_project()
            assert solver.perf()["launches"] == 64 * batches  # (the projection leaves the filter's figures)
            assert np.abs(s - expected.conj() @ expected.T).max() <= 1e-10 * np.abs(s).max()
    finally:
        solver.set_lanes_per_row(0)
        solver.subspace_end()
    after = c.system.apply(None, x.T, coefficients=coef, scale=c.scale).T
    assert np.array_equal(after, expected)  # bdg_apply_series itself: the same bits as before


# ------------------------------------------------------------------ the whole iteration
def _check_against_eigh(c, energies, vectors, restated):
    assert energies.shape == (c.count,) and vectors.shape == (c.count, c.dense.shape[0])
    assert np.all(np.diff(energies) >= 0)
    deviation = float(np.abs(energies - c.energies).max())
    residual = float(np.linalg.norm(c.h @ vectors.T - vectors.T * energies, axis=0).max())
    orthonormality = cases.orthonormality(vectors)
    agreement = cases.subspace_deviation(c, vectors)
    own_orthonormality = cases.orthonormality(restated[1])
    own_agreement = cases.subspace_deviation(c, restated[1])
    print(c.name, "dE", deviation, "residual / a", residual / c.scale, "orthonormality", orthonormality,
          own_orthonormality, "subspace", agreement, own_agreement)
    assert deviation <= cases.TOL * c.scale and residual <= cases.TOL * c.scale
    assert orthonormality <= 20 * own_orthonormality and agreement <= 20 * own_agreement


@pytest.mark.parametrize("name", sorted(cases.SYSTEMS))
def test_eigenpairs_match_dense_eigh_and_the_restatement(name):
    c = cases.case(name)
    restated = cases.restated(name)
    energies, states = c.system.eigenpairs((c.lo, c.hi), method="subspace", moments=cases.MOMENTS, tol=cases.TOL,
                                           max_states=c.count, format="raw")
    report = c.system._solver().last_eigenpairs
    assert states.shape == (c.dense.shape[0], c.count)
    _check_against_eigh(c, energies, np.ascontiguousarray(states.T), restated)
    # the start block is the same bits, so the iterations agree unless rounding moves a residual across tol
    print(name, "iterations", report["iterations"], "restatement", restated[2],
          "" if report["iterations"] == restated[2] else "(differs: a residual crossed tol in another iteration)")
    assert report["converged"] and report["columns"] == restated[4] and abs(report["iterations"] - restated[2]) <= 1
    reshaped = c.system.eigenpairs((c.lo, c.hi), method="subspace", moments=cases.MOMENTS, max_states=c.count)
    assert reshaped[1].shape == (c.count, c.dense.shape[0] // 4, 4)
    assert np.array_equal(reshaped[0], energies) and np.array_equal(reshaped[1].reshape(c.count, -1), states.T)


@pytest.mark.parametrize("switch", ["BODGE_AMD_REAL", "BODGE_AMD_PH", "BODGE_AMD_DICT"])
def test_every_arithmetic_and_form_finds_the_same_states(switch, knobs):
    c = cases.case("ysr_real")
    knobs.set(switch, "0")
    energies, vectors = c.system.eigenpairs((c.lo, c.hi), method="subspace", moments=cases.MOMENTS, max_states=c.count)
    perf = c.system._solver().perf()
    assert perf["real_arithmetic"] == (0 if switch == "BODGE_AMD_REAL" else 1)
    if switch == "BODGE_AMD_PH":
        assert perf["ph_packed"] == 0
    if switch == "BODGE_AMD_DICT":
        assert perf["apply"] == 1 and perf["dict_blocks"] == 0
    _check_against_eigh(c, energies, vectors.reshape(c.count, -1), cases.restated("ysr_real"))


def test_the_count_is_estimated_when_it_is_not_given():
    c = cases.case("cube")
    energies, vectors = c.system.eigenpairs((c.lo, c.hi), method="subspace")
    report = c.system._solver().last_eigenpairs
    print("cube", report)
    assert report["moments"] == ep.default_moments(c.scale, c.lo, c.hi) and report["converged"]
    assert 8 <= report["columns"] <= ep.MAX_COLUMNS
    assert len(energies) == c.count and np.abs(energies - c.energies).max() <= cases.TOL * c.scale
    assert cases.orthonormality(vectors.reshape(c.count, -1)) <= 1e-12


# ------------------------------------------------------------------ the cases around it
def test_an_empty_window_returns_empty_arrays():
    c = cases.case("cube")
    lo, hi = 0.19, 0.26
    assert not ((c.levels >= lo) & (c.levels <= hi)).any() and np.abs(c.levels - lo).min() > 0.01
    for method in ("subspace", "auto"):
        energies, vectors = c.system.eigenpairs((lo, hi), method=method, max_states=2)
        assert energies.shape == (0,) and vectors.shape == (0, c.dense.shape[0] // 4, 4)
        energies, raw = c.system.eigenpairs((lo, hi), method=method, max_states=2, format="raw")
        assert energies.shape == (0,) and raw.shape == (c.dense.shape[0], 0)


def test_a_block_that_is_too_small_grows_once():
    """max_states = 4 gives 13 columns for 22 states: no guard column is left, the block doubles to 26 and the call
    still returns all 22 (the restatement: 23 iterations at M = 512; at M = 256 four guard columns are too few for
    40 iterations)."""
    c = cases.case("ysr_real")
    energies, vectors = c.system.eigenpairs((c.lo, c.hi), method="subspace", moments=512, max_states=4)
    report = c.system._solver().last_eigenpairs
    print("grown", report)
    assert report["columns"] == 26 and report["converged"]
    assert len(energies) == c.count == 22 and np.abs(energies - c.energies).max() <= cases.TOL * c.scale
    assert cases.orthonormality(vectors.reshape(22, -1)) <= 1e-12


def test_a_window_over_the_whole_band_names_the_limit():
    """All 240 levels of the 5x4x3 lattice lie inside: no guard column is ever left, the block doubles until it would
    pass 512 columns.  With the count estimated (240: 308 columns) and with a bound that is too small (133 columns)."""
    c = cases.case("cube")
    solver = c.system._solver()
    for options in ({}, {"max_states": 100}):
        with pytest.raises(ValueError, match="512 columns"):
            c.system.eigenpairs((-c.scale, c.scale), method="subspace", moments=128, **options)
        # (the block has been given back, and the handle is usable)
        with pytest.raises(ValueError, match="no subspace block"):
            backend.check(solver._lib.bdg_subspace_refill(solver._handle, 0, 1, 0, 0))
    assert len(c.system.eigenpairs((c.lo, c.hi), method="subspace", max_states=c.count)[0]) == c.count


@pytest.mark.parametrize("ender", ["dense", "lanczos"])
def test_a_dense_solve_or_a_lanczos_run_ends_the_block(ender):
    c = cases.case("cube")
    solver = c.system._solver()
    coef = ep.window_coefficients(c.scale, c.lo, c.hi, 16)
    solver.subspace_begin(6)
    if ender == "dense":
        levels, _ = solver.eigh(vectors=False)
        assert np.abs(levels - c.levels).max() < 1e-10
    else:
        solver.lanczos_begin(2)
    for call in (lambda: solver.subspace_filter(c.scale, coef), lambda: solver.subspace_project(),
                 lambda: solver.subspace_rotate(np.eye(6), np.zeros(6)), lambda: solver.subspace_refill(0, 1),
                 lambda: solver.subspace_read(0, 1), lambda: solver.subspace_write(0, np.zeros((1, solver.dim)))):
        with pytest.raises(ValueError, match="no subspace block"):
            call()
    solver.subspace_end()  # (no error without a block)
    solver.subspace_begin(6)
    solver.subspace_filter(c.scale, coef)
    assert np.isfinite(solver.subspace_project()[0]).all()
    solver.subspace_end()


def test_slabs_are_refused():
    from bodge_amd.solver import SlabGroup

    c = cases.case("cube")
    with SlabGroup.from_hamiltonian(c.system, 2) as group:
        with pytest.raises(ValueError, match="slab"):
            group.members[0].subspace_begin(4)


def test_auto_is_diagonalize_cut_to_the_window():
    c = cases.case("cube")
    everything, states = c.system.diagonalize(format="raw")
    keep = (everything >= c.lo) & (everything <= c.hi)
    energies, raw = c.system.eigenpairs((c.lo, c.hi), format="raw")  # 4N = 240: the dense route
    assert np.array_equal(energies, everything[keep]) and raw.shape == (240, c.count)
    projector = lambda v: v @ v.conj().T
    assert np.abs(projector(raw) - projector(states[:, keep])).max() < 1e-10
    reshaped = c.system.eigenpairs((c.lo, c.hi))
    assert np.array_equal(reshaped[1].reshape(c.count, -1), raw.T)
    # a window on the negative side: nothing is folded
    energies, raw = c.system.eigenpairs((-c.hi, 0.0), format="raw")
    assert np.allclose(energies, -c.energies[::-1], rtol=0, atol=1e-10)
    assert np.abs(c.dense @ raw - raw * energies).max() < 1e-9
    subspace = c.system.eigenpairs((-c.hi, 0.0), format="raw", method="subspace", max_states=c.count)
    assert np.abs(subspace[0] - energies).max() <= cases.TOL * c.scale
    assert np.abs(projector(subspace[1]) - projector(raw)).max() < 1e-6
