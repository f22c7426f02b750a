"""The kernels only the Lanczos process runs, against the references of tests/lanczos_cases.py: K1 with per-column
scalars in every arithmetic mode, kernel form and lane count, the Lanczos helpers (lanczos_combine, column_norms,
lanczos_scalars, lanczos_accumulate, sitemajor_from_planar(_real)) and the block algebra of the device Rayleigh-Ritz
step (block_gram, block_mix, small_hermitian_eigh, combinations).

Tolerances.  Trajectories (α, β over 16 iterations) and everything else "at the bound of (a)": 20 times the distance
between the float64 and the long-double restatement of the same system (lanczos_cases.reference_distance, computed
here from the references alone; tests/test_lanczos_host.py pins it).  Local relations over 64 iterations: 20 times the
figure of the float64 restatement's own vectors.  Accumulation: a derived element-wise bound.  Rayleigh-Ritz: 20 times
what ritz_pairs_reference reaches on the same block.  Bit-level contracts carry none.  Every test prints its figures
before it asserts; DESIGN.md ("Lanczos tests") records them.
"""

import contextlib
import warnings

import numpy as np
import pytest

import lanczos_cases as lc
from oracle import cheb_ref

pytestmark = pytest.mark.gpu

RAD, Z4 = cheb_ref.VEC_RADEMACHER, cheb_ref.VEC_Z4
FACTOR = 20  # this suite's convention (fermi_cases / apply_cases): summation order and FMAs of the device
U = 2.0 ** -53
# arithmetic -> knobs; with Rademacher vectors on a real matrix: RealPH, Real, ComplexPH, Complex
ARITHMETIC = {
    "packed": {},
    "full": {"BODGE_AMD_PH": "0"},
    "complex_packed": {"BODGE_AMD_REAL": "0"},
    "complex_full": {"BODGE_AMD_REAL": "0", "BODGE_AMD_PH": "0"},
}
IS_REAL = {name: name not in ("plane9x13_flux", "plane10x12_flux", "random357") for name in lc.SYSTEMS}
IS_PH = {name: True for name in lc.SYSTEMS}  # (random357 too: every block of a Hamiltonian has the Nambu form)


@pytest.fixture(scope="module")
def solver_cls(hip_library):
    from bodge_amd.solver import DeviceSolver

    return DeviceSolver


def _lanes(real, n_vectors):
    per_payload = 2 if real else 1
    need, lanes = (n_vectors + per_payload - 1) // per_payload, 4
    while lanes < need:
        lanes *= 2
    return lanes


def _expected_form(name, n_vectors, kind, arithmetic, dictionary_off):
    real = IS_REAL[name] and kind == RAD and "complex" not in arithmetic
    packed = IS_PH[name] and "full" not in arithmetic
    lanes = _lanes(real, n_vectors)
    # the dictionary form with per-column scalars exists for 4 lanes per row; disorder17x16 streams its 272 diagonal blocks
    dictionary = lanes == 4 and not dictionary_off and name not in ("disorder17x16", "random357")
    return dict(real_arithmetic=int(real), ph_packed=int(packed), lanes_per_row=lanes, dictionary=dictionary)


def _assert_form(perf, expected, launches):
    print("perf:", {key: perf[key] for key in ("lanes_per_row", "vectors_per_launch", "real_arithmetic", "ph_packed",
                                                 "dict_blocks", "grid", "lds_bytes", "launches")})
    assert perf["lanes_per_row"] == expected["lanes_per_row"]
    assert perf["vectors_per_launch"] == expected["lanes_per_row"] * (2 if expected["real_arithmetic"] else 1)
    assert perf["real_arithmetic"] == expected["real_arithmetic"] and perf["ph_packed"] == expected["ph_packed"]
    assert (perf["dict_blocks"] > 0) == expected["dictionary"]
    assert perf["pipelined"] == 0 and perf["steps_per_launch"] == 1 and perf["grid"] > 0 and perf["lds_bytes"] > 0
    assert perf["launches"] == launches


def _tolerance(name, like=None):
    """Absolute bound on α and β: FACTOR x (float64 against long double), as a fraction of ‖H‖²."""
    return FACTOR * lc.reference_distance(like or name) * lc.norm_bound(name) ** 2


# ------------------------------------------------------------------ a. every instantiation
def _instantiations():
    cases = []
    # every (mode, form) pair at 4 lanes per row: the dictionary form for rows of <= 3, 5, 7 blocks, the generic form
    # through the knob, on streamed on-site blocks and on a matrix that is no stencil.  3 real vectors: one payload
    # with a live and a dead column, one dead payload; 1 and 4 complex vectors: three dead payloads, none.
    for arithmetic in ARITHMETIC:
        count = 4 if "complex" in arithmetic else 3
        for name in ("chain101", "plane9x13", "cube5x6x7"):
            cases.append((name, count, RAD, arithmetic, False))
        cases.append(("plane9x13", count, RAD, arithmetic, True))
        cases.append(("disorder17x16", count, RAD, arithmetic, False))
    cases += [("random357", 1, Z4, "packed", False), ("random357", 4, Z4, "full", False),
              ("random357", 4, RAD, "packed", True), ("plane9x13_flux", 3, RAD, "packed", False),
              ("plane9x13_flux", 4, Z4, "full", False), ("plane9x13_flux", 1, Z4, "packed", True)]
    # every lane count in real and in complex arithmetic, both ends of each range (odd counts: zero-padded columns)
    for count in (1, 8, 9, 16, 17, 32, 33, 64):
        cases.append(("plane9x13", count, RAD, "packed", False))
    for count in (1, 5, 8, 16, 32, 33, 64):
        cases.append(("plane9x13", count, Z4, "packed", False))
    cases += [("cube5x6x7", 16, RAD, "full", False), ("cube5x6x7", 16, Z4, "full", False),
              ("chain101", 9, RAD, "complex_full", False), ("disorder17x16", 13, RAD, "packed", False),
              ("disorder17x16", 7, Z4, "packed", False), ("random357", 11, Z4, "packed", False),
              ("plane9x13_flux", 21, RAD, "packed", False)]
    return cases


@pytest.mark.parametrize("name,n_vectors,kind,arithmetic,dictionary_off", _instantiations())
def test_tridiagonal_entries_in_every_kernel_form(solver_cls, knobs, name, n_vectors, kind, arithmetic, dictionary_off):
    """α_j, β_{j+1} (j < 16) of every column against the long-double process; perf() says which kernel ran."""
    knobs.update(ARITHMETIC[arithmetic])
    if dictionary_off:
        knobs.set("BODGE_AMD_DICT", "0")
    expected = _expected_form(name, n_vectors, kind, arithmetic, dictionary_off)
    ref_alpha, ref_beta = lc.long_double_run(name, n_vectors, 3, kind)
    with solver_cls.from_hamiltonian(lc.build(name)) as dev:
        dev.lanczos_begin(n_vectors, seed=3, kind=kind, max_iter=lc.HORIZON)
        assert dev.perf()["launches"] == 0
        alpha, beta = dev.lanczos_advance(lc.HORIZON)
        perf = dev.perf()
    distance = lc.trajectory_distance(name, alpha, beta, ref_alpha, ref_beta)
    print(f"{name} {n_vectors} vectors kind {kind} {arithmetic} dict_off={dictionary_off}: device {distance:.2e}, "
          f"references {lc.reference_distance(name):.2e} of |H|^2")
    _assert_form(perf, expected, 2 * lc.HORIZON)
    assert alpha.shape == beta.shape == (lc.HORIZON, n_vectors)
    assert np.abs(alpha - ref_alpha).max() <= _tolerance(name) and np.abs(beta - ref_beta).max() <= _tolerance(name)


def test_every_mode_form_and_lane_count_is_among_the_cases():
    seen = {(e["real_arithmetic"], e["ph_packed"], e["dictionary"], e["lanes_per_row"])
            for e in (_expected_form(*case) for case in _instantiations())}
    for real in (0, 1):
        for packed in (0, 1):
            assert (real, packed, True, 4) in seen and (real, packed, False, 4) in seen
        for lanes in ((4, 8, 16, 32) if real else (4, 8, 16, 32, 64)):
            assert any(s[0] == real and not s[2] and s[3] == lanes for s in seen), (real, lanes)


# ------------------------------------------------------------------ b. the device's own Lanczos vectors
VECTOR_CASES = {"plane9x13": (8, RAD), "plane9x13_flux": (4, Z4), "cube5x6x7": (3, RAD), "disorder17x16": (8, RAD)}
_device_runs = {}


def _device_vectors(solver_cls, name):
    """v_0 .. v_63 of every column, (64, 4N, C), as lanczos_ritz_vectors returns them for coef[j, l, c] = δ_jl, and
    α, β of a first pass on a second handle.  Default knobs; computed once per session."""
    if name not in _device_runs:
        n_vectors, kind = VECTOR_CASES[name]
        m = lc.LOCAL_HORIZON
        coef = np.zeros((m, m, n_vectors))
        coef[np.arange(m), np.arange(m), :] = 1.0
        with solver_cls.from_hamiltonian(lc.build(name)) as first, solver_cls.from_hamiltonian(lc.build(name)) as second:
            first.lanczos_begin(n_vectors, seed=1, kind=kind, max_iter=m)
            alpha, beta = first.lanczos_advance(m)
            second.lanczos_begin(n_vectors, seed=1, kind=kind, max_iter=m)
            vectors = second.lanczos_ritz_vectors(coef)                    # (levels = j, C, 4N)
        _device_runs[name] = (alpha, beta, np.ascontiguousarray(np.moveaxis(vectors, 1, 2)))
    return _device_runs[name]


@pytest.mark.parametrize("name", sorted(VECTOR_CASES))
def test_lanczos_vectors_obey_the_local_relations(solver_cls, name):
    """‖v_j‖ = 1, α_j = ‖H v_j‖², the three-term residual and the neighbour overlaps of the device's vectors over 64
    iterations, in long double, each held to 20 times the figure of the float64 restatement's own vectors; v_0 is the
    oracle's start vector over its norm to 2 ulp (layout and column order)."""
    n_vectors, kind = VECTOR_CASES[name]
    alpha, beta, vectors = _device_vectors(solver_cls, name)
    assert vectors.shape == (lc.LOCAL_HORIZON, 4 * lc.build(name).lattice.size, n_vectors)
    start = lc.start_block(name, n_vectors, 1, kind)
    start = start / np.sqrt(start.shape[0])
    ulps = np.abs(vectors[0] - start).max() / np.spacing(np.abs(start).max())
    m = lc.LOCAL_HORIZON - 1
    device = lc.local_figures(name, alpha[:m], beta[:m], vectors)
    reference = lc.reference_local_figures(name, n_vectors, 1, kind, m)
    print(f"{name}: v_0 off by {ulps:.2f} ulp; device {device}; restatement {reference}")
    assert ulps <= 2.0
    if kind == RAD and IS_REAL[name]:
        assert not vectors.imag.any()  # (sitemajor_from_planar_real)
    for key, value in device.items():
        assert value <= FACTOR * reference[key], (key, value, reference[key])


# ------------------------------------------------------------------ c. Ritz accumulation
def _planted_coefficients(n_iter, levels, n_vectors, real):
    rng = np.random.default_rng(100 * n_iter + levels)
    coef = rng.standard_normal((n_iter, levels, n_vectors))
    if levels >= 3:
        coef[:, 1, :] = 0.0                    # a whole level
    if real:
        coef[:, :, 4:6] = 0.0                  # both columns of payload 2 in every level: the f0 == 0 && f1 == 0 skip
        coef[:, :, 2] = 0.0                    # column 2r zero, column 2r + 1 not
        dead = [2, 4, 5]
    else:
        coef[:, :, 2] = 0.0                    # the column of payload 2 in every level
        dead = [2]
    if n_iter > 1:
        coef[n_iter // 2, 0, 0] = 0.0          # a single zero in a live column
    return coef, dead


@pytest.mark.parametrize("n_iter", [1, 7, 40])
@pytest.mark.parametrize("levels", [1, 3, 64])
@pytest.mark.parametrize("name", ["plane9x13", "plane9x13_flux"])
def test_ritz_accumulation_element_by_element(solver_cls, name, levels, n_iter):
    """y[l, c] = Σ_j coef[j, l, c] v_j^(c) on the device's own vectors (b).  The device adds fl(coef/β_j)·(β_j v_j) with
    one FMA per term, the vectors of (b) are fl((1/β_j)·(β_j v_j)): two roundings per term apart, then n_iter sums,
    hence |error| <= 2 (n_iter + 1) 2^-53 Σ_j |coef_j| |v_j| element by element.  Zero columns stay exact zeros."""
    n_vectors, kind = VECTOR_CASES[name]
    _, _, vectors = _device_vectors(solver_cls, name)
    coef, dead = _planted_coefficients(n_iter, levels, n_vectors, kind == RAD)
    with solver_cls.from_hamiltonian(lc.build(name)) as dev:
        dev.lanczos_begin(n_vectors, seed=1, kind=kind, max_iter=lc.LOCAL_HORIZON)
        got = dev.lanczos_ritz_vectors(coef)
    assert got.shape == (levels, n_vectors, vectors.shape[1])
    reference = lc.ritz_accumulate_reference(vectors, coef)
    bound = 2 * (n_iter + 1) * U * lc.ritz_accumulate_reference(np.abs(vectors), np.abs(coef)).real
    excess = np.abs(got - reference) - bound
    print(f"{name} levels {levels} n_iter {n_iter}: largest error {np.abs(got - reference).max():.2e}, "
          f"largest error / bound {np.max(np.abs(got - reference)[bound > 0] / bound[bound > 0]):.3f}")
    assert np.all(excess <= 0)
    assert not got[:, dead, :].any()
    if levels >= 3:
        assert not got[1].any()
    live = [c for c in range(n_vectors) if c not in dead]
    assert np.all(np.abs(got[0][live]).max(axis=1) > 0)


# ------------------------------------------------------------------ d. bit-level contracts
@pytest.mark.parametrize("name,n_vectors,kind", [("plane9x13", 8, RAD), ("plane9x13_flux", 4, Z4), ("cube5x6x7", 3, RAD)])
def test_runs_repeat_and_split_bit_for_bit(solver_cls, name, n_vectors, kind):
    begin = dict(n_vectors=n_vectors, seed=4, kind=kind, max_iter=lc.HORIZON)
    with solver_cls.from_hamiltonian(lc.build(name)) as dev:
        dev.lanczos_begin(**begin)
        whole = dev.lanczos_advance(16)
        dev.lanczos_begin(**begin)
        again = dev.lanczos_advance(16)
        dev.lanczos_begin(**begin)
        pieces = [dev.lanczos_advance(n) for n in (5, 7, 4)]
        dev.lanczos_begin(**begin)
        rng = np.random.default_rng(8)
        dev.lanczos_ritz_vectors(rng.standard_normal((10, 2, n_vectors)))
        tail = dev.lanczos_advance(6)
    for i in (0, 1):
        assert np.array_equal(whole[i], again[i])
        assert np.array_equal(whole[i], np.vstack([piece[i] for piece in pieces]))
        assert np.array_equal(whole[i][10:], tail[i])  # the second pass does not disturb the process


@pytest.mark.parametrize("name,kind", [("plane9x13", RAD), ("plane9x13_flux", Z4)])
def test_columns_are_independent(solver_cls, name, kind):
    """Column 3 of vectors 0 .. 7 against column 0 of vectors 3 .. 10: the same start vector in another payload
    (and, in real arithmetic, in the other half of one)."""
    with solver_cls.from_hamiltonian(lc.build(name)) as dev:
        dev.lanczos_begin(8, seed=4, first_id=0, kind=kind, max_iter=lc.HORIZON)
        one = dev.lanczos_advance(lc.HORIZON)
        dev.lanczos_begin(8, seed=4, first_id=3, kind=kind, max_iter=lc.HORIZON)
        other = dev.lanczos_advance(lc.HORIZON)
    distance = max(np.abs(one[i][:, 3] - other[i][:, 0]).max() for i in (0, 1))
    identical = all(np.array_equal(one[i][:, 3], other[i][:, 0]) for i in (0, 1))
    print(f"{name}: column 3 of (8, first_id 0) against column 0 of (8, first_id 3): {distance:.2e}, bit-identical: {identical}")
    assert distance <= _tolerance(name)
    assert not np.array_equal(one[0][:, 3], one[0][:, 0])  # (different start vectors do differ)


# ------------------------------------------------------------------ e. device Rayleigh-Ritz
def _library_refuses_advance(dev, n_vectors):
    """After a run has ended `DeviceSolver.lanczos_advance` refuses on the Python side already (its count of start
    vectors, `_lanczos_vectors`, is 0; solver.py names this use).  Putting the count back reaches the library's own
    refusal, as test_lanczos_run_is_ended_by_any_other_use_of_the_handle does."""
    with pytest.raises(ValueError):
        dev.lanczos_advance(1)
    dev._lanczos_vectors = n_vectors
    with pytest.raises(ValueError):
        dev.lanczos_advance(1)


@contextlib.contextmanager
def _two_pass_on_device(name, vectors, k=3):
    """`lowest_eigenpairs(k, vectors=vectors, method="lanczos")` at its default tol on the device, recording what the
    public logic hands to bdg_lanczos_ritz_pairs and ALL the states that call finds (the front end asks for k).
    Yields (system, its device handle, the record, the front end's result); the handle is closed on the way out."""
    system = lc.SYSTEMS[name]()
    dev = system._solver()
    try:
        seen = {}
        inner = dev.lanczos_ritz_pairs

        def recording(coef, eps, k_asked, rank_tol=1e-4):
            values, states, found = inner(coef, eps, 64, rank_tol)
            seen.update(coef=np.array(coef), eps=np.array(eps), values=values, states=states, found=found)
            return values[:k_asked], states[:k_asked], found

        dev.lanczos_ritz_pairs = recording
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("error")  # "only ... levels converged" is a failure of the case
                front = system.lowest_eigenpairs(k, vectors=vectors, max_iter=lc.TWO_PASS_MAX_ITER, method="lanczos",
                                                 format="raw")
        finally:
            del dev.lanczos_ritz_pairs
        yield system, dev, seen, front
    finally:
        dev.close()


def _orthonormality(states, values, levels):
    gram = states.conj() @ states.T
    overall = np.abs(gram - np.eye(len(states))).max()
    inside = 0.0
    for value, _, _ in levels:
        members = np.flatnonzero(np.abs(values - value) <= 1e-7)
        inside = max(inside, np.abs(gram[np.ix_(members, members)] - np.eye(len(members))).max())
    return overall, inside


def _rayleigh_defect(name, values, states):
    matrix = lc.sparse_long_double(name)
    v = np.asarray(states, dtype=lc.CLD).T
    quotient = np.sum(v.conj() * (matrix @ v), axis=0).real / np.sum(np.abs(v) ** 2, axis=0)
    return float(np.abs(quotient - values).max())


@pytest.mark.parametrize("vectors", [1, 2, 3, 4, 8, 16])
@pytest.mark.parametrize("name", ["square12", "plane10x12_flux"])
def test_device_rayleigh_ritz_against_reference_and_dense(solver_cls, name, vectors):
    levels = lc.levels_of(name, 3)
    matrix = lc.sparse_matrix(name)
    with _two_pass_on_device(name, vectors) as (system, dev, seen, front):
        coef, eps, values, states = seen["coef"], seen["eps"], seen["values"], seen["states"]
        # the same Ritz block on a second, identically begun handle, through the numpy steps
        with solver_cls.from_hamiltonian(system) as second:
            second.lanczos_begin(vectors, seed=0, max_iter=lc.TWO_PASS_MAX_ITER)
            block = second.lanczos_ritz_vectors(coef)
        ref_values, ref_states, ref_found = lc.ritz_pairs_reference(matrix, block, eps)
        expected = [min(multiplicity, vectors) for _, multiplicity, _ in levels]
        assert list(ref_found) == expected and seen["found"] == sum(expected) == len(values)
        assert lc.states_per_level(values, levels) == expected
        assert np.array_equal(front[0], values[:3]) and np.array_equal(front[1], states[:3].T)

        dense_values = np.concatenate([[value] * count for (value, _, _), count in zip(levels, expected)])
        projector = sum(p for _, _, p in levels)
        overall, inside = _orthonormality(states, values, levels)
        ref_overall, ref_inside = _orthonormality(ref_states, ref_values, levels)
        rayleigh, ref_rayleigh = _rayleigh_defect(name, values, states), _rayleigh_defect(name, ref_values, ref_states)
        ref_outside = np.abs(ref_states.T - projector @ ref_states.T).max()
        apart = np.abs(states.T @ states.conj() - ref_states.T @ ref_states.conj()).max()
        residual = np.linalg.norm(matrix @ states.T - states.T * values, axis=0).max()
        print(f"{name} {vectors} vectors, n_iter {coef.shape[0]}, found {expected}: orthonormality {overall:.1e} (reference "
              f"{ref_overall:.1e}), inside a level {inside:.1e} ({ref_inside:.1e}), Rayleigh quotient {rayleigh:.1e} "
              f"({ref_rayleigh:.1e}), values to dense {np.abs(values - dense_values).max():.1e}, projector to reference "
              f"{apart:.1e} (reference outside dense {ref_outside:.1e}), residual {residual:.1e}")
        assert overall <= FACTOR * ref_overall and inside <= FACTOR * ref_inside
        assert rayleigh <= FACTOR * ref_rayleigh
        assert np.abs(values - dense_values).max() <= 1e-10
        assert apart <= FACTOR * ref_outside
        assert residual <= 1e-8
        _library_refuses_advance(dev, vectors)  # after ritz_pairs the run is over


def test_rank_tolerance_output_limits_and_end_of_run(solver_cls):
    """rank_tol = 0.5 keeps fewer states of the four-fold level than 1e-4 (the counts the reference gives on the same
    block); max_out = 0 returns the count alone; asking for more than there is returns what there is."""
    name, vectors = "square12", 8
    with _two_pass_on_device(name, vectors) as (system, _, seen, _front):
        coef, eps = seen["coef"], seen["eps"]
    begin = dict(n_vectors=vectors, seed=0, max_iter=lc.TWO_PASS_MAX_ITER)
    with solver_cls.from_hamiltonian(system) as second:
        second.lanczos_begin(**begin)
        block = second.lanczos_ritz_vectors(coef)
        loose = lc.ritz_pairs_reference(lc.sparse_matrix(name), block, eps, 1e-4)
        tight = lc.ritz_pairs_reference(lc.sparse_matrix(name), block, eps, 0.5)
        assert tight[2].sum() < loose[2].sum() == 10
        second.lanczos_begin(**begin)
        values, states, found = second.lanczos_ritz_pairs(coef, eps, 64, rank_tol=0.5)
        assert found == tight[2].sum() == len(values) and np.abs(values - tight[0]).max() <= 1e-10
        second.lanczos_begin(**begin)
        values, states, found = second.lanczos_ritz_pairs(coef, eps, 0)
        assert found == 10 and values.shape == (0,) and states.shape == (0, 4 * 144)
        second.lanczos_begin(**begin)
        values, states, found = second.lanczos_ritz_pairs(coef, eps, 4)
        assert found == 10 and values.shape == (4,) and np.abs(values - loose[0][:4]).max() <= 1e-10
        _library_refuses_advance(second, vectors)


# ------------------------------------------------------------------ f. grid-stride sizes
def test_grid_stride_loops_wrap_on_a_large_plane(solver_cls):
    """16 510 sites, 8 real vectors: lanczos_combine / column_norms cover 66 040 payload rows with 512 x 256 threads
    at 4 lanes per row, block_gram 66 040 rows with 256 x 256 threads: every loop goes round.  α, β over 12 iterations
    against the float64 restatement at the bound of (a), with the reference distance of the 9 x 13 plane (same
    stencil, same local terms; this size has no long-double form); one device Rayleigh-Ritz on an unconverged Ritz
    block against the numpy steps on the same block."""
    from scipy.linalg import eigh_tridiagonal

    name, n_vectors, m = "plane130x127", 8, 12
    matrix = lc.sparse_matrix(name)
    ref_alpha, ref_beta, _ = lc.lanczos_reference(matrix, lc.start_block(name, n_vectors, 2, RAD), m)
    with solver_cls.from_hamiltonian(lc.build(name)) as dev:
        dev.lanczos_begin(n_vectors, seed=2, max_iter=m)
        alpha, beta = dev.lanczos_advance(m)
        perf = dev.perf()
        distance = lc.trajectory_distance(name, alpha, beta, ref_alpha, ref_beta)
        print(f"{name}: device to float64 restatement {distance:.2e} of |H|^2, reference distance of plane9x13 "
              f"{lc.reference_distance('plane9x13'):.2e}")
        _assert_form(perf, dict(real_arithmetic=1, ph_packed=1, lanes_per_row=4, dictionary=True), 2 * m)
        tolerance = _tolerance(name, like="plane9x13")
        assert np.abs(alpha - ref_alpha).max() <= tolerance and np.abs(beta - ref_beta).max() <= tolerance
        # lowest Ritz vector of every column's 12-step tridiagonal matrix: one level, not converged (no matter)
        coef = np.zeros((m, 1, n_vectors))
        theta = np.zeros(n_vectors)
        for c in range(n_vectors):
            w, s = eigh_tridiagonal(alpha[:, c], beta[:-1, c], select="i", select_range=(0, 0))
            coef[:, 0, c], theta[c] = s[:, 0], w[0]
        eps = np.array([np.sqrt(theta.mean())])
        dev.lanczos_begin(n_vectors, seed=2, max_iter=m)
        block = dev.lanczos_ritz_vectors(coef)
        dev.lanczos_begin(n_vectors, seed=2, max_iter=m)
        values, states, found = dev.lanczos_ritz_pairs(coef, eps, 16)
    ref_values, ref_states, ref_found = lc.ritz_pairs_reference(matrix, block, eps)
    z = (matrix @ block[0].T + eps[0] * block[0].T)
    z = z / np.linalg.norm(z, axis=0)
    weakest = np.linalg.eigvalsh(z.conj().T @ z)[0]
    # a dot product over n = 4 x 16 510 entries is off by at most n 2^-53 of its size; the Gram and projection steps
    # take four of them in a row, and the orthonormalisation divides by the smallest Gram weight
    bound = 4 * matrix.shape[0] * U * lc.norm_bound(name) / weakest
    overlap = states.conj() @ ref_states.T  # (8, 8): unitary when the two orthonormal sets span the same space
    apart = np.abs(overlap @ overlap.conj().T - np.eye(len(states))).max()
    print(f"{name}: Rayleigh-Ritz found {found} (reference {ref_found}), smallest Gram weight {weakest:.2e}, values apart "
          f"{np.abs(values - ref_values).max():.2e}, spans apart {apart:.2e}, bound {bound:.2e}")
    assert found == ref_found.sum() == len(values) == n_vectors
    assert np.abs(values - ref_values).max() <= bound and apart <= bound / lc.norm_bound(name)
    assert np.abs(states.conj() @ states.T - np.eye(len(states))).max() <= bound / lc.norm_bound(name)


def test_grid_stride_loops_wrap_at_32_lanes_per_row(solver_cls):
    """1056 sites, 64 real vectors (32 lanes per row): 135 168 payloads for the 131 072 threads of the norm kernels.
    The bound takes the reference distance of the 9 x 13 plane (same stencil and local terms), which the host test
    pins; the long-double side of this size is the CSR product."""
    name, n_vectors, m = "plane33x32", 64, 12
    ref_alpha, ref_beta, _ = lc.lanczos_reference(lc.sparse_long_double(name), lc.start_block(name, n_vectors, 2, RAD), m, lc.LD)
    with solver_cls.from_hamiltonian(lc.build(name)) as dev:
        dev.lanczos_begin(n_vectors, seed=2, max_iter=m)
        alpha, beta = dev.lanczos_advance(m)
        perf = dev.perf()
    distance = lc.trajectory_distance(name, alpha, beta, ref_alpha, ref_beta)
    print(f"{name}: device {distance:.2e}, reference distance of plane9x13 {lc.reference_distance('plane9x13'):.2e} of |H|^2")
    _assert_form(perf, dict(real_arithmetic=1, ph_packed=1, lanes_per_row=32, dictionary=False), 2 * m)
    tolerance = _tolerance(name, like="plane9x13")
    assert np.abs(alpha - ref_alpha).max() <= tolerance and np.abs(beta - ref_beta).max() <= tolerance


# ------------------------------------------------------------------ g. refusals
def test_refusals_leave_the_handle_usable(api, solver_cls):
    from bodge_amd.solver import SlabGroup

    name = "plane9x13"
    system = lc.build(name)
    bsr = system.matrix("bsr")
    scale = cheb_ref.spectral_bound(bsr)
    oracle = cheb_ref.recurrence_dots(bsr, scale, 16, cheb_ref.random_block(bsr.shape[0], 6, range(3), RAD))

    def still_usable(dev):
        got = dev.dots_random(scale, 8, 3, seed=6)
        assert np.allclose(got[0], oracle[0], rtol=0, atol=1e-12 * bsr.shape[0])
        assert np.allclose(got[1], oracle[1], rtol=0, atol=1e-12 * bsr.shape[0])

    def begin(dev, n=4, **options):
        dev.lanczos_begin(n, seed=1, **{"max_iter": 8, **options})

    refused = {
        "no vectors": lambda dev: begin(dev, 0),
        "65 vectors": lambda dev: begin(dev, 65),
        "max_iter 0": lambda dev: begin(dev, max_iter=0),
        "unknown vector kind": lambda dev: begin(dev, kind=7),
        "advance past max_iter": lambda dev: (begin(dev), dev.lanczos_advance(9)),
        "advance past max_iter in two calls": lambda dev: (begin(dev), dev.lanczos_advance(5), dev.lanczos_advance(4)),
        "advance(0)": lambda dev: (begin(dev), dev.lanczos_advance(0)),
        "Ritz pass on an advanced process": lambda dev: (begin(dev), dev.lanczos_advance(2), dev.lanczos_ritz_vectors(np.ones((2, 1, 4)))),
        "Ritz pairs on an advanced process": lambda dev: (begin(dev), dev.lanczos_advance(2), dev.lanczos_ritz_pairs(np.ones((2, 1, 4)), np.ones(1), 2)),
        "no levels": lambda dev: (begin(dev), dev.lanczos_ritz_vectors(np.ones((2, 0, 4)))),
        "65 levels": lambda dev: (begin(dev), dev.lanczos_ritz_vectors(np.ones((2, 65, 4)))),
        "n_iter above max_iter": lambda dev: (begin(dev), dev.lanczos_ritz_vectors(np.ones((9, 1, 4)))),
        "17 real vectors in ritz_pairs": lambda dev: (begin(dev, 17), dev.lanczos_ritz_pairs(np.ones((2, 1, 17)), np.ones(1), 2)),
        "32 real vectors in ritz_pairs": lambda dev: (begin(dev, 32), dev.lanczos_ritz_pairs(np.ones((2, 1, 32)), np.ones(1), 2)),
        "rank_tol -0.1": lambda dev: (begin(dev), dev.lanczos_ritz_pairs(np.ones((2, 1, 4)), np.ones(1), 2, rank_tol=-0.1)),
        "rank_tol 1.0": lambda dev: (begin(dev), dev.lanczos_ritz_pairs(np.ones((2, 1, 4)), np.ones(1), 2, rank_tol=1.0)),
    }
    with solver_cls.from_hamiltonian(system) as dev:
        for what, call in refused.items():
            with pytest.raises(ValueError):
                call(dev)
                pytest.fail(f"not refused: {what}")
            still_usable(dev)
        begin(dev, 17)  # (17 real vectors run; only the device Rayleigh-Ritz is limited to 16 columns)
        assert dev.lanczos_advance(2)[0].shape == (2, 17)
    with SlabGroup.from_hamiltonian(system, 2) as group:
        with pytest.raises(ValueError):
            group.members[0].lanczos_begin(4, seed=1, max_iter=8)  # a row slab: ncols != nb
        got = group.dots_random(scale, 8, 3, seed=6)
        assert np.allclose(got[0], oracle[0], rtol=0, atol=1e-12 * bsr.shape[0])
