"""apply() / evolve() on the GPU: the stored-source Clenshaw kernels against the numpy restatement and dense eigh in
every kernel form and arithmetic mode, the batches bit for bit, the physics of a time evolution, fermi_matrix
column by column, and bdg_spmv."""

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import apply as ap
from bodge_amd import chebyshev as cheb

import apply_cases as cases

pytestmark = pytest.mark.gpu

TIMES = np.array([10.0, -3.0])
TEMPERATURE = 0.1

# The tolerance of the device result is 20 times the error of the numpy restatement (apply_cases.stored_source_clenshaw,
# sparse H) against V g(E) V† x from numpy.linalg.eigh, measured in the test on the case it runs: three random complex
# unit vectors, largest entry of the difference; "evolve" = the times above in one call (cut-off 1e-12: M = 85 .. 109),
# "fermi" = the Fermi function at T = 0.1 (M = 410 .. 568).  As measured: 6e-14 .. 8e-14 and 1.2e-13 .. 2.8e-13
# (DESIGN.md §13); a restatement that is itself off by more than the pins of tests/test_apply_host.py fails here too.
ARITHMETIC = {
    "packed": {},
    "real_full": {"BODGE_AMD_PH": "0"},
    "complex_packed": {"BODGE_AMD_REAL": "0"},
    "complex_full": {"BODGE_AMD_REAL": "0", "BODGE_AMD_PH": "0"},
}


# ------------------------------------------------------------------ against the restatement and dense eigh
@pytest.mark.parametrize("name", sorted(cases.SYSTEMS))
@pytest.mark.parametrize("form", ["dictionary", "streamed"])
@pytest.mark.parametrize("arithmetic", sorted(ARITHMETIC))
def test_device_matches_restatement_and_dense(name, form, arithmetic, knobs):
    system = cases.SYSTEMS[name]()
    knobs.update(ARITHMETIC[arithmetic])
    if form == "streamed":
        knobs.set("BODGE_AMD_DICT", "0")
    h = system.matrix("csr")
    scale = cases.scale_of(system)
    x = cases.unit_vectors(system)
    is_real = np.abs(np.asarray(system.matrix("dense")).imag).max() == 0

    moved = system.evolve(x.T, TIMES)  # raw layout: (T, 4N, V)
    perf = system._solver().perf()
    coef = ap.evolution_coefficients(scale, TIMES, 12.0)
    restated = cases.stored_source_clenshaw(h, scale, coef, x)  # (V, T, 4N)
    exact = cases.dense_function(system, lambda e: np.exp(-1j * np.outer(TIMES, e)), x)
    got = np.moveaxis(moved, (0, 1, 2), (1, 2, 0))
    own = np.abs(restated - exact).max()
    assert own < 1e-11
    tolerance = 20 * own
    print(name, form, arithmetic, "evolve", len(coef), np.abs(got - restated).max(), np.abs(got - exact).max(), tolerance)
    assert np.abs(got - restated).max() <= tolerance and np.abs(got - exact).max() <= tolerance

    assert perf["apply"] in (1, 2) and perf["clenshaw"] == 0 and perf["green"] == 0 and perf["green_local"] == 0
    assert perf["launches"] == len(coef) and perf["vector_steps"] == len(coef) * 6  # 3 vectors x 2 times: one batch
    assert perf["lanes_per_row"] == 8 and perf["bytes_per_launch"] > 0 and perf["window_ms"] > 0 and perf["kernel_ms"] > 0
    assert perf["bytes_moved"] == perf["bytes_per_launch"] * perf["launches"]
    if form == "streamed" or name == "disordered_300":  # (300 distinct on-site blocks: more than a table holds)
        assert perf["apply"] == 1 and perf["dict_blocks"] == 0
    elif name in ("dictionary", "cube"):
        assert perf["apply"] == 2 and perf["dict_blocks"] > 0
    assert perf["real_arithmetic"] == (1 if is_real and "complex" not in arithmetic else 0)
    assert perf["vectors_per_launch"] == 8 * (2 if perf["real_arithmetic"] else 1)
    if arithmetic.endswith("full"):
        assert perf["ph_packed"] == 0

    occupied = system.apply(lambda e: cheb.fermi_function(e, TEMPERATURE), x.reshape(3, -1, 4))  # reshape layout
    coef = cases.fermi_coefficients(scale, TEMPERATURE, 12.0)[:, None]
    restated = cases.stored_source_clenshaw(h, scale, coef, x)[:, 0]
    exact = cases.dense_function(system, lambda e: cheb.fermi_function(e, TEMPERATURE), x)
    got = occupied.reshape(3, -1)
    own = np.abs(restated - exact).max()
    assert own < 1e-12
    tolerance = 20 * own
    print(name, form, arithmetic, "fermi", len(coef), np.abs(got - restated).max(), np.abs(got - exact).max(), tolerance)
    assert np.abs(got - restated).max() <= tolerance and np.abs(got - exact).max() <= tolerance
    assert system._solver().perf()["launches"] == len(coef)


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("name", ["dictionary", "disordered_complex"])
def test_columns_do_not_depend_on_their_batch(name):
    """The recurrence of a column does not depend on its neighbours in the batch: 1, 5 and 70 columns (70: more than
    one batch) give the same bits column by column."""
    system = cases.SYSTEMS[name]()
    solver = system._solver()
    scale = cases.scale_of(system)
    x = cases.unit_vectors(system, 70, seed=3)
    coef = ap.evolution_coefficients(scale, np.array([4.0]), 12.0)
    many = solver.apply_series(scale, coef, x)
    perf = solver.perf()
    width = perf["lanes_per_row"]
    assert many.shape == (70, 1, solver.dim) and width in (32, 64)
    assert perf["launches"] == -(-70 // width) * len(coef) > len(coef) and perf["vector_steps"] == 70 * len(coef)
    five = solver.apply_series(scale, coef, x[:5])
    assert solver.perf()["lanes_per_row"] == 8 and solver.perf()["launches"] == len(coef)
    one = solver.apply_series(scale, coef, x[:1])
    assert solver.perf()["lanes_per_row"] == 4
    last = solver.apply_series(scale, coef, x[69:])
    print(name, np.abs(many[:5] - five).max(), np.abs(many[:1] - one).max(), np.abs(many[69:] - last).max())
    assert np.array_equal(many[:5], five) and np.array_equal(many[:1], one) and np.array_equal(many[69:], last)
    # ... and with fixed lanes, vectors and functions mixed over many batches
    times = np.array([4.0, -1.0, 0.5])
    coef3 = ap.evolution_coefficients(scale, times, 12.0)
    solver.set_lanes_per_row(4)
    try:
        narrow = solver.apply_series(scale, coef3, x[:6])  # 18 columns in batches of 4: vectors straddle batches
        assert solver.perf()["lanes_per_row"] == 4 and solver.perf()["launches"] == 5 * len(coef3)
    finally:
        solver.set_lanes_per_row(0)
    wide = solver.apply_series(scale, coef3, x[:6])
    assert solver.perf()["launches"] == len(coef3)
    assert np.array_equal(narrow, wide)
    assert np.array_equal(wide[:5, 0, :], solver.apply_series(scale, coef3[:, :1], x[:5])[:, 0, :])


def test_many_times_equal_single_calls_bit_for_bit():
    system = cases.SYSTEMS["disordered_real"]()
    solver = system._solver()
    x = cases.unit_vectors(system, 2).reshape(2, -1, 4)
    times = np.array([0.5, 2.0, -7.0, 12.0, 3.0])
    solver.set_lanes_per_row(8)
    try:
        together = system.evolve(x, times)
        coef = ap.evolution_coefficients(cases.scale_of(system), times, 12.0)
        assert together.shape == (5,) + x.shape and solver.perf()["launches"] == 2 * len(coef)  # 10 columns: two batches
        for f, t in enumerate(times):
            # (one call makes all series as long as the longest; the coefficients a shorter one lacks are < 1e-12, so
            # the single-time call is given the same length to run the same recurrence)
            single = system.apply(None, x, coefficients=coef[:, f])
            assert single.shape == x.shape and np.array_equal(together[f], single), t
            assert np.abs(system.evolve(x, float(t)) - together[f]).max() <= 1e-11
    finally:
        solver.set_lanes_per_row(0)


# ------------------------------------------------------------------ physics
@pytest.mark.parametrize("name", ["dictionary", "disordered_complex"])
def test_evolution_is_unitary_and_reversible(name):
    system = cases.SYSTEMS[name]()
    x = cases.unit_vectors(system, 3).T
    t = 500.0 / cases.scale_of(system)
    moved = system.evolve(x, t)
    drift = np.abs(np.linalg.norm(moved, axis=0) - 1).max()
    back = system.evolve(moved, -t)
    print(name, drift, np.abs(back - x).max())
    assert drift <= 1e-12
    assert np.abs(back - x).max() <= 1e-11
    gram = moved.conj().T @ moved  # inner products are kept as well
    assert np.abs(gram - x.conj().T @ x).max() <= 1e-11


def test_an_eigenstate_only_acquires_its_phase():
    system = cases.SYSTEMS["dictionary"]()
    h = system.matrix("csr")
    times = np.array([0.3, 25.0])
    # exact eigenvectors (numpy.linalg.eigh of the dense matrix, residual of round-off size): the phase to 1e-11
    w, v = np.linalg.eigh(np.asarray(system.matrix("dense")))
    picked = [0, len(w) // 2, len(w) - 1]  # both ends of the spectrum and the first level above the gap
    moved = system.evolve(v[:, picked], times)
    for f, t in enumerate(times):
        for column, n in enumerate(picked):
            error = np.abs(moved[f, :, column] - np.exp(-1j * w[n] * t) * v[:, n]).max()
            print("eigh", t, n, error)
            assert error <= 1e-11, (t, n)
    # ... and the states diagonalize() returns, in both of its layouts.  An approximate eigenvector with residual
    # |H v - E v| = ρ is off its phase by at most ρ t after the time t; the device solver's vectors must be good
    # enough for that allowance to stay of the size of the bound itself.
    energies, states = system.diagonalize()  # (n, N, 4)
    residual = max(np.linalg.norm(h @ states[n].reshape(-1) - energies[n] * states[n].reshape(-1)) for n in range(3))
    print("diagonalize residual", residual)
    assert residual <= 1e-12
    for format, vectors in (("reshape", states[:3]), ("raw", system.diagonalize(format="raw")[1][:, :3])):
        moved = system.evolve(vectors, times)
        for f, t in enumerate(times):
            for n in range(3):
                before = vectors[n] if format == "reshape" else vectors[:, n]
                after = moved[f, n] if format == "reshape" else moved[f, :, n]
                assert np.abs(after - np.exp(-1j * energies[n] * t) * before).max() <= 1e-11 + residual * t, (format, t, n)


def test_apply_of_the_fermi_function_gives_the_columns_of_fermi_matrix():
    system = cases.uniform_swave((6, 5, 1))
    temperature = 0.1
    reference = system.fermi_matrix(temperature, distance=None)
    n = system.lattice.size
    source = (2, 1, 0)
    i = system.lattice[source]
    units = np.zeros((4, 4 * n))
    units[np.arange(4), 4 * i + np.arange(4)] = 1.0
    columns = system.apply(lambda e: cheb.fermi_function(e, temperature), units.T)  # (4N, 4)
    for target in (source, (3, 1, 0), (2, 2, 0)):
        j = system.lattice[target]
        block = reference.block(target, source)  # f(H)[4j:4j+4, 4i:4i+4]
        assert np.abs(columns[4 * j : 4 * j + 4, :] - block).max() <= 1e-11, target


def test_the_identity_function_is_the_matrix_vector_product():
    for name in ("dictionary", "disordered_complex", "cube"):
        system = cases.SYSTEMS[name]()
        solver = system._solver()
        x = cases.unit_vectors(system, 2)
        product = system.apply(lambda e: e, x.T, moments=2)
        scale = cases.scale_of(system)
        for v in range(2):
            expected = solver.spmv(x[v])
            # c_1 = scale up to the quadrature's round-off, and one multiplication by it: a few ulps of |H x| <= scale
            assert np.abs(product[:, v] - expected).max() <= 16 * np.finfo(float).eps * scale, name


# ------------------------------------------------------------------ refusals
def test_slab_handles_are_refused():
    from bodge_amd.solver import SlabGroup

    system = cases.uniform_swave((8, 4, 1))
    with SlabGroup.from_hamiltonian(system, 2) as group:
        member = group.members[0]
        with pytest.raises(ValueError, match="slab"):
            member.apply_series(1.0, np.ones((2, 1)), np.ones((1, member.dim)))


def test_a_lanczos_run_on_the_handle_is_ended():
    system = cases.uniform_swave()
    solver = system._solver()
    solver.lanczos_begin(2, max_iter=64)
    solver.lanczos_advance(2)
    system.evolve(cases.unit_vectors(system, 1)[0], 1.0)
    with pytest.raises(ValueError, match="lanczos_begin"):
        solver.lanczos_advance(1)


# ------------------------------------------------------------------ a lattice of some size
@pytest.mark.timeout(300)
def test_64x64_wave_packet_keeps_norm_and_energy():
    system = cases.uniform_swave((64, 64, 1), mu=0.5, gap=1.0, zeeman=0.0)
    n = system.lattice.size
    psi = np.zeros((n, 4), dtype=np.complex128)
    sites = system.lattice.site_array()
    envelope = np.exp(-((sites[:, 0] - 32.0) ** 2 + (sites[:, 1] - 30.0) ** 2) / 18.0 + 0.6j * sites[:, 0])
    psi[:, 0] = envelope / np.linalg.norm(envelope)
    times = np.linspace(0.0, 30.0, 16)
    moved = system.evolve(psi, times)
    perf = system._solver().perf()
    assert moved.shape == (16, n, 4) and perf["apply"] == 2 and perf["lanes_per_row"] == 16
    h = system.matrix("csr")
    energy = [np.vdot(m.reshape(-1), h @ m.reshape(-1)).real for m in moved]
    norms = np.linalg.norm(moved.reshape(16, -1), axis=1)
    assert np.abs(norms - 1).max() <= 1e-12 and np.abs(np.array(energy) - energy[0]).max() <= 1e-11
    assert np.array_equal(moved[0], psi) or np.abs(moved[0] - psi).max() <= 1e-14
    spread = [(np.abs(m) ** 2).sum(axis=1) @ ((sites[:, 0] - 32.0) ** 2) for m in moved]
    assert spread[-1] > 4 * spread[0]  # the packet moves and spreads
