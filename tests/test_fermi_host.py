"""fermi_matrix without a GPU: the probe-Clenshaw algorithm restated in numpy against dense f(H), the
colouring, the coefficient rule, the particle-hole columns, the helpers' contractions and the register
budget of the new kernels."""

import os
import shutil
import sys

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import chebyshev as cheb
from bodge_amd import fermi

import fermi_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ systems and dense oracle
def swave(shape=(5, 4, 1), mu=0.5, gap=0.3, zeeman=0.2, periodic=False, hop=-1.0):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    with system as (H, Δ):
        H.set_sites(-mu * ba.σ0 - zeeman * ba.σ3)
        Δ.set_sites(gap * ba.jσ2)
        H.set_bonds(hop * ba.σ0)
        if periodic:
            H.set_edges(hop * ba.σ0)
    return system


def pwave_complex(shape=(5, 5, 1)):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    spin = ba.pwave("e_z * (p_x + jp_y)")
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -0.7 * ba.σ0
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * ba.σ0
            Δ[i, j] = 0.4 * spin(i, j)
    return system


def dense_fermi(system, temperature):
    """V f(E) V^† of the dense matrix, cut to the skeleton: (nnzb, 4, 4)."""
    h = np.asarray(system.matrix("dense"))
    w, v = np.linalg.eigh(h)
    full = (v * cheb.fermi_function(w, temperature)) @ v.conj().T
    n = system.lattice.size
    indptr, indices = system._matrix.indptr, system._matrix.indices
    rows = np.repeat(np.arange(n), np.diff(indptr))
    return full.reshape(n, 4, n, 4)[rows, :, indices, :]


def probe_clenshaw(system, temperature, distance=None, components=4, moments=None):
    """The algorithm of bdg_fermi_blocks in numpy (fermi_cases.restated_blocks: probes per (colour, component),
    Clenshaw's recurrence, the extraction of the pattern columns) with the colouring and the coefficients of
    fermi_matrix, and the particle-hole columns when components = 2."""
    scale = cases.scale_of(system)
    coef = cases.fermi_coefficients(system, temperature, moments)
    colours, n_colours = fermi.site_colours(system, distance)
    indptr, indices = system._matrix.indptr, system._matrix.indices
    out = cases.restated_blocks(system, scale, coef, colours, n_colours, components, indptr, indices)
    if components == 2:
        rows = np.repeat(np.arange(system.lattice.size), np.diff(indptr))
        fermi._particle_hole_columns(out, np.flatnonzero(rows == indices))
    return out


# ------------------------------------------------------------------ the two references of the GPU tests
@pytest.mark.parametrize("name", sorted(cases.apply_cases.SYSTEMS))
@pytest.mark.parametrize("n_colours", cases.COLOUR_COUNTS)
def test_restated_and_dense_probed_blocks_agree_on_random_colourings(name, n_colours):
    """The restatement of the probed recurrence and V f(E) V† times the probe matrix on colourings that respect no
    distance (adjacent sites of one colour, sites that are not probed, empty colours), 4 components, T = 0.1.
    Measured: 1.0e-14 .. 2.7e-14 with largest entries 0.8 .. 1.5."""
    restated, dense, largest, own = cases.references(name, cases.TEMPERATURE, ("random", n_colours, 0))
    colours, _ = cases.colouring(name, ("random", n_colours, 0))
    print(name, n_colours, "largest", largest, "restated - dense", own)
    assert largest > 0.1
    assert own <= 1e-12
    indices = cases.pattern_of(cases.system_of(name))[1]
    assert not restated[colours[indices] < 0].any() and not dense[colours[indices] < 0].any()


# ------------------------------------------------------------------ algorithm
@pytest.mark.parametrize("temperature", [0.1, 0.5])
def test_probe_clenshaw_restatement_matches_dense(temperature):
    for system in (swave(), swave((4, 3, 2), periodic=True), pwave_complex((4, 4, 1))):
        exact = dense_fermi(system, temperature)
        got = probe_clenshaw(system, temperature)
        assert np.abs(got - exact).max() < 1e-11


def test_particle_hole_columns_equal_the_four_column_result():
    system = swave((6, 5, 1), periodic=True)
    assert system.has_symmetric_spectrum(1e-12)
    four = probe_clenshaw(system, 0.2, distance=3, components=4)
    two = probe_clenshaw(system, 0.2, distance=3, components=2)
    assert np.abs(two - four).max() < 1e-12
    exact = probe_clenshaw(system, 0.2, components=4)
    assert np.abs(fermi.FermiMatrix(system.lattice, system._matrix.indptr, system._matrix.indices, exact, 0.2,
                                    "check").blocks - dense_fermi(system, 0.2)).max() < 1e-11


def test_probing_error_falls_with_distance():
    system = swave((16, 16, 1), mu=0.5, gap=1.0, zeeman=0.0)
    exact = dense_fermi(system, 0.1)
    errors = [np.abs(probe_clenshaw(system, 0.1, distance=d, components=2) - exact).max() for d in (3, 5, 9)]
    # measured 1.8e-2, 1.7e-3, 2e-15 (d = 9 rounds up to 16 = the extent: one site per colour, exact)
    assert errors[0] > errors[1] > errors[2]
    assert errors[0] < 0.05 and errors[1] < 5e-3 and errors[2] < 1e-11


# ------------------------------------------------------------------ colouring
def _wrapped_distance(a, b, shape):
    """Hops between two sites in the graph of the block skeleton, which holds the wrap-around pair of
    every axis (zero blocks included): the periodic lattice distance."""
    return sum(min(d, length - d) for d, length in zip(np.abs(np.subtract(a, b)), shape))


@pytest.mark.parametrize("shape,distance", [
    ((10, 7, 1), 3),    # 3 divides neither: 5 and 7
    ((9, 8, 1), 4),     # x: 9 (no divisor in 4..8), y: 4
    ((12, 5, 3), 4),
    ((6, 6, 6), 5),
    ((16, 16, 1), 5),   # 5 -> 8
])
def test_same_colour_sites_are_at_least_distance_apart(shape, distance):
    periods = fermi.colour_periods(shape, distance)
    for length, period in zip(shape, periods):
        assert period >= min(distance, length) and length % period == 0
    colours, n_colours = fermi.cubic_colours(shape, periods)
    coords = ba.CubicLattice(shape).site_array()
    assert colours.min() >= 0 and colours.max() < n_colours
    for c in range(n_colours):
        members = coords[colours == c]
        for p in range(len(members)):
            for q in range(p):
                assert _wrapped_distance(members[p], members[q], shape) >= distance


def test_site_colours_of_a_system():
    system = swave((10, 7, 1))
    colours, n = fermi.site_colours(system, 3)
    assert n == 5 * 7  # 3 -> 5 (divides 10), 3 -> 7 (divides 7)
    assert fermi.site_colours(system, None)[1] == system.lattice.size
    assert fermi.site_colours(system, 50)[1] == system.lattice.size
    with pytest.raises(ValueError):
        fermi.site_colours(system, 2)


def test_open_axes_get_their_zero_wrap_blocks_right():
    """The pattern holds the (zero) wrap-around blocks of open axes too; with the divisor rule the probes give
    them to the accuracy of the bond blocks instead of mixing in a site next to the far face."""
    system = swave((12, 9, 1), mu=0.5, gap=0.8, zeeman=0.0)
    exact = dense_fermi(system, 0.1)
    got = probe_clenshaw(system, 0.1, distance=6, components=2)
    assert np.abs(got - exact).max() < 1e-2  # (measured 4.8e-3; a colour period of 6 along y, not dividing 9: 0.5)


def test_graph_colouring_of_a_general_pattern():
    system = swave((7, 6, 1), periodic=True)
    indptr, indices, _ = system.bsr_arrays()
    colours, n = fermi.graph_colours(indptr, indices, 4)
    coords = system.lattice.site_array()
    for c in range(n):
        members = coords[colours == c]
        for p in range(len(members)):
            for q in range(p):
                assert _wrapped_distance(members[p], members[q], (7, 6, 1)) >= 4


# ------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("temperature", [0.02, 0.05, 0.2, 1.0])
def test_moments_rule_reaches_1e11_on_dense_f(temperature):
    system = swave((6, 5, 1), mu=0.3, zeeman=0.1)
    h = np.asarray(system.matrix("dense"))
    scale = 1.01 * system.gershgorin_bound()
    m = cheb.moments_for_fermi(scale, temperature, 12)
    coef = cheb.chebyshev_coefficients(lambda x: cheb.fermi_function(scale * x, temperature), m)
    w, v = np.linalg.eigh(h)
    series = np.polynomial.chebyshev.chebval(w / scale, coef)
    exact = cheb.fermi_function(w, temperature)
    assert np.abs(series - exact).max() < 1e-11
    got = (v * series) @ v.conj().T
    assert np.abs(got - (v * exact) @ v.conj().T).max() < 1e-11
    grid = np.linspace(-scale, scale, 20001)
    assert np.abs(np.polynomial.chebyshev.chebval(grid / scale, coef) - cheb.fermi_function(grid, temperature)).max() < 1e-11
    # and the rule is not wasteful: half of it misses 1e-10 somewhere on the interval
    short = coef[: m // 2]
    assert np.abs(np.polynomial.chebyshev.chebval(grid / scale, short) - cheb.fermi_function(grid, temperature)).max() > 1e-10
    with pytest.raises(ValueError):
        cheb.moments_for_fermi(scale, 0.0)


# ------------------------------------------------------------------ helpers
def _fermi_matrix(system, temperature):
    return fermi.FermiMatrix(system.lattice, system._matrix.indptr.astype(np.int32),
                             system._matrix.indices.astype(np.int32), dense_fermi(system, temperature),
                             temperature, "dense-numpy")


def _free_energy(system, temperature):
    w = np.linalg.eigvalsh(np.asarray(system.matrix("dense")))
    return -(temperature / 2) * np.sum(np.logaddexp(w / (2 * temperature), -w / (2 * temperature)))


def test_helpers_are_slices_of_the_blocks():
    system = swave((4, 3, 1), zeeman=0.3)
    fm = _fermi_matrix(system, 0.1)
    h = np.asarray(system.matrix("dense"))
    w, v = np.linalg.eigh(h)
    full = (v * cheb.fermi_function(w, 0.1)) @ v.conj().T
    i, j = (1, 1, 0), (2, 1, 0)
    a, b = system.lattice[i], system.lattice[j]
    assert np.allclose(fm.block(i, j), full[4 * a:4 * a + 4, 4 * b:4 * b + 4], atol=1e-14)
    assert np.allclose(fm.pairing(i, j), full[4 * a:4 * a + 2, 4 * b + 2:4 * b + 4], atol=1e-14)
    diag = np.array([full[4 * s:4 * s + 4, 4 * s:4 * s + 4] for s in range(system.lattice.size)])
    assert np.allclose(fm.density(), (diag[:, 0, 0] + diag[:, 1, 1]).real, atol=1e-14)
    assert np.allclose(fm.pair_amplitude(), diag[:, 0, 3], atol=1e-14)
    assert np.allclose(fm.magnetization()[:, 2], (diag[:, 0, 0] - diag[:, 1, 1]).real, atol=1e-14)
    assert np.allclose(fm.magnetization()[:, 0], 2 * diag[:, 0, 1].real, atol=1e-14)
    assert fm.magnetization()[:, 2].sum() > 0 or fm.magnetization()[:, 2].sum() < 0  # the field polarises
    with pytest.raises(IndexError):
        fm.block((0, 0, 0), (3, 2, 0))


def test_expectation_is_the_derivative_of_the_free_energy():
    """½ tr(f(H) dH) = dF/dλ with F = -(T/2) Σ_E ln 2cosh(E/2T) (dense numpy on both sides)."""
    temperature, step = 0.2, 1e-5
    for label, build, dh in (
        ("mu", lambda x: swave((4, 4, 1), mu=0.5 + x), lambda: swave((4, 4, 1), mu=1.0, gap=0, zeeman=0, hop=0)),
        ("t", lambda x: swave((4, 4, 1), hop=-1.0 + x), lambda: swave((4, 4, 1), mu=0, gap=0, zeeman=0, hop=1.0)),
    ):
        system = build(0.0)
        derivative = (_free_energy(build(step), temperature) - _free_energy(build(-step), temperature)) / (2 * step)
        # dH/dμ = -σ0 on the sites: the Hamiltonian built with mu=1 and nothing else; dH/dt = the bonds at t = 1
        value = _fermi_matrix(system, temperature).expectation(dh()._data)
        assert abs(value.imag) < 1e-12
        assert abs(value.real - derivative) < 1e-6 * abs(derivative), label


# ------------------------------------------------------------------ kernels
@pytest.fixture(scope="module")
def resources():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    return kernel_resources.collect()


def _row(resources, name):
    matches = [row for key, row in resources.items() if key.startswith(f"void bdg::{name}(")]
    assert len(matches) == 1, (name, [k for k in resources if "FermiTail" in k or "clenshaw" in k][:8])
    return matches[0]


@pytest.mark.timeout(900)
def test_clenshaw_kernels_do_not_spill_and_keep_their_occupancy(resources):
    """The Clenshaw steps are the one-step kernels without the dot products and with a source term: the same
    register class (no scratch, at most 128 VGPRs, 4 waves per SIMD), in every mode and lane count."""
    for mode in ("RealPHMode", "ComplexPHMode", "RealMode", "ComplexMode"):
        lanes = (4, 8, 16, 32) if mode.startswith("Real") else (4, 8, 16, 32, 64)
        for rl in lanes:
            for maxb in (3, 5, 7):
                row = _row(resources, f"cheb_clenshaw_dict<bdg::{mode}, {rl}, {maxb}>")
                assert row["scratch"] == 0 and row["vgpr"] <= 128 and row["occupancy"] >= 4, (mode, rl, maxb, row)
        for rl in (4, 8, 16, 32, 64):
            row = _row(resources, f"cheb_family<bdg::{mode}, {rl}, bdg::FermiTail>")
            assert row["scratch"] == 0 and row["vgpr"] <= 128 and row["occupancy"] >= 4, (mode, rl, row)
    for per_lane in (1, 2):
        row = _row(resources, f"fermi_extract<{per_lane}>")
        assert row["scratch"] == 0
