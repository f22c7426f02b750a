"""green_map() on the GPU: the full-width batches against bdg_green_moments site by site (bit for bit), the chunked
device table, the map against the dense inverse on every site, against ldos and green(), and the perf record."""

import numpy as np
import pytest

import bodge_amd as ba

pytestmark = pytest.mark.gpu

ENERGIES = np.array([-0.4, -0.2, 0.0, 0.2, 0.4, 0.6, 0.8, 1.0, 0.2])  # both signs, unordered, one repeat


# ------------------------------------------------------------------ systems
def swave(shape=(8, 7, 1), mu=0.5, gap=0.3, zeeman=0.2, hop=-1.0):
    """Real, particle-hole packed, a handful of distinct blocks: the dictionary kernel."""
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    with system as (H, Δ):
        H.set_sites(-mu * ba.σ0 - zeeman * ba.σ3)
        Δ.set_sites(gap * ba.jσ2)
        H.set_bonds(hop * ba.σ0)
    return system


def complex_system(shape=(6, 5, 1)):
    """σ2 on-site term, complex s-wave gap, σ1 in the hopping: no real form, spin not conserved."""
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -0.5 * ba.σ0 + 0.3 * ba.σ2
            Δ[i, i] = 0.3 * np.exp(0.7j) * ba.jσ2
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * ba.σ0 + 0.2 * ba.σ1
    return system


def disordered(shape=(20, 15, 1)):
    """A different on-site matrix on every site: 300 distinct blocks, more than a dictionary holds."""
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    rng = np.random.default_rng(11)
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -(0.5 + 0.4 * rng.random()) * ba.σ0 + 0.3 * rng.random() * ba.σ3
            Δ[i, i] = (0.2 + 0.2 * rng.random()) * ba.jσ2
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * ba.σ0
    return system


SYSTEMS = {
    "swave_dictionary": lambda: swave(),
    "complex_streamed": complex_system,
    "disordered": disordered,
    "cube": lambda: swave((4, 4, 3)),
}


def dense_local_green(system, indices, z):
    h = np.asarray(system.matrix("dense"))
    out = np.empty((len(indices), len(z), 4, 4), dtype=np.complex128)
    for k, zk in enumerate(z):
        g = np.linalg.inv(zk * np.eye(h.shape[0]) - h)
        for s, j in enumerate(indices):
            out[s, k] = g[4 * j : 4 * j + 4, 4 * j : 4 * j + 4]
    return out


def relative_error(got, exact):
    return np.array([np.abs(g - e).max() / np.abs(e).max() for g, e in zip(got, exact)])


# ------------------------------------------------------------------ against bdg_green_moments, site by site
@pytest.mark.parametrize("name", sorted(SYSTEMS))
@pytest.mark.parametrize("columns", [2, 4])
def test_moments_are_those_of_one_site_per_call_bit_for_bit(name, columns, knobs):
    """The recurrence of a vector does not depend on its neighbours in the batch: with the same lanes per row the
    moments of a full-width batch are those of bdg_green_moments called for one site, bit for bit."""
    system = SYSTEMS[name]()
    if name == "complex_streamed":
        knobs.set("BODGE_AMD_DICT", "0")
    solver = system._solver()
    scale = 1.01 * system.gershgorin_bound()
    moments = 160
    rng = np.random.default_rng(3)
    order = rng.permutation(system.lattice.size).astype(np.int32)  # (unordered site lists)
    lanes = 8
    solver.set_lanes_per_row(lanes)
    try:
        probe = solver.green_local_moments(scale, 4, order[:1], columns)
        perf = solver.perf()
        batch = lanes * (2 if perf["real_arithmetic"] else 1) // columns  # sites of a full batch
        assert batch >= 2 and probe.shape == (4, 1, 4, columns)
        expected_form = {"swave_dictionary": 2, "cube": 2, "complex_streamed": 1, "disordered": 1}[name]
        assert perf["green_local"] == expected_form and perf["green"] == 0 and perf["lanes_per_row"] == lanes
        single = {}

        def one_site(j):
            if j not in single:
                rows = 4 * int(j) + np.arange(columns, dtype=np.int64)
                single[j] = solver.green_moments(scale, moments, rows, np.array([j], dtype=np.int32))[:, 0]
                assert solver.perf()["lanes_per_row"] == lanes and solver.perf()["green_local"] == 0
            return single[j]

        for n_sites in (2 * batch, batch + 1, 1):  # full batches, a partial last batch, a single site
            sites = order[:n_sites]
            local = solver.green_local_moments(scale, moments, sites, columns)
            perf = solver.perf()
            n_batches = -(-n_sites // batch)
            assert local.shape == (moments, n_sites, 4, columns)
            assert perf["launches"] == n_batches * (moments - 1), (perf, n_sites, batch)
            assert perf["vector_steps"] == (moments - 1) * n_sites * columns
            for s, j in enumerate(sites.tolist()):
                reference = one_site(j)
                difference = np.abs(local[:, s] - reference).max()
                print(name, columns, n_sites, s, j, difference)
                assert np.array_equal(local[:, s], reference), (name, columns, n_sites, s, j, difference)
        # moment 0 is the unit matrix's columns, moment 1 the site's own block of H / scale
        assert np.array_equal(local[0, 0], np.eye(4)[:, :columns])
        j = int(order[0])
        h = np.asarray(system.matrix("dense"))[4 * j : 4 * j + 4, 4 * j : 4 * j + columns]
        assert np.abs(local[1, 0] - h / scale).max() <= 1e-15
    finally:
        solver.set_lanes_per_row(0)


def test_argument_errors_of_the_entry_point():
    system = swave()
    solver = system._solver()
    scale = 1.01 * system.gershgorin_bound()
    with pytest.raises(ValueError, match="twice"):
        solver.green_local_moments(scale, 8, np.array([3, 5, 3], dtype=np.int32), 2)
    with pytest.raises(ValueError, match="out of range"):
        solver.green_local_moments(scale, 8, np.array([system.lattice.size], dtype=np.int32), 2)
    with pytest.raises(ValueError, match="components"):
        solver.green_local_moments(scale, 8, np.array([0], dtype=np.int32), 3)


# ------------------------------------------------------------------ the device table in ranges
@pytest.mark.parametrize("columns", [2, 4])
def test_chunked_device_table_is_bit_identical(columns, knobs):
    system = swave()
    solver = system._solver()
    scale = 1.01 * system.gershgorin_bound()
    sites = np.arange(system.lattice.size, dtype=np.int32)[::-1].copy()  # 56 sites: two or four batches, the last partial
    whole = solver.green_local_moments(scale, 100, sites, columns)
    perf = solver.perf()
    assert perf["green_ranges"] == 1 and whole.shape == (100, 56, 4, columns)
    batch = perf["vectors_per_launch"] // columns
    knobs.set("BODGE_AMD_GREEN_TABLE_BYTES", str(30 * batch * 4 * columns * 16))  # 30 moments per range
    chunked = solver.green_local_moments(scale, 100, sites, columns)
    assert solver.perf()["green_ranges"] == 4
    assert np.array_equal(whole, chunked)
    knobs.set("BODGE_AMD_GREEN_TABLE_BYTES", "1")  # (less than one moment: one moment per range)
    single = solver.green_local_moments(scale, 10, sites, columns)
    assert solver.perf()["green_ranges"] == 10
    assert np.array_equal(whole[:10], single)


# ------------------------------------------------------------------ the map against the dense inverse
# Error of the numpy restatement of the algorithm (tests/test_green_map_host.py: batches of unit vectors, one
# recurrence, own-site rows, series) against inv(z - H) on these systems and energies, as measured on the CPU: max
# over all sites and the two broadening modes, relative to the largest entry of the block.  The tolerance of the
# device result is 20 times that, capped at 1e-10.
MAP_ENERGIES = {"swave_12x10": np.linspace(-1.0, 1.0, 9), "complex": ENERGIES}
RESTATEMENT_ERROR = {"swave_12x10": 7.19e-13, "complex": 1.08e-12}
MAP_SYSTEMS = {"swave_12x10": lambda: swave((12, 10, 1)), "complex": complex_system}


@pytest.mark.parametrize("name", sorted(MAP_SYSTEMS))
def test_map_of_every_site_matches_the_dense_inverse(name):
    system = MAP_SYSTEMS[name]()
    energies = MAP_ENERGIES[name]
    tolerance = min(20 * RESTATEMENT_ERROR[name], 1e-10)  # 1.4e-11 / 2.2e-11
    n = system.lattice.size
    for broadening in (None, 0.05):
        g = system.green_map(energies, broadening=broadening)
        assert g.blocks.shape == (n, energies.size, 4, 4) and g.blocks.dtype == np.complex128
        assert g.sites == list(system.lattice.sites()) and np.array_equal(g.energies, energies)
        assert g.info["columns"] == 2 and g.info["hole_columns_derived"]
        exact = dense_local_green(system, np.arange(n), energies + 1j * g.broadening)
        error = relative_error(g.blocks, exact)
        print(name, broadening, g.info["moments"], error.max())
        assert np.all(error <= tolerance), (name, broadening, error.max())
    four = system.green_map(energies, broadening=0.05, _all_columns=True)
    assert four.info["columns"] == 4 and not four.info["hole_columns_derived"]
    assert np.all(relative_error(four.blocks, exact) <= tolerance)


# ------------------------------------------------------------------ a line cut against ldos and green()
@pytest.mark.parametrize("name", sorted(MAP_SYSTEMS))
def test_line_cut_equals_ldos_and_green_site_by_site(name):
    """`ldos` is pinned to the reference's goldens (1e-9 relative).  green() at one site runs the same recurrence
    (test above: the same moments bit for bit), so its blocks differ from the map's only by the order in which the
    host sums the series of M complex terms: at most 4·u·M·Σ|w_n μ_n| in absolute terms (u = 1.1e-16, 4u per complex
    multiply-add), with |μ_n| <= 1 and Σ|w_n| <= 2/Γ (a geometric series of ratio exp(-Γ/a) times 2/a)."""
    system = MAP_SYSTEMS[name]()
    assert system.has_symmetric_spectrum(1e-12)
    energies = np.array([0.3, -0.5, 0.0, 0.1, -0.1, 0.9, 0.3, -0.9, 0.7, 0.5])
    y = 2
    cut = [(x, y, 0) for x in range(system.lattice.shape[0])]
    g = system.green_map(energies, cut)
    assert g.ldos().shape == (len(cut), energies.size)
    bound = 4 * 1.1e-16 * g.info["moments"] * 2 / g.broadening.min()
    for s, site in enumerate(cut):
        expected = np.asarray(system.ldos(site, energies))
        print(name, site, np.abs(g.ldos()[s] / expected - 1).max())
        assert np.allclose(g.ldos()[s], expected, rtol=1e-9, atol=0)
        one = system.green(site, energies)
        assert one.info["moments"] == g.info["moments"]
        print(name, site, np.abs(g.blocks[s] - one.blocks[0]).max(), bound)
        assert np.abs(g.blocks[s] - one.blocks[0]).max() <= bound
        assert np.allclose(g.spin_ldos()[s], one.spin_ldos(), rtol=0, atol=bound)
        assert np.array_equal(g.site(site), g.blocks[s])


# ------------------------------------------------------------------ the perf record
def test_perf_record_of_a_map_call(knobs):
    """Full width: 64 vectors per launch on these small lattices (the width rule: the widest power of two up to 64
    whose vector buffer stays within 96 MB), not the 4 of a green() call; one step launch per moment after the
    zeroth (which green_local_pick reads off the start vectors) and per batch, as bdg_green_moments counts them."""
    system = swave((12, 10, 1))
    g = system.green_map(np.array([0.0, 0.2, 0.4]), broadening=0.1)
    perf = g.info["perf"]
    moments = g.info["moments"]
    assert perf["green_local"] == 2 and perf["green"] == 0 and perf["dict_blocks"] > 0
    assert perf["real_arithmetic"] == 1 and perf["vectors_per_launch"] == 64 and perf["lanes_per_row"] == 32
    batches = -(-120 // 32)  # 32 sites of two columns per batch
    assert perf["launches"] == batches * (moments - 1)
    assert perf["vector_steps"] == (moments - 1) * 240
    assert perf["green_ranges"] == 1 and perf["window_ms"] > 0 and perf["kernel_ms"] > 0 and perf["bytes_per_launch"] > 0
    one = system.green((3, 3, 0), np.array([0.0, 0.2, 0.4]), broadening=0.1)
    assert one.info["perf"]["vectors_per_launch"] <= 8 and one.info["perf"]["green_local"] == 0

    streamed = complex_system()
    knobs.set("BODGE_AMD_DICT", "0")
    g = streamed.green_map(np.array([0.0, 0.2, 0.4]), broadening=0.1)
    perf = g.info["perf"]
    assert perf["green_local"] == 1 and perf["dict_blocks"] == 0 and perf["real_arithmetic"] == 0
    assert perf["vectors_per_launch"] == 64 and perf["lanes_per_row"] == 64  # 30 sites x 2 columns: one batch
    assert perf["launches"] == g.info["moments"] - 1


# ------------------------------------------------------------------ a lattice of some size
@pytest.mark.timeout(300)
def test_64x64_line_cut_against_ldos():
    system = swave((64, 64, 1), mu=0.5, gap=1.0, zeeman=0.0)
    energies = np.linspace(0.0, 1.2, 13)
    cut = [(x, 30, 0) for x in range(0, 64, 2)]
    g = system.green_map(energies, cut)
    assert 1000 <= g.info["moments"] <= 10000 and g.info["perf"]["launches"] == g.info["moments"] - 1
    for x in (0, 15, 31):
        expected = np.asarray(system.ldos(cut[x], energies))
        assert np.allclose(g.ldos()[x], expected, rtol=1e-9, atol=0)
    assert np.abs(g.anomalous()).max() > 1e-3  # a gapped s-wave site has a pair amplitude at every energy
