"""green() on the GPU: the picked recurrence against the dense inverse in every kernel form, against the existing
ldos, reciprocity, the chunked device table, the particle-hole columns, refusals and a 64x64 lattice."""

import numpy as np
import pytest

import bodge_amd as ba

from test_gpu_apply import ARITHMETIC

pytestmark = pytest.mark.gpu

ENERGIES = np.array([-0.4, -0.2, 0.0, 0.2, 0.4, 0.6, 0.8, 1.0, 0.2])  # both signs, unordered, one repeat
SOURCE = (2, 1, 0)
TARGETS = [SOURCE, (3, 1, 0), (0, 4, 0)]  # local, a neighbour, a far site


# ------------------------------------------------------------------ systems (those of the fermi_matrix tests)
def swave(shape=(6, 5, 1), mu=0.5, gap=0.3, zeeman=0.2, hop=-1.0, periodic=False):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    with system as (H, Δ):
        H.set_sites(-mu * ba.σ0 - zeeman * ba.σ3)
        Δ.set_sites(gap * ba.jσ2)
        H.set_bonds(hop * ba.σ0)
        if periodic:
            H.set_edges(hop * ba.σ0)
    return system


def pwave_chiral(shape=(5, 5, 1)):
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


def dwave_bonds(shape=(6, 6, 1), mu=0.4, amplitude=0.3, hop=-1.0):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    spin = ba.dwave()
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -mu * ba.σ0
        for i, j in lattice.bonds():
            H[i, j] = hop * ba.σ0
            Δ[i, j] = amplitude * spin(i, j)
    return system


def ssd_envelope(shape=(6, 6, 1)):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    envelope = ba.ssd(system)
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -0.5 * envelope(i, i) * ba.σ0
            Δ[i, i] = 0.4 * envelope(i, i) * ba.jσ2
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * envelope(i, j) * ba.σ0
    return system


def phases(shape=(5, 6, 1)):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -0.3 * ba.σ0 + 0.1 * ba.σ1
            Δ[i, i] = 0.3 * ba.jσ2
        for i, j in lattice.bonds():
            step = np.subtract(j, i)
            H[i, j] = -np.exp(1j * (0.7 * step[0] + 0.3 * step[1])) * ba.σ0
    return system


SYSTEMS = {
    "swave_zeeman": lambda: swave(),
    "pwave_chiral": pwave_chiral,
    "dwave": dwave_bonds,
    "ssd": ssd_envelope,
    "phases": phases,
}

# Error of the numpy restatement of the algorithm (tests/test_green_host.py: unit vectors, recurrence, picked
# rows, series) against inv(z - H) on these systems with SOURCE, TARGETS and ENERGIES, as measured on the CPU:
# max over the three targets and the two broadening modes, relative to the largest entry of the block.  The
# tolerance of the device result is 20 times that, capped at 1e-10.
RESTATEMENT_ERROR = {"swave_zeeman": 1.53e-12, "pwave_chiral": 7.81e-13, "dwave": 9.82e-13, "ssd": 1.03e-12,
                     "phases": 1.52e-12}


def dense_green(system, source, targets, z):
    """inv(z - H) of the dense matrix (numpy), cut to the blocks (target, source): (T, K, 4, 4)."""
    h = np.asarray(system.matrix("dense"))
    i = system.lattice[source]
    out = np.empty((len(targets), len(z), 4, 4), dtype=np.complex128)
    for k, zk in enumerate(z):
        g = np.linalg.inv(zk * np.eye(h.shape[0]) - h)
        for t, target in enumerate(targets):
            j = system.lattice[target]
            out[t, k] = g[4 * j : 4 * j + 4, 4 * i : 4 * i + 4]
    return out


def relative_error(got, exact):
    return np.array([np.abs(g - e).max() / np.abs(e).max() for g, e in zip(got, exact)])


# ------------------------------------------------------------------ against the dense inverse
@pytest.mark.parametrize("name", sorted(SYSTEMS))
@pytest.mark.parametrize("form", ["dictionary", "streamed"])
@pytest.mark.parametrize("arithmetic", sorted(ARITHMETIC))
def test_blocks_match_the_dense_inverse(name, form, arithmetic, knobs):
    system = SYSTEMS[name]()
    if form == "streamed":
        knobs.set("BODGE_AMD_DICT", "0")
    knobs.update(ARITHMETIC[arithmetic])
    tolerance = min(20 * RESTATEMENT_ERROR[name], 1e-10)
    for broadening in (None, 0.05):
        g = system.green(SOURCE, ENERGIES, TARGETS, broadening=broadening)
        assert g.blocks.shape == (3, ENERGIES.size, 4, 4) and g.blocks.dtype == np.complex128
        assert g.broadening.shape == ENERGIES.shape and np.array_equal(g.energies, ENERGIES)
        exact = dense_green(system, SOURCE, TARGETS, ENERGIES + 1j * g.broadening)
        error = relative_error(g.blocks, exact)
        print(name, form, arithmetic, broadening, g.info["moments"], error)
        assert np.all(error <= tolerance), (name, form, arithmetic, broadening, error)
        perf = g.info["perf"]
        assert perf["green"] in (1, 2) and perf["launches"] == g.info["moments"] - 1
        assert perf["bytes_per_launch"] > 0 and perf["window_ms"] > 0 and perf["kernel_ms"] > 0
        assert perf["vector_steps"] == perf["launches"] * g.info["columns"]
        if form == "streamed":
            assert perf["green"] == 1 and perf["dict_blocks"] == 0
        if arithmetic == "complex_full":
            assert perf["real_arithmetic"] == 0 and perf["ph_packed"] == 0
        if arithmetic.startswith("complex"):
            assert perf["real_arithmetic"] == 0
        if arithmetic.endswith("full"):
            assert perf["ph_packed"] == 0
    if form == "dictionary" and name in ("swave_zeeman", "dwave"):
        assert perf["green"] == 2 and perf["dict_blocks"] > 0
    if arithmetic in ("packed", "real_full") and name in ("swave_zeeman", "dwave", "ssd"):
        assert perf["real_arithmetic"] == 1


def test_targets_may_repeat_and_default_to_the_source():
    system = swave()
    local = system.green(SOURCE, ENERGIES)
    assert local.targets == [SOURCE] and local.blocks.shape == (1, ENERGIES.size, 4, 4)
    twice = system.green(SOURCE, ENERGIES, [(3, 1, 0), SOURCE, (3, 1, 0)])
    assert np.array_equal(twice.blocks[0], twice.blocks[2])
    # (the same moments; the host sums the series in a different order for one target and for two)
    assert np.abs(twice.blocks[1] - local.blocks[0]).max() <= 1e-13 * np.abs(local.blocks).max()
    assert np.allclose(local.ldos(), local.spin_ldos().sum(-1), rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="not the source"):
        twice.ldos(0)


# ------------------------------------------------------------------ against ldos
@pytest.mark.parametrize("name", ["swave_zeeman", "pwave_chiral", "phases"])
def test_ldos_helper_equals_the_existing_ldos(name):
    """`ldos` is pinned to the reference's goldens; on a particle-hole symmetric system its values at E < 0 (from
    the hole rows at |E|) are the electron LDOS at E."""
    system = SYSTEMS[name]()
    assert system.has_symmetric_spectrum(1e-12)
    energies = np.array([0.3, -0.5, 0.0, 0.1, -0.1, 0.9, 0.3, -0.9, 0.7, 0.5])
    expected = np.asarray(system.ldos(SOURCE, energies))
    got = system.green(SOURCE, energies).ldos()
    print(name, np.abs(got / expected - 1).max())
    assert got.shape == expected.shape
    assert np.allclose(got, expected, rtol=1e-9, atol=0)


# ------------------------------------------------------------------ reciprocity
@pytest.mark.parametrize("name", ["swave_zeeman", "dwave"])
def test_reciprocity_on_a_real_symmetric_hamiltonian(name):
    """H real symmetric: G(z) is complex symmetric, G_ji = G_ij^T block by block, from two independent recurrences."""
    system = SYSTEMS[name]()
    assert np.abs(np.asarray(system.matrix("dense")).imag).max() == 0
    i, j = SOURCE, (0, 4, 0)
    forward = system.green(i, ENERGIES, [j]).blocks[0]   # G[j, i]
    backward = system.green(j, ENERGIES, [i]).blocks[0]  # G[i, j]
    defect = np.abs(forward - backward.transpose(0, 2, 1)).max()
    largest = max(np.abs(forward).max(), np.abs(backward).max())
    print(name, defect / largest)
    assert defect <= 1e-12 * largest


# ------------------------------------------------------------------ the device table in ranges, batches
def test_chunked_device_table_is_bit_identical(knobs):
    system = swave((8, 7, 1))
    solver = system._solver()
    scale = 1.01 * system.gershgorin_bound()
    rows = 4 * system.lattice[SOURCE] + np.arange(4)
    targets = np.array([system.lattice[t] for t in TARGETS], dtype=np.int32)
    whole = solver.green_moments(scale, 100, rows, targets)
    assert solver.perf()["green_ranges"] == 1
    assert whole.shape == (100, 3, 4, 4)
    knobs.set("BODGE_AMD_GREEN_TABLE_BYTES", str(30 * 3 * 4 * 4 * 16))  # 30 moments per range
    chunked = solver.green_moments(scale, 100, rows, targets)
    assert solver.perf()["green_ranges"] == 4
    assert np.array_equal(whole, chunked)
    knobs.set("BODGE_AMD_GREEN_TABLE_BYTES", "1")  # (less than one moment: one moment per range)
    single = solver.green_moments(scale, 10, rows, targets)
    assert solver.perf()["green_ranges"] == 10
    assert np.array_equal(whole[:10], single)
    # moment 0 is the unit matrix on the source's own block, 0 elsewhere
    assert np.array_equal(whole[0, 0], np.eye(4)) and not whole[0, 1:].any()


def test_source_rows_in_several_batches():
    """More source rows than a batch holds (lanes override): the batches' columns land side by side in the table."""
    system = swave((8, 7, 1))
    solver = system._solver()
    scale = 1.01 * system.gershgorin_bound()
    rows = np.concatenate([4 * system.lattice[s] + np.arange(4) for s in [SOURCE, (5, 5, 0), (0, 0, 0)]])
    targets = np.array([system.lattice[t] for t in TARGETS], dtype=np.int32)
    wide = solver.green_moments(scale, 64, rows, targets)
    assert solver.perf()["launches"] == 63
    solver.set_lanes_per_row(4)
    narrow = solver.green_moments(scale, 64, rows, targets)
    perf = solver.perf()
    assert perf["lanes_per_row"] == 4 and perf["launches"] == 63 * 2 and perf["vector_steps"] == 63 * 12
    assert np.abs(wide - narrow).max() <= 1e-13
    with pytest.raises(ValueError, match="twice"):
        solver.green_moments(scale, 8, rows, np.array([3, 5, 3], dtype=np.int32))
    with pytest.raises(ValueError, match="out of range"):
        solver.green_moments(scale, 8, rows, np.array([system.lattice.size], dtype=np.int32))
    with pytest.raises(ValueError, match="out of range"):
        solver.green_moments(scale, 8, np.array([4 * system.lattice.size]), targets)


# ------------------------------------------------------------------ columns, refusals
def test_two_and_four_columns_agree():
    system = pwave_chiral((6, 6, 1))
    halved = system.green(SOURCE, ENERGIES, TARGETS)
    four = system.green(SOURCE, ENERGIES, TARGETS, _all_columns=True)
    assert halved.info["columns"] == 2 and halved.info["hole_columns_derived"]
    assert four.info["columns"] == 4 and not four.info["hole_columns_derived"]
    assert np.abs(halved.blocks - four.blocks).max() <= 1e-12 * np.abs(four.blocks).max()


def test_slab_handles_are_refused():
    from bodge_amd.solver import SlabGroup

    system = swave((8, 4, 1))
    scale = 1.01 * system.gershgorin_bound()
    with SlabGroup.from_hamiltonian(system, 2) as group:
        member = group.members[0]
        with pytest.raises(ValueError, match="slab"):
            member.green_moments(scale, 16, np.arange(4), np.array([0], dtype=np.int32))


def test_a_lanczos_run_on_the_handle_is_ended():
    system = swave()
    solver = system._solver()
    solver.lanczos_begin(2, max_iter=64)
    solver.lanczos_advance(2)
    solver.green_moments(1.01 * system.gershgorin_bound(), 16, np.arange(4), np.array([0], dtype=np.int32))
    with pytest.raises(ValueError, match="lanczos_begin"):
        solver.lanczos_advance(1)


# ------------------------------------------------------------------ a lattice of some size
@pytest.mark.timeout(300)
def test_64x64_lattice_against_ldos():
    system = swave((64, 64, 1), mu=0.5, gap=1.0, zeeman=0.0)
    site = (31, 30, 0)
    energies = np.linspace(0.0, 1.2, 13)
    g = system.green(site, energies, [site, (32, 30, 0), (40, 45, 0)])
    assert 1000 <= g.info["moments"] <= 10000
    expected = np.asarray(system.ldos(site, energies))
    assert np.allclose(g.ldos(), expected, rtol=1e-9, atol=0)
    assert np.abs(g.anomalous()).max() > 1e-3  # a gapped s-wave site has a pair amplitude at every energy
    assert np.abs(g.blocks[2]).max() < np.abs(g.blocks[0]).max()
