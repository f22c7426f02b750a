"""green() without a GPU: the picked recurrence restated in numpy against the dense inverse, the particle-hole
moment relation, the helpers' slices, the argument errors and the register budget of the new kernels."""

import os
import shutil
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import bodge_amd as ba
from bodge_amd import chebyshev as cheb
from bodge_amd import green as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENERGIES = np.array([-0.4, -0.2, 0.0, 0.2, 0.4, 0.6, 0.8, 1.0, 0.2])  # both signs, unordered, one repeat
SOURCE = (2, 1, 0)
TARGETS = [SOURCE, (3, 1, 0), (0, 4, 0)]  # local, a neighbour, a far site


# ------------------------------------------------------------------ systems and dense oracle
def swave_real(shape=(6, 5, 1), mu=0.5, gap=0.3, zeeman=0.2, hop=-1.0):
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


def dense_green(system, source, targets, z):
    """inv(z - H) of the dense matrix, cut to the blocks (target, source): (T, K, 4, 4)."""
    h = np.asarray(system.matrix("dense"))
    i = system.lattice[source]
    out = np.empty((len(targets), len(z), 4, 4), dtype=np.complex128)
    for k, zk in enumerate(z):
        g = np.linalg.inv(zk * np.eye(h.shape[0]) - h)
        for t, target in enumerate(targets):
            j = system.lattice[target]
            out[t, k] = g[4 * j : 4 * j + 4, 4 * i : 4 * i + 4]
    return out


def picked_moments(system, source, targets, moments, scale, columns=4):
    """The algorithm of bdg_green_moments in numpy: unit start vectors e_{4i+b}, the recurrence, the rows of the
    target sites picked from every t_n: (M, T, 4, columns)."""
    h = sp.csr_matrix(system.matrix("csr"))
    i = system.lattice[source]
    rows = np.concatenate([4 * system.lattice[t] + np.arange(4) for t in targets])
    prev = np.zeros((h.shape[0], columns), dtype=np.complex128)
    cur = prev.copy()
    cur[4 * i + np.arange(columns), np.arange(columns)] = 1.0
    mu = np.empty((moments, len(targets), 4, columns), dtype=np.complex128)
    for n in range(moments):
        mu[n] = cur[rows].reshape(len(targets), 4, columns)
        cur, prev = (1.0 if n == 0 else 2.0) * (h @ cur) / scale - prev, cur
    return mu


def relative_error(got, exact):
    """Per target: max |Δ| over energies and entries, relative to the largest entry of the exact blocks."""
    return np.array([np.abs(g - e).max() / np.abs(e).max() for g, e in zip(got, exact)])


# ------------------------------------------------------------------ algorithm
# Error of this restatement against inv(z - H), as measured (max over the three targets and the two broadening
# modes): the truncation of the series at `moments_for_resolvent(a, min Γ, 12)` plus the round-off of M ≈ 10³
# steps.  The tolerance is 20 times that, and no looser than 1e-10.
RESTATEMENT_ERROR = {"swave_real": 1.53e-12, "complex": 1.18e-12}
SYSTEMS = {"swave_real": swave_real, "complex": complex_system}


@pytest.mark.parametrize("name", sorted(SYSTEMS))
@pytest.mark.parametrize("broadening", [None, 0.05])
def test_picked_recurrence_restatement_matches_the_dense_inverse(name, broadening):
    system = SYSTEMS[name]()
    scale = 1.01 * system.gershgorin_bound()
    gamma = gr.reference_broadening(ENERGIES) if broadening is None else np.full(ENERGIES.shape, broadening)
    moments = cheb.moments_for_resolvent(scale, float(gamma.min()), 12)
    z = ENERGIES + 1j * gamma
    mu = picked_moments(system, SOURCE, TARGETS, moments, scale)
    got = gr.blocks_from_moments(mu, scale, z)
    error = relative_error(got, dense_green(system, SOURCE, TARGETS, z))
    print(name, broadening, moments, error)
    tolerance = min(20 * RESTATEMENT_ERROR[name], 1e-10)  # 3.1e-11 / 2.4e-11
    assert np.all(error <= tolerance), (name, broadening, error)
    # the series of the operator is the series of `resolvent_series` entry by entry
    entry = cheb.resolvent_series(mu[:, 1, 2, 3], scale, z[4])
    assert abs(entry - got[1, 4, 2, 3]) <= 1e-14 * np.abs(got).max()


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_particle_hole_columns_equal_the_four_column_moments(name):
    """μ_n[a, b] = (-1)ⁿ conj μ_n[a⊕2, b⊕2]: two start vectors per source site give all four columns."""
    system = SYSTEMS[name]()
    assert system.has_symmetric_spectrum(1e-12)
    scale = 1.01 * system.gershgorin_bound()
    four = picked_moments(system, SOURCE, TARGETS, 700, scale, columns=4)
    two = picked_moments(system, SOURCE, TARGETS, 700, scale, columns=2)
    assert np.abs(gr.hole_columns(two) - four).max() < 1e-12


def test_default_broadening_is_the_rule_of_ldos():
    eps = np.unique(np.abs(ENERGIES))
    gam = np.gradient(eps)
    got = gr.reference_broadening(ENERGIES)
    assert got.shape == ENERGIES.shape
    for e, g in zip(ENERGIES, got):
        assert g == gam[np.flatnonzero(eps == abs(e))[0]]
    with pytest.raises(ValueError, match="green"):
        gr.reference_broadening(np.array([0.3, -0.3, 0.3]))


# ------------------------------------------------------------------ helpers
def synthetic(targets=(SOURCE, (3, 1, 0))):
    rng = np.random.default_rng(5)
    blocks = rng.normal(size=(len(targets), 7, 4, 4)) + 1j * rng.normal(size=(len(targets), 7, 4, 4))
    energies = np.linspace(-1, 1, 7)
    return gr.GreenFunction(blocks, energies, np.full(7, 0.1), SOURCE, list(targets), {"moments": 8})


def test_helpers_are_slices_of_the_blocks():
    g = synthetic()
    b = g.blocks[0]
    assert g.ldos().shape == (7,) and g.spin_ldos().shape == (7, 2)
    assert g.spin_density().shape == (7, 3) and g.anomalous().shape == (7, 2, 2)
    assert np.allclose(g.ldos(), g.spin_ldos().sum(-1), rtol=0, atol=1e-15)
    assert np.allclose(g.spin_density()[:, 2], g.spin_ldos()[:, 0] - g.spin_ldos()[:, 1], rtol=0, atol=1e-15)
    assert np.array_equal(g.spin_ldos()[:, 0], -b[:, 0, 0].imag / np.pi)
    assert np.array_equal(g.spin_ldos()[:, 1], -b[:, 1, 1].imag / np.pi)
    assert np.allclose(g.spin_density()[:, 0], -(b[:, 0, 1] + b[:, 1, 0]).imag / np.pi, rtol=0, atol=1e-15)
    assert np.allclose(g.spin_density()[:, 1], -(1j * b[:, 0, 1] - 1j * b[:, 1, 0]).imag / np.pi, rtol=0, atol=1e-15)
    assert np.array_equal(g.anomalous(), b[:, 0:2, 2:4])
    assert np.array_equal(g.anomalous(1), g.blocks[1][:, 0:2, 2:4])  # (defined for any target)
    assert g.source == SOURCE and g.targets == [SOURCE, (3, 1, 0)] and g.info["moments"] == 8


def test_local_helpers_refuse_a_non_local_target():
    g = synthetic()
    for helper in (g.ldos, g.spin_ldos, g.spin_density):
        with pytest.raises(ValueError, match="not the source"):
            helper(1)


def test_argument_errors_are_raised_before_any_device_work():
    system = swave_real((4, 4, 1))
    site = (1, 1, 0)
    with pytest.raises(ValueError, match="green"):
        system.green(site, [0.1, 0.2], broadening=0.0)
    with pytest.raises(ValueError, match="green"):
        system.green(site, [0.1, 0.2], broadening=[0.1, -0.1])
    with pytest.raises(ValueError, match="green"):
        system.green(site, [0.1, 0.2], broadening=[0.1, 0.1, 0.1])
    with pytest.raises(ValueError, match="green"):
        system.green(site, [0.1, 100.0], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green(site, [0.1, 0.2], targets=[], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green(site, [0.1, -0.1])  # default broadening: one distinct |E|
    assert ba.GreenFunction is gr.GreenFunction


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
    assert len(matches) == 1, (name, [k for k in resources if "green" in k][:8])
    return matches[0]


@pytest.mark.timeout(900)
def test_green_kernels_do_not_spill_and_keep_their_occupancy(resources):
    """The picked steps are the Clenshaw steps with a store of the target rows instead of the source term: the
    same register class (no scratch, at most 128 VGPRs, 4 waves per SIMD), in every mode and lane count."""
    for mode in ("RealPHMode", "ComplexPHMode", "RealMode", "ComplexMode"):
        lanes = (4, 8, 16, 32) if mode.startswith("Real") else (4, 8, 16, 32, 64)
        for rl in lanes:
            for maxb in (3, 5, 7):
                row = _row(resources, f"cheb_family_dict<bdg::{mode}, {rl}, {maxb}, bdg::GreenTail>")
                assert row["scratch"] == 0 and row["vgpr"] <= 128 and row["occupancy"] >= 4, (mode, rl, maxb, row)
        for rl in (4, 8, 16, 32, 64):
            row = _row(resources, f"cheb_family<bdg::{mode}, {rl}, bdg::GreenTail>")
            assert row["scratch"] == 0 and row["vgpr"] <= 128 and row["occupancy"] >= 4, (mode, rl, row)
    for per_lane in (1, 2):
        row = _row(resources, f"green_pick<{per_lane}>")
        assert row["scratch"] == 0
