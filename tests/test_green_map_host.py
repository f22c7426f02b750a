"""green_map() without a GPU: the full-width picked recurrence restated in numpy against the dense inverse on every
site, the particle-hole moment relation, the helpers' slices, the argument errors and the register budget of the new
kernels."""

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


# ------------------------------------------------------------------ systems and dense oracle (those of test_green_host.py)
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


def dense_local_green(system, indices, z):
    """inv(z - H) of the dense matrix, cut to the diagonal blocks of the sites: (S, K, 4, 4)."""
    h = np.asarray(system.matrix("dense"))
    out = np.empty((len(indices), len(z), 4, 4), dtype=np.complex128)
    for k, zk in enumerate(z):
        g = np.linalg.inv(zk * np.eye(h.shape[0]) - h)
        for s, j in enumerate(indices):
            out[s, k] = g[4 * j : 4 * j + 4, 4 * j : 4 * j + 4]
    return out


def local_moments(system, indices, moments, scale, columns=4, batch=None):
    """The algorithm of bdg_green_local_moments in numpy: the sites go in batches of `batch`; in a batch vector
    v = columns * s + b starts at e_{4 j_s + b}, all vectors run one recurrence, and of every t_n the four rows of
    site j_s are picked from the vectors of slot s only: (M, S, 4, columns)."""
    h = sp.csr_matrix(system.matrix("csr"))
    indices = np.asarray(indices)
    batch = batch or max(1, 64 // columns)
    mu = np.empty((moments, indices.size, 4, columns), dtype=np.complex128)
    for s0 in range(0, indices.size, batch):
        own = indices[s0 : s0 + batch]
        width = own.size * columns
        start = (4 * own[:, None] + np.arange(columns)[None, :]).reshape(-1)  # start row of vector v
        rows = 4 * np.repeat(own, columns)[None, :] + np.arange(4)[:, None]    # [a, v]: row a of the site of vector v
        prev = np.zeros((h.shape[0], width), dtype=np.complex128)
        cur = prev.copy()
        cur[start, np.arange(width)] = 1.0
        for n in range(moments):
            picked = cur[rows, np.arange(width)[None, :]]                      # [a, v]
            mu[n, s0 : s0 + batch] = picked.reshape(4, own.size, columns).transpose(1, 0, 2)
            cur, prev = (1.0 if n == 0 else 2.0) * (h @ cur) / scale - prev, cur
    return mu


def relative_error(got, exact):
    """Per site: max |Δ| over energies and entries, relative to the largest entry of the exact blocks."""
    return np.array([np.abs(g - e).max() / np.abs(e).max() for g, e in zip(got, exact)])


# ------------------------------------------------------------------ algorithm
# Error of this restatement against inv(z - H), as measured: max over all 30 sites and the two broadening modes.  The
# recurrence of a vector is that of `picked_moments` in test_green_host.py, whose error on its three targets is
# 1.53e-12 / 1.18e-12; over every site the maximum is the one below.  The tolerance is 20 times that, and no looser
# than 1e-10.
RESTATEMENT_ERROR = {"swave_real": 1.15e-12, "complex": 1.08e-12}
SYSTEMS = {"swave_real": swave_real, "complex": complex_system}


@pytest.mark.parametrize("name", sorted(SYSTEMS))
@pytest.mark.parametrize("broadening", [None, 0.05])
def test_batched_restatement_matches_the_dense_inverse_on_every_site(name, broadening):
    system = SYSTEMS[name]()
    indices = np.arange(system.lattice.size)
    assert indices.size == 30
    scale = 1.01 * system.gershgorin_bound()
    gamma = gr.reference_broadening(ENERGIES) if broadening is None else np.full(ENERGIES.shape, broadening)
    moments = cheb.moments_for_resolvent(scale, float(gamma.min()), 12)
    z = ENERGIES + 1j * gamma
    mu = local_moments(system, indices, moments, scale)  # 16 sites in the first batch, 14 in the second
    got = gr.blocks_from_moments(mu, scale, z)
    error = relative_error(got, dense_local_green(system, indices, z))
    print(name, broadening, moments, error.max())
    tolerance = min(20 * RESTATEMENT_ERROR[name], 1e-10)  # 2.3e-11 / 2.2e-11
    assert np.all(error <= tolerance), (name, broadening, error)
    # a vector's recurrence does not depend on its neighbours in the batch
    alone = local_moments(system, indices[7:8], 64, scale, batch=1)
    assert np.array_equal(alone[:, 0], mu[:64, 7])


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_derived_hole_columns_equal_the_four_column_moments(name):
    """μ_n[a, b] = (-1)ⁿ conj μ_n[a⊕2, b⊕2] on the local blocks: two start vectors per site give all four columns."""
    system = SYSTEMS[name]()
    assert system.has_symmetric_spectrum(1e-12)
    scale = 1.01 * system.gershgorin_bound()
    indices = np.arange(system.lattice.size)
    four = local_moments(system, indices, 700, scale, columns=4)
    two = local_moments(system, indices, 700, scale, columns=2)
    assert two.shape == (700, 30, 4, 2)
    assert np.abs(gr.hole_columns(two) - four).max() < 1e-12


# ------------------------------------------------------------------ helpers
SITES = [(2, 1, 0), (3, 1, 0), (0, 4, 0)]


def synthetic(sites=SITES):
    rng = np.random.default_rng(7)
    blocks = rng.normal(size=(len(sites), 7, 4, 4)) + 1j * rng.normal(size=(len(sites), 7, 4, 4))
    return gr.GreenMap(blocks, np.linspace(-1, 1, 7), np.full(7, 0.1), list(sites), {"moments": 8})


def test_helpers_are_slices_of_the_blocks():
    g = synthetic()
    assert ba.GreenMap is gr.GreenMap
    assert g.ldos().shape == (3, 7) and g.spin_ldos().shape == (3, 7, 2)
    assert g.spin_density().shape == (3, 7, 3) and g.anomalous().shape == (3, 7, 2, 2)
    assert g.sites == SITES and g.info["moments"] == 8
    for s, coord in enumerate(SITES):
        b = g.blocks[s]
        # the definitions of GreenFunction, site by site
        one = gr.GreenFunction(b[None], g.energies, g.broadening, coord, [coord])
        assert np.array_equal(g.ldos()[s], -(b[:, 0, 0] + b[:, 1, 1]).imag / np.pi)
        assert np.array_equal(g.ldos()[s], one.ldos())
        assert np.array_equal(g.spin_ldos()[s], one.spin_ldos())
        assert np.array_equal(g.spin_ldos()[s, :, 0], -b[:, 0, 0].imag / np.pi)
        assert np.array_equal(g.spin_ldos()[s, :, 1], -b[:, 1, 1].imag / np.pi)
        assert np.allclose(g.spin_density()[s], one.spin_density(), rtol=0, atol=1e-15)
        assert np.allclose(g.spin_density()[s, :, 0], -(b[:, 0, 1] + b[:, 1, 0]).imag / np.pi, rtol=0, atol=1e-15)
        assert np.allclose(g.spin_density()[s, :, 2], g.spin_ldos()[s, :, 0] - g.spin_ldos()[s, :, 1], rtol=0, atol=1e-15)
        assert np.array_equal(g.anomalous()[s], b[:, 0:2, 2:4])
        assert np.array_equal(g.site(coord), b)
    with pytest.raises(ValueError, match="not among"):
        g.site((5, 4, 0))


class FakeSolver:
    """Stands in for the device: the numpy restatement behind DeviceSolver.green_local_moments."""

    def __init__(self, system):
        self.system = system
        self.calls = []

    def green_local_moments(self, scale, n_moments, block_rows, n_components=4):
        block_rows = np.asarray(block_rows)
        assert len(set(block_rows.tolist())) == block_rows.size, "a block row listed twice"
        self.calls.append((n_moments, block_rows.copy(), n_components))
        return local_moments(self.system, block_rows, n_moments, scale, columns=n_components)

    def perf(self):
        return {"green_local": 2}


def test_sites_default_to_index_order_may_repeat_and_go_in_groups(monkeypatch):
    system = swave_real((4, 3, 1))
    fake = FakeSolver(system)
    monkeypatch.setattr(system, "_solver", lambda: fake)
    energies = np.array([-0.3, 0.1, 0.5])
    every = system.green_map(energies, broadening=0.2)
    assert every.sites == list(system.lattice.sites()) and every.blocks.shape == (12, 3, 4, 4)
    assert [system.lattice[c] for c in every.sites] == list(range(12))
    assert every.info["columns"] == 2 and every.info["hole_columns_derived"] and len(fake.calls) == 1
    exact = dense_local_green(system, np.arange(12), energies + 0.2j)
    assert relative_error(every.blocks, exact).max() < 1e-10
    # repeated sites: computed once, returned at every position
    cut = [(1, 2, 0), (3, 0, 0), (1, 2, 0)]
    some = system.green_map(energies, cut, broadening=0.2)
    assert some.sites == cut and fake.calls[-1][1].tolist() == sorted({system.lattice[c] for c in cut})
    assert np.array_equal(some.blocks[0], some.blocks[2])
    assert np.abs(some.blocks[1] - every.site((3, 0, 0))).max() <= 1e-13 * np.abs(every.blocks).max()
    # all four columns on request
    four = system.green_map(energies, cut, broadening=0.2, _all_columns=True)
    assert four.info["columns"] == 4 and fake.calls[-1][2] == 4
    assert np.abs(four.blocks - some.blocks).max() <= 1e-12 * np.abs(some.blocks).max()
    # a host table limit of five sites' moments: groups of five sites, the same blocks
    monkeypatch.setattr(gr, "HOST_TABLE_LIMIT", 5 * every.info["moments"] * 4 * 2 * 16)
    before = len(fake.calls)
    grouped = system.green_map(energies, broadening=0.2)
    assert [c[1].size for c in fake.calls[before:]] == [5, 5, 2] and len(grouped.info["perf"]) == 3
    assert np.abs(grouped.blocks - every.blocks).max() <= 1e-13 * np.abs(every.blocks).max()


def test_argument_errors_are_raised_before_any_device_work(monkeypatch):
    system = swave_real((4, 4, 1))

    def no_device():
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(system, "_solver", no_device)
    sites = [(1, 1, 0), (2, 1, 0)]
    with pytest.raises(ValueError, match="green"):
        system.green_map([0.1, 0.2], [], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_map([], sites, broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_map([0.1, 0.2], sites, broadening=[0.1, 0.1, 0.1])
    with pytest.raises(ValueError, match="green"):
        system.green_map([0.1, 0.2], sites, broadening=0.0)
    with pytest.raises(ValueError, match="green"):
        system.green_map([0.1, 0.2], sites, broadening=[0.1, -0.1])
    with pytest.raises(ValueError, match="green"):
        system.green_map([0.1, 100.0], sites, broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_map([0.1, 0.2], sites, broadening=0.1, moments=0)
    with pytest.raises(ValueError, match="green"):
        system.green_map([0.1, -0.1], sites)  # default broadening: one distinct |E|
    with pytest.raises(ValueError, match="out of bounds"):
        system.green_map([0.1, 0.2], [(1, 1, 0), (4, 0, 0)], broadening=0.1)
    with pytest.raises(AssertionError, match="device work"):
        system.green_map([0.1, 0.2], sites, broadening=0.1)  # (valid arguments do reach the device)


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
    assert len(matches) == 1, (name, [k for k in resources if "green_local" in k][:8])
    return matches[0]


@pytest.mark.timeout(900)
def test_green_local_kernels_do_not_spill_and_keep_their_occupancy(resources):
    """The full-width steps are the picked steps of green() with another store: the same register class (no scratch,
    at most 128 VGPRs, 4 waves per SIMD), in every mode and lane count."""
    for mode in ("RealPHMode", "ComplexPHMode", "RealMode", "ComplexMode"):
        lanes = (4, 8, 16, 32) if mode.startswith("Real") else (4, 8, 16, 32, 64)
        for rl in lanes:
            for maxb in (3, 5, 7):
                row = _row(resources, f"cheb_family_dict<bdg::{mode}, {rl}, {maxb}, bdg::GreenLocalTail>")
                assert row["scratch"] == 0 and row["vgpr"] <= 128 and row["occupancy"] >= 4, (mode, rl, maxb, row)
        for rl in (4, 8, 16, 32, 64):
            row = _row(resources, f"cheb_family<bdg::{mode}, {rl}, bdg::GreenLocalTail>")
            assert row["scratch"] == 0 and row["vgpr"] <= 128 and row["occupancy"] >= 4, (mode, rl, row)
    for per_lane in (1, 2):
        row = _row(resources, f"green_local_pick<{per_lane}>")
        assert row["scratch"] == 0
