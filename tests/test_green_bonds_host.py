"""green_bonds() without a GPU: the pattern recurrence restated in numpy against the dense resolvent on every model, the
hole-column rule on off-diagonal blocks, the algebra of `GreenBonds` (local, spectral, sum rule, expectation), the public
function over a stand-in for the device, the argument errors of the function and of the entry point, and the register
budget of the new kernels."""

import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import chebyshev as cheb
from bodge_amd import correlation as corr
from bodge_amd import green as gr

import green_bonds_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = sorted(cases.SYSTEMS)
SYMMETRIC = [name for name in MODELS if name != "periodic"]  # (random_periodic has no particle-hole symmetric blocks)


# ------------------------------------------------------------------ algorithm
@pytest.mark.parametrize("name", MODELS)
def test_restatement_matches_the_dense_resolvent_on_the_whole_skeleton(name):
    """Default moments for Γ = 0.1 (digits = 12).  Measured 2.3e-13 ... 9.7e-13 (cases.RESTATEMENT_ERROR): the pin is
    1e-12, and the recorded figure - the yardstick of the device tolerance - may not understate what is measured."""
    system = cases.system_of(name)
    assert system.has_symmetric_spectrum(1e-12) == (name in SYMMETRIC)
    got, exact = cases.restated(name, 4), cases.dense(name)
    indptr, indices = cases.pattern_of(system)
    assert got.shape == exact.shape == (indices.size, cases.ENERGIES.size, 4, 4)
    d = cases.distance(got, exact)
    print(name, "sites", system.lattice.size, "blocks", indices.size, "moments", cases.moments_of(system), "distance", d)
    assert d <= 1e-12
    assert d <= 1.02 * cases.RESTATEMENT_ERROR[name]
    off = cases.block_rows(indptr) != indices
    if off.any():  # the bonds carry weight of their own: the test is not one of the diagonal alone
        assert np.abs(exact[off]).max() > 1e-2


def test_rows_of_the_models_are_what_the_cases_say():
    """Open d-wave lattice: H has rows of 3, 4 and 5 blocks, the pattern 5 everywhere (zero wrap-around blocks); the
    periodic lattice has blocks of H on its wrap-around pairs; the cube has rows of 7; the single site one block."""
    d = cases.system_of("dwave_open")
    trimmed = np.diff(d.bsr_arrays()[0])
    assert sorted(set(trimmed.tolist())) == [3, 4, 5] and set(np.diff(cases.pattern_of(d)[0]).tolist()) == {5}
    p = cases.system_of("periodic")
    assert set(np.diff(p.bsr_arrays()[0]).tolist()) == {5}
    assert np.diff(cases.pattern_of(cases.system_of("cube"))[0]).max() == 7
    assert np.diff(cases.system_of("cube").bsr_arrays()[0]).max() == 7
    assert cases.pattern_of(cases.system_of("single"))[1].tolist() == [0]
    anomalous = np.abs(np.asarray(d.matrix("dense")).reshape(30, 4, 30, 4)[np.arange(30), :2, np.arange(30), 2:]).max()
    assert anomalous == 0  # the d-wave pairing sits on the bonds


@pytest.mark.parametrize("name", SYMMETRIC)
def test_derived_hole_columns_equal_the_four_column_blocks_off_the_diagonal_too(name):
    """μ_n[a, b] = (-1)ⁿ conj μ_n[a⊕2, b⊕2] block by block: two start vectors per site give all four columns."""
    two, four = cases.restated(name, 2), cases.restated(name, 4)
    print(name, np.abs(two - four).max())
    assert np.abs(two - four).max() <= 1e-14
    system = cases.system_of(name)
    indptr, indices = cases.pattern_of(system)
    mu = cases.bond_moments(system.matrix("csr"), indptr, indices, 40, cases.scale_of(system), 4)
    assert np.abs(gr.hole_columns(mu[..., 0:2]) - mu).max() <= 1e-15


def test_batches_and_partial_patterns_do_not_change_the_restated_moments():
    """A vector's recurrence does not depend on its neighbours in the batch, nor a block on the rest of the pattern."""
    system = cases.system_of("dwave_open")
    h, scale = system.matrix("csr"), cases.scale_of(system)
    indptr, indices = cases.pattern_of(system)
    whole = cases.bond_moments(h, indptr, indices, 48, scale, 2)
    assert np.array_equal(whole, cases.bond_moments(h, indptr, indices, 48, scale, 2, batch=7))
    cut = [system.lattice[(x, 2, 0)] for x in range(6)]
    part_indptr, part_indices = cases.pattern_of(system, cut)
    assert part_indices.size == 30 and set(part_indices.tolist()) == set(cut)
    part = cases.bond_moments(h, part_indptr, part_indices, 48, scale, 2)
    in_whole, in_part = cases.shared_blocks(indptr, indices, part_indptr, part_indices)
    assert in_part.size == 30 and np.array_equal(whole[:, in_whole], part[:, in_part])


# ------------------------------------------------------------------ GreenBonds on restated blocks
def _bonds(name, columns=None):
    system = cases.system_of(name)
    indptr, indices = cases.pattern_of(system, columns)
    if columns is None:
        blocks = np.array(cases.restated(name, 4))
    else:
        blocks = cases.restate(system, indptr, indices, cases.Z, cases.moments_of(system), 4)
    gamma = np.full(cases.ENERGIES.shape, cases.GAMMA)
    return system, gr.GreenBonds(system.lattice, indptr, indices, blocks, cases.ENERGIES, gamma, {"moments": 1})


def test_block_local_and_anomalous_are_slices_of_the_blocks():
    assert ba.GreenBonds is gr.GreenBonds
    system, g = _bonds("dwave_open")
    n = system.lattice.size
    rows = cases.block_rows(g.indptr)
    local = g.local()
    assert isinstance(local, gr.GreenMap) and local.sites == list(system.lattice.sites())
    assert np.array_equal(local.blocks, g.blocks[rows == g.indices]) and local.blocks.shape == (n, 4, 4, 4)
    assert np.all(local.ldos() > 0)
    j, i = (3, 2, 0), (2, 2, 0)
    k = np.flatnonzero((rows == system.lattice[j]) & (g.indices == system.lattice[i]))[0]
    assert np.array_equal(g.block(j, i), g.blocks[k]) and g.block(j, i).shape == (4, 4, 4)
    assert np.array_equal(g.anomalous(j, i), g.blocks[k][:, 0:2, 2:4])
    # d-wave: the pair function changes sign between an x bond and a y bond
    fx, fy = g.anomalous((3, 2, 0), (2, 2, 0)), g.anomalous((2, 3, 0), (2, 2, 0))
    assert np.abs(fx).max() > 1e-3 and np.all(np.real(fx[:, 0, 1] * np.conj(fy[:, 0, 1])) < 0)
    with pytest.raises(IndexError):
        g.block((0, 0, 0), (3, 3, 0))


def test_spectral_is_hermitian_under_the_mirror_and_sums_to_the_lorentzians():
    system, g = _bonds("peierls")
    a = g.spectral()
    mirror = g._find(g.indices.astype(np.int64), cases.block_rows(g.indptr))
    assert np.abs(a - a[mirror].conj().transpose(0, 1, 3, 2)).max() <= 1e-15
    # A = Σ_m |m><m| L_Γ(ε - E_m): ½ tr(A H) over the pattern, which holds every block of H, is ½ Σ_m E_m L_Γ(ε - E_m)
    w = np.linalg.eigvalsh(np.asarray(system.matrix("dense")))
    lorentz = (cases.GAMMA / np.pi) / ((cases.ENERGIES[:, None] - w[None, :]) ** 2 + cases.GAMMA**2)
    value = g.expectation(system)
    assert value.shape == cases.ENERGIES.shape
    assert np.abs(value - 0.5 * lorentz @ w).max() <= 1e-10
    assert np.abs(value - g.expectation(system._data)).max() == 0
    assert np.abs(value - g.expectation(system.matrix("csr"))).max() <= 1e-13


def test_expectation_of_the_current_blocks_is_real():
    for name in ("peierls", "dwave_open"):
        system, g = _bonds(name)
        current = corr.current_operator(system, 0)
        value = g.expectation(current)
        print(name, value)
        assert value.shape == cases.ENERGIES.shape and np.abs(value.imag).max() <= 1e-13
        with pytest.raises(ValueError, match="shape"):
            g.expectation(np.zeros((3, 4, 4)))


def test_spectral_needs_the_mirror_block():
    system = cases.system_of("dwave_open")
    cut = [system.lattice[(x, 2, 0)] for x in range(6)]  # (the y neighbours of the cut are no column sites)
    _, g = _bonds("dwave_open", cut)
    assert g.blocks.shape[0] == 30 and g.local().sites == [(x, 2, 0) for x in range(6)]
    with pytest.raises(IndexError):
        g.spectral()
    with pytest.raises(IndexError):
        g.expectation(np.zeros((30, 4, 4)))


def test_sum_rule_of_the_spectral_blocks_against_dense_fermi():
    """∫ dε f(ε) A_ji(ε) on [-a, a] (trapezoid, step h) against f(H)_ji from eigh.  With A = Σ_m |m><m| L_Γ(ε - E_m) an
    entry is off by at most the largest error of a single level (|entries| <= operator norm), which is at most
      smoothing  |∫_R f(E + x) L_Γ(x) dx - f(E)| <= ∫ min(c x² / 2, ½)·2 L_Γ(x) dx <= c Γ X / π + Γ / (π X) = 2 Γ √c / π
                 at X = 1/√c, c = max |f''| = 1 / (6 √3 T²) (the odd part of f about E cancels under the even L_Γ);
      tails      the weight of L_Γ(ε - E_m) outside [-a, a], f <= 1: (arctan(Γ/(a - E)) + arctan(Γ/(a + E))) / π at the
                 level closest to the ends (the spectrum of the dense reference);
      grid       trapezoid rule on a function analytic in |Im ε| < Γ: 2 M / (exp(2π α / h) - 1) with α = 0.8 Γ and
                 M = ∫ |f L_Γ|(x ± iα) dx <= 1.001 / √(1 - 0.8²) (|f| <= 1 / cos(α / T) there); the end corrections of
                 the finite interval are of order h² L_Γ'(a - E) and far below the rest.
    T = 0.3, Γ = 0.02, h = Γ / 2: 1.32e-2 + 6.4e-3 + 1.4e-4 = 1.97e-2, computed below and not tuned; the error
    measured is 3.9e-3."""
    temperature, gamma = 0.3, 0.02
    system = systems_swave_4x4()
    scale = cases.scale_of(system)
    steps = int(np.ceil(2 * scale / (gamma / 2)))
    energies = np.linspace(-scale, scale, steps + 1)
    h = energies[1] - energies[0]
    w, v = np.linalg.eigh(np.asarray(system.matrix("dense")))
    c = 1.0 / (6 * np.sqrt(3) * temperature**2)
    smoothing = 2 * gamma * np.sqrt(c) / np.pi
    tails = float(np.max(np.arctan(gamma / (scale - w)) + np.arctan(gamma / (scale + w)))) / np.pi
    alpha = 0.8 * gamma
    grid = 2 * (1.0 / np.cos(alpha / temperature)) / np.sqrt(1 - 0.8**2) / np.expm1(2 * np.pi * alpha / h)
    tolerance = smoothing + tails + grid
    print("sum rule tolerance", smoothing, tails, grid)

    indptr, indices = cases.pattern_of(system)
    moments = cheb.moments_for_resolvent(scale, gamma, 12.0)
    mu = cases.bond_moments(system.matrix("csr"), indptr, indices, moments, scale, 4)
    weights = gr.moment_weights(moments, scale, energies + 1j * gamma)
    blocks = (weights @ mu.reshape(moments, -1)).reshape(energies.size, indices.size, 4, 4).transpose(1, 0, 2, 3)
    g = gr.GreenBonds(system.lattice, indptr, indices, blocks, energies, np.full(energies.shape, gamma))
    quadrature = np.full(energies.size, h)
    quadrature[[0, -1]] = h / 2
    integral = np.einsum("e,keab->kab", quadrature * cheb.fermi_function(energies, temperature), g.spectral())
    n = system.lattice.size
    full = (v * cheb.fermi_function(w, temperature)) @ v.conj().T
    exact = full.reshape(n, 4, n, 4)[cases.block_rows(indptr), :, indices.astype(np.int64), :]
    error = np.abs(integral - exact).max()
    print("sum rule", energies.size, "energies", moments, "moments", error, tolerance)
    assert error <= tolerance
    # and ∫ f(ε)·expectation(dH) dε against FermiMatrix.expectation(dH), dH the hopping: the same bound times Σ|dH|/2
    from bodge_amd import fermi

    dh = np.array(system._data)
    dh[cases.block_rows(indptr) == indices] = 0
    fm = fermi.FermiMatrix(system.lattice, indptr, indices, exact, temperature, "dense-numpy")
    value = np.sum(quadrature * cheb.fermi_function(energies, temperature) * g.expectation(dh))
    assert abs(value - fm.expectation(dh)) <= tolerance * 0.5 * np.abs(dh).sum()


def systems_swave_4x4():
    import systems

    return systems.swave_square(ba, L=4, gap=0.3, mu=1.0)


# ------------------------------------------------------------------ the public function over a stand-in for the device
class FakeSolver:
    """Stands in for the device: the numpy restatement behind DeviceSolver.green_bond_blocks."""

    def __init__(self, system):
        self.system = system
        self.calls = []

    def green_bond_blocks(self, scale, weights, indptr, indices, n_components=4):
        assert indptr.dtype == np.int32 and indices.dtype == np.int32 and int(indptr[-1]) == indices.size
        self.calls.append((np.unique(indices), n_components))
        mu = cases.bond_moments(self.system.matrix("csr"), indptr, indices, weights.shape[1], scale, n_components)
        if n_components == 2:
            mu = gr.hole_columns(mu)
        return cases.contract(mu, weights).transpose(1, 0, 2, 3)

    def perf(self):
        return {"green_bonds": 2}


def test_sites_pattern_groups_and_columns_of_the_public_function(monkeypatch):
    system = cases.SYSTEMS["dwave_open"]()
    fake = FakeSolver(system)
    monkeypatch.setattr(system, "_solver", lambda: fake)
    every = system.green_bonds(cases.ENERGIES, broadening=cases.GAMMA)
    indptr, indices = cases.pattern_of(system)
    assert np.array_equal(every.indptr, indptr) and np.array_equal(every.indices, indices)
    assert every.indptr.dtype == np.int32 and every.indices.dtype == np.int32 and every.lattice is system.lattice
    assert every.blocks.shape == (150, 4, 4, 4) and np.array_equal(every.energies, cases.ENERGIES)
    assert every.info["columns"] == 2 and every.info["hole_columns_derived"] and len(fake.calls) == 1
    assert every.info["moments"] == cases.moments_of(system) and every.info["perf"]["green_bonds"] == 2
    assert cases.distance(every.blocks, cases.dense("dwave_open")) <= 20 * cases.RESTATEMENT_ERROR["dwave_open"]
    # a cut, given out of order and with a repeat: the blocks whose column is on the cut, the same numbers
    cut = [(4, 2, 0), (0, 2, 0), (2, 2, 0), (4, 2, 0)]
    some = system.green_bonds(cases.ENERGIES, cut, broadening=cases.GAMMA)
    assert fake.calls[-1][0].tolist() == sorted({system.lattice[c] for c in cut}) and some.blocks.shape[0] == 15
    in_every, in_some = cases.shared_blocks(every.indptr, every.indices, some.indptr, some.indices)
    assert in_some.size == 15 and np.abs(every.blocks[in_every] - some.blocks[in_some]).max() <= 1e-13
    # all four columns on request
    four = system.green_bonds(cases.ENERGIES, cut, broadening=cases.GAMMA, _all_columns=True)
    assert four.info["columns"] == 4 and fake.calls[-1][1] == 4
    assert np.abs(four.blocks - some.blocks).max() <= 1e-13
    # a host limit of 40 blocks' results: groups of 8 sites (5 blocks each), the same blocks
    monkeypatch.setattr(gr, "HOST_TABLE_LIMIT", 40 * cases.ENERGIES.size * 256)
    before = len(fake.calls)
    grouped = system.green_bonds(cases.ENERGIES, broadening=cases.GAMMA)
    assert [c[0].size for c in fake.calls[before:]] == [8, 8, 8, 6] and len(grouped.info["perf"]) == 4
    assert np.abs(grouped.blocks - every.blocks).max() <= 1e-13


def test_argument_errors_are_raised_before_any_device_work(monkeypatch):
    system = cases.SYSTEMS["swave"]()

    def no_device():
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(system, "_solver", no_device)
    sites = [(1, 1, 0), (2, 1, 0)]
    with pytest.raises(ValueError, match="green"):
        system.green_bonds([0.1, 0.2], [], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_bonds([], sites, broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_bonds([0.1, 100.0], sites, broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_bonds([0.1, cases.scale_of(system)], sites, broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_bonds([0.1, 0.2], sites, broadening=[0.1, 0.1, 0.1])
    with pytest.raises(ValueError, match="green"):
        system.green_bonds([0.1, 0.2], sites, broadening=0.0)
    with pytest.raises(ValueError, match="green"):
        system.green_bonds([0.1, 0.2], sites, broadening=0.1, moments=0)
    with pytest.raises(ValueError, match="out of bounds"):
        system.green_bonds([0.1, 0.2], [(1, 1, 0), (6, 0, 0)], broadening=0.1)
    with pytest.raises(AssertionError, match="device work"):
        system.green_bonds([0.1, 0.2], sites, broadening=0.1)  # (valid arguments do reach the device)


def test_entry_point_argument_errors_do_not_need_a_gpu(hip_library):
    """The errors that come before the handle is looked at, in the order of the header."""
    from bodge_amd import backend

    weights = np.zeros(2 * 8)
    indptr = np.array([0, 1], dtype=np.int32)
    indices = np.zeros(1, dtype=np.int32)
    out = np.zeros(32)
    w, p, i, o = backend.as_f64p(weights), backend.as_i32p(indptr), backend.as_i32p(indices), backend.as_f64p(out)

    def call(scale=1.0, n_moments=8, n_weights=1, weights=w, indptr=p, indices=i, components=2, out=o):
        rc = hip_library.bdg_green_bond_blocks(None, scale, n_moments, n_weights, weights, indptr, indices, components, out)
        return rc, hip_library.bdg_last_error()

    assert call(n_moments=0) == (-1, b"n_moments must be >= 1")
    assert call(n_moments=0, n_weights=0, scale=0.0, weights=None)[1] == b"n_moments must be >= 1"
    assert call(n_weights=0, scale=-1.0) == (-1, b"n_weights must be >= 1")
    rc, message = call(n_weights=4 * 65535 + 1, scale=-1.0)
    assert rc == -1 and b"weight rows" in message
    assert call(scale=0.0, weights=None) == (-1, b"scale must be positive")
    assert call(scale=float("nan")) == (-1, b"scale must be positive")
    for name in ("weights", "indptr", "indices", "out"):
        assert call(**{name: None}) == (-1, b"null argument"), name
    assert call(components=3) == (-1, b"null system handle")  # (the pattern and the components need the handle's size)
    assert "bdg_green_bond_blocks" in backend.SIGNATURES and ("green_bonds", ctypes.c_int32) in backend.Perf._fields_


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
    assert len(matches) == 1, (name, [k for k in resources if "GreenBond" in k or "green_bond" in k][:8])
    return matches[0]


@pytest.mark.timeout(900)
def test_green_bond_kernels_keep_the_waves_of_the_local_kernels_without_scratch(resources):
    """The pattern walk sits behind the store of t_{n+1}: it may not cost the tile loop a wave.  Every GreenBondTail
    instance reaches at least the waves per SIMD of the GreenLocalTail instance of the same mode, form, blocks per row
    and lanes, with no scratch (read from the code objects, as tests/test_fermi_host.py does)."""
    pairs = []
    for mode in ("RealPHMode", "ComplexPHMode", "RealMode", "ComplexMode"):
        lanes = (4, 8, 16, 32) if mode.startswith("Real") else (4, 8, 16, 32, 64)
        for rl in lanes:
            for maxb in (3, 5, 7):
                pairs.append(f"cheb_family_dict<bdg::{mode}, {rl}, {maxb}, bdg::%s>")
        for rl in (4, 8, 16, 32, 64):
            pairs.append(f"cheb_family<bdg::{mode}, {rl}, bdg::%s>")
    assert len(pairs) == 74
    for pattern in pairs:
        bond, local = _row(resources, pattern % "GreenBondTail"), _row(resources, pattern % "GreenLocalTail")
        assert bond["scratch"] == 0 and bond["occupancy"] >= local["occupancy"], (pattern, bond, local)
        assert bond["occupancy"] >= 4 and bond["vgpr"] <= 128, (pattern, bond)
    for name in ("green_bond_pick<1>", "green_bond_pick<2>", "green_bond_contract<2>", "green_bond_contract<4>"):
        row = _row(resources, name)
        assert row["scratch"] == 0, (name, row)
