"""green_states() and spectral_function() without a GPU: the projected recurrence restated in numpy against the dense
P† (z - H)^-1 P, against the Bloch blocks of a torus, the particle-hole relation between a state and its conjugate, the
sum over a complete basis, the host driver on a fake solver, the argument errors and the register budget of the kernels."""

import os
import re
import shutil
import sys

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import green as gr

import green_states_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ algorithm
@pytest.mark.parametrize("name", sorted(cases.SYSTEMS))
@pytest.mark.parametrize("broadening", cases.BROADENINGS)
def test_restatement_matches_the_dense_reference(name, broadening):
    """Measured (cases.RESTATEMENT_ERROR): swave 9.61e-13, complex 8.54e-13, disordered 9.74e-13, cube 1.05e-12, torus
    9.96e-13, each the larger of the two broadening modes; the two state sets share their worst state."""
    for set_name in sorted(cases.STATE_SETS):
        states, z, moments, scale, restated, exact = cases.reference(name, set_name, broadening)
        error = cases.relative_error(restated, exact)
        print(name, set_name, broadening, moments, error.max())
        assert restated.shape == (states.shape[0], z.size, 4, 4)
        assert np.all(error <= cases.tolerance(name)), (name, set_name, broadening, error)
    assert cases.RESTATEMENT_ERROR[name] > 1e-13 and cases.tolerance(name) <= 1e-10


def test_a_state_does_not_depend_on_its_batch():
    system = cases.SYSTEMS["swave"]()
    states = cases.mixed_states(system)
    scale = cases.scale_of(system)
    whole = cases.state_moments(system, states, 64, scale, columns=4, batch=16)
    alone = cases.state_moments(system, states[5:6], 64, scale, columns=4, batch=1)
    assert np.abs(alone[:, 0] - whole[:, 5]).max() <= 1e-15
    # a unit amplitude projects what the picked recurrence of green_map picks
    j = system.lattice.size // 3
    unit = cases.state_moments(system, cases.unit_state(system.lattice, j)[None], 64, scale, columns=4)
    assert np.array_equal(unit[0, 0], np.eye(4))
    h = np.asarray(system.matrix("dense"))[4 * j : 4 * j + 4, 4 * j : 4 * j + 4]
    assert np.abs(unit[1, 0] - h / scale).max() <= 1e-15


@pytest.mark.parametrize("broadening", cases.BROADENINGS)
def test_torus_blocks_of_allowed_momenta_are_the_bloch_blocks(broadening):
    """On the torus |k b> spans an invariant subspace of H for every allowed k: the projected resolvent is the inverse of
    z - H_k (4x4).  Measured: 1.1e-12 relative to the largest entry of a block; held to the restatement's tolerance."""
    system = cases.SYSTEMS["torus"]()
    lattice = system.lattice
    momenta = cases.allowed_momenta(lattice)[[0, 1, 7, 13, 29, 47]]
    z, moments, scale = cases.series(system, broadening)
    mu = cases.state_moments(system, lattice.plane_waves(momenta), moments, scale)
    got = gr.blocks_from_moments(mu, scale, z)
    error = cases.relative_error(got, cases.bloch_green(system, momenta, z))
    print(broadening, moments, error.max())
    assert np.all(error <= cases.tolerance("torus")), error


@pytest.mark.parametrize("name", sorted(cases.SYSTEMS))
def test_hole_columns_follow_from_the_conjugate_state(name):
    """μ_n[q][a][b] = (-1)ⁿ conj μ_n[p][a⊕2][b⊕2] with w_p = conj(w_q), for H = -τx H* τx."""
    system = cases.SYSTEMS[name]()
    assert system.has_symmetric_spectrum(1e-12)
    states = cases.closed_states(system)
    partner = gr._conjugate_partners(states)
    assert partner is not None and partner.tolist() == [0, 2, 1, 4, 3, 5, 6]
    scale = cases.scale_of(system)
    four = cases.state_moments(system, states, 500, scale, columns=4)
    two = cases.state_moments(system, states, 500, scale, columns=2)
    assert two.shape == (500, 7, 4, 2)
    difference = np.abs(gr.hole_columns_of_states(two, partner) - four).max()
    print(name, difference)
    assert difference < 1e-12
    assert gr._conjugate_partners(cases.mixed_states(system)) is None  # (π/2, 0, 0) has no partner there


def test_allowed_momenta_are_a_complete_basis():
    """The N plane waves of the allowed momenta of an open lattice are orthonormal, so summing the blocks over them is
    the trace over sites: the sum of the local blocks (unit amplitudes).  Measured 8e-16 relative; held to 1e-12."""
    system = cases.SYSTEMS["swave"]()
    lattice = system.lattice
    waves = lattice.plane_waves(cases.allowed_momenta(lattice))
    assert waves.shape == (56, 56)
    assert np.abs(waves.conj() @ waves.T - np.eye(56)).max() < 1e-14
    z, _, scale = cases.series(system, 0.2)
    moments = 300
    in_waves = gr.blocks_from_moments(cases.state_moments(system, waves, moments, scale), scale, z).sum(0)
    in_sites = gr.blocks_from_moments(cases.state_moments(system, np.eye(56), moments, scale), scale, z).sum(0)
    difference = np.abs(in_waves - in_sites).max() / np.abs(in_sites).max()
    print(difference)
    assert difference <= 1e-12


def test_plane_waves_of_minus_k_are_the_conjugates_bit_for_bit():
    lattice = ba.CubicLattice((7, 5, 3))
    rng = np.random.default_rng(5)
    momenta = np.concatenate([rng.uniform(-np.pi, np.pi, size=(40, 3)), cases.allowed_momenta(lattice)[:30]])
    waves = lattice.plane_waves(momenta)
    assert waves.shape == (70, 105) and waves.dtype == np.complex128
    assert np.array_equal(lattice.plane_waves(-momenta), np.conj(waves))
    assert np.allclose(np.abs(waves), 1 / np.sqrt(105), rtol=1e-15, atol=0)
    one = lattice.plane_waves(momenta[3])
    assert one.shape == (1, 105) and np.array_equal(one[0], waves[3])
    r = lattice.site_array()
    assert np.allclose(waves[3] * np.sqrt(105), np.exp(1j * (r @ momenta[3])), rtol=0, atol=1e-14)
    with pytest.raises(ValueError, match="plane_waves"):
        lattice.plane_waves(np.zeros((2, 2)))


# ------------------------------------------------------------------ helpers
def synthetic(n_states=3):
    rng = np.random.default_rng(7)
    blocks = rng.normal(size=(n_states, 7, 4, 4)) + 1j * rng.normal(size=(n_states, 7, 4, 4))
    states = rng.normal(size=(n_states, 12)) + 0j
    return gr.GreenStates(blocks, np.linspace(-1, 1, 7), np.full(7, 0.1), states, {"moments": 8})


def test_helpers_are_slices_of_the_blocks():
    g = synthetic()
    assert ba.GreenStates is gr.GreenStates
    assert g.spectral().shape == (3, 7) and g.spin_spectral().shape == (3, 7, 2)
    assert g.spin_density().shape == (3, 7, 3) and g.anomalous().shape == (3, 7, 2, 2)
    assert g.info["moments"] == 8 and g.momenta is None and g.states.shape == (3, 12)
    # the definitions of GreenMap, with the state axis in the place of its site axis
    as_map = gr.GreenMap(g.blocks, g.energies, g.broadening, [(q, 0, 0) for q in range(3)])
    assert np.array_equal(g.spectral(), as_map.ldos())
    assert np.array_equal(g.spin_spectral(), as_map.spin_ldos())
    assert np.array_equal(g.spin_density(), as_map.spin_density())
    assert np.array_equal(g.anomalous(), as_map.anomalous())
    b = g.blocks
    assert np.array_equal(g.spectral(), -(b[:, :, 0, 0] + b[:, :, 1, 1]).imag / np.pi)
    assert np.array_equal(g.spin_spectral()[:, :, 1], -b[:, :, 1, 1].imag / np.pi)
    assert np.array_equal(g.anomalous(), b[:, :, 0:2, 2:4])


# ------------------------------------------------------------------ the host driver on a fake solver
class FakeSolver:
    """Stands in for the device: the numpy restatement behind DeviceSolver.green_state_moments."""

    def __init__(self, system):
        self.system = system
        self.calls = []

    def green_state_moments(self, scale, n_moments, amplitudes, n_components=4):
        amplitudes = np.array(amplitudes)
        self.calls.append((n_moments, amplitudes, n_components))
        return cases.state_moments(self.system, amplitudes, n_moments, scale, columns=n_components)

    def perf(self):
        return {"green_states": 2}


def test_columns_groups_and_results_of_the_host_driver(monkeypatch):
    system = cases.swave((4, 3, 1))
    fake = FakeSolver(system)
    monkeypatch.setattr(system, "_solver", lambda: fake)
    energies = np.array([-0.3, 0.1, 0.5])
    z = energies + 0.2j
    closed = cases.closed_states(system)
    # closed under conjugation, symmetric spectrum: two columns, the hole columns derived
    two = system.green_states(closed, energies, broadening=0.2)
    assert two.blocks.shape == (7, 3, 4, 4) and two.info["columns"] == 2 and two.info["hole_columns_derived"]
    assert len(fake.calls) == 1 and fake.calls[-1][2] == 2 and fake.calls[-1][1].shape == (7, 12)
    assert np.array_equal(two.states, closed) and np.array_equal(two.energies, energies) and two.momenta is None
    exact = cases.dense_state_green(system, closed, z)
    assert cases.relative_error(two.blocks, exact).max() < 1e-10
    # all four columns on request: the same blocks
    four = system.green_states(closed, energies, broadening=0.2, _all_columns=True)
    assert four.info["columns"] == 4 and not four.info["hole_columns_derived"] and fake.calls[-1][2] == 4
    assert np.abs(four.blocks - two.blocks).max() <= 1e-12 * np.abs(two.blocks).max()
    # a state without its conjugate among the states: four columns
    mixed = cases.mixed_states(system)
    got = system.green_states(mixed, energies, broadening=0.2)
    assert got.info["columns"] == 4 and not got.info["hole_columns_derived"] and fake.calls[-1][2] == 4
    assert cases.relative_error(got.blocks, cases.dense_state_green(system, mixed, z)).max() < 1e-10
    # one state, given as (N,); not normalised: the blocks scale with |w|²
    single = system.green_states(3.0 * closed[5], energies, broadening=0.2)
    assert single.blocks.shape == (1, 3, 4, 4) and single.info["columns"] == 2
    assert np.abs(single.blocks[0] - 9.0 * two.blocks[5]).max() <= 1e-12 * np.abs(single.blocks).max()
    # a host table limit of three states' moments: partners stay in one group, a repeated state is computed once per group
    order = [1, 0, 3, 5, 2, 6, 4, 1]  # k, 0, packet, standing, -k, unit, conj(packet), k again
    shuffled = closed[order]
    monkeypatch.setattr(gr, "HOST_TABLE_LIMIT", 3 * two.info["moments"] * 4 * 2 * 16)
    before = len(fake.calls)
    grouped = system.green_states(shuffled, energies, broadening=0.2)
    groups = [c[1] for c in fake.calls[before:]]
    assert [g.shape[0] for g in groups] == [3, 3, 3] and len(grouped.info["perf"]) == 3  # (-k goes again with the second k)
    for rows in groups:  # every group is closed under conjugation
        assert gr._conjugate_partners(rows) is not None
    assert grouped.info["columns"] == 2
    assert np.abs(grouped.blocks - two.blocks[order]).max() <= 1e-12 * np.abs(two.blocks).max()
    assert np.abs(grouped.blocks[0] - grouped.blocks[7]).max() <= 1e-13 * np.abs(two.blocks).max()


def test_spectral_function_is_green_states_of_the_plane_waves(monkeypatch):
    system = cases.swave((4, 3, 1), periodic=(0, 1))
    fake = FakeSolver(system)
    monkeypatch.setattr(system, "_solver", lambda: fake)
    energies = np.array([-0.3, 0.1, 0.5])
    momenta = cases.allowed_momenta(system.lattice)[[0, 5, 7]]
    momenta = np.concatenate([momenta, -momenta[1:]])
    a = system.spectral_function(momenta, energies, broadening=0.2)
    assert np.array_equal(a.momenta, momenta) and a.blocks.shape == (5, 3, 4, 4)
    assert a.info["columns"] == 2 and np.array_equal(a.states, system.lattice.plane_waves(momenta))
    exact = cases.bloch_green(system, momenta, energies + 0.2j)
    assert cases.relative_error(a.blocks, exact).max() < 1e-10
    assert np.all(a.spectral() > 0)
    one = system.spectral_function(momenta[1], energies, broadening=0.2)  # (3,): one momentum, no partner: four columns
    assert one.blocks.shape == (1, 3, 4, 4) and one.info["columns"] == 4 and one.momenta.shape == (1, 3)
    assert np.abs(one.blocks[0] - a.blocks[1]).max() <= 1e-12 * np.abs(a.blocks).max()


def test_argument_errors_are_raised_before_any_device_work(monkeypatch):
    system = cases.swave((4, 4, 1))

    def no_device():
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(system, "_solver", no_device)
    states = cases.closed_states(system)
    bad = states.copy()
    bad[2, 5] = np.nan
    with pytest.raises(ValueError, match="green"):
        system.green_states(np.zeros((0, 16)), [0.1, 0.2], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_states(states, [], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_states(states[:, :15], [0.1, 0.2], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_states(states[0, :15], [0.1, 0.2], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_states(bad, [0.1, 0.2], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_states(np.where(np.isnan(bad), np.inf, bad), [0.1, 0.2], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_states(states, [0.1, 0.2], broadening=[0.1, 0.1, 0.1])
    with pytest.raises(ValueError, match="green"):
        system.green_states(states, [0.1, 0.2], broadening=0.0)
    with pytest.raises(ValueError, match="green"):
        system.green_states(states, [0.1, 100.0], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.green_states(states, [0.1, 0.2], broadening=0.1, moments=0)
    with pytest.raises(ValueError, match="green"):
        system.green_states(states, [0.1, -0.1])  # default broadening: one distinct |E|
    with pytest.raises(ValueError, match="green"):
        system.spectral_function(np.zeros((0, 3)), [0.1, 0.2], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.spectral_function(np.zeros((2, 2)), [0.1, 0.2], broadening=0.1)
    with pytest.raises(ValueError, match="green"):
        system.spectral_function([[0.1, np.nan, 0.0]], [0.1, 0.2], broadening=0.1)
    with pytest.raises(AssertionError, match="device work"):
        system.green_states(states, [0.1, 0.2], broadening=0.1)  # (valid arguments do reach the device)
    with pytest.raises(AssertionError, match="device work"):
        system.spectral_function([0.1, 0.2, 0.0], [0.1, 0.2], broadening=0.1)


# ------------------------------------------------------------------ kernels
@pytest.fixture(scope="module")
def resources():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    return kernel_resources.collect()


def expected_instances():
    names = []
    for mode in ("RealPHMode", "ComplexPHMode", "RealMode", "ComplexMode"):
        names += [f"cheb_family<bdg::{mode}, {rl}, bdg::GreenStateTail>" for rl in (4, 8, 16, 32, 64)]
        lanes = (4, 8, 16, 32) if mode.startswith("Real") else (4, 8, 16, 32, 64)
        names += [f"cheb_family_dict<bdg::{mode}, {rl}, {maxb}, bdg::GreenStateTail>" for rl in lanes for maxb in (3, 5, 7)]
    return names


@pytest.mark.timeout(900)
def test_green_state_kernels_do_not_spill_and_keep_their_occupancy(resources):
    """The eight accumulators of the projection live in a wave-private LDS row, not in registers (held in registers the
    streamed-block form spilled 20 - 68 bytes per lane in every mode and the dictionary form 20 - 36 bytes in
    ComplexPHMode).  As built: no scratch anywhere and 4 waves per SIMD, the register class of the picked kernels; the
    dictionary form needs at most 120 VGPRs, the streamed-block form at most 120 and 128 in ComplexPHMode."""
    emitted = sorted(re.match(r"void bdg::(cheb_family.*)\(bdg::GreenStateTail::Args\)", key).group(1)
                     for key in resources if key.startswith("void bdg::cheb_family") and "bdg::GreenStateTail>" in key)
    assert emitted == sorted(expected_instances())
    for name in emitted:
        row = resources[f"void bdg::{name}(bdg::GreenStateTail::Args)"]
        limit = 128 if name.startswith("cheb_family<bdg::ComplexPHMode") else 120
        assert row["scratch"] == 0 and row["vgpr"] <= limit and row["occupancy"] >= 4, (name, row)
    helpers = [key for key in resources if re.search(r"bdg::green_state_(start|reduce|project)", key)]
    assert len(helpers) == 7  # start, reduce, project<4 .. 64>
    for key in helpers:
        assert resources[key]["scratch"] == 0, key
