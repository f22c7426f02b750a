"""fermi_matrix on the GPU: probe-Clenshaw blocks against a dense numpy oracle, Hellmann-Feynman against the
existing free_energy, identities, the probing error, the dense route and the argument errors."""

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import chebyshev as cheb

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ systems
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
    "periodic_7x4": lambda: swave((7, 4, 1), periodic=True),
    "cubic_3d": lambda: swave((3, 3, 3), mu=0.2),
}


def dense_fermi(system, temperature):
    """V f(E) V^† of the dense matrix (numpy), cut to the block skeleton."""
    h = np.asarray(system.matrix("dense"))
    w, v = np.linalg.eigh(h)
    full = (v * cheb.fermi_function(w, temperature)) @ v.conj().T
    n = system.lattice.size
    indptr, indices = system._matrix.indptr, system._matrix.indices
    rows = np.repeat(np.arange(n), np.diff(indptr))
    return full.reshape(n, 4, n, 4)[rows, :, indices, :]


# ------------------------------------------------------------------ exact mode
@pytest.mark.parametrize("name", sorted(SYSTEMS))
@pytest.mark.parametrize("form", ["dictionary", "streamed"])
def test_exact_probing_matches_dense(name, form, knobs):
    system = SYSTEMS[name]()
    if form == "streamed":
        knobs.set("BODGE_AMD_DICT", "0")
    for temperature in (0.05, 0.2, 1.0):
        fm = system.fermi_matrix(temperature, method="chebyshev")
        assert fm.method == "chebyshev"
        err = np.abs(fm.blocks - dense_fermi(system, temperature)).max()
        assert err <= 1e-10, (name, form, temperature, err)
        perf = fm.info["perf"]
        assert perf["clenshaw"] in (1, 2) and perf["launches"] > 0 and perf["bytes_moved"] > 0 and perf["window_ms"] > 0
        if form == "streamed":
            assert perf["clenshaw"] == 1 and perf["dict_blocks"] == 0
    if form == "dictionary" and name in ("swave_zeeman", "dwave", "periodic_7x4", "cubic_3d"):
        assert fm.info["perf"]["clenshaw"] == 2 and fm.info["perf"]["dict_blocks"] > 0


def test_complex_arithmetic_of_a_real_matrix_and_all_four_columns(knobs):
    system = swave((6, 6, 1), periodic=True)
    exact = dense_fermi(system, 0.1)
    halved = system.fermi_matrix(0.1, method="chebyshev")
    four = system.fermi_matrix(0.1, method="chebyshev", _all_columns=True)
    assert halved.info["components"] == 2 and four.info["components"] == 4
    assert halved.info["perf"]["real_arithmetic"] == 1
    assert np.abs(four.blocks - exact).max() <= 1e-10
    assert np.abs(four.blocks - halved.blocks).max() <= 1e-10
    knobs.set("BODGE_AMD_REAL", "0")
    knobs.set("BODGE_AMD_PH", "0")
    complex_run = system.fermi_matrix(0.1, method="chebyshev")
    assert complex_run.info["perf"]["real_arithmetic"] == 0 and complex_run.info["perf"]["ph_packed"] == 0
    assert np.abs(complex_run.blocks - exact).max() <= 1e-10


def test_batches_side_by_side_and_lanes_override():
    """Many colours: several batches on the handle's stream sets; a lanes override narrows the batches."""
    system = swave((10, 9, 1), periodic=True)
    exact = dense_fermi(system, 0.3)
    wide = system.fermi_matrix(0.3, method="chebyshev")
    assert wide.info["perf"]["launches"] > wide.info["moments"]  # more than one batch
    assert np.abs(wide.blocks - exact).max() <= 1e-10
    system._solver().set_lanes_per_row(4)
    narrow = system.fermi_matrix(0.3, method="chebyshev")
    assert narrow.info["perf"]["lanes_per_row"] == 4
    assert np.abs(narrow.blocks - exact).max() <= 1e-10


def test_colours_shared_over_devices():
    system = swave((6, 6, 1))
    one = system.fermi_matrix(0.2, method="chebyshev")
    two = system.fermi_matrix(0.2, method="chebyshev", devices=[0, 0])
    assert np.abs(one.blocks - two.blocks).max() <= 1e-12


# ------------------------------------------------------------------ Hellmann-Feynman
def _derivative(build, temperature, step=1e-5):
    plus = build(step).free_energy(temperature, method="dense")
    minus = build(-step).free_energy(temperature, method="dense")
    return (plus - minus) / (2 * step)


@pytest.mark.parametrize("temperature", [0.1, 0.5])
def test_expectation_is_the_derivative_of_the_free_energy(temperature):
    """dF/dλ = ½ tr(f(H) ∂H/∂λ) - ¼ tr ∂H/∂λ, the last term 0 for particle-hole symmetric ∂H."""
    cases = {
        "mu": (lambda x: dwave_bonds(mu=0.4 + x), lambda: dwave_bonds(mu=1.0, amplitude=0.0, hop=0.0)),
        "t": (lambda x: dwave_bonds(hop=-1.0 + x), lambda: dwave_bonds(mu=0.0, amplitude=0.0, hop=1.0)),
        "d-wave": (lambda x: dwave_bonds(amplitude=0.3 + x), lambda: dwave_bonds(mu=0.0, amplitude=1.0, hop=0.0)),
    }
    for label, (build, derivative_of_h) in cases.items():
        fm = build(0.0).fermi_matrix(temperature, method="chebyshev")
        value = fm.expectation(derivative_of_h())
        reference = _derivative(build, temperature)
        assert abs(value.imag) < 1e-10
        assert abs(value.real - reference) <= 1e-6 * abs(reference), (label, value, reference)


# ------------------------------------------------------------------ identities
def test_trace_hermiticity_and_particle_hole_relation():
    system = pwave_chiral((6, 6, 1))
    fm = system.fermi_matrix(0.1, method="chebyshev", _all_columns=True)
    n = system.lattice.size
    diag = fm.blocks[fm._diag]
    assert abs(np.trace(diag, axis1=1, axis2=2).sum() - 2 * n) <= 1e-10 * n
    rows = np.repeat(np.arange(n), np.diff(fm.indptr))
    mirror = fm._find(fm.indices.astype(np.int64), rows)
    assert np.abs(fm.blocks - fm.blocks[mirror].conj().transpose(0, 2, 1)).max() <= 1e-10
    flip = [2, 3, 0, 1]
    relation = -fm.blocks[:, flip][:, :, flip].conj()
    relation[fm._diag] += np.eye(4)
    assert np.abs(fm.blocks - relation).max() <= 1e-10


def test_helpers_on_a_self_consistent_update():
    system = swave((8, 8, 1), mu=0.5, gap=0.3, zeeman=0.0)
    fm = system.fermi_matrix(0.1, method="chebyshev")
    pair = fm.pair_amplitude()
    assert pair.shape == (64,) and np.all(np.abs(pair) > 1e-3)
    assert np.allclose(fm.magnetization(), 0.0, atol=1e-10)
    assert np.all((fm.density() > 0) & (fm.density() < 2))
    assert np.allclose(fm.pairing((1, 1, 0), (1, 2, 0)), fm.block((1, 1, 0), (1, 2, 0))[0:2, 2:4])


# ------------------------------------------------------------------ probing error
# 32x32 gapped s-wave (μ = 0.5, Δ = 1) at T = 0.05; colour periods 4, 8, 16 and 32 (divisors of 32; 32 = one
# site per colour).  Max |Δblock| against the exact result, as measured, pinned with a margin
# of 2.  The reference is the exact mode (distance=None), which the tests above hold to 1e-10 of dense f(H):
# a numpy eigensolve of this 4096-row matrix takes minutes.
PROBING_ERRORS = {3: 1.82e-2, 5: 2.20e-3, 9: 1.39e-5, 17: 0.0}


def test_probing_error_falls_with_distance():
    system = swave((32, 32, 1), mu=0.5, gap=1.0, zeeman=0.0)
    exact = system.fermi_matrix(0.05, method="chebyshev").blocks
    errors = []
    for d in sorted(PROBING_ERRORS):
        fm = system.fermi_matrix(0.05, method="chebyshev", distance=d)
        errors.append(np.abs(fm.blocks - exact).max())
        assert errors[-1] <= 2 * PROBING_ERRORS[d] + 1e-12, (d, errors[-1])
        assert errors[-1] >= PROBING_ERRORS[d] / 2, (d, errors[-1])
    assert errors[0] > errors[1] > errors[2] and errors[3] <= 1e-12, errors


# ------------------------------------------------------------------ dense route
def test_dense_and_chebyshev_routes_agree():
    system = dwave_bonds((5, 5, 1))
    cheb_route = system.fermi_matrix(0.1, method="chebyshev")
    dense_route = system.fermi_matrix(0.1, method="dense")
    auto = system.fermi_matrix(0.1)
    assert dense_route.method == "dense" and auto.method == "dense"
    assert np.abs(cheb_route.blocks - dense_route.blocks).max() <= 1e-10
    assert np.abs(dense_route.blocks - dense_fermi(system, 0.1)).max() <= 1e-10


def test_zero_temperature_gives_one_half_on_exact_zero_modes():
    lattice = ba.CubicLattice((4, 1, 1))
    system = ba.Hamiltonian(lattice)
    with system as (H, Δ):
        for x in range(1, 4):
            H[(x, 0, 0), (x, 0, 0)] = -0.7 * ba.σ0
            Δ[(x, 0, 0), (x, 0, 0)] = 0.2 * ba.jσ2
    fm = system.fermi_matrix(0.0)
    assert fm.method == "dense"
    assert np.abs(fm.block((0, 0, 0), (0, 0, 0)) - 0.5 * np.eye(4)).max() <= 1e-12
    h = np.asarray(system.matrix("dense"))[4:8, 4:8]
    w, v = np.linalg.eigh(h)
    expected = (v * (w < 0)) @ v.conj().T
    assert np.abs(fm.block((1, 0, 0), (1, 0, 0)) - expected).max() <= 1e-12


# ------------------------------------------------------------------ errors
def test_argument_errors():
    system = swave((4, 4, 1))
    with pytest.raises(ValueError):
        system.fermi_matrix(0.0, method="chebyshev")
    with pytest.raises(ValueError):
        system.fermi_matrix(-0.1, method="chebyshev")
    with pytest.raises(ValueError):
        system.fermi_matrix(-0.1, method="dense")
    with pytest.raises(ValueError):
        system.fermi_matrix(-0.1)
    with pytest.raises(ValueError):
        system.fermi_matrix(0.1, method="chebyshev", distance=2)
    with pytest.raises(ValueError):
        system.fermi_matrix(0.1, method="lanczos")


def test_slab_handles_are_refused():
    from bodge_amd.solver import SlabGroup

    system = swave((8, 4, 1))
    scale = 1.01 * system.gershgorin_bound()
    coef = cheb.chebyshev_coefficients(lambda x: cheb.fermi_function(scale * x, 0.5), 64)
    with SlabGroup.from_hamiltonian(system, 2) as group:
        member = group.members[0]
        n = member.n_sites
        indptr = np.arange(n + 1, dtype=np.int32)
        indices = np.arange(n, dtype=np.int32)
        with pytest.raises(ValueError, match="slab"):
            member.fermi_blocks(scale, coef, np.zeros(n, dtype=np.int32), 1, 2, indptr, indices)
