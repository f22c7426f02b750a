"""green_states() and spectral_function() on the GPU: a unit amplitude against bdg_green_local_moments (bit for bit), the
independence of a state from its batch, every mode and kernel form against the numpy restatement and the dense
reference, several tiles per workgroup, the switches, the API and the perf record."""

import numpy as np
import pytest

from bodge_amd import backend
from bodge_amd import green as gr
from bodge_amd.solver import DeviceSolver

import green_states_cases as cases

pytestmark = pytest.mark.gpu

OTHER_FAMILIES = ("green", "green_local", "clenshaw", "apply", "correlation")


def rounding_bound(moments, n_sites, mu):
    """(32·M + N)·2⁻⁵³·max(1, max|μ|): 32 roundings per entry and step of the recurrence (derived in
    test_gpu_clenshaw_switches.py) and the summation of N products with Σ|w||t| <= 1 for normalised states."""
    return (32 * moments + n_sites) * 2.0**-53 * max(1.0, float(np.abs(mu).max()))


# ------------------------------------------------------------------ 1. a unit amplitude is the picked recurrence
@pytest.mark.parametrize("name", ["swave", "complex", "disordered", "cube"])
@pytest.mark.parametrize("columns", [2, 4])
def test_unit_amplitudes_equal_the_local_moments_bit_for_bit(name, columns, knobs):
    """w = 1 on site j: the recurrence is that of bdg_green_local_moments, conj(1)·x is exact and every other row adds
    an exact zero, through the lanes, the waves and the workgroups (most of which have no tile at all here)."""
    system = cases.SYSTEMS[name]()
    if name == "complex":
        knobs.set("BODGE_AMD_DICT", "0")
    solver = system._solver()
    scale = cases.scale_of(system)
    n = system.lattice.size
    moments, lanes = 160, 8
    sites = np.random.default_rng(3).permutation(n)[:5].astype(np.int32)
    states = np.zeros((sites.size, n), dtype=np.complex128)
    states[np.arange(sites.size), sites] = 1.0
    solver.set_lanes_per_row(lanes)
    try:
        got = solver.green_state_moments(scale, moments, states, columns)
        perf = solver.perf()
        expected_form = 1 if name == "complex" else cases.EXPECTED_FORM[name]
        assert perf["green_states"] == expected_form and perf["lanes_per_row"] == lanes
        assert all(perf[family] == 0 for family in OTHER_FAMILIES)
        tiles = cases.tiles_of(n, lanes)
        assert perf["grid"] > tiles, (perf["grid"], tiles)  # workgroups without a tile write zeros
        assert n % (4 * (64 // lanes)) != 0                 # ... and the last tile is ragged
        batch = lanes // columns
        assert perf["launches"] == -(-sites.size // batch) * (moments - 1)
        assert perf["vector_steps"] == (moments - 1) * sites.size * columns
        local = solver.green_local_moments(scale, moments, sites, columns)
        assert solver.perf()["green_states"] == 0 and solver.perf()["lanes_per_row"] == lanes
        difference = np.abs(got - local).max()
        print(name, columns, perf["grid"], tiles, difference)
        assert got.shape == local.shape == (moments, sites.size, 4, columns)
        assert np.array_equal(got, local), (name, columns, difference)
        assert np.array_equal(got[0, 0], np.eye(4)[:, :columns])
    finally:
        solver.set_lanes_per_row(0)


# ------------------------------------------------------------------ 2. a state does not depend on its batch
@pytest.mark.parametrize("name", ["swave", "disordered"])
@pytest.mark.parametrize("columns", [2, 4])
def test_a_state_does_not_depend_on_its_batch(name, columns):
    system = cases.SYSTEMS[name]()
    solver = system._solver()
    scale = cases.scale_of(system)
    states = cases.mixed_states(system)  # 8 states
    moments, lanes = 120, 8
    batch = lanes // columns             # 4 or 2 states
    solver.set_lanes_per_row(lanes)
    try:
        alone = [solver.green_state_moments(scale, moments, states[q : q + 1], columns)[:, 0] for q in range(8)]
        perf = solver.perf()
        assert perf["launches"] == moments - 1 and perf["vector_steps"] == (moments - 1) * columns
        for order in (np.arange(2 * batch), np.arange(batch + 1), np.arange(8)[::-1], np.array([5, 0, 7])):
            got = solver.green_state_moments(scale, moments, states[order], columns)
            perf = solver.perf()
            assert perf["lanes_per_row"] == lanes and perf["green_states"] == cases.EXPECTED_FORM[name]
            assert perf["launches"] == -(-order.size // batch) * (moments - 1), (perf, order)
            assert perf["vector_steps"] == (moments - 1) * order.size * columns
            for position, q in enumerate(order.tolist()):
                assert np.array_equal(got[:, position], alone[q]), (name, columns, order, position)
    finally:
        solver.set_lanes_per_row(0)


# ------------------------------------------------------------------ 3. every mode and form against the references
@pytest.mark.parametrize("name", sorted(cases.SYSTEMS))
def test_every_mode_and_form_matches_the_restatement_and_the_dense_reference(name, knobs):
    """Tolerance: 20 times the restatement's recorded error against the dense reference, capped at 1e-10
    (cases.tolerance); the distance from the restatement itself is printed."""
    system = cases.SYSTEMS[name]()
    solver = system._solver()
    solver.green_state_moments(cases.scale_of(system), 2, cases.mixed_states(system)[:1], 4)
    plain = solver.perf()
    modes = [(r, p) for r in ((1, 0) if plain["real_arithmetic"] else (0,)) for p in ((1, 0) if plain["ph_packed"] else (0,))]
    forms = (2, 1) if plain["green_states"] == 2 else (1,)
    assert plain["ph_packed"] == 1 and (plain["real_arithmetic"] == 1) == (name != "complex")
    seen = set()
    for set_name in sorted(cases.STATE_SETS):
        states, z, moments, scale, restated, exact = cases.reference(name, set_name, None)
        for form in forms:
            for real, ph in modes:
                knobs.set("BODGE_AMD_DICT", "1" if form == 2 else "0")
                knobs.set("BODGE_AMD_REAL", str(real))
                knobs.set("BODGE_AMD_PH", str(ph))
                mu = solver.green_state_moments(scale, moments, states, 4)
                perf = solver.perf()
                assert (perf["green_states"], perf["real_arithmetic"], perf["ph_packed"]) == (form, real, ph)
                assert perf["lanes_per_row"] == 32 and perf["vectors_per_launch"] == (64 if real else 32)
                assert perf["grid"] > cases.tiles_of(system.lattice.size, 32)  # (workgroups without a tile here too)
                seen.add((form, real, ph))
                got = gr.blocks_from_moments(mu, scale, z)
                error = cases.relative_error(got, exact).max()
                print(name, set_name, form, real, ph, moments, "dense", error, "restatement",
                      cases.relative_error(got, restated).max())
                assert error <= cases.tolerance(name), (name, set_name, form, real, ph, error)
    assert len(seen) == len(forms) * len(modes)


# ------------------------------------------------------------------ 5. several tiles per workgroup
@pytest.mark.timeout(120)
def test_accumulators_are_carried_across_the_tiles_of_a_workgroup(knobs):
    """One workgroup per CU at 4 lanes on 150 x 120 sites: 282 tiles of 64 block rows for at most 256 workgroups, so
    some of them add two tiles into their accumulators.  The partial sums depend on which tiles a workgroup sweeps, so
    neither the default grid nor BODGE_AMD_ALTERNATE=0 gives the same bits: both are held to the rounding bound."""
    system = cases.swave((150, 120, 1))
    lattice = system.lattice
    n = lattice.size
    k = cases.allowed_momentum(lattice)
    states = np.concatenate([lattice.plane_waves(np.array([[0.0, 0.0, 0.0], [np.pi / 2, 0.0, 0.0], k, -k])),
                             [cases.gaussian_packet(lattice, (0.9, -0.4, 0.0), width=9.0), cases.standing_wave(lattice)]])
    assert np.allclose(np.linalg.norm(states, axis=1), 1.0, rtol=1e-12)
    scale = cases.scale_of(system)
    moments, lanes = 40, 4
    expected = cases.state_moments(system, states, moments, scale, columns=4)
    bound = rounding_bound(moments, n, expected)
    solver = system._solver()
    solver.set_lanes_per_row(lanes)
    try:
        default = solver.green_state_moments(scale, moments, states, 4)
        knobs.set("BODGE_AMD_BLOCKS_PER_CU", "1")
        got = solver.green_state_moments(scale, moments, states, 4)
        perf = solver.perf()
        tiles = cases.tiles_of(n, lanes)
        assert tiles == 282 and perf["grid"] < tiles and perf["lanes_per_row"] == lanes, (perf["grid"], tiles)
        assert perf["launches"] == 6 * (moments - 1) and perf["vector_steps"] == (moments - 1) * 24
        knobs.set("BODGE_AMD_ALTERNATE", "0")
        forward = solver.green_state_moments(scale, moments, states, 4)
        for label, result in (("default grid", default), ("one workgroup per CU", got), ("no alternation", forward)):
            difference = np.abs(result - expected).max()
            print(label, difference, bound)
            assert difference <= bound, (label, difference, bound)
    finally:
        solver.set_lanes_per_row(0)


# ------------------------------------------------------------------ 6. switches
@pytest.mark.parametrize("name", ["swave", "disordered"])
def test_switches_do_not_change_a_bit(name, knobs):
    system = cases.SYSTEMS[name]()
    solver = system._solver()
    scale = cases.scale_of(system)
    states = cases.mixed_states(system)
    moments = 100
    whole = solver.green_state_moments(scale, moments, states, 4)
    perf = solver.perf()
    assert perf["green_ranges"] == 1 and whole.shape == (moments, 8, 4, 4)
    for value in ("1", "2", "3"):
        knobs.set("BODGE_AMD_STREAM_VECTORS", value)
        assert np.array_equal(solver.green_state_moments(scale, moments, states, 4), whole), value
    knobs.unset("BODGE_AMD_STREAM_VECTORS")
    # 30 moments of partials and table per range
    per_moment = (perf["grid"] * perf["lanes_per_row"] * 4 + (perf["lanes_per_row"] // 4) * 16) * 16
    knobs.set("BODGE_AMD_GREEN_TABLE_BYTES", str(30 * per_moment))
    chunked = solver.green_state_moments(scale, moments, states, 4)
    assert solver.perf()["green_ranges"] == 4
    assert np.array_equal(whole, chunked)
    knobs.set("BODGE_AMD_GREEN_TABLE_BYTES", "1")  # (less than one moment: one moment per range)
    single = solver.green_state_moments(scale, 10, states, 4)
    assert solver.perf()["green_ranges"] == 10
    assert np.array_equal(whole[:10], single)
    knobs.unset("BODGE_AMD_GREEN_TABLE_BYTES")
    # the other direction of the odd launches hands other tiles to a workgroup: other partial sums
    knobs.set("BODGE_AMD_ALTERNATE", "0")
    forward = solver.green_state_moments(scale, moments, states, 4)
    bound = rounding_bound(moments, system.lattice.size, whole)
    print(name, np.abs(forward - whole).max(), bound)
    assert np.abs(forward - whole).max() <= bound


# ------------------------------------------------------------------ 7. API
def test_spectral_function_of_the_torus_is_the_bloch_green_function():
    system = cases.SYSTEMS["torus"]()
    momenta = cases.allowed_momenta(system.lattice)
    for broadening in cases.BROADENINGS:
        a = system.spectral_function(momenta, cases.ENERGIES, broadening=broadening)
        assert a.blocks.shape == (48, cases.ENERGIES.size, 4, 4) and np.array_equal(a.momenta, momenta)
        exact = cases.bloch_green(system, momenta, cases.ENERGIES + 1j * a.broadening)
        error = cases.relative_error(a.blocks, exact)
        print(broadening, a.info["moments"], error.max())
        assert np.all(error <= cases.tolerance("torus")), error.max()
    assert np.all(a.spectral() > 0) and np.abs(a.anomalous()).max() > 1e-3
    # without the components -π (whose waves have no conjugate among the others) the set is closed under k -> -k
    inner = cases.symmetric_momenta(system.lattice)
    assert inner.shape == (35, 3)
    b = system.spectral_function(inner, cases.ENERGIES, broadening=0.05)
    assert b.info["columns"] == 2 and b.info["hole_columns_derived"]
    error = cases.relative_error(b.blocks, cases.bloch_green(system, inner, cases.ENERGIES + 0.05j))
    print("two columns", error.max())
    assert np.all(error <= cases.tolerance("torus")), error.max()


MAP_RESTATEMENT_ERROR = 1.15e-12  # test_green_map_host.py: the s-wave model's restatement against inv(z - H)


def test_sum_rule_and_column_choice_and_perf_record():
    """Σ_k A(k, ε) over the N allowed momenta of the open 8 x 7 lattice is the trace over sites: Σ_j ldos_j(ε) of
    green_map.  Either call is within its tolerance (relative to the largest entry of each block) of the exact blocks;
    -Im(G00 + G11)/π of a block off by δ is off by at most 2δ/π."""
    system = cases.SYSTEMS["swave"]()
    energies = np.linspace(-1.0, 1.0, 9)
    momenta = cases.allowed_momenta(system.lattice)
    a = system.spectral_function(momenta, energies, broadening=0.05)
    g = system.green_map(energies, broadening=0.05)
    assert a.info["moments"] == g.info["moments"]
    bound = (cases.tolerance("swave") * np.abs(a.blocks).max(axis=(1, 2, 3)).sum() +
             min(20 * MAP_RESTATEMENT_ERROR, 1e-10) * np.abs(g.blocks).max(axis=(1, 2, 3)).sum()) * 2 / np.pi
    difference = np.abs(a.spectral().sum(0) - g.ldos().sum(0)).max()
    print(difference, bound)
    assert difference <= bound
    # two columns (hole columns from the partner -k) against all four: either within its tolerance of the exact blocks
    inner = cases.symmetric_momenta(system.lattice)  # 7 x 7 momenta
    two = system.spectral_function(inner, energies, broadening=0.05)
    assert two.info["columns"] == 2 and two.info["hole_columns_derived"] and two.blocks.shape == (49, 9, 4, 4)
    four = system.spectral_function(inner, energies, broadening=0.05, _all_columns=True)
    assert four.info["columns"] == 4 and not four.info["hole_columns_derived"]
    scale_of_blocks = np.abs(four.blocks).max(axis=(1, 2, 3))
    difference = (np.abs(two.blocks - four.blocks).max(axis=(1, 2, 3)) / scale_of_blocks).max()
    print(difference)
    assert difference <= 2 * cases.tolerance("swave")
    # the perf record: 49 states of two columns in batches of 16 states (32 columns, real arithmetic)
    perf = two.info["perf"]
    moments = two.info["moments"]
    assert perf["green_states"] == 2 and all(perf[family] == 0 for family in OTHER_FAMILIES)
    assert perf["real_arithmetic"] == 1 and perf["lanes_per_row"] == 32 and perf["vectors_per_launch"] == 64
    assert perf["launches"] == 4 * (moments - 1) and perf["vector_steps"] == (moments - 1) * 98
    assert perf["green_ranges"] >= 1 and perf["window_ms"] > 0 and perf["kernel_ms"] > 0
    partials = perf["grid"] * 32 * 4 * 16
    assert perf["bytes_per_launch"] > 16 * 56 * 16 + partials  # amplitudes of 16 states on 56 sites, and the partials
    # complex arithmetic: 64 columns
    other = cases.SYSTEMS["complex"]()
    b = other.green_states(cases.closed_states(other), energies, broadening=0.1, _all_columns=True)
    perf = b.info["perf"]
    assert perf["green_states"] in (1, 2) and perf["real_arithmetic"] == 0 and perf["lanes_per_row"] == 32  # 7 x 4 columns
    wide = other.green_states(np.concatenate([cases.closed_states(other)] * 3), energies, broadening=0.1, _all_columns=True)
    assert wide.info["perf"]["lanes_per_row"] == 64 and wide.info["perf"]["vectors_per_launch"] == 64
    assert wide.info["perf"]["launches"] == 2 * (wide.info["moments"] - 1)  # 21 states x 4 columns: 16 + 5
    assert np.array_equal(wide.blocks[7:14], wide.blocks[0:7])


def test_argument_errors_of_the_entry_point():
    system = cases.SYSTEMS["swave"]()
    solver = system._solver()
    lib = solver._lib
    scale = cases.scale_of(system)
    n = system.lattice.size
    w = np.ones((1, n), dtype=np.complex128)
    out = np.zeros((8, 1, 4, 4), dtype=np.complex128)
    wp, op = backend.as_f64p(w.view(np.float64)), backend.as_f64p(out.view(np.float64))

    def refused(handle, scale_, moments, states, amplitudes, components, result, message):
        assert lib.bdg_green_state_moments(handle, scale_, moments, states, amplitudes, components, result) == -1
        assert message in lib.bdg_last_error().decode(), lib.bdg_last_error()

    refused(None, scale, 8, 1, wp, 4, op, "null system handle")
    refused(solver._handle, scale, 8, 1, None, 4, op, "null argument")
    refused(solver._handle, scale, 8, 1, wp, 4, None, "null argument")
    refused(solver._handle, 0.0, 8, 1, wp, 4, op, "scale")
    refused(solver._handle, float("nan"), 8, 1, wp, 4, op, "scale")
    refused(solver._handle, scale, 0, 1, wp, 4, op, "n_moments")
    refused(solver._handle, scale, 8, 0, wp, 4, op, "n_states")
    refused(solver._handle, scale, 8, 1, wp, 3, op, "n_components")
    assert np.all(out == 0)
    # the order of the checks: the handle before the pointers, the pointers before the numbers
    refused(None, 0.0, 0, 0, None, 3, None, "null system handle")
    refused(solver._handle, 0.0, 0, 0, None, 3, op, "null argument")
    refused(solver._handle, 0.0, 0, 0, wp, 3, op, "scale")
    refused(solver._handle, scale, 0, 0, wp, 3, op, "n_moments")
    refused(solver._handle, scale, 8, 0, wp, 3, op, "n_states")
    # a row slab is refused
    matrix = system.matrix("bsr")
    half = n // 2
    indptr = matrix.indptr[: half + 1]
    slab = DeviceSolver(indptr, matrix.indices[: indptr[-1]], matrix.data[: indptr[-1]], n_cols=n)
    ws = np.ones((1, half), dtype=np.complex128)
    refused(slab._handle, scale, 8, 1, backend.as_f64p(ws.view(np.float64)), 4, op, "slabs are not supported")
    # the Python wrapper's own checks
    with pytest.raises(ValueError, match="green_state_moments"):
        solver.green_state_moments(scale, 8, np.ones((1, n + 1)), 4)
    with pytest.raises(ValueError, match="green_state_moments"):
        solver.green_state_moments(scale, 8, w, 3)
