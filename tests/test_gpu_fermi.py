"""fermi_matrix on the GPU: probe-Clenshaw blocks against a dense numpy oracle, Hellmann-Feynman against the
existing free_energy, identities, the probing error, the dense route and the argument errors; bdg_fermi_blocks with
arbitrary colourings, patterns and coefficients against the numpy restatement and the dense probed blocks of
tests/fermi_cases.py in every kernel form, arithmetic mode and lane width, its batches bit for bit, and its refusals."""

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import chebyshev as cheb
from bodge_amd import fermi

import fermi_cases as cases
from test_gpu_apply import ARITHMETIC

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ systems (tests/fermi_cases.py)
swave, pwave_chiral, dwave_bonds, ssd_envelope, phases = (cases.swave, cases.pwave_chiral, cases.dwave_bonds,
                                                          cases.ssd_envelope, cases.phases)
SYSTEMS = cases.EXACT_MODE_SYSTEMS


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


# ------------------------------------------------------------------ arbitrary colourings against two references
# bdg_fermi_blocks through solver.fermi_blocks with colourings that respect no distance (tests/fermi_cases.py): the result
# is then far from f(H), but it is exactly the sum of f(H)'s columns over the sites of one colour, and both references
# say what that is - the numpy restatement of the probed recurrence (sparse H) and V f(E) V† times the probe matrix from
# numpy.linalg.eigh.  The tolerance of the device result is 20 times the distance of the two references, one number per
# (system, temperature): the largest over the system's colourings (fermi_cases.TOLERANCE_COLOURINGS), measured in the
# test, never per sub-case - the docstring of test_gpu_correlation.test_gram_kernel_shapes tells how a per-case
# measurement degenerates by luck.  The pin of tests/test_fermi_host.py (1e-12) is asserted first.
T = cases.TEMPERATURE


def _tolerance(name, keys=cases.TOLERANCE_COLOURINGS):
    own = cases.reference_distance(name, T, keys)
    assert own <= 1e-12, (name, own)
    return 20 * own


def _hold(label, got, restated, dense, tolerance):
    to_restated, to_dense = np.abs(got - restated).max(initial=0.0), np.abs(got - dense).max(initial=0.0)
    print(*label, "device - restated", to_restated, "device - dense", to_dense, "tolerance", tolerance)
    assert to_restated <= tolerance and to_dense <= tolerance, (label, to_restated, to_dense, tolerance)


def _fresh_system(name, form, arithmetic, knobs):
    knobs.update(ARITHMETIC[arithmetic])
    if form == "streamed":
        knobs.set("BODGE_AMD_DICT", "0")
    return cases.SYSTEMS[name]()  # (a fresh handle: the dictionary switch is read at upload)


def _assert_plan(perf, system, name, form, arithmetic, n_colours, components, moments, lanes_override=0):
    """The perf record of a bdg_fermi_blocks call: form, arithmetic, lanes and batches as run_fermi_blocks derives them."""
    real = cases.is_real(system) and "complex" not in arithmetic
    lanes, _, batches = cases.batch_plan(real, n_colours, components, lanes_override)
    assert perf["real_arithmetic"] == (1 if real else 0)
    assert perf["ph_packed"] == (0 if arithmetic.endswith("full") else int(cases.is_particle_hole_packed(system)))
    assert perf["lanes_per_row"] == lanes and perf["vectors_per_launch"] == lanes * (2 if real else 1)
    assert perf["launches"] == batches * moments, (perf["launches"], batches, moments)
    assert perf["vector_steps"] == moments * components * n_colours
    assert perf["grid"] >= cases.tiles_of(system.lattice.size, lanes)  # one tile per workgroup
    assert perf["apply"] == perf["green"] == perf["green_local"] == 0
    # (no dictionary kernel in real arithmetic at 64 lanes, as for the one-step kernels: the streamed form runs)
    if form == "streamed" or name == "disordered_300" or (real and lanes == 64):
        assert perf["clenshaw"] == 1 and perf["dict_blocks"] == 0
    elif name in cases.DICTIONARY_SYSTEMS:
        assert perf["clenshaw"] == 2 and perf["dict_blocks"] > 0
    else:
        assert perf["clenshaw"] in (1, 2)
    return batches


@pytest.mark.parametrize("name", cases.REFERENCE_SYSTEMS)
@pytest.mark.parametrize("form", ["dictionary", "streamed"])
@pytest.mark.parametrize("arithmetic", sorted(ARITHMETIC))
def test_random_colourings_match_restatement_and_dense(name, form, arithmetic, knobs):
    """Several sites per colour, adjacent ones included, sites that are not probed, empty colours: 1 colour (one batch
    with padding lanes), 5 colours, 33 colours (2 components: 66 vectors in two batches, the last with one colour;
    4 components: 132 vectors in three batches on two streams), in every arithmetic mode and both kernel forms."""
    system = _fresh_system(name, form, arithmetic, knobs)
    solver = system._solver()
    scale = cases.scale_of(system)
    coef = cases.fermi_coefficients(system, T)
    indptr, indices = cases.pattern_of(system)
    tolerance = _tolerance(name)
    for n_colours in cases.COLOUR_COUNTS:
        key = ("random", n_colours, 0)
        colours, _ = cases.colouring(name, key)
        restated, dense, _, _ = cases.references(name, T, key)
        for components in (2, 4):
            got = solver.fermi_blocks(scale, coef, colours, n_colours, components, indptr, indices)
            expected = (restated, dense) if components == 4 else (cases.two_components(restated), cases.two_components(dense))
            _hold((name, form, arithmetic, n_colours, components), got, *expected, tolerance)
            assert not got[colours[indices] < 0].any()  # not probed: exactly zero
            assert not got[:, :, components:].any()
            batches = _assert_plan(solver.perf(), system, name, form, arithmetic, n_colours, components, len(coef))
            if n_colours == 33:
                assert batches == (3 if components == 4 else 2) and solver.perf()["streams"] == 2


@pytest.mark.parametrize("name", ["dictionary", "disordered_complex"])
@pytest.mark.parametrize("form", ["dictionary", "streamed"])
@pytest.mark.parametrize("lanes", [4, 8, 16, 32, 64])
def test_lane_widths_match_restatement_and_dense(name, form, lanes, knobs):
    """set_lanes_per_row fixes the lanes and narrows the batches: 33 colours in 4 components are 33 batches of one colour
    at 4 complex lanes and 3 batches at 64.  `dictionary` is a real matrix: two vectors per lane, and at 64 lanes the
    streamed form although the matrix has a dictionary (there is no real dictionary kernel of that width)."""
    system = _fresh_system(name, form, "packed", knobs)
    solver = system._solver()
    scale = cases.scale_of(system)
    coef = cases.fermi_coefficients(system, T)
    indptr, indices = cases.pattern_of(system)
    tolerance = _tolerance(name)
    solver.set_lanes_per_row(lanes)
    try:
        for n_colours, components in ((5, 2), (33, 4)):
            key = ("random", n_colours, 0)
            colours, _ = cases.colouring(name, key)
            restated, dense, _, _ = cases.references(name, T, key)
            got = solver.fermi_blocks(scale, coef, colours, n_colours, components, indptr, indices)
            expected = (restated, dense) if components == 4 else (cases.two_components(restated), cases.two_components(dense))
            _hold((name, form, lanes, n_colours, components), got, *expected, tolerance)
            perf = solver.perf()
            assert perf["lanes_per_row"] == lanes
            _assert_plan(perf, system, name, form, "packed", n_colours, components, len(coef), lanes_override=lanes)
    finally:
        solver.set_lanes_per_row(0)
    if name == "dictionary":
        assert perf["real_arithmetic"] == 1 and perf["clenshaw"] == (1 if form == "streamed" or lanes == 64 else 2)


@pytest.mark.parametrize("name", ["dictionary", "disordered_complex"])
@pytest.mark.parametrize("components", [2, 4])
def test_probed_columns_do_not_depend_on_their_batch(name, components):
    """The recurrence of a probe does not depend on its neighbours in the batch (the twin of test_gpu_apply.
    test_columns_do_not_depend_on_their_batch): the sites of one colour probed alone, as one of 5 colours, as one of 33
    (colour 17: inside a full batch, colour 32: alone in the ragged last batch) and with all
    other colours marked -1 give the same bits on the blocks of that colour, whatever the lanes (4 .. 64) and the
    batch the colour lands in.  Two identical calls are bit-identical."""
    system = cases.SYSTEMS[name]()
    solver = system._solver()
    scale = cases.scale_of(system)
    coef = cases.fermi_coefficients(system, T)
    indptr, indices = cases.pattern_of(system)
    n = system.lattice.size
    among33, _ = cases.colouring(name, ("random", 33, 0))
    many = solver.fermi_blocks(scale, coef, among33, 33, components, indptr, indices)
    wide_lanes = solver.perf()["lanes_per_row"]
    assert np.array_equal(many, solver.fermi_blocks(scale, coef, among33, 33, components, indptr, indices))
    rng = np.random.default_rng(4)
    for colour in (17, 32):
        members = among33 == colour
        assert members.any()
        mine = members[indices]
        among5 = np.where(members, 3, rng.choice(np.array([-1, 0, 1, 2, 4]), n)).astype(np.int32)
        five = solver.fermi_blocks(scale, coef, among5, 5, components, indptr, indices)
        alone = solver.fermi_blocks(scale, coef, np.where(members, 0, -1), 1, components, indptr, indices)
        assert solver.perf()["lanes_per_row"] == 4 < wide_lanes
        others_off = solver.fermi_blocks(scale, coef, np.where(members, colour, -1), 33, components, indptr, indices)
        assert solver.perf()["lanes_per_row"] == wide_lanes
        assert not others_off[~mine].any() and not alone[~mine].any() and np.abs(many[mine]).max() > 0.1
        print(name, components, colour, int(members.sum()), np.abs(many[mine] - alone[mine]).max(),
              np.abs(many[mine] - five[mine]).max(), np.abs(many[mine] - others_off[mine]).max())
        assert np.array_equal(many[mine], alone[mine])
        assert np.array_equal(many[mine], five[mine])
        assert np.array_equal(many[mine], others_off[mine])


@pytest.mark.parametrize("name", ["dictionary", "disordered_complex"])
@pytest.mark.parametrize("components", [2, 4])
def test_shared_out_colours_add_up_bit_for_bit(name, components):
    """How `devices=[...]` shares the work (fermi._fermi_blocks_devices): contiguous ranges of the colours renumbered from
    0, every other site marked -1.  Every block is filled by exactly one part and a probe does not depend on its batch,
    so the parts add up to the one-call result bit for bit, unequal ranges included; the middle part is held to the
    references as well."""
    system = cases.SYSTEMS[name]()
    solver = system._solver()
    scale = cases.scale_of(system)
    coef = cases.fermi_coefficients(system, T)
    indptr, indices = cases.pattern_of(system)
    colours, n_colours = cases.colouring(name, ("random", 33, 0))
    whole = solver.fermi_blocks(scale, coef, colours, n_colours, components, indptr, indices)
    total = np.zeros_like(whole)
    for lo, hi in ((0, 9), (9, 21), (21, 33)):
        mine, count = cases.shared_out_colours(colours, n_colours, lo, hi)
        part = solver.fermi_blocks(scale, coef, mine, count, components, indptr, indices)
        assert not part[mine[indices] < 0].any() and solver.perf()["vector_steps"] == len(coef) * components * count
        if (lo, hi) == (9, 21):
            restated, dense, _, _ = cases.references(name, T, ("shared", 33, 0, 9, 21))
            expected = (restated, dense) if components == 4 else (cases.two_components(restated), cases.two_components(dense))
            _hold((name, components, "colours 9 .. 20"), part, *expected, _tolerance(name))
        total += part
    assert np.array_equal(total, whole)


DISTANCE_KEYS = (("distance", 3), ("distance", 5))


@pytest.mark.parametrize("distance,n_colours", [(3, 9), (5, 36)])
def test_finite_distance_matches_dense_probed_blocks(distance, n_colours):
    """The real `distance` path of fermi_matrix on a 12x12 gapped s-wave lattice (periods 3 and 6: 16 and 4 sites per
    colour) against the references with fermi.site_colours' colouring, after the particle-hole columns: the probing
    error itself (test_probing_error_falls_with_distance) is in the references as it is in the device result."""
    name = "gapped_12x12"
    system = cases.SYSTEMS[name]()
    fm = system.fermi_matrix(T, method="chebyshev", distance=distance)
    assert fm.info["colours"] == n_colours and fm.info["components"] == 2 and fm.info["distance"] == distance
    key = ("distance", distance)
    colours, count = fermi.site_colours(system, distance)
    assert count == n_colours and np.array_equal(colours, cases.colouring(name, key)[0])
    indptr, indices = cases.pattern_of(system)
    diag = np.flatnonzero(np.repeat(np.arange(system.lattice.size), np.diff(indptr)) == indices)
    expected = []
    for reference in cases.references(name, T, key)[:2]:
        blocks = cases.two_components(reference)
        fermi._particle_hole_columns(blocks, diag)
        expected.append(blocks)
    assert fm.info["moments"] == len(cases.fermi_coefficients(system, T))
    _hold((name, distance), fm.blocks, *expected, _tolerance(name, DISTANCE_KEYS))
    _assert_plan(fm.info["perf"], system, name, "dictionary", "packed", n_colours, 2, fm.info["moments"])


def _odd_pattern(n):
    """Not H's skeleton: empty rows (most of them, the first included), a far pair, a column twice in one row, columns
    in no order, the last row."""
    rows = {1: [5, n - 1, 5], 3: [0], 4: [4], n - 1: [n - 1, 0, 2]}
    indptr = np.zeros(n + 1, dtype=np.int32)
    for j, columns in rows.items():
        indptr[j + 1] = len(columns)
    return np.cumsum(indptr, dtype=np.int32), np.concatenate([rows[j] for j in sorted(rows)]).astype(np.int32)


@pytest.mark.parametrize("name", ["dictionary", "disordered_complex"])
@pytest.mark.parametrize("series", ["fermi", "one_coefficient", "two_coefficients", "unit_7"])
def test_patterns_and_short_series(name, series):
    """A pattern that is not H's skeleton, and series of one coefficient (no recurrence launch but the last: the result
    is c_0 on the probes, exactly), of two, and the single unit coefficient e_7, whose result is T_7(H/scale) on the
    probes (the dense polynomial from eigh).  The tolerance is the system's (above): measured on these few entries, or on
    a series of one term, the distance of the references is a few units in the last place or zero."""
    system = cases.SYSTEMS[name]()
    solver = system._solver()
    scale = cases.scale_of(system)
    full = cases.fermi_coefficients(system, T)
    coef = {"fermi": full, "one_coefficient": full[:1], "two_coefficients": full[:2], "unit_7": np.eye(8)[7]}[series]
    colours, n_colours = cases.colouring(name, ("random", 5, 0))
    tolerance = _tolerance(name)
    for label, (indptr, indices) in (("odd", _odd_pattern(system.lattice.size)), ("skeleton", cases.pattern_of(system))):
        restated = cases.restated_blocks(system, scale, coef, colours, n_colours, 4, indptr, indices)
        dense = cases.dense_probed_blocks(system, lambda e: np.polynomial.chebyshev.chebval(e / scale, coef), colours,
                                          n_colours, 4, indptr, indices, name)
        got = solver.fermi_blocks(scale, coef, colours, n_colours, 4, indptr, indices)
        assert got.shape == (len(indices), 4, 4)
        _hold((name, series, label), got, restated, dense, tolerance)
        assert not got[colours[indices] < 0].any()
        _assert_plan(solver.perf(), system, name, "dictionary", "packed", n_colours, 4, len(coef))
        if series == "one_coefficient":
            assert solver.perf()["launches"] == 1 and np.array_equal(got, restated)
        if label == "odd":
            assert np.array_equal(got[0], got[2])  # the column that is twice in row 1
    assert np.abs(dense).max() > 0.1


# ------------------------------------------------------------------ errors
def test_refusals_of_the_library():
    system = swave((4, 4, 1))
    solver = system._solver()
    scale = cases.scale_of(system)
    coef = cases.fermi_coefficients(system, 0.5)
    indptr, indices = cases.pattern_of(system)
    colours = np.arange(16, dtype=np.int32)
    with pytest.raises(ValueError, match="site colour 15 out of range"):
        solver.fermi_blocks(scale, coef, colours, 15, 2, indptr, indices)
    bad = indices.copy()
    bad[3] = 16
    with pytest.raises(ValueError, match="pattern column 16 out of range"):
        solver.fermi_blocks(scale, coef, colours, 16, 2, indptr, bad)
    bad[3] = -1
    with pytest.raises(ValueError, match="pattern column -1 out of range"):
        solver.fermi_blocks(scale, coef, colours, 16, 2, indptr, bad)
    with pytest.raises(ValueError, match="n_components must be 2 or 4"):
        solver.fermi_blocks(scale, coef, colours, 16, 3, indptr, indices)
    with pytest.raises(ValueError, match="n_moments must be >= 1"):
        solver.fermi_blocks(scale, coef[:0], colours, 16, 2, indptr, indices)
    # ... and the handle still works
    assert np.abs(solver.fermi_blocks(scale, coef, colours, 16, 2, indptr, indices)).max() > 0.1


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
