"""green_map(distance=...) and green_bonds(distance=...) on the GPU: bdg_green_probe_blocks on the shapes whose colours
hold several sites, in both forms of the matrix, every arithmetic mode, two and four columns, 4 and 64 lanes, signs +1
and ±1, against the numpy restatement and the probed dense sum; ranges of the device table, several tiles per workgroup,
explicit signs and one site per colour (bdg_green_bond_blocks) bit for bit; lane widths; the sample statistics; a subset
of sites; the public functions."""

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import green as gr

import family_tile_cases
import green_bonds_cases as cases
import green_probe_cases as probe

pytestmark = pytest.mark.gpu

NAMES = sorted(probe.SHAPES)
ARITHMETIC = {
    "packed": {},
    "real_full": {"BODGE_AMD_PH": "0"},
    "complex_packed": {"BODGE_AMD_REAL": "0"},
    "complex_full": {"BODGE_AMD_REAL": "0", "BODGE_AMD_PH": "0"},
}


def effective(name, arithmetic):
    """(real, packed) as the library will decide them for this shape under the switches of `arithmetic`."""
    return (probe.IS_REAL[name] and "complex" not in arithmetic, not arithmetic.endswith("full"))


def modes_of(name):
    seen, out = set(), []
    for arithmetic in ARITHMETIC:
        if effective(name, arithmetic) not in seen:
            seen.add(effective(name, arithmetic))
            out.append(arithmetic)
    return out


def fresh(build, form, arithmetic, knobs):
    """A new system and handle under the switches of (form, arithmetic): the dictionary switch is read at upload."""
    for switch in ("BODGE_AMD_REAL", "BODGE_AMD_PH"):
        if switch in ARITHMETIC[arithmetic]:
            knobs.set(switch, ARITHMETIC[arithmetic][switch])
        else:
            knobs.unset(switch)
    knobs.set("BODGE_AMD_DICT", "1" if form == "dictionary" else "0")
    system = build()
    return system, system._solver()


def batches_of(perf, lanes, colours, columns):
    per_lane = 2 if perf["real_arithmetic"] else 1
    batch = max(1, min(lanes * per_lane, 64, colours * columns) // columns)
    return -(-colours // batch)


def probe_blocks(solver, system, indptr, indices, colour, n_colours, columns, signs, moments=None, z=cases.Z):
    """One device call at the series weights of z: (mean, stderr) as (nnz, K, 4, 4)."""
    scale = cases.scale_of(system)
    weights = gr.moment_weights(moments or cases.moments_of(system), scale, z)
    mean, stderr = solver.green_probe_blocks(scale, weights, colour, n_colours, indptr, indices, columns, signs)
    return mean.transpose(1, 0, 2, 3), None if stderr is None else stderr.transpose(1, 0, 2, 3)


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name,form,arithmetic", [(name, form, arithmetic) for name in NAMES
                                                  for form in ("dictionary", "streamed") for arithmetic in modes_of(name)])
def test_device_matches_restatement_and_probed_dense_sum(name, form, arithmetic, knobs):
    """The default moments for Γ = 0.1.  Device - restated <= 32·M·2⁻⁵³·max(1, max over blocks of Σ_{i' in colour}
    |G_ji'|): the bound of DESIGN.md §10 at the size of what is actually summed.  Device - probed dense sum <= 20 x the
    restatement's own distance (probe.RESTATEMENT_ERROR).  4 lanes in complex arithmetic at two columns: 6, 12, 12 and
    24 batches of two colours."""
    reference = probe.system_of(name)
    indptr, indices = probe.pattern(name)
    colour, n_colours = probe.colours(name)
    moments = cases.moments_of(reference)
    system, solver = fresh(lambda: probe.build(name), form, arithmetic, knobs)
    real, packed = effective(name, arithmetic)
    try:
        for lanes in (4, 64):
            solver.set_lanes_per_row(lanes)
            for columns in (2, 4):
                for kind in probe.SIGNS:
                    signs = None if kind == "plus" else probe.signs_of(kind, colour.size)
                    got, stderr = probe_blocks(solver, system, indptr, indices, colour, n_colours, columns, signs)
                    perf = solver.perf()
                    dictionary = form == "dictionary" and not (real and lanes == 64)
                    assert perf["green_probe"] == (2 if dictionary else 1) and perf["green_bonds"] == 0
                    assert perf["real_arithmetic"] == int(real) and perf["ph_packed"] == int(packed)
                    assert perf["lanes_per_row"] == lanes and stderr is None
                    batches = batches_of(perf, lanes, n_colours, columns)
                    assert perf["launches"] == batches * (moments - 1), (perf["launches"], batches)
                    assert perf["vector_steps"] == (moments - 1) * n_colours * columns
                    if lanes == 4 and columns == 2 and not real:
                        assert batches == n_colours // 2
                    restated, (exact, _) = probe.restated(name, kind, columns), probe.probed(name, kind)
                    bound = 32 * moments * 2.0**-53 * probe.reference_magnitude(name, kind)
                    to_restated, to_dense = np.abs(got - restated).max(), cases.distance(got, exact)
                    print(name, form, arithmetic, "lanes", lanes, "columns", columns, kind, "batches", batches,
                          "device - restated", to_restated, "bound", bound, "device - probed dense", to_dense, "limit",
                          20 * probe.RESTATEMENT_ERROR[(name, kind)])
                    assert to_restated <= bound
                    assert to_dense <= 20 * probe.RESTATEMENT_ERROR[(name, kind)]
    finally:
        solver.set_lanes_per_row(0)


# ------------------------------------------------------------------ 2. bit for bit
@pytest.mark.parametrize("columns", [2, 4])
def test_ranges_of_the_device_table_do_not_change_one_bit(columns, knobs):
    system = probe.build("dwave_8x6")
    solver = system._solver()
    indptr, indices = probe.pattern("dwave_8x6")
    colour, n_colours = probe.colours("dwave_8x6")
    signs = probe.signs_of("z2", 48, 2)
    whole, whole_error = probe_blocks(solver, system, indptr, indices, colour, n_colours, columns, signs, moments=40)
    perf = solver.perf()
    assert perf["green_ranges"] == 1 and whole.shape == (240, 4, 4, 4) and np.abs(whole_error).max() > 1e-3
    blocks = 10 * min(perf["vectors_per_launch"] // columns, n_colours)  # of the largest batch: 2 sites x 5 per colour
    knobs.set("BODGE_AMD_GREEN_TABLE_BYTES", str(15 * blocks * 4 * columns * 16))  # 15 moments per range
    chunked, chunked_error = probe_blocks(solver, system, indptr, indices, colour, n_colours, columns, signs, moments=40)
    assert solver.perf()["green_ranges"] == 3
    assert np.array_equal(whole, chunked) and np.array_equal(whole_error, chunked_error)
    knobs.set("BODGE_AMD_GREEN_TABLE_BYTES", "1")                                   # (one moment per range)
    single, single_error = probe_blocks(solver, system, indptr, indices, colour, n_colours, columns, signs, moments=40)
    assert solver.perf()["green_ranges"] == 40
    assert np.array_equal(whole, single) and np.array_equal(whole_error, single_error)


@pytest.mark.parametrize("shape", [(67, 3, 1), family_tile_cases.SHAPE])
def test_blocks_per_cu_does_not_change_one_bit(shape, knobs):
    """BODGE_AMD_BLOCKS_PER_CU=1 against 8 at distance 3.  67 x 3 sites: 201 colours of one site, as few tiles as
    workgroups.  67 x 63 sites have the same periods (67, 3, 1), 201 colours of 21 sites, and at 32 lanes 528 tiles:
    with =1 every workgroup of a 256-CU device walks two or three of them (the method of test_gpu_family_tiles.py)."""
    from apply_cases import uniform_swave

    system = uniform_swave(shape)
    solver = system._solver()
    colour, n_colours = probe.colours_of(system, 3)
    assert n_colours == 201 and np.bincount(colour).tolist() == [shape[1] // 3] * 201
    indptr, indices = cases.pattern_of(system)
    signs = probe.signs_of("z2", colour.size)
    z = np.array([-0.3, 0.2, 0.9]) + 0.1j
    lanes, tiles = 32, family_tile_cases.tiles_of(colour.size, 32)
    solver.set_lanes_per_row(lanes)
    try:
        knobs.set("BODGE_AMD_BLOCKS_PER_CU", "8")
        reference, _ = probe_blocks(solver, system, indptr, indices, colour, n_colours, 2, signs, family_tile_cases.M, z)
        before = solver.perf()
        assert before["lanes_per_row"] == lanes and before["grid"] >= tiles and before["green_probe"] in (1, 2)
        knobs.set("BODGE_AMD_BLOCKS_PER_CU", "1")
        capped, _ = probe_blocks(solver, system, indptr, indices, colour, n_colours, 2, signs, family_tile_cases.M, z)
        perf = solver.perf()
        if shape == family_tile_cases.SHAPE:
            assert tiles > 2 * perf["grid"], (tiles, perf["grid"])
        assert perf["launches"] == before["launches"] == 7 * (family_tile_cases.M - 1) and np.abs(reference).max() > 1e-3
        print(shape, "grid", perf["grid"], "tiles", tiles, np.abs(capped - reference).max())
        assert np.array_equal(capped, reference)
    finally:
        solver.set_lanes_per_row(0)


def test_one_sample_equals_the_same_signs_passed_as_sample_0_of_1():
    system = probe.build("peierls_8x6")
    options = dict(broadening=cases.GAMMA, moments=64, distance=4)
    drawn = system.green_bonds(cases.ENERGIES, signs="z2", seed=11, **options)
    given = system.green_bonds(cases.ENERGIES, signs=gr.z2_signs(11, 1, 48), **options)
    assert np.array_equal(drawn.blocks, given.blocks) and drawn.stderr is None and given.stderr is None
    plain = system.green_bonds(cases.ENERGIES, **options)
    ones = system.green_bonds(cases.ENERGIES, signs=np.ones((1, 48)), **options)
    assert np.array_equal(plain.blocks, ones.blocks) and not np.array_equal(plain.blocks, drawn.blocks)


@pytest.mark.parametrize("form", ["dictionary", "streamed"])
@pytest.mark.parametrize("columns", [2, 4])
def test_one_site_per_colour_equals_green_bond_blocks_bit_for_bit(form, columns, knobs):
    """dwave_open (6, 5, 1) at a distance of its extents: every site a colour of its own, signs +1.  The start vectors
    are the unit vectors of bdg_green_bond_blocks in other slots (colour = x + 6 y, site index = y + 5 x), and a vector's
    recurrence does not depend on its slot."""
    system, solver = fresh(cases.SYSTEMS["dwave_open"], form, "packed", knobs)
    indptr, indices = cases.pattern_of(system)
    colour, n_colours = probe.colours_of(system, 6)
    assert n_colours == 30 and not np.array_equal(colour, np.arange(30))
    scale, moments = cases.scale_of(system), cases.moments_of(system)
    weights = gr.moment_weights(moments, scale, cases.Z)
    for lanes in (8, 16):
        solver.set_lanes_per_row(lanes)
        try:
            probed, _ = solver.green_probe_blocks(scale, weights, colour, n_colours, indptr, indices, columns)
            assert solver.perf()["green_probe"] == (2 if form == "dictionary" else 1) and solver.perf()["lanes_per_row"] == lanes
            launches = solver.perf()["launches"]
            bonds = solver.green_bond_blocks(scale, weights, indptr, indices, columns)
            assert solver.perf()["launches"] == launches and solver.perf()["green_probe"] == 0
        finally:
            solver.set_lanes_per_row(0)
        print(form, columns, lanes, np.abs(probed - bonds).max())
        assert np.array_equal(probed, bonds)
    assert cases.distance(probed.transpose(1, 0, 2, 3), cases.dense("dwave_open")) <= 20 * cases.RESTATEMENT_ERROR["dwave_open"]


# ------------------------------------------------------------------ 3. lane widths
def test_lane_widths_agree_under_the_rounding_bound():
    name = "cube_6x4x4"
    system = probe.build(name)
    solver = system._solver()
    indptr, indices = probe.pattern(name)
    colour, n_colours = probe.colours(name)
    signs = probe.signs_of("z2", colour.size)
    moments = cases.moments_of(system)
    bound = 32 * moments * 2.0**-53 * probe.reference_magnitude(name, "z2")
    results = {}
    try:
        for lanes in (4, 8, 16, 32):
            solver.set_lanes_per_row(lanes)
            results[lanes], _ = probe_blocks(solver, system, indptr, indices, colour, n_colours, 2, signs)
            assert solver.perf()["lanes_per_row"] == lanes
    finally:
        solver.set_lanes_per_row(0)
    for lanes in (8, 16, 32):
        print(lanes, np.abs(results[lanes] - results[4]).max(), bound)
        assert np.abs(results[lanes] - results[4]).max() <= bound


# ------------------------------------------------------------------ 4. samples
@pytest.mark.parametrize("columns", [2, 4])
def test_three_samples_are_the_welford_update_of_three_single_sample_calls(columns):
    """The mean within 8·2⁻⁵³·max|x| of the restated update (three updates of a few roundings each; the device's FMA
    in M2 does not enter the mean), S(S-1)·stderr² within 64·S·2⁻⁵³·max|x|²; launches = samples x batches x (M - 1)."""
    name, count, moments = "dwave_9x8", 3, 200
    system = probe.build(name)
    solver = system._solver()
    indptr, indices = probe.pattern(name)
    colour, n_colours = probe.colours(name)
    signs = probe.signs_of("z2", colour.size, count)
    mean, stderr = probe_blocks(solver, system, indptr, indices, colour, n_colours, columns, signs, moments)
    perf = solver.perf()
    batches = batches_of(perf, perf["lanes_per_row"], n_colours, columns)
    assert perf["launches"] == count * batches * (moments - 1) and perf["green_probe"] in (1, 2)
    assert perf["vector_steps"] == count * n_colours * columns * (moments - 1)
    singles = [probe_blocks(solver, system, indptr, indices, colour, n_colours, columns, signs[s : s + 1], moments)[0]
               for s in range(count)]
    assert solver.perf()["launches"] == batches * (moments - 1)
    expected_mean, expected_stderr = probe.welford(singles)
    largest = np.abs(np.stack(singles)).max()
    print(columns, "mean", np.abs(mean - expected_mean).max(), 8 * 2.0**-53 * largest, "largest", largest)
    assert np.abs(mean - expected_mean).max() <= 8 * 2.0**-53 * largest
    factor = count * (count - 1)
    for part in ("real", "imag"):
        difference = np.abs(factor * getattr(stderr, part) ** 2 - factor * getattr(expected_stderr, part) ** 2).max()
        print(columns, part, "S(S-1) stderr^2", difference, 64 * count * 2.0**-53 * largest**2)
        assert difference <= 64 * count * 2.0**-53 * largest**2
    assert stderr.real.max() > 1e-3 and stderr.real.min() >= 0 and stderr.imag.min() >= 0
    # and the host's own statistics of the three samples
    stack = np.stack(singles)
    assert np.abs(mean - stack.mean(axis=0)).max() <= 64 * count * 2.0**-53 * largest
    assert np.abs(stderr.real - stack.real.std(axis=0, ddof=1) / np.sqrt(count)).max() <= 1e-12 * max(1.0, largest)


# ------------------------------------------------------------------ 5. a subset of sites
def test_a_line_cut_leaves_the_other_sites_out_of_the_probes():
    name, moments = "dwave_9x8", cases.moments_of(probe.system_of("dwave_9x8"))
    system = probe.build(name)
    cut = [(x, 3, 0) for x in range(9)]
    cut_sites = [system.lattice[c] for c in cut]
    line = system.green_bonds(cases.ENERGIES, cut, broadening=cases.GAMMA, distance=3)
    assert line.info["colours"] == 3 and line.blocks.shape == (45, 4, 4, 4) and line.info["moments"] == moments
    indptr, indices = cases.pattern_of(probe.system_of(name), cut_sites)
    assert np.array_equal(line.indptr, indptr) and np.array_equal(line.indices, indices)
    colour, n_colours = probe.colours_of(probe.system_of(name), 3, cut_sites)
    xi = probe.signs_of("plus", 72)[0]
    restated = probe.restate_sample(probe.system_of(name), indptr, indices, colour, n_colours, xi, cases.Z, moments, 2)
    exact, size = probe.probed_dense(probe.dense(name), indptr, indices, colour, xi)
    bound = 32 * moments * 2.0**-53 * max(1.0, float(size.max()))
    print("cut: device - restated", np.abs(line.blocks - restated).max(), bound, cases.distance(line.blocks, exact))
    assert np.abs(line.blocks - restated).max() <= bound
    assert cases.distance(line.blocks, exact) <= 20 * probe.RESTATEMENT_ERROR[(name, "plus")]
    every = system.green_bonds(cases.ENERGIES, broadening=cases.GAMMA, distance=3)
    in_every, in_line = cases.shared_blocks(every.indptr, every.indices, line.indptr, line.indices)
    assert in_line.size == 45
    print("cut - all sites", np.abs(every.blocks[in_every] - line.blocks[in_line]).max())
    assert np.abs(every.blocks[in_every] - line.blocks[in_line]).max() > 1e-3  # (three sites per colour, not six)


# ------------------------------------------------------------------ 6. the public functions
def test_public_functions_and_their_helpers():
    name = "dwave_9x8"
    system = probe.build(name)
    mapped = system.green_map(cases.ENERGIES, broadening=cases.GAMMA, distance=3)
    info = mapped.info
    assert (info["distance"], info["periods"], info["colours"], info["samples"], info["seed"]) == (3, (3, 4, 1), 12, 1, 0)
    assert info["perf"]["green_probe"] in (1, 2) and info["columns"] == 2 and mapped.stderr is None
    assert mapped.blocks.shape == (72, 4, 4, 4) and mapped.sites == list(system.lattice.sites())
    indptr, indices = probe.pattern(name)
    diagonal = cases.block_rows(indptr) == indices
    restated = probe.restated(name, "plus", 2)[diagonal]
    bound = 32 * info["moments"] * 2.0**-53 * probe.reference_magnitude(name, "plus")
    assert info["moments"] == cases.moments_of(system) and np.abs(mapped.blocks - restated).max() <= bound
    assert mapped.ldos().shape == (72, 4) and mapped.spin_ldos().shape == (72, 4, 2)
    assert mapped.anomalous().shape == (72, 4, 2, 2) and mapped.site((4, 3, 0)).shape == (4, 4, 4)
    assert np.array_equal(mapped.ldos(), -(mapped.blocks[:, :, 0, 0] + mapped.blocks[:, :, 1, 1]).imag / np.pi)

    bonds = system.green_bonds(cases.ENERGIES, broadening=cases.GAMMA, distance=3, samples=3, seed=7)
    info = bonds.info
    assert (info["distance"], info["colours"], info["samples"], info["seed"]) == (3, 12, 3, 7)
    batches = batches_of(info["perf"], info["perf"]["lanes_per_row"], 12, 2)
    assert info["perf"]["launches"] == 3 * batches * (info["moments"] - 1) and info["perf"]["green_probe"] in (1, 2)
    assert bonds.blocks.shape == bonds.stderr.shape == (360, 4, 4, 4) and bonds.stderr.real.max() > 1e-3
    signs = probe.signs_of("z2", 72, 3, seed=7)
    colour, n_colours = probe.colours(name)
    samples = [probe.restate_sample(probe.system_of(name), indptr, indices, colour, n_colours, xi, cases.Z,
                                    info["moments"], 2) for xi in signs]
    expected_mean, expected_stderr = probe.welford(samples)
    print("public: mean", np.abs(bonds.blocks - expected_mean).max(), "stderr", np.abs(bonds.stderr - expected_stderr).max(), bound)
    size = max(probe.reference_magnitude(name, "z2"), probe.reference_magnitude(name, "plus"))
    assert np.abs(bonds.blocks - expected_mean).max() <= 32 * info["moments"] * 2.0**-53 * size
    # the standard error through the Python plumbing (transpose, the blocks of a group): every sample is within the
    # rounding bound r of its restatement, so S(S-1)·stderr² = Σ(x - mean)² moves by at most 2·S·(2·spread)·(2r) + O(r²)
    # with spread = max|x| - far above the 64·S·2⁻⁵³·max|x|² of the update itself, which it includes
    spread = max(float(np.abs(x).max()) for x in samples)
    r = 32 * info["moments"] * 2.0**-53 * size
    for part in ("real", "imag"):
        m2, expected_m2 = 6 * getattr(bonds.stderr, part) ** 2, 6 * getattr(expected_stderr, part) ** 2
        assert np.abs(m2 - expected_m2).max() <= 8 * 3 * spread * r + 64 * 3 * 2.0**-53 * spread**2
    local = bonds.local()
    assert np.array_equal(local.blocks, bonds.blocks[diagonal]) and np.array_equal(local.stderr, bonds.stderr[diagonal])
    assert local.ldos().shape == (72, 4) and bonds.block((3, 2, 0), (2, 2, 0)).shape == (4, 4, 4)
    assert bonds.anomalous((3, 2, 0), (2, 2, 0)).shape == (4, 2, 2) and bonds.spectral().shape == (360, 4, 4, 4)
    value = bonds.expectation(ba.correlation.current_operator(system, 0))
    assert value.shape == cases.ENERGIES.shape and np.all(np.isfinite(value))
    # the unprobed call is another route and, on this small lattice, another result
    exact = system.green_map(cases.ENERGIES, broadening=cases.GAMMA)
    assert "distance" not in exact.info and exact.info["perf"]["green_probe"] == 0
    assert np.abs(exact.blocks - mapped.blocks).max() > 1e-2


def test_argument_errors_of_the_entry_point_behind_the_handle():
    system = probe.build("dwave_8x6")
    solver = system._solver()
    scale = cases.scale_of(system)
    indptr, indices = probe.pattern("dwave_8x6")
    colour, n_colours = probe.colours("dwave_8x6")
    weights = np.ones((2, 8), dtype=np.complex128)
    with pytest.raises(ValueError, match="has colour 23 of 23"):
        solver.green_probe_blocks(scale, weights, colour, n_colours - 1, indptr, indices, 2)
    same = np.array(colour)
    same[indices[indptr[7] + 1]] = same[indices[indptr[7]]]
    rows = [same[indices[indptr[j]:indptr[j + 1]]] for j in range(48)]
    first = next(j for j, row in enumerate(rows) if np.unique(row).size < row.size)  # (the site has other rows too)
    values, counts = np.unique(rows[first], return_counts=True)
    twice = int(values[counts > 1][0])
    assert first <= 7 and (counts > 1).sum() == 1
    with pytest.raises(ValueError, match=f"pattern row {first} holds two column sites of colour {twice}$"):
        solver.green_probe_blocks(scale, weights, same, n_colours, indptr, indices, 2)
    bad = indices.copy()
    bad[[0, 1]] = bad[[1, 0]]
    with pytest.raises(ValueError, match="canonical"):
        solver.green_probe_blocks(scale, weights, colour, n_colours, indptr, bad, 2)
    with pytest.raises(ValueError, match="signs"):
        solver.green_probe_blocks(scale, weights, colour, n_colours, indptr, indices, 2, np.zeros((1, 48)))
    # the call ends a Lanczos run on the handle, as its siblings do
    solver.lanczos_begin(2)
    mean, stderr = solver.green_probe_blocks(scale, weights, colour, n_colours, indptr, indices, 2)
    assert mean.shape == (2, 240, 4, 4) and stderr is None
    with pytest.raises(ValueError, match="lanczos_begin"):
        solver.lanczos_advance(1)
