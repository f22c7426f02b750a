"""green_map(distance=...) and green_bonds(distance=...) without a GPU: the probing recurrence restated in numpy against
the probed dense sum on shapes whose colours hold several sites (and against the true G, which it is not), Welford's
update against numpy's mean and standard deviation, the public functions over a stand-in for the device (colours of
unlisted sites, groups of whole colours, info, stderr, errors before device work, distance=None untouched), and the
argument errors of the entry point in the order of the header."""

import ctypes

import numpy as np
import pytest

from bodge_amd import green as gr

import green_bonds_cases as cases
import green_probe_cases as probe

NAMES = sorted(probe.SHAPES)


# ------------------------------------------------------------------ algorithm
def test_shapes_have_the_colours_the_cases_say():
    for name in NAMES:
        _, shape, distance, periods, count, per_colour = probe.SHAPES[name]
        system = probe.system_of(name)
        colour, n_colours = probe.colours(name)
        from bodge_amd import fermi

        assert fermi.colour_periods(shape, distance) == periods and n_colours == count
        assert np.bincount(colour).tolist() == [per_colour] * count
        indptr, indices = probe.pattern(name)
        for j in range(system.lattice.size):  # one colour per pattern row: one writer per table entry
            row = colour[indices[indptr[j]:indptr[j + 1]]]
            assert np.unique(row).size == row.size


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", probe.SIGNS)
def test_restatement_matches_the_probed_dense_sum_and_not_the_true_blocks(name, kind):
    """Default moments for Γ = 0.1 (digits = 12), C = 4 and 2.  The distance from the probed dense sum is the series'
    truncation and the recurrence's rounding: the pin is 1e-12, and the recorded figure - the yardstick of the device
    tolerance - may not understate what is measured.  The true G is something else: O(1) away on these shapes."""
    system = probe.system_of(name)
    indptr, indices = probe.pattern(name)
    exact, size = probe.probed(name, kind)
    truth = probe.dense(name)[:, cases.block_rows(indptr), :, np.asarray(indices, dtype=np.int64), :]  # (nnz, K, 4, 4)
    assert truth.shape == exact.shape == size.shape == (indices.size, cases.ENERGIES.size, 4, 4)
    for columns in (4, 2):
        got = probe.restated(name, kind, columns)
        d = cases.distance(got, exact)
        print(name, kind, "C", columns, "sites", system.lattice.size, "colours", probe.colours(name)[1], "moments",
              cases.moments_of(system), "distance", d, "from the true G", cases.distance(got, truth))
        assert d <= 1e-12
        assert d <= 1.02 * probe.RESTATEMENT_ERROR[(name, kind)]
    away = cases.distance(exact, truth)
    print(name, kind, "probed dense sum - true G", away)
    assert away > 0.05  # the contamination by the other sites of the colour: nothing a tolerance would cover
    assert float(size.max()) >= float(np.abs(exact).max()) * (1 - 1e-12)


def test_probed_dense_sum_is_the_true_blocks_with_one_site_per_colour():
    system = cases.system_of("dwave_open")  # (6, 5, 1): distance >= the extents gives every site a colour of its own
    indptr, indices = cases.pattern_of(system)
    colour, count = probe.colours_of(system, 6)
    assert count == system.lattice.size and np.unique(colour).size == count
    g = probe.dense_resolvent(system, cases.Z)
    for kind in probe.SIGNS:
        xi = probe.signs_of(kind, count)[0]
        total, size = probe.probed_dense(g, indptr, indices, colour, xi)
        assert np.array_equal(total, cases.dense("dwave_open")) and np.array_equal(size, np.abs(total))
        got = probe.restate_sample(system, indptr, indices, colour, count, xi, cases.Z, cases.moments_of(system), 2)
        assert cases.distance(got, total) <= 20 * cases.RESTATEMENT_ERROR["dwave_open"]


def test_sites_without_a_colour_are_no_sources_and_return_zero():
    system = probe.system_of("dwave_9x8")
    cut = [system.lattice[(x, 3, 0)] for x in range(9)]
    colour, count = probe.colours_of(system, 3, cut)
    assert count == 3 and np.flatnonzero(colour >= 0).tolist() == sorted(cut)
    indptr, indices = probe.pattern("dwave_9x8")
    xi = probe.signs_of("plus", 72)[0]
    got = probe.restate_sample(system, indptr, indices, colour, count, xi, cases.Z, 64, 2)
    listed = np.isin(indices, cut)
    assert np.abs(got[~listed]).max() == 0 and np.abs(got[listed]).max() > 0.1
    total, _ = probe.probed_dense(probe.dense("dwave_9x8"), indptr, indices, colour, xi)
    assert np.abs(total[~listed]).max() == 0
    # fewer sources, less contamination: the cut's blocks differ from those of the run over all sites
    every, _ = probe.probed("dwave_9x8", "plus")
    assert np.abs(total[listed] - every[listed]).max() > 1e-3


# ------------------------------------------------------------------ sample statistics
@pytest.mark.parametrize("count", [3, 5])
def test_welford_matches_numpy_mean_and_standard_error(count):
    """Every update is a handful of rounded operations on values of the samples' size: the mean within
    64·S·2⁻⁵³·max|x|, S(S-1)·stderr² within 64·S·2⁻⁵³·max|x|²."""
    system = probe.system_of("dwave_8x6")
    indptr, indices = probe.pattern("dwave_8x6")
    colour, n_colours = probe.colours("dwave_8x6")
    signs = probe.signs_of("z2", system.lattice.size, count)
    assert np.array_equal(signs, gr.z2_signs(probe.SEED, count, system.lattice.size))
    samples = [probe.restate_sample(system, indptr, indices, colour, n_colours, xi, cases.Z, 96, 2) for xi in signs]
    mean, stderr = probe.welford(samples)
    stack = np.stack(samples)
    largest = np.abs(stack).max()
    assert np.abs(mean - stack.mean(axis=0)).max() <= 64 * count * 2.0**-53 * largest
    for part in ("real", "imag"):
        expected = getattr(stack, part).std(axis=0, ddof=1) / np.sqrt(count)
        m2, expected_m2 = count * (count - 1) * getattr(stderr, part) ** 2, count * (count - 1) * expected**2
        assert np.abs(m2 - expected_m2).max() <= 64 * count * 2.0**-53 * largest**2
        assert expected.max() > 1e-3  # the signs do change the samples
    one_mean, one_stderr = probe.welford(samples[:1])
    assert np.array_equal(one_mean, samples[0]) and not one_stderr.any()


# ------------------------------------------------------------------ the public functions over a stand-in for the device
class FakeSolver:
    """Stands in for the device: the numpy restatement behind DeviceSolver.green_probe_blocks."""

    def __init__(self, system):
        self.system = system
        self.calls = []

    def green_probe_blocks(self, scale, weights, colours, n_colours, indptr, indices, n_components=4, signs=None):
        assert indptr.dtype == np.int32 and indices.dtype == np.int32 and int(indptr[-1]) == indices.size
        assert colours.dtype == np.int32 and colours.shape == (self.system.lattice.size,) and colours.max() == n_colours - 1
        assert signs is None or (signs.dtype == np.int8 and signs.shape[1] == colours.size)
        self.calls.append((colours.copy(), n_colours, np.unique(indices), n_components, None if signs is None else signs.copy()))
        rows = signs if signs is not None else np.ones((1, colours.size), dtype=np.int8)
        h, moments = self.system.matrix("csr"), weights.shape[1]
        samples = []
        for xi in rows:
            mu = probe.probe_moments(h, indptr, indices, colours, n_colours, xi, moments, scale, n_components)
            if n_components == 2:
                mu = gr.hole_columns(mu)
            samples.append(cases.contract(mu, weights) * xi.astype(float)[indices][:, None, None, None])
        mean, stderr = probe.welford(samples)
        return mean.transpose(1, 0, 2, 3), (stderr.transpose(1, 0, 2, 3) if len(samples) > 1 else None)

    def green_bond_blocks(self, *args, **kwargs):
        raise AssertionError("the unprobed entry point in a probed call")

    def perf(self):
        return {"green_probe": 2}


class UnprobedOnly:
    """A solver that has the unprobed entry points alone."""

    def __init__(self):
        self.calls = 0

    def green_bond_blocks(self, scale, weights, indptr, indices, n_components=4):
        self.calls += 1
        return np.zeros((weights.shape[0], indices.size, 4, 4), dtype=np.complex128)

    def green_local_moments(self, scale, moments, sites, n_components=4):
        self.calls += 1
        return np.zeros((moments, len(sites), 4, n_components), dtype=np.complex128)

    def green_probe_blocks(self, *args, **kwargs):
        raise AssertionError("the probed entry point in a call without distance=")

    def perf(self):
        return {}


MOMENTS = 64  # (the surface, not the series: few moments keep the stand-in quick)


def test_probed_green_bonds_colours_groups_info_and_stderr(monkeypatch):
    system = probe.build("dwave_9x8")
    fake = FakeSolver(system)
    monkeypatch.setattr(system, "_solver", lambda: fake)
    options = dict(broadening=cases.GAMMA, moments=MOMENTS)
    every = system.green_bonds(cases.ENERGIES, distance=3, **options)
    indptr, indices = probe.pattern("dwave_9x8")
    assert np.array_equal(every.indptr, indptr) and np.array_equal(every.indices, indices) and len(fake.calls) == 1
    colour, n_colours, _, columns, signs = fake.calls[0]
    assert np.array_equal(colour, probe.colours("dwave_9x8")[0]) and n_colours == 12 and columns == 2 and signs is None
    info = every.info
    assert (info["distance"], info["periods"], info["colours"], info["samples"], info["seed"]) == (3, (3, 4, 1), 12, 1, 0)
    assert info["columns"] == 2 and info["perf"]["green_probe"] == 2 and info["moments"] == MOMENTS
    assert every.stderr is None and every.local().stderr is None and every.blocks.shape == (360, 4, 4, 4)
    xi = probe.signs_of("plus", 72)[0]
    expected = probe.restate_sample(system, indptr, indices, colour, 12, xi, cases.Z, MOMENTS, 2)
    assert np.array_equal(every.blocks, expected)

    # a cut, out of order and with a repeat: the other sites get colour -1 and the colours in use are numbered from 0
    cut = [(4, 3, 0), (0, 3, 0), (8, 3, 0), (4, 3, 0), (5, 3, 0)]
    some = system.green_bonds(cases.ENERGIES, cut, distance=3, **options)
    colour, n_colours, column_sites, _, _ = fake.calls[-1]
    listed = sorted({system.lattice[c] for c in cut})
    assert np.flatnonzero(colour >= 0).tolist() == listed == column_sites.tolist() and n_colours == 3
    assert some.info["colours"] == 3 and some.blocks.shape[0] == 5 * 4
    in_every, in_some = cases.shared_blocks(every.indptr, every.indices, some.indptr, some.indices)
    assert in_some.size == 20 and np.abs(every.blocks[in_every] - some.blocks[in_some]).max() > 1e-3  # (fewer sources)

    # three samples: "z2" signs from the seed, the mean and the standard error, local() carries its slice
    noisy = system.green_bonds(cases.ENERGIES, distance=3, samples=3, seed=7, **options)
    signs = fake.calls[-1][4]
    assert np.array_equal(signs, probe.signs_of("z2", 72, 3, seed=7)) and noisy.info["samples"] == 3 and noisy.info["seed"] == 7
    assert noisy.stderr.shape == noisy.blocks.shape and noisy.stderr.dtype == np.complex128 and noisy.stderr.real.max() > 1e-3
    local = noisy.local()
    diagonal = cases.block_rows(indptr) == indices
    assert np.array_equal(local.stderr, noisy.stderr[diagonal]) and np.array_equal(local.blocks, noisy.blocks[diagonal])
    assert local.ldos().shape == (72, 4) and noisy.anomalous((3, 2, 0), (2, 2, 0)).shape == (4, 2, 2)
    explicit = system.green_bonds(cases.ENERGIES, distance=3, samples=3, signs=signs, **options)
    assert np.array_equal(explicit.blocks, noisy.blocks) and np.array_equal(explicit.stderr, noisy.stderr)
    single = system.green_bonds(cases.ENERGIES, distance=3, signs="z2", seed=7, **options)
    assert single.stderr is None and np.array_equal(fake.calls[-1][4], signs[:1])

    # a host limit of 100 blocks' results: 360 blocks in 12 colours of 30 go in groups of 3 whole colours
    monkeypatch.setattr(gr, "HOST_TABLE_LIMIT", 100 * cases.ENERGIES.size * 256)
    before = len(fake.calls)
    grouped = system.green_bonds(cases.ENERGIES, distance=3, **options)
    calls = fake.calls[before:]
    assert [c[1] for c in calls] == [3, 3, 3, 3] and len(grouped.info["perf"]) == 4
    whole = probe.colours("dwave_9x8")[0]
    for g, (colour, _, column_sites, _, _) in enumerate(calls):
        assert np.array_equal(colour, np.where((whole >= 3 * g) & (whole < 3 * g + 3), whole - 3 * g, -1))
        assert column_sites.tolist() == np.flatnonzero(colour >= 0).tolist()
    assert np.array_equal(grouped.blocks, every.blocks)  # (a block carries its own colour alone: the groups change nothing)
    xi = probe.signs_of("plus", 72)[0]
    for g, (colour, _, _, _, _) in enumerate(calls):
        part = np.flatnonzero(colour[indices] >= 0)
        expected = probe.restate_sample(system, indptr, indices, colour, 3, xi, cases.Z, MOMENTS, 2)
        assert np.array_equal(grouped.blocks[part], expected[part])


def test_probed_green_map_returns_the_diagonal_blocks_in_the_order_of_the_sites(monkeypatch):
    system = probe.build("dwave_8x6")
    fake = FakeSolver(system)
    monkeypatch.setattr(system, "_solver", lambda: fake)
    options = dict(broadening=cases.GAMMA, moments=MOMENTS)
    every = system.green_map(cases.ENERGIES, distance=4, samples=3, **options)
    colour, n_colours, column_sites, columns, signs = fake.calls[-1]
    assert n_colours == 24 and columns == 2 and column_sites.size == 48 and signs.shape == (3, 48)
    assert every.blocks.shape == every.stderr.shape == (48, 4, 4, 4) and every.sites == list(system.lattice.sites())
    assert every.info["distance"] == 4 and every.info["periods"] == (4, 6, 1) and every.info["colours"] == 24
    assert every.ldos().shape == (48, 4) and every.anomalous().shape == (48, 4, 2, 2)
    bonds = system.green_bonds(cases.ENERGIES, distance=4, samples=3, **options)
    assert np.array_equal(bonds.local().blocks, every.blocks) and np.array_equal(bonds.local().stderr, every.stderr)
    sites = [(5, 2, 0), (1, 2, 0), (5, 2, 0)]
    some = system.green_map(cases.ENERGIES, sites, distance=4, **options)
    colour = fake.calls[-1][0]
    assert np.flatnonzero(colour >= 0).tolist() == sorted({system.lattice[s] for s in sites}) and fake.calls[-1][1] == 1
    assert some.blocks.shape == (3, 4, 4, 4) and np.array_equal(some.blocks[0], some.blocks[2]) and some.sites == sites
    assert not np.array_equal(some.blocks[0], some.blocks[1]) and some.stderr is None


def test_argument_errors_are_raised_before_any_device_work(monkeypatch):
    system = probe.build("dwave_8x6")

    def no_device():
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(system, "_solver", no_device)
    n = system.lattice.size
    for call in (system.green_map, system.green_bonds):
        with pytest.raises(ValueError, match="distance"):
            call([0.1, 0.2], broadening=0.1, distance=2)
        with pytest.raises(ValueError, match="samples"):
            call([0.1, 0.2], broadening=0.1, distance=4, samples=0)
        with pytest.raises(ValueError, match="signs"):
            call([0.1, 0.2], broadening=0.1, distance=4, signs="u1")
        with pytest.raises(ValueError, match="signs"):
            call([0.1, 0.2], broadening=0.1, distance=4, samples=2, signs=np.ones((3, n)))
        with pytest.raises(ValueError, match="signs"):
            call([0.1, 0.2], broadening=0.1, distance=4, signs=np.zeros((1, n)))
        with pytest.raises(ValueError, match="signs"):
            call([0.1, 0.2], broadening=0.1, distance=4, signs=np.full((1, n), 1j))
        with pytest.raises(ValueError, match="random signs"):
            call([0.1, 0.2], broadening=0.1, distance=4, samples=2, signs=np.ones((2, n)))
        with pytest.raises(ValueError, match="green"):
            call([], broadening=0.1, distance=4)
        with pytest.raises(AssertionError, match="device work"):
            call([0.1, 0.2], broadening=0.1, distance=4)  # (valid arguments do reach the device)


def test_calls_without_distance_never_touch_the_probed_entry_point(monkeypatch):
    system = probe.build("dwave_8x6")
    solver = UnprobedOnly()
    monkeypatch.setattr(system, "_solver", lambda: solver)
    g = system.green_bonds(cases.ENERGIES, broadening=cases.GAMMA, moments=8)
    m = system.green_map(cases.ENERGIES, broadening=cases.GAMMA, moments=8)
    assert solver.calls == 2 and g.stderr is None and m.stderr is None and g.local().stderr is None
    assert "distance" not in g.info and "distance" not in m.info


# ------------------------------------------------------------------ the entry point
def test_entry_point_argument_errors_do_not_need_a_gpu(hip_library):
    """The errors that come before the handle is looked at, in the order of the header; those that need the number of
    block rows through bdg_host_probe_check, which runs the same checks without a handle."""
    from bodge_amd import backend

    weights = np.zeros(2 * 8)
    colours = np.zeros(1, dtype=np.int32)
    signs = np.ones(1, dtype=np.int8)
    indptr = np.array([0, 1], dtype=np.int32)
    indices = np.zeros(1, dtype=np.int32)
    out = np.zeros(32)
    w, c, s = backend.as_f64p(weights), backend.as_i32p(colours), backend.as_i8p(signs)
    p, i, o = backend.as_i32p(indptr), backend.as_i32p(indices), backend.as_f64p(out)

    def call(scale=1.0, n_moments=8, n_weights=1, weights=w, n_colours=1, colours=c, n_samples=1, signs=s, indptr=p,
             indices=i, components=2, out=o):
        rc = hip_library.bdg_green_probe_blocks(None, scale, n_moments, n_weights, weights, n_colours, colours, n_samples,
                                                signs, indptr, indices, components, out, None)
        return rc, hip_library.bdg_last_error()

    assert call(n_moments=0, n_weights=0, n_colours=0) == (-1, b"n_moments must be >= 1")
    assert call(n_weights=0, n_colours=0, scale=-1.0) == (-1, b"n_weights must be >= 1")
    rc, message = call(n_weights=4 * 65535 + 1, n_colours=0)
    assert rc == -1 and b"weight rows" in message
    assert call(n_colours=0, n_samples=0, scale=0.0) == (-1, b"n_colours must be >= 1")
    assert call(n_samples=0, scale=0.0, weights=None) == (-1, b"n_samples must be >= 1")
    assert call(scale=0.0, weights=None) == (-1, b"scale must be positive")
    assert call(scale=float("nan")) == (-1, b"scale must be positive")
    for name in ("weights", "colours", "indptr", "indices", "out"):
        assert call(**{name: None, "signs": None, "n_samples": 2}) == (-1, b"null argument"), name
    assert call(signs=None, n_samples=2) == (-1, b"signs must be given for more than one sample")
    assert call(signs=None, components=3) == (-1, b"null system handle")  # (the rest needs the handle's size)
    assert "bdg_green_probe_blocks" in backend.SIGNATURES and ("green_probe", ctypes.c_int32) in backend.Perf._fields_
    # the flag took the padding before gram_ms: the record keeps its 200 bytes and the fields before it their places
    assert ctypes.sizeof(backend.Perf) == 200 and backend.Perf.green_probe.offset == backend.Perf.gemm_flops.offset + 8 == 176
    assert backend.Perf.gram_ms.offset == 184 and backend.Perf.green_bonds.offset == 144

    # the checks behind the handle, on a pattern of 4 block rows: row 1 holds the columns 0 and 2
    indptr = np.array([0, 1, 3, 4, 5], dtype=np.int32)
    indices = np.array([0, 0, 2, 2, 3], dtype=np.int32)
    colours = np.array([0, 1, 2, -1], dtype=np.int32)
    signs = np.array([[1, -1, 1, -1], [-1, -1, 1, 1]], dtype=np.int8)

    def check(nb=4, n_colours=3, colours=colours, n_samples=2, signs=signs, indptr=indptr, indices=indices, components=2):
        rc = hip_library.bdg_host_probe_check(
            nb, n_colours, None if colours is None else backend.as_i32p(colours), n_samples,
            None if signs is None else backend.as_i8p(signs), backend.as_i32p(indptr), backend.as_i32p(indices), components)
        return rc, hip_library.bdg_last_error()

    assert check()[0] == 0
    assert check(signs=None, n_samples=1)[0] == 0
    assert check(nb=0)[0] == -1 and check(n_colours=0)[0] == -1 and check(n_samples=0)[0] == -1 and check(colours=None)[0] == -1
    assert check(signs=None) == (-1, b"signs must be given for more than one sample")
    bad_signs = signs.copy()
    bad_signs[1, 2] = 0
    same_colour = np.array([0, 1, 0, -1], dtype=np.int32)
    # in order: the pattern, the components, the colours' range, the signs, one colour per row
    assert check(indptr=np.array([1, 1, 3, 4, 5], dtype=np.int32), components=3, n_colours=2)[1] == b"pattern indptr must start at 0"
    assert check(indptr=np.array([0, 3, 1, 4, 5], dtype=np.int32), components=3)[1] == b"pattern indptr is not monotone"
    assert check(indptr=np.zeros(5, dtype=np.int32), components=3)[1] == b"the pattern has no block"
    assert b"out of range" in check(indices=np.array([0, 0, 4, 2, 3], dtype=np.int32), components=3)[1]
    assert b"canonical" in check(indices=np.array([0, 2, 0, 2, 3], dtype=np.int32), components=3)[1]
    assert check(components=3, n_colours=2, signs=bad_signs) == (-1, b"n_components must be 2 or 4")
    assert check(n_colours=2, signs=bad_signs, colours=colours) == (-1, b"site 2 has colour 2 of 2 colours")
    assert check(signs=bad_signs, colours=same_colour) == (-1, b"sign 0 of site 2 in sample 1 is not +1 or -1")
    assert check(colours=same_colour) == (-1, b"pattern row 1 holds two column sites of colour 0")
    assert check(colours=np.array([-1, 1, -1, -1], dtype=np.int32))[0] == 0  # (sites without a colour may share a row)
