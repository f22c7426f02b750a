"""The 3-D rolling kernel (cheb_roll3, K8) where its units are runs of equal length (RollArgs.chunk > 0): a run of plane-steps
cut mid-column, units of two pieces, reversed marches on piece bounds - the default launch shape of BASELINE config 4,
which small lattices never reach.  Every test first proves from the perf record that it entered that branch
(`roll_chunk` equal to the restated RollPlan::chunk_for), then compares every column with the CPU oracle.

Cases, restatements and references: roll_unit_cases.py.  The lattices are sized for 256 CUs with one
workgroup per CU: on a device with another CU count the tests fail and say so.  Dictionary storage only (the stencil
kernels read the block dictionary)."""

import numpy as np
import pytest

import roll_unit_cases as rc
from oracle import cheb_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def devices(hip_library):
    """One device handle per (shape, kind), uploaded on first use and closed after the module."""
    from bodge_amd.solver import DeviceSolver

    made = {}

    def get(shape, kind):
        if (shape, kind) not in made:
            made[shape, kind] = DeviceSolver.from_hamiltonian(rc.palette_system(shape, kind))
        return made[shape, kind]

    yield get
    for dev in made.values():
        dev.close()


def _call(dev, name):
    case = rc.CASES[name]
    _, scale = rc.matrix_of(case.shape, case.kind)
    if case.start[0] == "unit":
        return dev.dots_unit(scale, case.steps, rc.unit_rows(name))
    kind = cheb_ref.VEC_Z4 if case.start[0] == "z4" else cheb_ref.VEC_RADEMACHER
    return dev.dots_random(scale, case.steps, case.start[1], seed=case.start[2], kind=kind)


def _bound(name):
    """1e-12 x 4N: the figure of every recurrence test here."""
    return 1e-12 * 4 * int(np.prod(rc.CASES[name].shape))


def _assert_entered(perf, name):
    """The call ran the rolling kernel, one step per launch, one workgroup per CU of a 256-CU device, and its last launch
    had the units of `chunk` plane-steps that the restated chunk_for gives."""
    case, plan = rc.CASES[name], rc.plan_of(name)
    assert perf["rolling"] == 1 and perf["steps_per_launch"] == 1, perf
    assert perf["grid"] == rc.GRID, (f"grid {perf['grid']}: these cases are sized for a device of 256 CUs "
                                     f"(BODGE_AMD_BLOCKS_PER_CU=1: one workgroup per CU, 1024 wave slots)")
    x_lo, x_hi, _, chunk = rc.launches(name)[-1]
    assert chunk == plan.chunk_for(x_hi - x_lo) == case.chunk
    assert perf["roll_chunk"] == chunk, (perf["roll_chunk"], chunk)
    assert perf["lanes_per_row"] == case.lanes and perf["streams"] == case.share, perf
    assert (perf["real_arithmetic"], perf["ph_packed"]) == rc.MODES[name], perf
    assert 0 < perf["dict_blocks"] <= 96, perf


def _distance(got, ref):
    return max(np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max())


def _report(label, distance, bound):
    print(f"[roll units] {label}: {distance:.3e} = {distance / bound:.1e} of the bound {bound:.3e}")


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E-full", "E-complex", "E-complex-full"])
def test_chunked_units_against_the_oracle_and_the_one_step_kernels(devices, knobs, name):
    """Random start vectors, whole-lattice launches: every column and every step against the oracle, bit-equal when
    repeated, and the same call through the one-step kernels.  A, D, E: an odd number of steps, so both marching
    directions run and the last launch stores nothing; B, E-complex: two lane groups side by side, each cut for half
    the wave slots, pieces of one plane; C: 2 lanes per site, windows of 30 positions; D, E: the other arithmetic modes."""
    case = rc.CASES[name]
    dev = devices(case.shape, case.kind)
    knobs.update(rc.COMMON_KNOBS)
    knobs.update(case.knobs)
    got = _call(dev, name)
    perf = dev.perf()
    again = _call(dev, name)
    knobs.set("BODGE_AMD_SWEEP", "0")
    plain = _call(dev, name)
    plain_perf = dev.perf()
    _assert_entered(perf, name)
    assert perf["launches"] == case.steps * case.share
    assert got[0].shape == (case.steps, case.start[1])
    ref = rc.reference(name)
    _report(f"{name} oracle", _distance(got, ref), _bound(name))
    _report(f"{name} one-step kernels", _distance(got, plain), _bound(name))
    assert _same_bits(got, again)
    assert _distance(got, ref) <= _bound(name)
    assert plain_perf["rolling"] == 0 and plain_perf["roll_chunk"] == 0 and plain_perf["steps_per_launch"] == 1
    assert _distance(got, plain) <= _bound(name)
    assert _distance(plain, ref) <= _bound(name)


def test_cache_policy_and_stores_change_no_bit(devices, knobs):
    """Same unit cutting, same arithmetic, same partial sums: non-temporal loads and stores (BODGE_AMD_STREAM_VECTORS = 3 is
    cheb_roll3<..., true>, otherwise chosen only beyond the Infinity Cache) and a last launch that stores its vectors
    give the bits of case A.  Forward marches only (BODGE_AMD_ALTERNATE=0) regroup nothing either, and meet the oracle."""
    case = rc.CASES["A"]
    dev = devices(case.shape, case.kind)
    knobs.update(rc.COMMON_KNOBS)
    base = _call(dev, "A")
    _assert_entered(dev.perf(), "A")
    for knob, values in (("BODGE_AMD_STREAM_VECTORS", "123"), ("BODGE_AMD_KEEP_LAST", "1")):
        for value in values:
            knobs.set(knob, value)
            got = _call(dev, "A")
            _assert_entered(dev.perf(), "A")
            assert _same_bits(got, base), (knob, value, _distance(got, base))
        knobs.unset(knob)
    knobs.set("BODGE_AMD_ALTERNATE", "0")
    forward = _call(dev, "A")
    _assert_entered(dev.perf(), "A")
    _report("A forward marches, oracle", _distance(forward, rc.reference("A")), _bound("A"))
    assert _distance(forward, rc.reference("A")) <= _bound("A")
    # (a reversed march adds a wave's planes in the other order: round-off only)
    assert _distance(forward, base) <= 1e-13 * 4 * int(np.prod(case.shape))


def _banded(dev, name):
    """The unit-start run behind another run's vectors in every buffer, as the band test of test_gpu_parity.py does."""
    _, scale = rc.matrix_of(rc.CASES[name].shape, rc.CASES[name].kind)
    dev.dots_random(scale, 5, 8, seed=1)
    return _call(dev, name)


@pytest.mark.parametrize("name", ["F9", "F14", "F16-low"])
def test_bands_of_planes_from_unit_start_vectors(devices, knobs, name):
    """Unit start vectors on plane 12: launch n advances planes [12 - n - 1, 12 + n + 2) only.  Launches 0-7 take
    whole-column segments, then the units are cut: 8 plane-steps on planes 3..21 (x_lo > 0, pieces of one plane), 8, 9,
    and 10 from the launch on that reaches both ends.  The chunk changes from launch to launch.  F16-low starts on plane 5:
    its cut launches (12-15) cover planes [0, 19) ... [0, 22), a band that is not centred in the lattice."""
    case = rc.CASES[name]
    dev = devices(case.shape, case.kind)
    knobs.update(rc.COMMON_KNOBS)
    got = _banded(dev, name)
    perf = dev.perf()
    again = _banded(dev, name)
    knobs.set("BODGE_AMD_SWEEP", "0")
    plain = _call(dev, name)
    plain_perf = dev.perf()
    _assert_entered(perf, name)
    assert perf["launches"] == case.steps
    assert perf["bytes_moved"] < perf["launches"] * perf["bytes_per_launch"]  # (the early launches are bands)
    ref = rc.reference(name)
    _report(f"{name} oracle", _distance(got, ref), 1e-13)
    assert _same_bits(got, again)
    assert _distance(got, ref) <= 1e-13
    assert plain_perf["rolling"] == 0 and plain_perf["steps_per_launch"] == 1
    for a, b in zip(plain, got):
        assert np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(a).max())


@pytest.mark.parametrize("name", ["A", "C", "F9", "F14"])
def test_whole_column_segments_as_the_ab_switch(devices, knobs, name):
    """BODGE_AMD_ROLL_CHUNKS=0: the same launches with whole-column segments.  Only the grouping of the workgroups'
    partial sums differs: 1e-13 x 4N, the figure test_gpu_fullsize.py uses for regrouped partial sums."""
    case = rc.CASES[name]
    unit = case.start[0] == "unit"
    dev = devices(case.shape, case.kind)
    knobs.update(rc.COMMON_KNOBS)
    chunked = _banded(dev, name) if unit else _call(dev, name)
    _assert_entered(dev.perf(), name)
    knobs.set("BODGE_AMD_ROLL_CHUNKS", "0")
    whole = _banded(dev, name) if unit else _call(dev, name)
    perf = dev.perf()
    assert perf["rolling"] == 1 and perf["roll_chunk"] == 0 and perf["lanes_per_row"] == case.lanes, perf
    ref = rc.reference(name)
    regrouped = 1e-13 * 4 * int(np.prod(case.shape))
    _report(f"{name} whole-column segments, oracle", _distance(whole, ref), 1e-13 if unit else _bound(name))
    _report(f"{name} whole-column segments, chunked run", _distance(whole, chunked), regrouped)
    assert _distance(whole, ref) <= (1e-13 if unit else _bound(name))
    assert _distance(whole, chunked) <= regrouped


def test_slab_members_read_their_neighbours_planes_from_chunked_units(devices, knobs):
    """Two slabs of 24 planes of a 48-plane lattice, same process: every member cuts its own 24 planes into units of 10
    plane-steps, and the units at either end of a column read the plane below / above the slab in the neighbour's
    buffer (lo_buf / hi_buf), in both marching directions.  Against the oracle, the undivided matrix and the same group
    through the one-step kernels with a halo exchange."""
    from bodge_amd.solver import SlabGroup

    name = "G"
    case = rc.CASES[name]
    system = rc.palette_system(case.shape, case.kind)
    knobs.update(rc.COMMON_KNOBS)
    with SlabGroup.from_hamiltonian(system, rc.SLABS[name]) as group:
        assert [p.n_own for p in group.plans] == [24 * 72 * 75] * 2
        split = _call(group, name)
        perfs = [member.perf() for member in group.members]
        again = _call(group, name)
        knobs.set("BODGE_AMD_SWEEP", "0")
        exchanged = _call(group, name)
        exchanged_perfs = [member.perf() for member in group.members]
    knobs.set("BODGE_AMD_SWEEP", "1")
    whole = _call(devices(case.shape, case.kind), name)
    whole_perf = devices(case.shape, case.kind).perf()
    for perf in perfs:
        _assert_entered(perf, name)
        assert perf["launches"] == case.steps
    assert whole_perf["rolling"] == 1 and whole_perf["roll_chunk"] == rc.RollPlan(386, 48).chunk_for(48) == 19
    ref = rc.reference(name)
    _report("G oracle", _distance(split, ref), _bound(name))
    _report("G undivided matrix", _distance(split, whole), _bound(name))
    _report("G one-step kernels with halo exchange", _distance(split, exchanged), _bound(name))
    assert _same_bits(split, again)
    assert _distance(split, ref) <= _bound(name)
    assert _distance(split, whole) <= _bound(name) and _distance(whole, ref) <= _bound(name)
    assert all(perf["rolling"] == 0 and perf["roll_chunk"] == 0 for perf in exchanged_perfs)
    assert _distance(split, exchanged) <= _bound(name)
