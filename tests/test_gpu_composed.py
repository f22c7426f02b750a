"""The composed three-step sweep (cheb_sweep3_composed, csrc/sweep.hpp "K7b, composed") on the GPU.

Random-start runs step by T_3: three array passes per three steps, u_{k-1} updated to u_{k+1} in place, and the sweeps' own
dot products turned back into d_n, e_n on the host (csrc/composed.hpp).  Forced on small lattices as test_gpu_parity.py
forces the classic sweep, and held to the project's two tolerances: 1e-12 * 4N against the oracle, 1e-13 * 4N against
the classic route (BODGE_AMD_SWEEP_COMPOSED=0) on the same vectors.

Lattices.  A 2-lane window owns 26 in-plane positions, a 4-lane window 10.  The stencil kernels are only eligible from 8
planes of 24 positions on (plans.hpp ensure_stencil), and a launch cuts at most one x-segment per 8 planes: (4, 11, 1) and
the periodic (8, 12, 1) therefore run the one-step kernels whatever the knobs say - they are held to the same numbers, and
to `composed == 0` - and on (9, 27, 1) BODGE_AMD_SWEEP_SEGMENTS=3 still cuts one segment.  (24, 31, 1) and the periodic
(24, 24, 1) are the same edge cases at sizes where the sweep engages with three segments: one position past three 4-lane
windows / a short second 2-lane window, seams with recomputed planes on either side, both rings.
"""

import numpy as np
import pytest

from oracle import cheb_ref

pytestmark = pytest.mark.gpu

STEPS = [1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 130]
VECTORS = [1, 4, 5, 8]
SEED = 7
# (shape, periodic, whether the three-step sweep engages when forced)
LATTICES = [((9, 27, 1), False, True), ((4, 11, 1), False, False), ((8, 12, 1), True, False),
            ((24, 31, 1), False, True), ((24, 24, 1), True, True)]
MODELS = ["swave", "peierls"]
CASES = [(shape, periodic, engages, model) for shape, periodic, engages in LATTICES for model in MODELS]
CASE_IDS = [f"{'x'.join(map(str, shape))}{'p' if periodic else ''}-{model}" for shape, periodic, _, model in CASES]


def _system(api, shape, periodic, model):
    lattice = api.CubicLattice(shape)
    system = api.Hamiltonian(lattice)
    with system as (H, Δ):
        H.set_sites(3.0 * api.σ0 - 0.05 * api.σ3)
        Δ.set_sites(-0.1 * api.jσ2)
        if model == "swave":  # real table, Rademacher vectors: RealPHMode
            H.set_bonds(-1.0 * api.σ0)
        else:  # Peierls phases on the x bonds, Z4 vectors: ComplexPHMode
            pairs = lattice.bond_array(axis=0, coords=True)
            phase = np.where(pairs[:, 1, 0] > pairs[:, 0, 0], np.exp(0.3j), np.exp(-0.3j))
            H.set_bonds(-phase[:, None, None] * api.σ0, axis=0)
            H.set_bonds(-1.0 * api.σ0, axis=1)
        if periodic:
            H.set_edges(-1.0 * api.σ0)
    return system


class Case:
    def __init__(self, api, solver_cls, shape, periodic, engages, model):
        system = _system(api, shape, periodic, model)
        self.bsr = system.matrix("bsr")
        self.n = self.bsr.shape[0]
        self.scale = cheb_ref.spectral_bound(self.bsr)
        self.kind = cheb_ref.VEC_RADEMACHER if model == "swave" else cheb_ref.VEC_Z4
        self.engages = engages
        self.dev = solver_cls.from_hamiltonian(system)
        # the oracle once, at the longest run and the widest call: shorter runs and narrower calls are its leading part
        start = cheb_ref.random_block(self.n, SEED, range(max(VECTORS)), self.kind)
        self.ref = cheb_ref.recurrence_dots(self.bsr, self.scale, 2 * max(STEPS), start)

    def run(self, steps, vectors):
        out = self.dev.dots_random(self.scale, steps, vectors, seed=SEED, kind=self.kind)
        return out, self.dev.perf()


@pytest.fixture(scope="module")
def cases(api, hip_library):
    from bodge_amd.solver import DeviceSolver

    built = {}

    def get(shape, periodic, engages, model):
        key = (shape, periodic, model)
        if key not in built:
            built[key] = Case(api, DeviceSolver, shape, periodic, engages, model)
        return built[key]

    yield get
    for case in built.values():
        case.dev.close()


def _distance(a, b, steps, vectors):
    return max(np.abs(a[0] - b[0][:steps, :vectors]).max(), np.abs(a[1] - b[1][:steps, :vectors]).max())


def _both_routes(case, knobs, steps, vectors, label):
    """One composed and one classic call under the knobs in force; the composed one against the oracle and the classic one."""
    knobs.set("BODGE_AMD_SWEEP_COMPOSED", "1")
    got, perf = case.run(steps, vectors)
    knobs.set("BODGE_AMD_SWEEP_COMPOSED", "0")
    classic, classic_perf = case.run(steps, vectors)
    knobs.unset("BODGE_AMD_SWEEP_COMPOSED")
    to_oracle = _distance(got, case.ref, steps, vectors) / case.n
    to_classic = _distance(got, classic, steps, vectors) / case.n
    print(f"{label} steps {steps} vectors {vectors}: {to_oracle:.2e} * 4N from the oracle, {to_classic:.2e} * 4N from the classic route")
    assert perf["composed"] == (1 if case.engages else 0) and classic_perf["composed"] == 0, (perf, classic_perf)
    assert perf["steps_per_launch"] == classic_perf["steps_per_launch"] == (3 if case.engages else 1)
    assert to_oracle <= 1e-12 and to_classic <= 1e-13
    return got, perf, classic_perf


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("shape,periodic,engages,model", CASES, ids=CASE_IDS)
def test_composed_sweep_matches_oracle_and_classic_route(cases, knobs, shape, periodic, engages, model, steps):
    """Every run length (first sweep alone, tails of one and two steps, chunk boundaries at 63) and every width of call
    (a partly empty lane group, a full one, two groups of which one is thin, two full ones on two streams)."""
    case = cases(shape, periodic, engages, model)
    knobs.set("BODGE_AMD_SWEEP", "1")
    for vectors in VECTORS:
        _both_routes(case, knobs, steps, vectors, "default")
    assert np.array_equal(case.run(1, 1)[0][0], [[float(case.n)]])  # d_0 = 4N exactly


KNOB_SETS = [
    {"BODGE_AMD_SWEEP_SEGMENTS": "1"},
    {"BODGE_AMD_SWEEP_SEGMENTS": "3"},
    {"BODGE_AMD_SWEEP_SEGMENTS": "3", "BODGE_AMD_SWEEP_ZIGZAG": "0"},
    {"BODGE_AMD_SWEEP_SEGMENTS": "3", "BODGE_AMD_ALTERNATE": "0"},
    {"BODGE_AMD_SWEEP_SEGMENTS": "1", "BODGE_AMD_SWEEP_ZIGZAG": "0", "BODGE_AMD_ALTERNATE": "0"},
    {"BODGE_AMD_STREAMS": "1"},
    {"BODGE_AMD_SWEEP_LANES": "2"},  # 26-position windows: the form the flagship workload runs
    {"BODGE_AMD_SWEEP_LANES": "2", "BODGE_AMD_SWEEP_SEGMENTS": "3"},
    {"BODGE_AMD_SWEEP_LANES": "2", "BODGE_AMD_SWEEP_SEGMENTS": "3", "BODGE_AMD_SWEEP_ZIGZAG": "0", "BODGE_AMD_ALTERNATE": "0"},
    {"BODGE_AMD_SWEEP_LANES": "2", "BODGE_AMD_STREAMS": "1"},
]


@pytest.mark.parametrize("knob_set", KNOB_SETS, ids=lambda k: ",".join(f"{n[10:]}={v}" for n, v in k.items()))
@pytest.mark.parametrize("shape,periodic,engages,model", CASES, ids=CASE_IDS)
def test_composed_sweep_across_seams_directions_streams_and_lane_counts(cases, knobs, shape, periodic, engages, model, knob_set):
    """The in-place update across segment seams and their recomputed planes, with zigzag and alternation on and off, on one
    stream and two, with 4 and 2 lanes per site."""
    case = cases(shape, periodic, engages, model)
    knobs.set("BODGE_AMD_SWEEP", "1")
    knobs.update(knob_set)
    for steps, vectors in [(7, 5), (65, 8), (6, 1)]:
        _, perf, _ = _both_routes(case, knobs, steps, vectors, str(knob_set))
        if engages:
            assert perf["lanes_per_row"] == int(knob_set.get("BODGE_AMD_SWEEP_LANES", 4))


@pytest.mark.parametrize("shape,periodic,engages,model", CASES, ids=CASE_IDS)
def test_composed_sweep_bits_do_not_depend_on_how_the_start_block_is_made_or_what_is_kept(cases, knobs, shape, periodic, engages, model):
    """Bit-identical: a repeated call (the buffers left half written by the call before), the start block written by the
    fill kernel instead of generated in the first sweep, and the last launch storing its vectors."""
    case = cases(shape, periodic, engages, model)
    knobs.set("BODGE_AMD_SWEEP", "1")
    knobs.set("BODGE_AMD_SWEEP_COMPOSED", "1")
    for lanes in ("4", "2"):
        knobs.set("BODGE_AMD_SWEEP_LANES", lanes)
        for steps, vectors in [(65, 8), (7, 5), (6, 4), (2, 1)]:
            first, perf = case.run(steps, vectors)
            assert perf["composed"] == (1 if engages else 0)
            again, _ = case.run(steps, vectors)
            knobs.set("BODGE_AMD_SWEEP_GEN", "0")
            filled, _ = case.run(steps, vectors)
            knobs.unset("BODGE_AMD_SWEEP_GEN")
            knobs.set("BODGE_AMD_KEEP_LAST", "1")
            kept, kept_perf = case.run(steps, vectors)
            knobs.unset("BODGE_AMD_KEEP_LAST")
            for other in (again, filled, kept):
                assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1])
            assert perf["bytes_moved"] < kept_perf["bytes_moved"]  # (the last launch's stores are counted)


def test_perf_record_and_byte_accounting_of_a_composed_run(cases, knobs):
    """`composed`, `steps_per_launch`, and the algorithmic bytes: a composed launch is the stencil words plus THREE vector
    passes; the first sweep generates u_0 and writes it with u_1 (two passes), the last launch of a run only reads u_k."""
    case = cases((24, 31, 1), False, True, "swave")
    knobs.set("BODGE_AMD_SWEEP", "1")
    knobs.set("BODGE_AMD_SWEEP_COMPOSED", "0")
    _, classic = case.run(10, 8)
    knobs.set("BODGE_AMD_SWEEP_COMPOSED", "1")
    _, perf = case.run(10, 8)
    assert perf["composed"] == 1 and perf["steps_per_launch"] == 3 and classic["composed"] == 0 and classic["steps_per_launch"] == 3
    assert perf["launches"] == classic["launches"] == perf["sweeps"] == 4 and perf["persistent"] == 0
    one_pass = 4 * perf["lanes_per_row"] * 16 * (case.n // 4)  # 4 components x lanes x 16 bytes per site
    assert classic["bytes_per_launch"] - perf["bytes_per_launch"] == one_pass
    fixed = perf["bytes_per_launch"] - 3 * one_pass  # stencil words and the block table
    # 10 steps = sweeps of 3, 3, 3 and a tail of 1: (u_0, u_1 written) + 2 x (u_k, u_{k-1} read, u_{k+1} written) + (u_k read)
    assert perf["bytes_moved"] == pytest.approx(4 * fixed + (2 + 3 + 3 + 1) * one_pass, rel=1e-12)
    knobs.set("BODGE_AMD_SWEEP_GEN", "0")  # the fill kernel writes u_0: the first sweep reads it and writes u_1
    _, filled = case.run(10, 8)
    assert filled["bytes_moved"] == pytest.approx(perf["bytes_moved"], rel=1e-12)
    knobs.unset("BODGE_AMD_SWEEP_GEN")
    # the route is for random-start runs with one launch per sweep: a unit-start call and a persistent launch stay classic
    rows = np.array([4 * (5 * 31 + 7), 4 * (12 * 31 + 20) + 2], dtype=np.int64)
    d_unit, e_unit = case.dev.dots_unit(case.scale, 9, rows)
    assert case.dev.perf()["composed"] == 0
    ref = cheb_ref.recurrence_dots(case.bsr, case.scale, 18, cheb_ref.unit_block(case.n, rows))
    assert np.abs(d_unit - ref[0]).max() <= 1e-13 and np.abs(e_unit - ref[1]).max() <= 1e-13
    knobs.set("BODGE_AMD_MARCH", "1")
    _, marched = case.run(10, 8)
    assert marched["composed"] == 0 and marched["persistent"] == 1
    knobs.unset("BODGE_AMD_MARCH")
    knobs.set("BODGE_AMD_SWEEP", "0")
    _, one_step = case.run(10, 8)
    assert one_step["composed"] == 0 and one_step["steps_per_launch"] == 1
