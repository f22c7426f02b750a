"""correlation() on the GPU: bdg_moment_matrix against the numpy restatement and the dense double sum in every kernel
form and arithmetic mode, the shapes at which the Gram kernel can go wrong, batches and moment blocking bit for bit,
and the Kubo response end to end."""

import functools

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import correlation as corr

import correlation_cases as cases

pytestmark = pytest.mark.gpu

ARITHMETIC = {
    "packed": {},
    "real_full": {"BODGE_AMD_PH": "0"},
    "complex_packed": {"BODGE_AMD_REAL": "0"},
    "complex_full": {"BODGE_AMD_REAL": "0", "BODGE_AMD_PH": "0"},
}
SYSTEMS = ["disordered_real", "disordered_complex", "dictionary", "cube"]


def _triples(system, A, B):
    return corr.as_operator(system, A), corr.as_operator(system, B)


def _device(system, A, B, M, X):
    """μ from the device for the operators and start vectors of a case (X = None: every unit row), and the perf record."""
    solver = system._solver()
    a, b = _triples(system, A, B)
    scale = cases.scale_of(system)
    if X is None:
        mu = solver.moment_matrix(scale, M, a, b, rows=np.arange(solver.dim, dtype=np.int64))
    else:
        mu = solver.moment_matrix(scale, M, a, b, x=X)
    return mu, solver.perf()


# ------------------------------------------------------------------ against the restatement and dense
# The tolerance of the device result is 20 times the distance of the numpy restatement (correlation_cases.
# restated_moment_matrix, sparse H) from the dense double sum over the eigenpairs of numpy.linalg.eigh, measured in the
# test on the case it runs; the pin of tests/test_correlation_host.py (1e-13 of the largest entry) is asserted first.
@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("form", ["dictionary", "streamed"])
@pytest.mark.parametrize("arithmetic", sorted(ARITHMETIC))
@pytest.mark.parametrize("pair", ["jj", "js"])
def test_device_matches_restatement_and_dense(name, form, arithmetic, pair, knobs):
    knobs.update(ARITHMETIC[arithmetic])
    if form == "streamed":
        knobs.set("BODGE_AMD_DICT", "0")
    system = cases.SYSTEMS[name]()  # (a fresh handle: the dictionary switch is read at upload)
    M = cases.M_SMALL
    restated, dense, largest, own = cases.references(name, pair, M)
    assert largest > 1e-3 and own <= 1e-13 * largest
    A, B, X = cases.operator_pair(system, pair)
    got, perf = _device(system, A, B, M, X)
    tolerance = 20 * own
    print(name, form, arithmetic, pair, "max|mu|", largest, "device - restated", np.abs(got - restated).max(),
          "device - dense", np.abs(got - dense).max(), "tolerance", tolerance)
    assert np.abs(got - restated).max() <= tolerance and np.abs(got - dense).max() <= tolerance

    n_vectors = 4 * system.lattice.size if X is None else len(X)
    lanes = perf["lanes_per_row"]
    batches = -(-n_vectors // lanes)
    assert perf["correlation"] == 1
    assert perf["apply"] == perf["clenshaw"] == perf["green"] == perf["green_local"] == 0
    assert perf["gram_flops"] == batches * 8.0 * M * M * (4 * system.lattice.size * lanes)
    assert perf["gram_ms"] > 0 and perf["window_ms"] > 0
    assert perf["launches"] == batches * (2 * M - 1)
    is_real = np.abs(np.asarray(system.matrix("dense")).imag).max() == 0
    assert perf["real_arithmetic"] == (1 if is_real and "complex" not in arithmetic else 0)
    assert lanes == (4 if X is not None else 32 if perf["real_arithmetic"] else 64)
    if form == "streamed":
        assert perf["dict_blocks"] == 0
    elif name in ("dictionary", "cube"):
        assert perf["dict_blocks"] > 0
    if arithmetic.endswith("full"):
        assert perf["ph_packed"] == 0


# ------------------------------------------------------------------ shapes of the Gram kernel
M_SHAPES = [1, 2, 17, 65, 130]


@functools.lru_cache(maxsize=None)
def _shape_references(name):
    """J_x, five unit vectors, and the restated and the dense μ at the largest M of the shape cases: computed once."""
    system = cases.system_of(name)
    scale = cases.scale_of(system)
    jx = corr.current_operator(system, 0)
    X = cases.unit_vectors(system, 5, seed=2)
    restated = cases.restated_moment_matrix(system.matrix("csr"), scale, jx, jx, max(M_SHAPES), X)
    dense = cases.dense_moment_matrix(system, scale, jx, jx, max(M_SHAPES), X)
    return jx, X, restated, dense


@pytest.mark.parametrize("name", ["cube", "dictionary"])
@pytest.mark.parametrize("M", M_SHAPES)
@pytest.mark.parametrize("lanes", [4, 8, 32])
@pytest.mark.parametrize("slice_entries", [None, 100, 4])
def test_gram_kernel_shapes(name, M, lanes, slice_entries, knobs):
    """Moments that fill no tile, one tile and a bit, two tiles and a bit; 5 vectors in batches of 4, 8 and 32 lanes (two
    batches, padding columns); slices of the default length (one or two per row), of 100 and of 4 entries (many, the
    last one ragged: K = 4·nb·lanes is no multiple of 100).

    The moments with n, m < M do not depend on M (forward recurrences), so one restatement and one dense matrix at
    M = 130 serve all cases through their leading M x M corner, and the tolerance is that of the other tests: 20 times the
    distance of the two, measured here on the 130 x 130 matrix (cube 3.5e-14, dictionary 2.7e-14 of a largest entry of 7.1
    and 8.6).  Measured per corner instead it degenerates: at M = 1 the two references agree to 9.6e-17 on `dictionary`,
    half a unit in the last place of the one entry, by luck and not by accuracy."""
    system = cases.system_of(name)
    jx, X, restated, dense = _shape_references(name)
    largest, own = np.abs(dense).max(), np.abs(restated - dense).max()
    assert largest > 1e-3 and own <= 1e-13 * largest
    restated, dense = restated[:M, :M], dense[:M, :M]
    if slice_entries is not None:
        knobs.set("BODGE_AMD_CORRELATION_SLICE", str(slice_entries))
    solver = system._solver()
    solver.set_lanes_per_row(lanes)
    try:
        got, perf = _device(system, jx, jx, M, X)
    finally:
        solver.set_lanes_per_row(0)
    tolerance = 20 * own
    print(name, M, lanes, slice_entries, "device - restated", np.abs(got - restated).max(), "device - dense",
          np.abs(got - dense).max(), "tolerance", tolerance)
    assert got.shape == (M, M) and perf["lanes_per_row"] == lanes
    assert np.abs(got - restated).max() <= tolerance and np.abs(got - dense).max() <= tolerance
    batches = -(-5 // lanes)
    assert perf["launches"] == batches * (2 * M - 1) and perf["vector_steps"] == 5 * (2 * M - 1)
    assert perf["gram_flops"] == batches * 8.0 * M * M * (4 * system.lattice.size * lanes)


def test_slice_must_be_a_multiple_of_four(knobs):
    system = cases.system_of("cube")
    jx = corr.current_operator(system, 0)
    for bad in ("6", "0", "-4"):
        knobs.set("BODGE_AMD_CORRELATION_SLICE", bad)
        with pytest.raises(ValueError, match="multiple of 4"):
            system.correlation(jx, jx, moments=4)


# ------------------------------------------------------------------ batches
def test_batches_accumulate_and_repeat_bit_for_bit():
    system = cases.system_of("disordered_complex")
    jx = corr.current_operator(system, 0)
    M = cases.M_SMALL
    X = cases.unit_vectors(system, 70, seed=3)
    single = np.array([_device(system, jx, jx, M, X[v : v + 1])[0] for v in range(70)])
    for count in (1, 5, 70):
        got, perf = _device(system, jx, jx, M, X[:count])
        expected = single[:count].sum(axis=0)
        largest = np.abs(expected).max()
        print(count, perf["lanes_per_row"], perf["launches"], np.abs(got - expected).max() / largest)
        assert np.abs(got - expected).max() <= 1e-13 * largest
        assert perf["lanes_per_row"] == {1: 4, 5: 8, 70: 64}[count]
        assert perf["launches"] == -(-count // perf["lanes_per_row"]) * (2 * M - 1)
        assert perf["vector_steps"] == count * (2 * M - 1)
        again, _ = _device(system, jx, jx, M, X[:count])
        assert np.array_equal(got, again)
    # the public call takes the layouts of apply and sums over the vectors as given
    public = system.correlation(jx, jx, moments=M, vectors=X[:5].T)
    assert public.info["route"] == "vectors" and public.info["vectors"] == 5
    assert np.array_equal(public.mu, _device(system, jx, jx, M, X[:5])[0])


# ------------------------------------------------------------------ moment blocking
def test_moment_blocking_gives_the_unblocked_moments(knobs):
    """disordered_300, M = 200, 8 vectors (8 lanes: a panel row is 4·300·8 = 9600 entries, 153 600 bytes).  A budget of
    exactly two panels of 64 rows forces Mb = 64 (chunks of 64, 64, 64 and 8 moments): the same μ to 1e-14 of its largest
    entry - and, as the slices do not depend on the chunks, expected bit for bit (printed).  Below two panels of 64 rows
    at 4 lanes the call gives up and names the bytes."""
    system = cases.system_of("disordered_300")
    jx = corr.current_operator(system, 0)
    X = cases.unit_vectors(system, 8, seed=4)
    M = 200
    whole, perf = _device(system, jx, jx, M, X)
    assert perf["lanes_per_row"] == 8 and perf["launches"] == 2 * M - 1
    row_bytes = 4 * 300 * 8 * 16
    knobs.set("BODGE_AMD_CORRELATION_BYTES", str(2 * 64 * row_bytes))
    blocked, perf = _device(system, jx, jx, M, X)
    largest = np.abs(whole).max()
    print("blocked - whole", np.abs(blocked - whole).max() / largest, "bit-identical:", np.array_equal(blocked, whole))
    assert perf["lanes_per_row"] == 8
    assert perf["launches"] == (M - 1) + 4 * M  # Y once, X once per chunk of Y
    assert perf["gram_flops"] == 8.0 * M * M * 9600  # (the chunks tile the same M x M entries)
    assert np.abs(blocked - whole).max() <= 1e-14 * largest
    # too small for 64 rows at 8 lanes: the batch is narrowed to 4 lanes ...
    knobs.set("BODGE_AMD_CORRELATION_BYTES", str(2 * 64 * row_bytes - 1))
    narrowed, perf = _device(system, jx, jx, M, X)
    assert perf["lanes_per_row"] == 4 and np.abs(narrowed - whole).max() <= 1e-13 * largest
    # ... and below that nothing fits
    knobs.set("BODGE_AMD_CORRELATION_BYTES", str(64 * row_bytes - 1))
    with pytest.raises(ValueError, match=str(64 * row_bytes)):
        _device(system, jx, jx, M, X)


# ------------------------------------------------------------------ end to end
def test_response_end_to_end_matches_the_dense_double_sum():
    system = cases.system_of("disordered_complex")
    jx = corr.current_operator(system, 0)
    moments = system.correlation(jx, jx, temperature=0.5, broadening=0.5)
    assert isinstance(moments, ba.MomentMatrix) and moments.info["route"] == "exact"
    assert moments.mu.shape == (moments.moments, moments.moments) and moments.moments >= 300
    omegas = [0.0, 0.7]
    got = moments.response(omegas, 0.5, 0.5)
    for w, value in zip(omegas, got):
        exact = cases.dense_response(system, jx, jx, w, 0.5, 0.5)
        print("omega", w, value, exact, abs(value - exact) / abs(exact))
        assert abs(value - exact) <= 1e-11 * abs(exact)
    # Hamiltonians are operators too: Tr[T_n H T_m H] contracted with F = 1 is Tr[H²]
    twice = system.correlation(system, system, moments=8)
    h = system.matrix("csr")
    assert abs(twice.expand(lambda x, y: np.ones(np.broadcast(x, y).shape)) - (h @ h).diagonal().sum()) <= 1e-10


def test_stochastic_trace_lies_within_its_standard_error():
    system = cases.system_of("disordered_300")
    jx = corr.current_operator(system, 0)
    M, R = 64, 64
    exact = system.correlation(jx, jx, moments=M)
    estimate = system.correlation(jx, jx, moments=M, vectors=R, seed=3)
    assert estimate.info["route"] == "stochastic" and estimate.info["vectors"] == R
    again = system.correlation(jx, jx, moments=M, vectors=R, seed=3)
    assert np.array_equal(estimate.mu, again.mu)
    assert not np.array_equal(estimate.mu, system.correlation(jx, jx, moments=M, vectors=R, seed=4).mu)
    X = corr.random_phase_vectors(system, R, seed=3)
    each = np.array([_device(system, jx, jx, M, X[v : v + 1])[0] for v in range(R)])
    largest = np.abs(exact.mu).max()
    assert np.abs(each.mean(axis=0) - estimate.mu).max() <= 1e-13 * largest
    spread = np.sqrt((np.abs(each - each.mean(axis=0)) ** 2).sum(axis=0) / (R - 1))
    standard_error = spread / np.sqrt(R)
    deviation = np.abs(estimate.mu - exact.mu)
    print("largest deviation in standard errors", (deviation / (standard_error + 1e-300)).max(), "largest |mu|", largest)
    assert (deviation <= 6 * standard_error + 1e-12 * largest).all()
    assert deviation.max() > 1e-9 * largest  # (an estimate, not the trace itself)


# ------------------------------------------------------------------ refusals that need a handle
def test_operators_are_checked_against_the_matrix_size():
    system = cases.system_of("cube")
    solver = system._solver()
    n = system.lattice.size
    good = corr.as_operator(system, corr.current_operator(system, 0))
    empty = (np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 4, 4), dtype=np.complex128))
    assert np.abs(solver.moment_matrix(1.0, 3, good, empty, rows=[0, 5])).max() == 0  # B = 0
    short = (good[0].copy(), good[1], good[2])
    short[0][-1] -= 1
    with pytest.raises(ValueError, match="operator A: indptr"):
        solver.moment_matrix(6.0, 3, short, good, rows=[0])
    outside = (good[0], good[1].copy(), good[2])
    outside[1][3] = n
    with pytest.raises(ValueError, match="operator B: column index"):
        solver.moment_matrix(6.0, 3, good, outside, rows=[0])
    with pytest.raises(ValueError, match="start row"):
        solver.moment_matrix(6.0, 3, good, good, rows=[4 * n])


def test_slab_handles_are_refused():
    from bodge_amd.solver import SlabGroup

    system = cases.uniform_swave((8, 4, 1))
    with SlabGroup.from_hamiltonian(system, 2) as group:
        member = group.members[0]
        empty = (np.zeros(member.n_sites + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 4, 4)))
        with pytest.raises(ValueError, match="slab"):
            member.moment_matrix(1.0, 2, empty, empty, rows=[0])


def test_a_lanczos_run_on_the_handle_is_ended():
    system = cases.SYSTEMS["dictionary"]()
    solver = system._solver()
    solver.lanczos_begin(2, max_iter=64)
    solver.lanczos_advance(2)
    jx = corr.current_operator(system, 0)
    system.correlation(jx, jx, moments=4, vectors=2)
    with pytest.raises(ValueError, match="lanczos_begin"):
        solver.lanczos_advance(1)
