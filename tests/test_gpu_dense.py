"""The dense eigensolvers of the library - one-sided Jacobi (csrc/kernels.hpp, dense.hpp) and one-stage Householder
(csrc/tridiag.hpp) - on matrices whose spectrum is known without trusting any eigensolver (tests/dense_cases.py),
against the derived bounds of DESIGN §19.  The two-stage band route (csrc/twostage.hpp) is NOT covered above 66 rows:
at n = 68, its first size with a band, it returned eigenvalues 1e-3 off on `toeplitz` and ended `split` with an illegal
memory access; until the cause is known no case here enters it.

    eigenvalues      max |w - truth|              <= m eps |A|        m = max(n, 64), eps = 2^-52, |A| = max |truth|
    residual         |A z - λ z|_2                <= m eps |A|        for every returned vector
    orthonormality   |z_i^H z_j - δ_ij|           <= m eps            Jacobi; the inverse-iteration routes between levels
                                                                       further apart than their cluster criterion:
                                                                       max(m eps, 2 m eps |A| / |λ_i - λ_j|)

numpy.linalg.eigh stays under 0.3 of each (tests/test_dense_host.py).  Every test prints a line `dense-stress <route>
<case> device: <ratios> | numpy: <ratios>`; the lines of one run are profiles/dense_stress_ratios.txt."""

import numpy as np
import pytest

import dense_cases as dc
from dense_cases import Case, EPS

pytestmark = pytest.mark.gpu


def _solver(case):
    from bodge_amd.solver import DeviceSolver

    return DeviceSolver(*dc.bsr_arrays(dc.matrix(case)))


def _judge(route, case, w, z=None, first=0, gap_term=True, numpy_too=True, work_norm=None):
    got = dc.ratios(case, w, z, first, gap_term, work_norm)
    ref = str(dc.reference_ratios(case)) if numpy_too else "-"
    print(f"dense-stress {route:<34} {case.id:<30} device: {got} | numpy: {ref}", flush=True)
    assert got.worst() <= 1.0, (route, case.id, str(got))
    return got


def _variants(sizes, phases=(False, True), scaled=True, real0=True):
    """(case, complex arithmetic forced on a real matrix) over the sizes."""
    out = []
    for n in sizes:
        cases = dc.cases_at(n, phases, scaled)
        out += [(case, False) for case in cases]
        if real0:
            out += [(case, True) for case in cases if not case.phases and not case.scale]
    return out


def _ids(variants):
    return [case.id + ("-real0" if real0 else "") for case, real0 in variants]


def _route(knobs, route, real0=False, **more):
    knobs.set("BODGE_AMD_EIGH", "jacobi" if route == "jacobi" else "tridiagonal")
    if route != "jacobi":
        knobs.set("BODGE_AMD_EIGH_STAGES", "2" if route == "two-stage" else "1")
    if real0:
        knobs.set("BODGE_AMD_EIGH_REAL", "0")
    knobs.update({f"BODGE_AMD_EIGH_{name}": value for name, value in more.items()})


def _tag(route, real0=False, **more):
    return route + ("/real0" if real0 else "") + "".join(f"/{k.lower()}={v}" for k, v in more.items())


def _eigenpairs(knobs, solver, case, tag, bound=-np.inf):
    """`eigh` and `eigh_above` on one handle of a forced tridiagonal route: the route has run (it refuses all vectors
    through `eigh`), the eigenvalues of the two calls are bit-identical, the vectors are those of w[first:]."""
    n = case.n
    with pytest.raises(ValueError):
        solver.eigh(vectors=True)
    w, none = solver.eigh(vectors=False)
    assert none is None
    w2, z = solver.eigh_above(bound)
    assert w2.tobytes() == w.tobytes()
    first = n - z.shape[1]
    assert z.shape == (n, n - first) and np.all(w[first:] > bound) and np.all(w[:first] <= bound)
    return w, z, first, _judge(tag, case, w, z, first)


# ------------------------------------------------------------------ Jacobi
JACOBI = _variants(dc.JACOBI_SIZES)


@pytest.mark.parametrize("case,real0", JACOBI, ids=_ids(JACOBI))
def test_jacobi(knobs, case, real0):
    """The Jacobi kernels with all vectors: real, complex (phases) and complex arithmetic on a real matrix.  The `scaled`
    cases are the regression test of the shift (it was 1.5 b + 1, b the Gershgorin bound: for |A| = 2^-40 the eigenvalues
    of A + shift lost eps x 1 instead of eps |A| - ratios of 1e10), every dense case that of the rotation's norm (cs, sn
    with cs^2 + sn^2 - 1 of positive mean let |v_p| and |g_p| drift: eigenvalue ratios up to 8.8, orthonormality 4.7)."""
    _route(knobs, "jacobi", real0)
    w, z = _solver(case).eigh(vectors=True)
    assert z.shape == (case.n, case.n)
    assert np.iscomplexobj(z) and (case.phases or real0 or np.all(z.imag == 0))
    _judge(_tag("jacobi", real0), case, w, z, gap_term=False)


@pytest.mark.parametrize("n,phases", [(2048, False), (2048, True), (2052, False), (2052, True)])
def test_jacobi_at_the_kernel_boundary(knobs, n, phases):
    """2048 rows: the last size of the 8-elements-per-thread kernel; 2052: the first of the wide one.  `clement`, whose
    truth is analytic."""
    case = Case("clement", n, phases)
    _route(knobs, "jacobi")
    w, z = _solver(case).eigh(vectors=True)
    _judge("jacobi", case, w, z, gap_term=False, numpy_too=False)


# ------------------------------------------------------------------ one stage
ONE_STAGE = _variants(dc.ONE_STAGE_SIZES)


@pytest.mark.parametrize("case,real0", ONE_STAGE, ids=_ids(ONE_STAGE))
def test_one_stage(knobs, case, real0):
    """K9, eigenvalues and ALL vectors (`eigh_above(-inf)`: more than the wrapper's first capacity n/2 + 8, so its second
    attempt runs).  `zero` is the regression test of the pivot floor eps |T|, which was 0 for the zero matrix: 0 / 0.

    `degenerate`, `split` and `glued` are the regression tests of the vectors in many-fold levels: with the
    row-scaled pivoting of the LU and one orthonormalisation of independently iterated members they came out with 1e-13 to
    1e-5 of OTHER levels (residual ratios up to 1e11 on `degenerate`, 7e4 on `split`, 78 on `glued`)."""
    _route(knobs, "one-stage", real0)
    _, z, first, _ = _eigenpairs(knobs, _solver(case), case, _tag("one-stage", real0))
    assert first == 0
    assert case.phases or real0 or np.all(z.imag == 0)


DEFERRED = [(case, defer) for n in (68, 132) for case in dc.cases_at(n, scaled=False) for defer in (1, 2, 3, 4)]


@pytest.mark.parametrize("case,defer", DEFERRED, ids=[f"{case.id}-defer{defer}" for case, defer in DEFERRED])
def test_one_stage_deferred_updates(knobs, case, defer):
    """`td_fused_pass<T, 1..4>`: the rank-2 updates of up to four steps kept pending (the default only from 5000 rows);
    67 and 131 steps leave a last run with fewer pending pairs than `defer`."""
    _route(knobs, "one-stage", DEFER=defer)
    _eigenpairs(knobs, _solver(case), case, _tag("one-stage", DEFER=defer))


CHUNKED = [(case, chunks) for case in dc.cases_at(132, scaled=False) for chunks in ("1", "3,16")]


@pytest.mark.parametrize("case,chunks", CHUNKED, ids=[f"{case.id}-chunks{chunks}" for case, chunks in CHUNKED])
def test_one_stage_back_transformation_chunks(knobs, case, chunks):
    """One row chunk per pass of the back-transformation, and three ragged ones of at least 16 rows."""
    _route(knobs, "one-stage", CHUNKS=chunks)
    _eigenpairs(knobs, _solver(case), case, _tag("one-stage", CHUNKS=chunks))


# ------------------------------------------------------------------ two stage
@pytest.mark.parametrize("n", [36, 64])
def test_two_stage_below_the_first_band_is_the_one_stage_route(knobs, n):
    """Up to 66 rows there is no band: the switch quietly gives the one-stage result bit for bit."""
    for case in (Case("wilkinson", n), Case("clement", n)):
        solver = _solver(case)
        _route(knobs, "two-stage")
        two_w, two_z = solver.eigh_above(-np.inf)
        _route(knobs, "one-stage")
        one_w, one_z = solver.eigh_above(-np.inf)
        assert two_w.tobytes() == one_w.tobytes() and two_z.tobytes() == one_z.tobytes()


# ------------------------------------------------------------------ 1028 rows: td_vector_step has 1024 threads
@pytest.mark.parametrize("family,phases", [("toeplitz", False), ("toeplitz", True), ("glued", False), ("glued", True)])
def test_1028_rows(knobs, family, phases):
    case = Case(family, 1028, phases)
    _route(knobs, "one-stage")
    _, _, first, _ = _eigenpairs(knobs, _solver(case), case, "one-stage")
    assert first == 0


# ------------------------------------------------------------------ default routing
@pytest.mark.parametrize("n", [512, 516])
def test_default_routing(knobs, n):
    """Eigenvalues alone: Jacobi up to 512 rows, the tridiagonal route above - each bit-identical to the forced route.
    Without vectors the Jacobi route has no |v_p| to divide the rotations' effect on |g_p| out with: its eigenvalues are
    the singular values of G = A + 1.5 b I to m eps |G|_2, and that is their bound here."""
    case = Case("toeplitz", n)
    solver = _solver(case)
    w, _ = solver.eigh(vectors=False)
    _judge("default/eigenvalues", case, w, work_norm=dc.shifted_norm(case) if n <= 512 else None)
    _route(knobs, "jacobi" if n <= 512 else "one-stage")
    forced, _ = solver.eigh(vectors=False)
    assert forced.tobytes() == w.tobytes()
    _route(knobs, "one-stage" if n <= 512 else "jacobi")
    other, _ = solver.eigh(vectors=False)
    assert other.tobytes() != w.tobytes()  # (the two routes round differently: the comparison above can tell them apart)
    knobs.clear()
    w2, z = solver.eigh_above(-np.inf)
    assert z.shape == (n, n)
    _judge("default/eigh_above", case, w2, z, gap_term=n > 512)


# ------------------------------------------------------------------ eigh_above bounds
def _odd_bound(case):
    """A bound in the widest gap near the middle of the spectrum that leaves an odd number of levels above it."""
    exact = dc.truth(case).astype(np.float64)
    n = case.n
    ks = [k for k in range(n // 4, 3 * n // 4) if (n - k) % 2 == 1]
    k = max(ks, key=lambda k: exact[k] - exact[k - 1])
    assert exact[k] - exact[k - 1] > 1e-8 * np.abs(exact).max()  # (1e6 times the bound on a level: the count is certain)
    return 0.5 * (exact[k] + exact[k - 1]), n - k


BOUNDED = [(route, Case(family, n, phases)) for route, all_phases in (("one-stage", (False, True)),)
           for n in (68, 132) for family in ("toeplitz", "clement", "ladder_above", "graded", "degenerate") for phases in all_phases]


@pytest.mark.parametrize("route,case", BOUNDED, ids=[f"{route}-{case.id}" for route, case in BOUNDED])
def test_eigh_above_bounds(knobs, route, case):
    """The bounds of `eigh_above`: 0.0; one that leaves an odd number of vectors (the real route stores column pairs);
    one above the whole spectrum; and on `degenerate` 1.0, inside an exactly degenerate level - however many members
    come out above it, the vectors returned are those of w[first:] - and 2.5 for the odd count."""
    _route(knobs, route)
    solver = _solver(case)
    exact = dc.truth(case).astype(np.float64)
    _, _, first, _ = _eigenpairs(knobs, solver, case, route + "/bound=0", bound=0.0)
    assert first == int(np.count_nonzero(exact <= 0.0))  # (no case has a level within rounding of 0)
    if case.family == "degenerate":
        _, _, first, _ = _eigenpairs(knobs, solver, case, route + "/bound=1", bound=1.0)
        assert 0 <= first <= case.n // 2
        _, _, first, _ = _eigenpairs(knobs, solver, case, route + "/bound=2.5", bound=2.5)
        assert first == case.n // 2 + case.n // 4 and (case.n - first) % 2 == 1  # 17 and 33 vectors
    else:
        bound, count = _odd_bound(case)
        _, z, _, _ = _eigenpairs(knobs, solver, case, route + "/bound=odd", bound=bound)
        assert z.shape[1] == count and count % 2 == 1
    w, z = solver.eigh_above(2.0 * exact.max() + 1.0)
    assert z.shape == (case.n, 0) and np.isfinite(w).all()
