"""Shared by tests/test_dense_host.py and tests/test_gpu_dense.py: dense matrices whose spectrum is known without
trusting any eigensolver, and the checker of an eigensolver's result against it.

Every case starts from a symmetric tridiagonal seed (d, e) in float64 and hides its structure behind a similarity that
is EXACT in floating point, so the matrix fed to the device has the seed's spectrum to the last bit:

* P  a signed permutation (any seed; sparse but scrambled over the full bandwidth, many exact zeros);
* H  a block-diagonal Householder reflector, blocks I - (2/s) 1 1^T with s the powers of two of n's binary expansion
     (68 = 64 + 4): for seeds with integer or small dyadic entries H T H is exactly representable and fully dense;
* phases  conjugation with a diagonal of entries from {1, i, -1, -i}: a complex Hermitian matrix, same spectrum;
* scale  multiplication by 2^k.

The truth is the seed's spectrum by Sturm-count bisection in long double (or the analytic formula where one exists)."""

import functools
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
CLD = np.clongdouble
EPS = 2.0 ** -52
CLUSTER = 1e-5  # levels closer than this times |A| are orthonormalised against each other by the inverse-iteration routes

SIMILARITY = {"toeplitz": "H", "clement": "P", "wilkinson": "H", "glued": "H", "degenerate": "H", "ladder_above": "P",
              "ladder_below": "P", "graded": "P", "split": "P", "zero": "P", "identity": "P"}
FAMILIES = tuple(SIMILARITY)


class Case(NamedTuple):
    family: str
    n: int
    phases: bool = False
    scale: int = 0  # the matrix is the family's times 2^scale

    @property
    def id(self):
        return f"{self.family}{'*2^%d' % self.scale if self.scale else ''}-{self.n}{'-phases' if self.phases else ''}"


# ------------------------------------------------------------------ seeds
def seed(family: str, n: int):
    """(d, e): diagonal (n) and off-diagonal (n - 1) of the tridiagonal seed, float64."""
    k = np.arange(n, dtype=np.float64)
    if family == "toeplitz":
        return np.full(n, 2.0), np.full(n - 1, -1.0)
    if family == "clement":
        j = np.arange(1, n, dtype=np.float64)
        return np.zeros(n), np.sqrt(j * (n - j))
    if family == "wilkinson":
        return np.floor(np.abs(k - (n - 1) / 2.0)), np.ones(n - 1)
    if family == "glued":
        d = np.floor(np.abs(k % 16 - 7.5))
        e = np.where(np.arange(1, n) % 16 == 0, 2.0 ** -20, 1.0)
        return d, e
    if family == "degenerate":
        d = np.full(n, 3.0)
        d[: n // 2] = 1.0
        d[n // 2: n // 2 + n // 4] = 2.0
        return d, np.zeros(n - 1)
    if family in ("ladder_above", "ladder_below"):
        gap = 2e-5 if family == "ladder_above" else 0.5e-5
        return 1.0 + k * gap, np.full(n - 1, 1e-9)
    if family == "graded":
        d = 2.0 ** (-40.0 * k / n)
        return d, 0.1 * np.sqrt(d[:-1] * d[1:])
    if family == "split":
        e = np.full(n - 1, -1.0)
        e[6::7] = 0.0
        return np.full(n, 2.0), e
    if family == "zero":
        return np.zeros(n), np.zeros(n - 1)
    if family == "identity":
        return np.full(n, 3.0), np.zeros(n - 1)
    raise KeyError(family)


# ------------------------------------------------------------------ truth
def bisect(d, e2, halvings: int = 80):
    """All eigenvalues (ascending, long double) of the symmetric tridiagonal matrix with diagonal d and SQUARED
    off-diagonal e2, by bisection on the Sturm count, vectorised over the eigenvalues."""
    d = np.asarray(d, dtype=LD)
    e2 = np.asarray(e2, dtype=LD)
    n = d.size
    off = np.sqrt(e2)
    radius = np.concatenate([[0], off]) + np.concatenate([off, [0]])
    span = max(abs((d - radius).min()), abs((d + radius).max()))
    lo = np.full(n, (d - radius).min() - span * LD(2.0) ** -40 - LD(1e-300), dtype=LD)
    hi = np.full(n, (d + radius).max() + span * LD(2.0) ** -40 + LD(1e-300), dtype=LD)
    pivmin = np.finfo(LD).tiny * max(LD(1), e2.max() if n > 1 else LD(1))
    index = np.arange(n)
    for _ in range(halvings):
        x = (lo + hi) / 2
        piv = d[0] - x
        piv = np.where(np.abs(piv) < pivmin, -pivmin, piv)  # (a zero pivot counts as negative, as in LAPACK's dstebz)
        count = (piv < 0).astype(np.int64)
        for i in range(1, n):
            piv = d[i] - x - e2[i - 1] / piv
            piv = np.where(np.abs(piv) < pivmin, -pivmin, piv)
            count += piv < 0
        above = count > index  # more than k eigenvalues below x: the k-th lies below x
        hi = np.where(above, x, hi)
        lo = np.where(above, lo, x)
    return (lo + hi) / 2


def analytic(family: str, n: int):
    """The spectrum in closed form (long double, ascending), or None."""
    if family == "toeplitz":
        return 2 - 2 * np.cos(np.arange(1, n + 1, dtype=LD) * (LD(np.pi) + LD(1.2246467991473532e-16)) / (n + 1))
    if family == "clement":
        return np.arange(-(n - 1), n, 2).astype(LD)
    if family == "degenerate":
        return np.sort(seed(family, n)[0]).astype(LD)
    if family in ("zero", "identity"):
        return seed(family, n)[0].astype(LD)
    return None


@functools.lru_cache(maxsize=None)
def _truth(family: str, n: int):
    exact = analytic(family, n)
    if exact is not None and (family != "clement" or n > 1100):
        # (clement: the seed's square roots are rounded, which moves a level by at most 2 max|δe| <= eps (n - 1) / 2 - a
        # 2n-th of the bound of §2; below 1100 rows the truth is the rounded seed's own spectrum, above it the formula)
        return exact
    d, e = seed(family, n)
    return bisect(d, e.astype(LD) ** 2)


def truth(case: Case):
    """The spectrum of `matrix(case)`: long double, ascending.  Do not modify."""
    return _truth(case.family, case.n) * LD(2.0) ** case.scale


# ------------------------------------------------------------------ similarities
def _blocks(n: int):
    """Powers of two summing to n, largest first, as (start, size)."""
    out, start = [], 0
    for bit in reversed(range(n.bit_length())):
        if n >> bit & 1:
            out.append((start, 1 << bit))
            start += 1 << bit
    return out


def _rng(case_or_family, n):
    return np.random.default_rng([sum(map(ord, case_or_family)), n])


def _permutation(family, n):
    rng = _rng(family, n)
    return rng.permutation(n), rng.choice([-1.0, 1.0], size=n)


_UNITS = np.array([1, 1j, -1, -1j])


def _phase_units(family, n):
    return _rng(family + "/phases", n).integers(0, 4, size=n)  # powers of i


def _tridiagonal_times(d, e, x):
    y = d[:, None] * x
    y[:-1] += e[:, None] * x[1:]
    y[1:] += e[:, None] * x[:-1]
    return y


def _reflect(n, x):
    """H x for the block-diagonal reflector, in the type of x."""
    y = x.copy()
    for start, size in _blocks(n):
        y[start:start + size] -= x[start:start + size].sum(axis=0, keepdims=True) * (x.dtype.type(2) / size)
    return y


def apply(case: Case, x):
    """A x in long double, through the factors of A = 2^scale Φ S T S^T Φ^H: O(n) work per column and no rounding error
    beyond long double's in the three products with T's entries."""
    x = np.asarray(x)
    ctype = CLD if np.iscomplexobj(x) or case.phases else LD
    x = x.astype(ctype).reshape(case.n, -1)
    d, e = (v.astype(LD) for v in seed(case.family, case.n))
    units = _UNITS.astype(CLD)[_phase_units(case.family, case.n)][:, None] if case.phases else None
    if case.phases:
        x = np.conj(units) * x
    if SIMILARITY[case.family] == "P":
        perm, sign = _permutation(case.family, case.n)
        inner = sign.astype(LD)[:, None] * x[perm]            # S^T x
        y = np.empty_like(inner)
        y[perm] = sign.astype(LD)[:, None] * _tridiagonal_times(d, e, inner)
    else:
        y = _reflect(case.n, _tridiagonal_times(d, e, _reflect(case.n, x)))
    if case.phases:
        y = units * y
    return y * LD(2.0) ** case.scale


def _dense(family: str, n: int, dtype):
    """S T S^T in `dtype` (float64 or long double): both give the same numbers when the similarity is exact."""
    d, e = (v.astype(dtype) for v in seed(family, n))
    t = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    if SIMILARITY[family] == "P":
        perm, sign = _permutation(family, n)
        a = np.zeros_like(t)
        a[np.ix_(perm, perm)] = sign.astype(dtype)[:, None] * t * sign.astype(dtype)[None, :]
        return a
    return _reflect(n, _reflect(n, t).T).T


@functools.lru_cache(maxsize=None)
def _matrix(case: Case):
    a = _dense(case.family, case.n, np.float64) * 2.0 ** case.scale
    if case.phases:
        units = _UNITS[_phase_units(case.family, case.n)]
        a = units[:, None] * a * np.conj(units)[None, :] + 0.0  # (+ 0.0: no negative zeros)
    a.setflags(write=False)
    return a


def matrix(case: Case):
    """The dense matrix of the case (float64, or complex128 with phases).  Read-only."""
    return _matrix(case)


def reflector_is_exact(family: str, n: int) -> bool:
    """H T H formed in float64 and in long double agree in every bit, and the result is symmetric: with 11 more mantissa
    bits the long double products and sums cannot round where float64's do not."""
    low, high = _dense(family, n, np.float64), _dense(family, n, LD)
    return bool(np.array_equal(low.astype(LD), high) and np.array_equal(low, low.T))


def bsr_arrays(a):
    """(indptr, indices, data) of the 4 x 4 block form: every block with a non-zero entry, and the diagonal blocks."""
    n = a.shape[0]
    nb = n // 4
    blocks = np.asarray(a, dtype=np.complex128).reshape(nb, 4, nb, 4).transpose(0, 2, 1, 3)
    keep = np.abs(blocks).max(axis=(2, 3)) > 0
    keep[np.arange(nb), np.arange(nb)] = True
    rows, cols = np.nonzero(keep)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    m = sp.bsr_matrix((blocks[rows, cols], cols.astype(np.int32), indptr), shape=(n, n), blocksize=(4, 4))
    return m.indptr, m.indices, m.data


# ------------------------------------------------------------------ the checker
class Ratios(NamedTuple):
    eigenvalues: float     # max |w - truth| / (m eps |A|)
    residual: float        # max |A z - λ z| / (m eps |A|); nan without vectors
    orthonormality: float  # max |z_i^H z_j - δ_ij| / its bound
    gap_constant: float    # max |z_i^H z_j| |λ_i - λ_j| / (eps |A|): recorded, not asserted

    def worst(self):
        return max(v for v in self[:3] if not np.isnan(v))

    def __str__(self):
        return "eig %.3f res %.3f orth %.3f gapc %.1f" % self


def _ratio(value, bound):
    value = float(value)
    if not np.isfinite(value):
        return np.inf
    if bound == 0:
        return 0.0 if value == 0 else np.inf
    return value / float(bound)


def shifted_norm(case: Case) -> float:
    """|G|_2 of the matrix the Jacobi route factors, G = A + 1.5 b I with b the largest absolute row sum of A (the
    library's Gershgorin bound; b >= |A|_2, so |G|_2 = 1.5 b + max(truth) is between 2.5 and 1.5 sqrt(n) + 1 times |A|_2)."""
    b = float(np.abs(matrix(case)).sum(axis=1).max())
    return 1.5 * b + float(truth(case).max()) if b > 0 else 0.0


def ratios(case: Case, w, z=None, first: int = 0, gap_term: bool = False, work_norm=None) -> Ratios:
    """The three ratios of §2 for eigenvalues w (all n of them) and, if given, the vectors z (n, n - first) of
    w[first:].  `gap_term`: the inverse-iteration routes' bound max(m eps, 2 m eps |A| / |λ_i - λ_j|), which follows from
    the residual bound, for levels further apart than the routes' cluster criterion; m eps on the diagonal and between
    closer levels, where only the cluster orthonormalisation can deliver it.  The Jacobi route gets m eps throughout.
    `work_norm`: the norm that takes the place of |A| in the eigenvalue and residual bounds, for a route that works on
    another matrix than A (Jacobi: `shifted_norm`); the orthonormality bound and the gap constant keep |A|."""
    n = case.n
    exact = truth(case)
    norm = float(np.abs(exact).max())
    m = max(n, 64)
    work = norm if work_norm is None else float(work_norm)
    w = np.asarray(w)
    if w.shape != (n,) or not np.isfinite(w).all() or np.any(np.diff(w) < 0):
        return Ratios(np.inf, np.nan, np.nan, np.nan)
    eig = _ratio(np.abs(w.astype(LD) - exact).max(), m * EPS * work)
    if z is None:
        return Ratios(eig, np.nan, np.nan, np.nan)
    z = np.asarray(z)
    k = n - first
    if z.shape != (n, k) or not np.isfinite(z).all():
        return Ratios(eig, np.inf, np.inf, np.nan)
    if k == 0:
        return Ratios(eig, 0.0, 0.0, 0.0)
    r = apply(case, z) - z.astype(CLD if np.iscomplexobj(z) else LD) * w[first:].astype(LD)[None, :]
    res = _ratio(np.sqrt((np.abs(r) ** 2).sum(axis=0)).max(), m * EPS * work)
    gram = np.abs(z.conj().T @ z - np.eye(k))
    lam = exact[first:].astype(np.float64)
    gaps = np.abs(lam[:, None] - lam[None, :])
    bound = np.full((k, k), m * EPS)
    if gap_term and norm > 0:
        apart = gaps > CLUSTER * norm
        bound[apart] = np.maximum(m * EPS, 2 * m * EPS * norm / gaps[apart])
    orth = _ratio((gram / bound).max(), 1.0)
    gapc = float((gram * gaps).max() / (EPS * norm)) if norm > 0 else 0.0
    return Ratios(eig, res, orth, gapc)


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """numpy.linalg.eigh of the case: (w, z).  Do not modify."""
    w, z = np.linalg.eigh(matrix(case))
    w.setflags(write=False)
    z.setflags(write=False)
    return w, z


@functools.lru_cache(maxsize=None)
def reference_ratios(case: Case) -> Ratios:
    w, z = reference(case)
    return ratios(case, w, z)


# ------------------------------------------------------------------ the cases
def families_at(n: int):
    """The families a size takes: `glued` needs two 16-row blocks, the ladders a few rungs, `zero` / `identity` have
    their three sizes."""
    out = []
    for family in FAMILIES:
        if family == "glued" and n < 32:
            continue
        if family in ("zero", "identity") and n not in (4, 8, 68):
            continue
        out.append(family)
    return out


def cases_at(n: int, phases=(False, True), scaled: bool = True):
    out = [Case(family, n, ph) for family in families_at(n) for ph in phases]
    if scaled:
        out += [Case(family, n, False, scale) for family in ("toeplitz", "wilkinson") for scale in (-40, 40)]
    return out


JACOBI_SIZES = (4, 8, 12, 36, 68, 260, 516)
ONE_STAGE_SIZES = (4, 8, 12, 36, 64, 68, 100, 132, 260, 516)
TWO_STAGE_SIZES = (68, 96, 100, 128, 132, 260, 516)   # 68: the first size with a band; 516: two 512-row parts in ts_gram
ALL_SIZES = tuple(sorted(set(JACOBI_SIZES + ONE_STAGE_SIZES + TWO_STAGE_SIZES)))
