"""All eigenpairs in an energy window by Chebyshev-filtered subspace iteration (`Hamiltonian.eigenpairs`).

    E, v = system.eigenpairs((lo, hi))      every eigenpair with lo <= E <= hi, ascending

A block X of B vectors stays on the device (`bdg_subspace_*`).  Every iteration applies the
Jackson-damped Chebyshev series p of the indicator of [lo, hi] to the block, X <- p(H) X, forms HX = H X and the two
B x B matrices S = X†X and G = X†HX, and leaves the Rayleigh-Ritz step to the host: S is diagonalised and directions
below 1e-12 of its largest eigenvalue are dropped, G is diagonalised in the whitened remainder, and the device
rotates X <- XQ, HX <- HXQ and returns the residual norms ‖HX_j − θ_j X_j‖.  Only B x B matrices cross PCIe until
the converged vectors are read.
"""

from __future__ import annotations

import warnings

import numpy as np

from .common import typecheck

MOMENTS_MIN = 128
MOMENTS_MAX = 4096
MAX_COLUMNS = 512       # largest block: a window that needs more raises
RANK_CUT = 1e-12        # directions of S below this fraction of its largest eigenvalue are dropped
COUNT_VECTORS = 32      # random vectors of the stochastic count (max_states=None)
COUNT_FIRST_ID = 1 << 32  # their ids: apart from those of the start block


def default_moments(scale: float, lo: float, hi: float) -> int:
    """M = ⌈8πa / (hi − lo)⌉ clamped to [128, 4096]: the Jackson kernel resolves πa/M, an eighth of the window.
    (4πa / (hi − lo) converges too: in 30 and 38 iterations where this takes 13 and 16)"""
    width = hi - lo
    if not width > 0:
        return MOMENTS_MAX
    return int(min(MOMENTS_MAX, max(MOMENTS_MIN, np.ceil(8.0 * np.pi * scale / width))))


def window_coefficients(scale: float, lo: float, hi: float, moments: int) -> np.ndarray:
    """Jackson-damped Chebyshev coefficients of the indicator of [lo, hi] on [−scale, scale], c_0 as it enters the
    sum: with θ = arccos(E/scale), c_0 = (θ_lo − θ_hi)/π and c_k = 2 (sin kθ_lo − sin kθ_hi)/(kπ), times the kernel.
    Edges beyond the band are clipped to it."""
    from .chebyshev import jackson_kernel

    theta_lo = float(np.arccos(np.clip(lo / scale, -1.0, 1.0)))
    theta_hi = float(np.arccos(np.clip(hi / scale, -1.0, 1.0)))
    k = np.arange(1, moments, dtype=np.float64)
    coef = np.empty(moments)
    coef[0] = (theta_lo - theta_hi) / np.pi
    coef[1:] = 2.0 * (np.sin(k * theta_lo) - np.sin(k * theta_hi)) / (k * np.pi)
    return coef * jackson_kernel(moments)


def filter_plateau(coef: np.ndarray, scale: float, lo: float, hi: float) -> float:
    """The largest value of the series on the window: 1 when the degree resolves the window, less when it does not."""
    grid = np.clip(np.linspace(lo, hi, 65) / scale, -1.0, 1.0)
    return float(np.polynomial.chebyshev.chebval(grid, coef).max())


def check_window(window, scale: float) -> tuple[float, float]:
    """(lo, hi) as floats, or ValueError: not two numbers, non-finite, lo > hi, or wholly outside [−scale, scale]."""
    try:
        lo, hi = (float(edge) for edge in window)
    except (TypeError, ValueError):
        raise ValueError("eigenpairs: window must be a pair (lo, hi) of real numbers") from None
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError("eigenpairs: the window edges must be finite")
    if lo > hi:
        raise ValueError(f"eigenpairs: the window ({lo}, {hi}) has lo > hi")
    if hi < -scale or lo > scale:
        raise ValueError(f"eigenpairs: the window ({lo}, {hi}) lies wholly outside the band [-{scale:g}, {scale:g}]")
    return lo, hi


def block_size(states: float, sigma: float = 0.0) -> int:
    """B = ⌈1.25 n + 3σ⌉ + 8 columns for n expected states: a quarter more and eight, the guard columns."""
    return int(np.ceil(1.25 * states + 3.0 * sigma)) + 8


def rayleigh_ritz(s: np.ndarray, g: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(θ (r,), Q (B, r)) from S = X†X and G = X†HX: XQ is orthonormal and diagonalises H in the span of X, the
    directions of S below RANK_CUT of its largest eigenvalue left out."""
    w, u = np.linalg.eigh(0.5 * (s + s.conj().T))
    keep = w > RANK_CUT * w[-1]
    white = u[:, keep] / np.sqrt(w[keep])
    small = white.conj().T @ g @ white
    theta, z = np.linalg.eigh(0.5 * (small + small.conj().T))
    return theta, white @ z


def _estimate_count(system, solver, scale: float, lo: float, hi: float, moments: int, seed: int) -> tuple[float, float]:
    """(n, σ): stochastic trace of the window's own Jackson series, Σ_k c_k <r|T_k(H/a)|r> averaged over random
    vectors r (|r|² = 4N), and the standard error of that mean."""
    from . import chebyshev as cheb

    even = moments + (moments & 1)
    d, e = solver.dots_random(scale, even // 2, COUNT_VECTORS, seed=seed, first_id=COUNT_FIRST_ID)
    per_vector = window_coefficients(scale, lo, hi, even) @ cheb.dots_to_moments(d, e)
    return float(np.mean(per_vector)), float(np.std(per_vector, ddof=1) / np.sqrt(len(per_vector)))


def _layout(values: np.ndarray, rows: np.ndarray, format: str):
    """(E, states) in the layouts of diagonalize() from the states as rows (k, 4N)."""
    if format == "raw":
        return values, np.ascontiguousarray(rows.T)
    return values, rows.reshape(len(values), rows.shape[1] // 4, 4)


@typecheck
def eigenpairs(system, window, *, moments: int | None = None, tol: float | int = 1e-9, max_iter: int = 40,
               max_states: int | None = None, seed: int = 0, format: str = "reshape", method: str = "auto"):
    """Every eigenpair of H with lo <= E <= hi for window = (lo, hi), ascending, in the layouts of `diagonalize()`:
    "reshape" -> (E (k,), v (k, N, 4)), "raw" -> (E, X (4N, k)); k = 0 for an empty window.  The vectors are
    orthonormal, inside degenerate levels too.  The window may lie anywhere in the band, on either side of zero or
    across it; nothing is folded by particle-hole symmetry.  ValueError for lo > hi, non-finite edges, or a window
    wholly outside [−a, a], a = 1.01 x the Gershgorin bound, before any device call.

    Chebyshev-filtered subspace iteration on a device-resident block.  The filter is the
    Jackson-damped Chebyshev series of degree `moments` = M of the window's indicator; `moments=None` takes
    M = ⌈8πa/(hi − lo)⌉ clamped to [128, 4096].  The filter rises from 0 to 1 over about πa/M around an edge and
    passes a level AT an edge at half weight - neither kept nor suppressed: **the window edges belong in spectral
    gaps wider than about πa/M**; with an edge closer than that to a level the iteration stalls (raise `moments`,
    or move the edge).
    `tol`: the run has converged when every Ritz value inside the window has residual ‖Hv − Ev‖ <= tol·a and at
    least one guard column is left (a Ritz value outside: without one the block may be too small to hold the
    window).  A Ritz value inside the window that is a mixture of states on both sides of it (a window in a gap)
    counts as a guard too: it is told from a state of the window by what the filter left of its vector, less than
    half of what it leaves of a state in the window (not in the first iteration and the one after the block grew,
    whose start vectors have to settle first).
    `max_states`: an upper bound on the number of states expected, the block gets B = ⌈1.25·max_states⌉ + 8 columns;
    None estimates the number n ± σ by a stochastic trace of the same series and takes B = ⌈1.25 n + 3σ⌉ + 8.  A block
    that turns out too small (no guard column left) is doubled, keeping its columns; beyond 512 columns the call
    raises ValueError.  After `max_iter` iterations without convergence a RuntimeWarning is issued and only the
    converged pairs are returned, as `lowest_eigenpairs` does.  `seed` seeds the start block (counter-based
    generator, column c = vector id c).  method="auto" answers matrices up to 4N = 2048 from the dense solver cut
    to the window; method="subspace" always runs the iteration, and leaves what it did on the device mirror:
    `system._solver().last_eigenpairs` = {"iterations", "columns", "moments", "converged"}."""
    from .observables import DENSE_AUTO_LIMIT, _scale_of

    if format not in ("raw", "reshape"):
        raise RuntimeError(f"Eigenstate format '{format}' is not yet supported.")
    if method not in ("auto", "subspace"):
        raise ValueError("eigenpairs: method must be 'auto' or 'subspace'")
    if moments is not None and moments < 2:
        raise ValueError("eigenpairs: moments must be >= 2")
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError("eigenpairs: tol must be positive")
    if max_iter < 1:
        raise ValueError("eigenpairs: max_iter must be >= 1")
    if max_states is not None and max_states < 1:
        raise ValueError("eigenpairs: max_states must be >= 1")
    scale = _scale_of(system)
    lo, hi = check_window(window, scale)
    dim = system.shape[0]
    empty = (np.zeros(0), np.zeros((0, dim), dtype=np.complex128))

    if method == "auto" and dim <= DENSE_AUTO_LIMIT:
        values, states = system._solver().eigh_above(float(np.nextafter(lo, -np.inf)))
        above = values[len(values) - states.shape[1]:]
        keep = above <= hi
        return _layout(np.ascontiguousarray(above[keep]), np.ascontiguousarray(states[:, keep].T), format)

    if moments is None:
        moments = default_moments(scale, lo, hi)
    coef = window_coefficients(scale, lo, hi, int(moments))
    kept_from = 0.5 * filter_plateau(coef, scale, lo, hi)  # a level at an edge passes at half the plateau
    too_many = ("eigenpairs: the window needs a block of {} columns, the limit is " + str(MAX_COLUMNS) +
                ": it holds more states than that - narrow it")
    if max_states is not None and block_size(max_states) > MAX_COLUMNS:
        raise ValueError(too_many.format(block_size(max_states)))
    solver = system._solver()
    if max_states is None:
        count, sigma = _estimate_count(system, solver, scale, lo, hi, int(moments), seed)
        columns = block_size(max(count, 0.0), sigma)
        if columns > MAX_COLUMNS:
            raise ValueError(too_many.format(columns))
    else:
        columns = block_size(max_states)

    solver.subspace_begin(columns, seed=seed, first_id=0)
    next_id = columns
    # |column|² before the filter: 4N for a start vector (entries ±1), 1 for a Ritz vector of the iteration before
    norm2 = np.full(columns, float(dim))
    try:
        converged = False
        settling = True
        for iteration in range(1, max_iter + 1):
            solver.subspace_filter(scale, coef)
            theta, q = rayleigh_ritz(*solver.subspace_project())
            residual = solver.subspace_rotate(q, theta)
            # what the filter left of the vector each Ritz vector came from: X Q_j = p(H) (X_before Q_j)
            gain = 1.0 / np.sqrt((np.abs(q) ** 2 * norm2[:, None]).sum(axis=0))
            rank = len(theta)
            norm2 = np.r_[np.ones(rank), np.full(columns - rank, float(dim))]
            if rank < columns:  # columns lost to rank: fresh start vectors
                solver.subspace_refill(rank, columns - rank, seed=seed, first_id=next_id)
                next_id += columns - rank
            inside = (theta >= lo) & (theta <= hi)
            done = inside & (residual <= tol * scale)
            genuine = done | (inside & (gain >= kept_from))
            if settling:
                # the block before this filter was mostly start vectors (the first iteration, the one after the
                # block grew): they hold every state of the window at a small amplitude, so the gains say nothing yet
                settling = False
                continue
            # guard columns: a Ritz value outside the window or a spurious one inside it, or - in a block no wider
            # than the matrix - a direction the filter annihilated
            if not ((~genuine).any() or rank < columns <= dim):
                # none left: the block may be too small for the window - twice the columns, the old ones kept
                if 2 * columns > MAX_COLUMNS:
                    raise ValueError(f"eigenpairs: all {columns} columns lie inside the window and the limit is "
                                     f"{MAX_COLUMNS} columns: the window holds more states than that - narrow it")
                kept = solver.subspace_read(0, rank)
                columns *= 2
                solver.subspace_begin(columns, seed=seed, first_id=next_id)
                next_id += columns
                solver.subspace_write(0, kept)
                norm2 = np.r_[np.ones(rank), np.full(columns - rank, float(dim))]
                settling = True
                continue
            if (done | ~genuine).all():
                converged = True
                break
        solver.last_eigenpairs = {"iterations": iteration, "columns": columns, "moments": int(moments),
                                  "converged": converged}
        if not converged:
            warnings.warn(f"eigenpairs: {int((genuine & ~done).sum())} of {int(genuine.sum())} Ritz values in the window "
                          f"did not converge to {tol:g} in {max_iter} iterations; returning the converged pairs (are "
                          f"the window edges in spectral gaps wider than {np.pi * scale / moments:.3g}?)", RuntimeWarning,
                          stacklevel=3)
        found = np.flatnonzero(done)
        if found.size == 0:
            return _layout(*empty, format)
        # (θ ascends, so the states in the window are neighbours; what lies between them and is not converged is skipped)
        rows = solver.subspace_read(int(found[0]), int(found[-1] - found[0] + 1))[found - found[0]]
        return _layout(np.ascontiguousarray(theta[found]), np.ascontiguousarray(rows), format)
    finally:
        solver.subspace_end()
