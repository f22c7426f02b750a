"""Functions of H on caller-supplied state vectors (`Hamiltonian.apply`, `Hamiltonian.evolve`).

    apply(f, X)      f(H) X       for any function that is smooth on the band, real or complex valued
    evolve(ψ, t)     exp(-iHt) ψ  for one time or many

Both are one Chebyshev series of H~ = H / scale per function, f(H) = Σ_k c_k T_k(H~), summed on the GPU by
Clenshaw's recurrence with the vectors as a stored source (`bdg_apply_series`): every (vector,
function) pair is one column of a batch, one launch per coefficient advances them all.  The host only makes
the coefficients and carries the layouts.

Vectors come in the layouts `diagonalize` produces - "raw": (4N,) or (4N, R) with the vectors as columns;
"reshape": (N, 4) or (R, N, 4) - and the result has the layout of the input, with one leading axis more when
several functions (a 2-D `coefficients` array) or an array of times were asked for.
"""

from __future__ import annotations

import numpy as np

from .common import typecheck

AUTO_MOMENTS_FROM = 64
AUTO_MOMENTS_LIMIT = 65536  # the automatic expansion order stops here: beyond, the function is not smooth on the band


# ---------------------------------------------------------------- layouts
def _to_rows(system, vectors) -> tuple[np.ndarray, str]:
    """(V, 4N) complex128 rows of the given vectors and the name of their layout."""
    n = system.lattice.size
    x = np.asarray(vectors)
    if x.dtype == object or not (np.issubdtype(x.dtype, np.number) or x.dtype == bool):
        raise ValueError("vectors: expected an array of numbers")
    if x.ndim == 1 and x.shape == (4 * n,):
        rows, layout = x[None, :], "raw1"
    elif x.ndim == 2 and x.shape[0] == 4 * n and x.shape[1] >= 1:
        rows, layout = x.T, "raw"
    elif x.ndim == 2 and x.shape == (n, 4):
        rows, layout = x.reshape(1, 4 * n), "reshape1"
    elif x.ndim == 3 and x.shape[0] >= 1 and x.shape[1:] == (n, 4):
        rows, layout = x.reshape(x.shape[0], 4 * n), "reshape"
    else:
        raise ValueError(f"vectors: expected shape ({4 * n},), ({4 * n}, R), ({n}, 4) or (R, {n}, 4), got {x.shape}")
    rows = np.ascontiguousarray(rows, dtype=np.complex128)
    if not np.isfinite(rows.view(np.float64)).all():
        raise ValueError("vectors: entries must be finite")
    return rows, layout


def _from_rows(system, y: np.ndarray, layout: str, leading: bool) -> np.ndarray:
    """(V, F, 4N) device result -> the caller's layout, functions first ((F, ...) when `leading`, else F = 1 dropped)."""
    n = system.lattice.size
    y = np.moveaxis(y, 1, 0)  # (F, V, 4N)
    if layout == "raw1":
        out = y[:, 0, :]
    elif layout == "raw":
        out = np.swapaxes(y, 1, 2)  # (F, 4N, V)
    elif layout == "reshape1":
        out = y[:, 0, :].reshape(y.shape[0], n, 4)
    else:
        out = y.reshape(y.shape[0], y.shape[1], n, 4)
    return np.ascontiguousarray(out if leading else out[0])


# ---------------------------------------------------------------- coefficient rules
def significant_length(coef: np.ndarray, digits: float) -> int:
    """1 + the last k with |c_k| >= 10^-digits of the largest coefficient (over all functions); at least 1."""
    size = np.abs(coef.reshape(coef.shape[0], -1)).max(axis=1)
    keep = np.flatnonzero(size >= 10.0 ** (-digits) * size.max(initial=0.0))
    return int(keep[-1]) + 1 if keep.size and size.max() > 0 else 1


def series_coefficients(function, scale: float, digits: float = 12.0) -> np.ndarray:
    """Complex Chebyshev coefficients of ε -> function(ε) on [-scale, scale], the order found automatically: M is
    doubled from 64 until every coefficient beyond M/2 is below 10^-digits of the largest one, and the series is
    then cut after its last coefficient above that threshold.  ValueError if 65 536 coefficients are not enough."""
    from .chebyshev import chebyshev_coefficients_complex

    m = AUTO_MOMENTS_FROM
    while True:
        coef = chebyshev_coefficients_complex(lambda x: function(scale * x), m)
        size = np.abs(coef)
        if not np.isfinite(size).all():
            raise ValueError("apply: the function is not finite on [-scale, scale]")
        if size[m // 2:].max() < 10.0 ** (-digits) * size.max() or size.max() == 0.0:
            return coef[: significant_length(coef, digits)]
        if m >= AUTO_MOMENTS_LIMIT:
            raise ValueError(
                f"apply: {AUTO_MOMENTS_LIMIT} Chebyshev coefficients do not reach 1e-{digits:g} of the largest one: the "
                "function is not smooth on the band [-scale, scale] (a step or a kink never converges geometrically; "
                "smooth it, or pass moments= / coefficients= to accept the truncation)")
        m *= 2


def evolution_coefficients(scale: float, times: np.ndarray, digits: float = 12.0) -> np.ndarray:
    """(M, len(times)) coefficients of exp(-i·scale·t·x) on [-1, 1]: c_k(t) = (2 - δ_k0) (-i)^k J_k(scale·t), M = 1 + the
    last k over all the times with |c_k| >= 10^-digits."""
    from scipy.special import jv

    z = scale * np.asarray(times, dtype=np.float64).reshape(-1)
    reach = float(np.abs(z).max(initial=0.0))
    margin = 20.0 * max(reach, 1.0) ** (1.0 / 3.0) + 40.0  # J_k(z) falls faster than exponentially from k = |z| on
    while True:
        order = np.arange(int(np.ceil(reach + margin)) + 1)
        bessel = jv(order[:, None], np.abs(z)[None, :])
        bessel = np.where((z < 0)[None, :] & (order[:, None] % 2 == 1), -bessel, bessel)  # J_k(-z) = (-1)^k J_k(z)
        coef = (2.0 * (-1j) ** (order % 4))[:, None] * bessel
        coef[0] *= 0.5
        size = np.abs(coef).max(axis=1)
        if size[-1] < 10.0 ** (-digits):
            keep = np.flatnonzero(size >= 10.0 ** (-digits))
            return np.ascontiguousarray(coef[: (int(keep[-1]) + 1 if keep.size else 1)])
        margin *= 2.0


# ---------------------------------------------------------------- the calls
def _run(system, coef: np.ndarray, scale: float, vectors, leading: bool) -> np.ndarray:
    rows, layout = _to_rows(system, vectors)
    solver = system._solver()
    y = solver.apply_series(scale, coef, rows)
    return _from_rows(system, y, layout, leading)


@typecheck
def apply(system, function, vectors, *, coefficients=None, moments: int | None = None,
          digits: float | int = 12.0, scale: float | int | None = None) -> np.ndarray:
    """f(H) X (see `Hamiltonian.apply`).

    `function`: vectorised callable on real energies, real or complex valued; or None with `coefficients` = the
    series on [-scale, scale] itself, f(ε) = Σ_k c_k T_k(ε/scale) with c_0 as it enters the sum: shape (M,), or
    (M, F) for F functions at once (the result then has a leading axis of length F).  `moments` fixes the number
    of coefficients computed from `function`; without it the order is found from the coefficients themselves
    (`series_coefficients`, relative threshold 10^-digits).  `scale` defaults to 1.01 x the Gershgorin bound."""
    from .observables import _scale_of

    if (function is None) == (coefficients is None):
        raise ValueError("apply: give either a function or coefficients=")
    digits = float(digits)
    scale = _scale_of(system) if scale is None else float(scale)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("apply: scale must be positive")
    leading = False
    if coefficients is not None:
        coef = np.asarray(coefficients)
        if coef.dtype == object or coef.ndim not in (1, 2) or coef.size == 0:
            raise ValueError("apply: coefficients must have shape (M,) or (M, F)")
        leading = coef.ndim == 2
        coef = np.ascontiguousarray(coef.reshape(coef.shape[0], -1), dtype=np.complex128)
        if not np.isfinite(coef.view(np.float64)).all():
            raise ValueError("apply: coefficients must be finite")
    elif not callable(function):
        raise ValueError("apply: function must be callable (or None with coefficients=)")
    elif moments is not None:
        from .chebyshev import chebyshev_coefficients_complex

        if moments < 1:
            raise ValueError("apply: moments must be >= 1")
        coef = chebyshev_coefficients_complex(lambda x: function(scale * x), int(moments))[:, None]
        if not np.isfinite(coef.view(np.float64)).all():
            raise ValueError("apply: the function is not finite on [-scale, scale]")
    else:
        coef = series_coefficients(function, scale, digits)[:, None]
    return _run(system, coef, scale, vectors, leading)


@typecheck
def evolve(system, vectors, times, *, digits: float | int = 12.0, scale: float | int | None = None) -> np.ndarray:
    """exp(-iHt) ψ (see `Hamiltonian.evolve`): one series per time, all of them columns of one device call.  A
    scalar `times` gives the layout of `vectors`; an array of times a leading time axis.  Negative times are
    allowed.  The series is exact up to its truncation at |c_k| < 10^-digits, so the map is unitary to that
    accuracy whatever the step: no time step needs choosing."""
    from .observables import _scale_of

    scale = _scale_of(system) if scale is None else float(scale)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("evolve: scale must be positive")
    t = np.asarray(times)
    if t.dtype == object or not (np.issubdtype(t.dtype, np.floating) or np.issubdtype(t.dtype, np.integer)):
        raise ValueError("evolve: times must be real numbers")
    if t.ndim > 1:
        raise ValueError("evolve: times must be a scalar or a one-dimensional array")
    if t.size == 0:
        raise ValueError("evolve: times is empty")
    t = t.astype(np.float64)
    if not np.isfinite(t).all():
        raise ValueError("evolve: times must be finite")
    coef = evolution_coefficients(scale, t.reshape(-1), float(digits))
    return _run(system, coef, scale, vectors, leading=t.ndim == 1)
