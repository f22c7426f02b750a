"""One operator's response at every site of the lattice (`Hamiltonian.response_map`).

`correlation(A, B)` answers one pair of operators.  A map - the susceptibility χ(r) from one impurity to every site -
follows from a single recurrence on the few columns A lives on.  With E the unit columns on the support of A and
X_n = T_n(H~) E,

    Tr[T_n A T_m B_j] = Σ_αβ Σ_γδ A[α,β] B_j[γ,δ] conj(X_m[(j,γ), β]) X_n[(j,δ), α]

for any 4×4 operator B_j on site j, so every site gets one 4×4 block per kernel F = Σ_nm c_nm T_n T_m,

    K_j[γ,δ] = Σ_nm c_nm Σ_αβ A[α,β] conj(X_m[(j,γ),β]) X_n[(j,δ),α],     Σ_ab A_ab (B_j)_ba F(E_a, E_b) = Σ_γδ B_j[γ,δ] K_j[γ,δ]

which the GPU computes (`bdg_response_map`): the recurrence, one dense product c^T·X on the fp64
matrix cores and a contraction per site.  The host makes A's support, the coefficients of the kernels, and contracts
the blocks with whatever on-site operator the caller asks for.

`blocks` are plain traces.  `contract`, `spin` and `density` carry the factor ½ of `MomentMatrix.response` and
`static`, which undoes the Nambu double counting for particle-hole symmetric operators.
"""

from __future__ import annotations

import warnings
from dataclasses import dataclass, field

import numpy as np

from .correlation import EXPAND_TAIL, _DIRECTIONS, _fermi_difference_quotient, as_operator

MAX_SUPPORT_SITES = 8  # 32 scalar rows: the columns of one recurrence


def spin_block(direction) -> np.ndarray:
    """diag(σ_k, -σ_k*): the on-site block of `spin_operator`."""
    from .common import σ1, σ2, σ3

    if direction not in _DIRECTIONS:
        raise ValueError("spin: direction must be 1, 2, 3 or 'x', 'y', 'z'")
    pauli = np.asarray((σ1, σ2, σ3)[_DIRECTIONS[direction] - 1], dtype=np.complex128)
    block = np.zeros((4, 4), dtype=np.complex128)
    block[:2, :2] = pauli
    block[2:, 2:] = -pauli.conj()
    return block


def density_block() -> np.ndarray:
    """diag(1, 1, -1, -1): the on-site block of the electron density in Nambu form."""
    return np.diag([1.0, 1.0, -1.0, -1.0]).astype(np.complex128)


def operator_support(system, A) -> tuple[np.ndarray, np.ndarray]:
    """(sites, a): the support of A - the union of its non-zero block rows and columns, ascending site indices - and A
    between the scalar rows 4·site + component of those sites, (4s, 4s) complex, no symmetry assumed."""
    indptr, indices, data = as_operator(system, A)
    if indices.size == 0:
        raise ValueError("response_map: the operator A is zero")
    block_rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    sites = np.union1d(block_rows, indices.astype(np.int64))
    if sites.size > MAX_SUPPORT_SITES:
        raise ValueError(f"response_map: the support of A is {sites.size} sites, more than the {MAX_SUPPORT_SITES} one "
                         "recurrence carries (32 columns); use correlation() for extended operators")
    a = np.zeros((sites.size, 4, sites.size, 4), dtype=np.complex128)
    a[np.searchsorted(sites, block_rows), :, np.searchsorted(sites, indices), :] = data
    return sites, a.reshape(4 * sites.size, 4 * sites.size)


def _tail_warning(c: np.ndarray, moments: int, digits: float, label: str) -> None:
    """The convergence warning of `MomentMatrix.expand` for one coefficient matrix: same tail rule, same `digits`."""
    size = np.abs(c)
    tail = max(1, min(moments // 8, EXPAND_TAIL))
    largest = float(size.max(initial=0.0))
    edge = max(float(size[-tail:, :].max(initial=0.0)), float(size[:, -tail:].max(initial=0.0)))
    if largest > 0 and edge > 10.0 ** (-float(digits)) * largest:
        warnings.warn(f"response_map{label}: the last {tail} rows or columns of the coefficients reach {edge / largest:.1e} "
                      f"of the largest one: {moments} moments have not converged to 1e-{float(digits):g}", RuntimeWarning,
                      stacklevel=4)


@dataclass
class ResponseMap:
    """The response of every site to one operator A.

    blocks       (kernels, sites, 4, 4) complex128 (without the kernel axis when `omega` was not a list):
                 Σ_γδ B[γ,δ] blocks[q, s][γ,δ] = Σ_ab A_ab (B_s)_ba F_q(E_a, E_b) for a 4×4 operator B on site s:
                 plain traces over the Nambu states
    sites        the sites of the site axis, in the order given
    omega        the frequencies of the kernels (None: the static limit or the caller's function)
    temperature  of the Fermi functions (None for the caller's function)
    scale        half-width of the band the polynomials live on
    moments      M
    info         support size, chunks of sites, the device's performance record
    """

    blocks: np.ndarray
    sites: list
    omega: np.ndarray | None
    temperature: float | None
    scale: float
    moments: int
    info: dict = field(default_factory=dict)

    def contract(self, B) -> np.ndarray:
        """½ Σ_γδ B[γ,δ] K[γ,δ] at every site for a 4×4 on-site operator B: χ_AB with B on that site, shape
        (kernels, sites) or (sites,).  The ½ is the one of `MomentMatrix.response` and `static`."""
        B = np.asarray(B, dtype=np.complex128)
        if B.shape != (4, 4):
            raise ValueError("contract: expected a 4×4 on-site operator")
        return 0.5 * np.einsum("gd,...gd->...", B, self.blocks)

    def spin(self, direction) -> np.ndarray:
        """χ between A and the spin component `direction` (1, 2, 3 or "x", "y", "z") at every site."""
        return self.contract(spin_block(direction))

    def density(self) -> np.ndarray:
        """χ between A and the electron density at every site."""
        return self.contract(density_block())


def response_map(system, A, *, temperature: float | None = None, broadening: float | None = None, omega=None,
                 function=None, moments: int | None = None, sites=None, scale: float | None = None,
                 digits: float = 12) -> ResponseMap:
    """The 4×4 response blocks of every site to the operator A (see `Hamiltonian.response_map`).

    `A`: anything `as_operator` takes, with a support of at most 8 sites; it need not be Hermitian.  Kernels:
    `omega=None` is the static limit (f(E_a) - f(E_b)) / (E_a - E_b) at `temperature`; `omega=[…]` with
    `broadening > 0` the Kubo kernel (f(E_a) - f(E_b)) / (ω + iη + E_a - E_b), one per ω; `function=F` the caller's
    F(x, y).  `moments=None` takes `moments_for_response(scale, temperature, broadening, digits)`.  `sites=None`: all
    sites, else a list of coordinates (the result's site axis is in the order given)."""
    from .chebyshev import chebyshev_coefficients_2d, fermi_function, moments_for_response
    from .observables import _scale_of

    scale = _scale_of(system) if scale is None else float(scale)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("response_map: scale must be positive")
    if function is not None and omega is not None:
        raise ValueError("response_map: give function= or omega=, not both")
    if function is None:
        if temperature is None or not float(temperature) > 0:
            raise ValueError("response_map: the temperature must be positive")
        temperature = float(temperature)
        if omega is not None and (broadening is None or not float(broadening) > 0):
            raise ValueError("response_map: the broadening must be positive (omega=None is the ω = 0, η = 0 limit)")
    eta = 0.0 if broadening is None else float(broadening)
    if moments is None:
        if temperature is None:
            raise ValueError("response_map: give moments= with function=")
        moments = moments_for_response(scale, float(temperature), eta if omega is not None else 0.0, float(digits))
    moments = int(moments)
    if moments < 1:
        raise ValueError("response_map: moments must be >= 1")

    if sites is None:
        site_list = list(system.lattice.sites())
        indices = np.arange(system.lattice.size, dtype=np.int64)
    else:
        site_list = [tuple(int(v) for v in site) for site in sites]
        indices = np.array([system.lattice[site] for site in site_list], dtype=np.int64)
    if not site_list:
        raise ValueError("response_map: sites is empty")
    support, a = operator_support(system, A)

    squeeze = True
    omegas = None
    if function is not None:
        kernels = [function]
    elif omega is None:
        kernels = [lambda x, y: _fermi_difference_quotient(x, y, temperature)]
    else:
        squeeze = np.ndim(omega) == 0
        omegas = np.atleast_1d(np.asarray(omega, dtype=np.float64)).reshape(-1)
        if omegas.size < 1:
            raise ValueError("response_map: omega is empty")
        kernels = [(lambda x, y, w=w: (fermi_function(x, temperature) - fermi_function(y, temperature))
                    / (w + 1j * eta + x - y)) for w in omegas]
    coef = np.empty((len(kernels), moments, moments), dtype=np.complex128)
    for q, F in enumerate(kernels):
        coef[q] = chebyshev_coefficients_2d(F, scale, moments)
        _tail_warning(coef[q], moments, digits, "" if omegas is None else f" (omega = {omegas[q]:g})")

    distinct, where = np.unique(indices, return_inverse=True)  # (a block row is listed once in a device call)
    rows = (4 * support[:, None] + np.arange(4)[None, :]).reshape(-1)
    solver = system._solver()
    blocks = solver.response_map(scale, rows, a, coef, distinct)[:, where.reshape(-1)]
    perf = solver.perf()
    lanes = max(1, int(perf["lanes_per_row"]))
    columns = -(-rows.size // lanes) * lanes
    # (every chunk of sites reruns the M - 1 steps of every batch of columns: the launches count the chunks)
    chunks = int(perf["launches"] // ((moments - 1) * (columns // lanes))) if moments > 1 else None  # (M = 1: no step)
    info = {"support": int(support.size), "columns": int(columns), "chunks": chunks, "perf": perf}
    blocks = np.ascontiguousarray(blocks[0] if squeeze else blocks)
    return ResponseMap(blocks=blocks, sites=site_list, omega=None if omegas is None else (omegas[0] if squeeze else omegas),
                       temperature=temperature, scale=scale, moments=moments, info=info)
