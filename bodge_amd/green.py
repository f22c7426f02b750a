"""Local and non-local blocks of the retarded Green's function (`Hamiltonian.green`, `Hamiltonian.green_map`).

G(z) = (z - H)^-1 at z = ε + iΓ for the whole 4N x 4N BdG matrix, Nambu basis (e↑, e↓, h↑, h↓) per site.
`GreenFunction.blocks[t, k]` = G(E_k + iΓ_k)[4j_t:4j_t+4, 4i:4i+4] for the source site i and the target
sites j_t.  The helpers are slices of these blocks, so no sign convention is hidden in them.

Route: the unit vectors e_{4i+b} of the source site run through the Chebyshev recurrence on
the GPU, and every step stores the rows of the target sites (`bdg_green_moments`): the moments
μ_n[ja, ib] = <e_{4j+a}|T_n(H/a)|e_{4i+b}>.  The blocks follow from the operator form of
`chebyshev.resolvent_series`,

    G(z)[ja, ib] = -i / (a·sqrt(1 - z̃²)) · Σ_n (2 - δ_n0) · exp(-i·n·arccos z̃) · μ_n[ja, ib],   z̃ = z/a.

With particle-hole symmetry (H = -τx H* τx) only the electron columns b = 0, 1 are run; the hole columns are
μ_n[a, b] = (-1)ⁿ·conj μ_n[a⊕2, b⊕2].  Probing several sources with one vector does not work here: G(ε + iΓ)
decays far too slowly with distance, so every source site gets its own start vectors.

Maps: `green_map` wants the local block G_jj at many sites j.  The start vectors of up to 32
sites share one batch of the recurrence, and a step stores for every vector the rows of its own site only
(`bdg_green_local_moments`), so a launch runs at full width and the moment table grows with the number of
sites, not with its square.

Extended states: `green_states` wants <w a|G|w b> for a state w spread over the lattice, with
|w b> = Σ_j w[j] e_{4j+b} - G(k, ε) for a plane wave (`spectral_function`).  The Nambu vectors of up to 64 / C
states share one batch, and a step projects t_n on the states with conj(w) instead of picking rows
(`bdg_green_state_moments`).  The hole columns of a state follow from the electron columns of its complex conjugate,
μ_n[q][a][b] = (-1)ⁿ·conj μ_n[p][a⊕2][b⊕2] with w_p = conj(w_q), so two columns are run when every state's conjugate is
among the states.
"""

from __future__ import annotations

import numpy as np

from .common import Coord

HOST_TABLE_LIMIT = 1 << 30  # bytes of one call's moment table on the host: more targets go in groups


def moment_weights(n_moments: int, scale: float, z: np.ndarray) -> np.ndarray:
    """(len(z), n_moments) weights w[k, n] with G(z_k) = Σ_n w[k, n] μ_n, for Im z > 0."""
    zt = np.asarray(z, dtype=np.complex128) / scale
    angle = np.arccos(zt)
    weights = np.exp(-1j * angle[:, None] * np.arange(n_moments)[None, :])
    weights[:, 1:] *= 2.0
    return weights * (-1j / (scale * np.sqrt(1 - zt * zt)))[:, None]


def hole_columns(mu: np.ndarray) -> np.ndarray:
    """(M, T, 4, 4) moments from the electron columns (M, T, 4, 2): μ_n[a, b] = (-1)ⁿ conj μ_n[a⊕2, b⊕2]."""
    full = np.empty(mu.shape[:3] + (4,), dtype=np.complex128)
    full[..., 0:2] = mu
    sign = np.where(np.arange(mu.shape[0]) & 1, -1.0, 1.0)[:, None, None, None]
    full[..., 2:4] = sign * mu[:, :, [2, 3, 0, 1], :].conj()
    return full


def blocks_from_moments(mu: np.ndarray, scale: float, z: np.ndarray) -> np.ndarray:
    """(T, K, 4, 4) blocks G(z_k) from the moments (M, T, 4, 4)."""
    return np.einsum("kn,ntab->tkab", moment_weights(mu.shape[0], scale, z), mu, optimize=True)


def reference_broadening(energies: np.ndarray) -> np.ndarray:
    """Γ per energy by the rule of `observables.ldos`: ε = unique(|E|), Γ = gradient(ε), E takes the Γ of |E|."""
    eps = np.unique(np.abs(energies))
    if eps.size < 2:
        raise ValueError("green: the default broadening needs at least two distinct |energies| (or pass broadening=...)")
    gam = np.gradient(eps)
    return gam[np.searchsorted(eps, np.abs(energies))]


def _series_arguments(system, energies, broadening, moments, digits, scale):
    """Energies, Γ per energy, moments and scale of a call, checked (the rules of `green`)."""
    from . import chebyshev as cheb
    from .observables import _scale_of

    energies = np.array(energies, dtype=float).reshape(-1)
    if energies.size == 0:
        raise ValueError("green: energies is empty")
    if broadening is None:
        gamma = reference_broadening(energies)
    else:
        gamma = np.asarray(broadening, dtype=float)
        if gamma.ndim == 0:
            gamma = np.full(energies.shape, float(gamma))
        elif gamma.shape != energies.shape:
            raise ValueError(f"green: broadening of shape {gamma.shape} for energies of shape {energies.shape}")
    if not np.all(gamma > 0):
        raise ValueError("green: the broadening must be positive")
    scale = _scale_of(system) if scale is None else float(scale)
    if np.any(np.abs(energies) >= scale):
        raise ValueError(f"green: |energy| must stay below the spectral bound {scale:.6g}")
    if moments is None:
        moments = cheb.moments_for_resolvent(scale, float(np.min(gamma)), digits)
    moments = int(moments)
    if moments < 1:
        raise ValueError("green: moments must be >= 1")

    return energies, gamma, moments, scale


class GreenFunction:
    """Blocks of G(ε + iΓ) from one source site to the target sites.

    `blocks` (T, K, 4, 4) complex128, `energies` and `broadening` (K,), `source` and `targets` lattice
    coordinates, `info` the route details (moments, scale, perf record, whether the hole columns were derived).
    """

    def __init__(self, blocks: np.ndarray, energies: np.ndarray, broadening: np.ndarray, source: Coord, targets,
                 info: dict | None = None):
        self.blocks = blocks
        self.energies = energies
        self.broadening = broadening
        self.source = tuple(source)
        self.targets = [tuple(t) for t in targets]
        self.info = dict(info or {})

    def _local(self, t: int, name: str) -> np.ndarray:
        if self.targets[t] != self.source:
            raise ValueError(f"{name}: target {self.targets[t]} is not the source site {self.source} (a local quantity)")
        return self.blocks[t]

    def ldos(self, t: int = 0) -> np.ndarray:
        """(K,) spin-summed electron LDOS -Im(G[0,0] + G[1,1])/π."""
        g = self._local(t, "ldos")
        return -(g[:, 0, 0] + g[:, 1, 1]).imag / np.pi

    def spin_ldos(self, t: int = 0) -> np.ndarray:
        """(K, 2) -Im G[0,0]/π and -Im G[1,1]/π."""
        g = self._local(t, "spin_ldos")
        return np.stack([-g[:, 0, 0].imag, -g[:, 1, 1].imag], axis=1) / np.pi

    def spin_density(self, t: int = 0) -> np.ndarray:
        """(K, 3) -Im tr(σ_k G[0:2, 0:2])/π for k = x, y, z."""
        from .common import σ1, σ2, σ3

        g = self._local(t, "spin_density")[:, 0:2, 0:2]
        return np.stack([-np.einsum("ab,kba->k", s, g).imag for s in (σ1, σ2, σ3)], axis=1) / np.pi

    def anomalous(self, t: int = 0) -> np.ndarray:
        """(K, 2, 2) the electron-hole block G[0:2, 2:4]."""
        return self.blocks[t][:, 0:2, 2:4].copy()


def green(system, source: Coord, energies, targets=None, *, broadening=None, moments: int | None = None,
          digits: float = 12.0, scale: float | None = None, _all_columns: bool = False) -> GreenFunction:
    """G(E + iΓ) from `source` to `targets` (see `Hamiltonian.green`)."""
    source = tuple(source)
    targets = [source] if targets is None else [tuple(t) for t in targets]
    if not targets:
        raise ValueError("green: targets is empty")
    energies, gamma, moments, scale = _series_arguments(system, energies, broadening, moments, digits, scale)

    site = int(system.lattice[source])
    target_sites = np.array([system.lattice[t] for t in targets], dtype=np.int64)
    distinct, where = np.unique(target_sites, return_inverse=True)  # (a block row has one slot in the device table)
    # particle-hole symmetry (H = -τx H* τx block by block) gives the hole columns from the electron columns
    derive = not _all_columns and system.has_symmetric_spectrum(1e-12)
    columns = 2 if derive else 4
    rows = 4 * site + np.arange(columns, dtype=np.int64)

    solver = system._solver()
    z = energies + 1j * gamma
    per_target = moments * 4 * columns * 16
    group = max(1, HOST_TABLE_LIMIT // per_target)
    blocks = np.empty((distinct.size, energies.size, 4, 4), dtype=np.complex128)
    perf = []
    for lo in range(0, distinct.size, group):
        mu = solver.green_moments(scale, moments, rows, distinct[lo : lo + group])
        perf.append(solver.perf())
        blocks[lo : lo + group] = blocks_from_moments(hole_columns(mu) if derive else mu, scale, z)
    info = {"moments": moments, "scale": scale, "columns": columns, "hole_columns_derived": derive,
            "perf": perf[0] if len(perf) == 1 else perf}
    return GreenFunction(np.ascontiguousarray(blocks[where.reshape(-1)]), energies, gamma, source, targets, info)


class GreenMap:
    """Local blocks of G(ε + iΓ) at many sites.

    `blocks` (S, K, 4, 4) complex128: blocks[s, k] = G(E_k + iΓ_k)[4j_s:4j_s+4, 4j_s:4j_s+4]; `energies` and
    `broadening` (K,), `sites` the lattice coordinates, `info` the route details as in `GreenFunction`.  The
    helpers are those of `GreenFunction` with one leading site axis more.
    """

    def __init__(self, blocks: np.ndarray, energies: np.ndarray, broadening: np.ndarray, sites, info: dict | None = None):
        self.blocks = blocks
        self.energies = energies
        self.broadening = broadening
        self.sites = [tuple(site) for site in sites]
        self.info = dict(info or {})

    def site(self, coord: Coord) -> np.ndarray:
        """(K, 4, 4) blocks of the site `coord` (its first position in `sites`)."""
        coord = tuple(coord)
        if coord not in self.sites:
            raise ValueError(f"site: {coord} is not among the mapped sites")
        return self.blocks[self.sites.index(coord)]

    def ldos(self) -> np.ndarray:
        """(S, K) spin-summed electron LDOS -Im(G[0,0] + G[1,1])/π."""
        g = self.blocks
        return -(g[:, :, 0, 0] + g[:, :, 1, 1]).imag / np.pi

    def spin_ldos(self) -> np.ndarray:
        """(S, K, 2) -Im G[0,0]/π and -Im G[1,1]/π."""
        g = self.blocks
        return np.stack([-g[:, :, 0, 0].imag, -g[:, :, 1, 1].imag], axis=2) / np.pi

    def spin_density(self) -> np.ndarray:
        """(S, K, 3) -Im tr(σ_k G[0:2, 0:2])/π for k = x, y, z."""
        from .common import σ1, σ2, σ3

        g = self.blocks[:, :, 0:2, 0:2]
        return np.stack([-np.einsum("ab,skba->sk", s, g).imag for s in (σ1, σ2, σ3)], axis=2) / np.pi

    def anomalous(self) -> np.ndarray:
        """(S, K, 2, 2) the electron-hole blocks G[0:2, 2:4]."""
        return self.blocks[:, :, 0:2, 2:4].copy()


def green_map(system, energies, sites=None, *, broadening=None, moments: int | None = None, digits: float = 12.0,
              scale: float | None = None, _all_columns: bool = False) -> GreenMap:
    """Local blocks G_jj(E + iΓ) at the sites `sites` (see `Hamiltonian.green_map`)."""
    if sites is None:
        sites = list(system.lattice.sites())
        indices = np.arange(system.lattice.size, dtype=np.int64)
    else:
        sites = [tuple(site) for site in sites]
        indices = np.array([system.lattice[site] for site in sites], dtype=np.int64)
    if not sites:
        raise ValueError("green: sites is empty")
    energies, gamma, moments, scale = _series_arguments(system, energies, broadening, moments, digits, scale)

    distinct, where = np.unique(indices, return_inverse=True)  # (a block row is listed once in a device call)
    derive = not _all_columns and system.has_symmetric_spectrum(1e-12)
    columns = 2 if derive else 4

    solver = system._solver()
    z = energies + 1j * gamma
    per_site = moments * 4 * columns * 16
    group = max(1, HOST_TABLE_LIMIT // per_site)
    if group > 64:
        group -= group % 64  # (whole device batches: a batch holds 64 / columns sites or a power of two less)
    blocks = np.empty((distinct.size, energies.size, 4, 4), dtype=np.complex128)
    perf = []
    for lo in range(0, distinct.size, group):
        mu = solver.green_local_moments(scale, moments, distinct[lo : lo + group], columns)
        perf.append(solver.perf())
        blocks[lo : lo + group] = blocks_from_moments(hole_columns(mu) if derive else mu, scale, z)
    info = {"moments": moments, "scale": scale, "columns": columns, "hole_columns_derived": derive,
            "perf": perf[0] if len(perf) == 1 else perf}
    return GreenMap(np.ascontiguousarray(blocks[where.reshape(-1)]), energies, gamma, sites, info)


class GreenStates:
    """Blocks of G(ε + iΓ) between the Nambu vectors of extended states.

    `blocks` (Q, K, 4, 4) complex128: blocks[q, k][a, b] = <w_q a|G(E_k + iΓ_k)|w_q b> with |w b> = Σ_j w[j] e_{4j+b};
    `energies` and `broadening` (K,), `states` the (Q, N) amplitudes, `momenta` the (Q, 3) wave vectors when the states
    are the plane waves of `spectral_function` (else None), `info` the route details as in `GreenFunction`.  The
    helpers are those of `GreenMap` with a state axis where it has a site axis.
    """

    def __init__(self, blocks: np.ndarray, energies: np.ndarray, broadening: np.ndarray, states: np.ndarray,
                 info: dict | None = None, momenta: np.ndarray | None = None):
        self.blocks = blocks
        self.energies = energies
        self.broadening = broadening
        self.states = states
        self.momenta = momenta
        self.info = dict(info or {})

    def spectral(self) -> np.ndarray:
        """(Q, K) spin-summed electron spectral function -Im(G[0,0] + G[1,1])/π: A(k, ε) for plane waves."""
        g = self.blocks
        return -(g[:, :, 0, 0] + g[:, :, 1, 1]).imag / np.pi

    def spin_spectral(self) -> np.ndarray:
        """(Q, K, 2) -Im G[0,0]/π and -Im G[1,1]/π."""
        g = self.blocks
        return np.stack([-g[:, :, 0, 0].imag, -g[:, :, 1, 1].imag], axis=2) / np.pi

    def spin_density(self) -> np.ndarray:
        """(Q, K, 3) -Im tr(σ_k G[0:2, 0:2])/π for k = x, y, z."""
        from .common import σ1, σ2, σ3

        g = self.blocks[:, :, 0:2, 0:2]
        return np.stack([-np.einsum("ab,qkba->qk", s, g).imag for s in (σ1, σ2, σ3)], axis=2) / np.pi

    def anomalous(self) -> np.ndarray:
        """(Q, K, 2, 2) the electron-hole blocks G[0:2, 2:4]: F(k, ε) for plane waves."""
        return self.blocks[:, :, 0:2, 2:4].copy()


def _conjugate_partners(states: np.ndarray):
    """partner[q] = a row equal (`np.array_equal`) to conj(states[q]), or None if some state has no such row."""
    def key(row):
        return (row.view(np.float64) + 0.0).tobytes()  # (+ 0.0: -0.0 and 0.0 compare equal, so they share a key)

    where = {}
    for q, row in enumerate(states):
        where.setdefault(key(row), q)
    partner = np.empty(states.shape[0], dtype=np.int64)
    for q, row in enumerate(states):
        p = where.get(key(np.conj(row)))
        if p is None:
            return None
        partner[q] = p
    return partner


def hole_columns_of_states(mu: np.ndarray, partner: np.ndarray) -> np.ndarray:
    """(M, Q, 4, 4) moments from the electron columns (M, Q, 4, 2) of states whose conjugates are among them:
    μ_n[q][a][b] = (-1)ⁿ conj μ_n[p][a⊕2][b⊕2] with w_p = conj(w_q), p = partner[q]."""
    full = np.empty(mu.shape[:3] + (4,), dtype=np.complex128)
    full[..., 0:2] = mu
    sign = np.where(np.arange(mu.shape[0]) & 1, -1.0, 1.0)[:, None, None, None]
    full[..., 2:4] = sign * mu[:, partner][:, :, [2, 3, 0, 1], :].conj()
    return full


def green_states(system, states, energies, *, broadening=None, moments: int | None = None, digits: float = 12.0,
                 scale: float | None = None, _all_columns: bool = False, _momenta=None) -> GreenStates:
    """<w a|G(E + iΓ)|w b> for the states `states` (see `Hamiltonian.green_states`)."""
    states = np.array(states, dtype=np.complex128)
    if states.ndim == 1:
        states = states[None, :]
    n_sites = system.lattice.size
    if states.ndim != 2 or states.shape[0] < 1:
        raise ValueError("green_states: states is empty (expected (Q, N) or (N,) amplitudes)")
    if states.shape[1] != n_sites:
        raise ValueError(f"green_states: states of {states.shape[1]} amplitudes for a lattice of {n_sites} sites")
    if not np.all(np.isfinite(states)):
        raise ValueError("green_states: the amplitudes must be finite")
    energies, gamma, moments, scale = _series_arguments(system, energies, broadening, moments, digits, scale)

    # particle-hole symmetry gives the hole columns of a state from the electron columns of its complex conjugate
    partner = None
    if not _all_columns and system.has_symmetric_spectrum(1e-12):
        partner = _conjugate_partners(states)
    derive = partner is not None
    columns = 2 if derive else 4

    # groups of states whose moment table stays under the host limit; a state and its partner share a group
    per_state = moments * 4 * columns * 16
    limit = max(1, HOST_TABLE_LIMIT // per_state)
    groups, current, placed = [], [], np.zeros(states.shape[0], dtype=bool)
    for q in range(states.shape[0]):
        if placed[q]:
            continue
        unit = [q] if not derive or partner[q] == q else [q, int(partner[q])]
        if current and len(current) + len(unit) > limit:
            groups.append(current)
            current = []
        current.extend(unit)
        placed[unit] = True
    groups.append(current)

    solver = system._solver()
    z = energies + 1j * gamma
    blocks = np.empty((states.shape[0], energies.size, 4, 4), dtype=np.complex128)
    perf = []
    for rows in groups:
        rows = np.asarray(rows, dtype=np.int64)
        distinct = np.unique(rows)
        mu = solver.green_state_moments(scale, moments, states[distinct], columns)
        perf.append(solver.perf())
        if derive:  # (partners within the group: a repeated row may have met its partner in an earlier group too)
            mu = hole_columns_of_states(mu, _conjugate_partners(states[distinct]))
        blocks[distinct] = blocks_from_moments(mu, scale, z)
    info = {"moments": moments, "scale": scale, "columns": columns, "hole_columns_derived": derive,
            "perf": perf[0] if len(perf) == 1 else perf}
    return GreenStates(blocks, energies, gamma, states, info, _momenta)


def spectral_function(system, momenta, energies, **options) -> GreenStates:
    """G(k, E + iΓ) in plane waves (see `Hamiltonian.spectral_function`)."""
    momenta = np.asarray(momenta, dtype=float)
    if momenta.size == 0:
        raise ValueError("green_states: momenta is empty")
    if momenta.ndim == 1:
        momenta = momenta[None, :]
    if momenta.ndim != 2 or momenta.shape[1] != 3:
        raise ValueError(f"green_states: expected momenta of shape (Q, 3) or (3,), not {momenta.shape}")
    if not np.all(np.isfinite(momenta)):
        raise ValueError("green_states: the momenta must be finite")
    return green_states(system, system.lattice.plane_waves(momenta), energies, _momenta=momenta, **options)
