"""Local and non-local blocks of the retarded Green's function (`Hamiltonian.green`, `Hamiltonian.green_map`,
`Hamiltonian.green_bonds`).

G(z) = (z - H)^-1 at z = ε + iΓ for the whole 4N x 4N BdG matrix, Nambu basis (e↑, e↓, h↑, h↓) per site.
`GreenFunction.blocks[t, k]` = G(E_k + iΓ_k)[4j_t:4j_t+4, 4i:4i+4] for the source site i and the target
sites j_t.  The helpers are slices of these blocks, so no sign convention is hidden in them.

Route: the unit vectors e_{4i+b} of the source site run through the Chebyshev recurrence on
the GPU, and every step stores the rows of the target sites (`bdg_green_moments`): the moments
μ_n[ja, ib] = <e_{4j+a}|T_n(H/a)|e_{4i+b}>.  The blocks follow from the operator form of
`chebyshev.resolvent_series`,

    G(z)[ja, ib] = -i / (a·sqrt(1 - z̃²)) · Σ_n (2 - δ_n0) · exp(-i·n·arccos z̃) · μ_n[ja, ib],   z̃ = z/a.

With particle-hole symmetry (H = -τx H* τx) only the electron columns b = 0, 1 are run; the hole columns are
μ_n[a, b] = (-1)ⁿ·conj μ_n[a⊕2, b⊕2].  G(ε + iΓ) decays slowly with distance in a band at small Γ, so by default
every source site gets its own start vectors; `green_map` and `green_bonds` probe several sources with one vector on
request (`distance=`, below).

Probing: `green_map(distance=d)` and `green_bonds(distance=d)` colour the sites as `fermi_matrix` does
and start one vector per colour and Nambu column, the sum of the colour's unit vectors with signs ξ = ±1
(`bdg_green_probe_blocks`).  The number of vectors no longer grows with the lattice; a block carries the other sites of
its colour, Σ ξ_i ξ_i' G_ji', a bias with ξ = +1 and zero-mean noise with random signs, whose mean and standard error
over `samples` are taken on the device.

Maps: `green_map` wants the local block G_jj at many sites j.  The start vectors of up to 32
sites share one batch of the recurrence, and a step stores for every vector the rows of its own site only
(`bdg_green_local_moments`), so a launch runs at full width and the moment table grows with the number of
sites, not with its square.

Bonds: `green_bonds` wants G_ji on every block (j, i) of H's skeleton whose column i is one of the
source sites - the bond anomalous function of a d- or p-wave superconductor, the spectral current.  The batches are
those of `green_map`; a step stores, on every block row j, the entries of the vectors that started on a site i with
(j, i) in the pattern, and the moments are contracted with the series weights on the device
(`bdg_green_bond_blocks`): only energies x blocks x 16 numbers come back.

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


# ---------------------------------------------------------------- probing
def z2_signs(seed: int, samples: int, n_sites: int) -> np.ndarray:
    """(samples, n_sites) int8 of ±1: sample s is np.random.default_rng(seed + s).choice([-1, 1], n_sites)."""
    return np.stack([np.random.default_rng(int(seed) + s).choice([-1, 1], n_sites) for s in range(samples)]).astype(np.int8)


def _probe_arguments(system, distance, samples, seed, signs, wanted: np.ndarray):
    """Colours and signs of a probed call, checked.  `wanted` (N,) bool marks the source sites; returns (colour (N,)
    int32 with -1 off the source sites and the colours in use numbered from 0, their number, the colour periods of a
    cubic lattice or None, signs (samples, N) int8 or None for one sample of all +1, samples)."""
    from . import fermi
    from .lattice import CubicLattice

    n = system.lattice.size
    distance, samples = int(distance), int(samples)
    if distance < 3:
        raise ValueError("green: distance must be >= 3 (or None for one start vector per site)")
    if samples < 1:
        raise ValueError("green: samples must be >= 1")
    if signs is None:
        signs = "z2" if samples > 1 else None
    if isinstance(signs, str):
        if signs != "z2":
            raise ValueError(f"green: signs must be None, 'z2' or a (samples, N) array of ±1, not {signs!r}")
        signs = z2_signs(seed, samples, n)
    elif signs is not None:
        signs = np.asarray(signs)
        if signs.shape != (samples, n):
            raise ValueError(f"green: signs of shape {signs.shape} for {samples} samples of {n} sites")
        if not np.all(np.abs(signs) == 1) or np.iscomplexobj(signs):
            raise ValueError("green: only signs of +1 and -1 are supported")
        signs = signs.astype(np.int8)
    if samples > 1 and (signs is None or np.all(signs == 1)):
        raise ValueError("green: samples > 1 needs random signs (all +1 gives the same sample every time)")
    colour, _ = fermi.site_colours(system, distance)
    colour = np.array(colour, dtype=np.int32)
    colour[~wanted] = -1
    used, compact = np.unique(colour[wanted], return_inverse=True)
    colour[wanted] = compact.astype(np.int32)
    periods = None
    if isinstance(system.lattice, CubicLattice):
        periods = fermi.colour_periods(system.lattice.shape, distance)
    return colour, int(used.size), periods, signs, samples


def _probed_blocks(solver, scale, weights, n_sites, rows, cols, columns, colour, n_colours, signs):
    """The probed blocks on the pattern (rows, cols) (canonical order) and their standard error or None, (nnz, K, 4, 4),
    with the perf records: groups of whole colours whose result (energies x blocks x 256 B) stays within the host
    limit; the sites of the other groups take no part in a group's call (colour -1)."""
    per_colour = np.bincount(colour[cols], minlength=n_colours) * weights.shape[0] * 256
    blocks = np.empty((cols.size, weights.shape[0], 4, 4), dtype=np.complex128)
    stderr = np.empty_like(blocks) if signs is not None and signs.shape[0] > 1 else None
    perf, lo = [], 0
    while lo < n_colours:
        hi = lo + max(1, int(np.searchsorted(np.cumsum(per_colour[lo:]), HOST_TABLE_LIMIT, side="right")))
        full = 64 // columns  # colours of the widest device batch; narrower ones (a power of two less) divide it
        if hi < n_colours and hi - lo > full:
            hi -= (hi - lo) % full  # (whole device batches, whatever the width: no group ends on a part-filled one)
        hi = min(hi, n_colours)
        part = np.flatnonzero((colour[cols] >= lo) & (colour[cols] < hi))
        part_indptr = np.zeros(n_sites + 1, dtype=np.int32)
        np.cumsum(np.bincount(rows[part], minlength=n_sites), out=part_indptr[1:])
        group = np.where((colour >= lo) & (colour < hi), colour - lo, -1).astype(np.int32)
        mean, error = solver.green_probe_blocks(scale, weights, group, hi - lo, part_indptr, cols[part].astype(np.int32),
                                                columns, signs)
        perf.append(solver.perf())
        blocks[part] = mean.transpose(1, 0, 2, 3)
        if stderr is not None:
            stderr[part] = error.transpose(1, 0, 2, 3)
        lo = hi
    return blocks, stderr, perf


class GreenMap:
    """Local blocks of G(ε + iΓ) at many sites.

    `blocks` (S, K, 4, 4) complex128: blocks[s, k] = G(E_k + iΓ_k)[4j_s:4j_s+4, 4j_s:4j_s+4]; `energies` and
    `broadening` (K,), `sites` the lattice coordinates, `info` the route details as in `GreenFunction`.  The
    helpers are those of `GreenFunction` with one leading site axis more.  `stderr` is None, or for a probed call with
    two samples or more an array of the shape of `blocks`: the standard error of the mean over the samples,
    sqrt(Σ(x - mean)² / (S(S - 1))), of Re in its real part and of Im in its imaginary part.
    """

    def __init__(self, blocks: np.ndarray, energies: np.ndarray, broadening: np.ndarray, sites, info: dict | None = None,
                 stderr: np.ndarray | None = None):
        self.blocks = blocks
        self.energies = energies
        self.broadening = broadening
        self.sites = [tuple(site) for site in sites]
        self.info = dict(info or {})
        self.stderr = stderr  # probed with samples >= 2: the standard error of Re (real part) and Im (imaginary part)

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
              scale: float | None = None, distance: int | None = None, samples: int = 1, seed: int = 0, signs=None,
              _all_columns: bool = False) -> GreenMap:
    """Local blocks G_jj(E + iΓ) at the sites `sites` (see `Hamiltonian.green_map`).

    distance=None: one start vector per site and Nambu column, exact up to the truncation of the series.  distance=d
    (>= 3) probes: the sites are coloured as for `fermi_matrix(distance=d)`, one start vector per colour and Nambu
    column carries all sites of the colour, and a block picks up Σ ξ_j ξ_j' G_jj' over the other sites j' of its colour
    (|G_jj'(ε + iΓ)| at range >= d: small inside a gap or at large Γ, not in a band at small Γ).
    `signs` None: ξ = +1 (the default for samples=1, a bias); "z2": ξ = ±1 per site from `seed` (the default for
    samples > 1: zero-mean noise, `blocks` the mean over the samples and `stderr` its standard error); or a
    (samples, N) array of ±1.  Sites not in `sites` are no sources."""
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

    if distance is not None:  # probing: the diagonal blocks of the sites are the pattern
        n = system.lattice.size
        wanted = np.zeros(n, dtype=bool)
        wanted[distinct] = True
        colour, n_colours, periods, signs, samples = _probe_arguments(system, distance, samples, seed, signs, wanted)
        weights = moment_weights(moments, scale, energies + 1j * gamma)
        blocks, stderr, perf = _probed_blocks(system._solver(), scale, weights, n, distinct, distinct, columns, colour,
                                              n_colours, signs)
        info = {"moments": moments, "scale": scale, "columns": columns, "hole_columns_derived": derive,
                "perf": perf[0] if len(perf) == 1 else perf, "distance": int(distance), "periods": periods,
                "colours": n_colours, "samples": samples, "seed": int(seed)}
        where = where.reshape(-1)
        return GreenMap(np.ascontiguousarray(blocks[where]), energies, gamma, sites, info,
                        None if stderr is None else np.ascontiguousarray(stderr[where]))

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


class GreenBonds:
    """Blocks of G(ε + iΓ) on a pattern of site pairs: the skeleton blocks (j, i) of H whose column i is a source site.

    `blocks` (nnz, K, 4, 4) complex128: blocks[k, e] = G(E_e + iΓ_e)[4j:4j+4, 4i:4i+4] for block k = (block row j,
    block column i); `indptr` / `indices` the pattern (int32, BSR, as in `FermiMatrix`), `energies` and `broadening`
    (K,), `lattice` the system's, `info` the route details as in `GreenFunction`.  The helpers are slices and sums of
    the blocks, so no sign convention is hidden in them.
    """

    def __init__(self, lattice, indptr: np.ndarray, indices: np.ndarray, blocks: np.ndarray, energies: np.ndarray,
                 broadening: np.ndarray, info: dict | None = None, skeleton=None, stderr: np.ndarray | None = None):
        self.lattice = lattice
        self.stderr = stderr  # as in `GreenMap`
        self.indptr = indptr
        self.indices = indices
        self.blocks = blocks
        self.energies = energies
        self.broadening = broadening
        self.info = dict(info or {})
        n = lattice.size
        self._rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
        self._keys = self._rows * n + indices
        self._mirror = None
        self._skeleton = skeleton  # (blocks of the system's skeleton, index of every pattern block in it) or None

    def _find(self, rows: np.ndarray, cols: np.ndarray) -> np.ndarray:
        wanted = rows * self.lattice.size + cols
        found = np.minimum(np.searchsorted(self._keys, wanted), len(self._keys) - 1)
        if np.any(self._keys[found] != wanted):
            raise IndexError("The pattern has no block for this pair of sites")
        return found

    def block(self, j: Coord, i: Coord) -> np.ndarray:
        """(K, 4, 4) G[4j:4j+4, 4i:4i+4] for lattice coordinates j (row, target) and i (column, source); a copy."""
        k = self._find(np.array([self.lattice[j]], dtype=np.int64), np.array([self.lattice[i]], dtype=np.int64))[0]
        return self.blocks[k].copy()

    def local(self) -> GreenMap:
        """The diagonal blocks G_ii of the source sites as a `GreenMap` (ldos(), spin_ldos(), ...), in index order."""
        diagonal = np.flatnonzero(self._rows == self.indices)
        coords = list(self.lattice.sites())
        sites = [coords[int(i)] for i in self.indices[diagonal]]
        stderr = None if self.stderr is None else np.ascontiguousarray(self.stderr[diagonal])
        return GreenMap(np.ascontiguousarray(self.blocks[diagonal]), self.energies, self.broadening, sites, self.info, stderr)

    def anomalous(self, j: Coord, i: Coord) -> np.ndarray:
        """(K, 2, 2) the electron-hole block G_ji[0:2, 2:4]: the pair function on the bond (j, i)."""
        return self.block(j, i)[:, 0:2, 2:4]

    def _mirrors(self) -> np.ndarray:
        if self._mirror is None:
            self._mirror = self._find(self.indices.astype(np.int64), self._rows)
        return self._mirror

    def spectral(self) -> np.ndarray:
        """(nnz, K, 4, 4) A_ji(ε) = (i/2π)(G_ji - conj(G_ij)ᵀ): the blocks of (i/2π)(G - G†), a broadened δ(ε - H).
        Needs the mirror block (i, j) of every block (j, i): IndexError where the pattern lacks one."""
        mirror = self.blocks[self._mirrors()]
        return (0.5j / np.pi) * (self.blocks - mirror.conj().transpose(0, 1, 3, 2))

    def _operator_blocks(self, dH) -> np.ndarray:
        """(nnz, 4, 4) blocks of dH on this pattern: a block array on the pattern, a Hamiltonian on the same lattice
        (its blocks), a block array on the system's skeleton, or a sparse (4N, 4N) matrix without entries elsewhere."""
        import scipy.sparse as sp

        if sp.issparse(dH):
            coo = sp.coo_matrix(dH)
            n = self.lattice.size
            if coo.shape != (4 * n, 4 * n):
                raise ValueError(f"expected an operator of shape {(4 * n, 4 * n)}, got {coo.shape}")
            keep = coo.data != 0
            row, col, values = coo.row[keep].astype(np.int64), coo.col[keep].astype(np.int64), coo.data[keep]
            try:
                where = self._find(row // 4, col // 4) if row.size else np.zeros(0, dtype=np.int64)
            except IndexError:
                raise ValueError("the operator has entries outside the pattern of these blocks") from None
            data = np.zeros(self.blocks.shape[:1] + (4, 4), dtype=np.complex128)
            np.add.at(data, (where, row % 4, col % 4), values)
            return data
        data = np.asarray(getattr(dH, "_data", dH))
        wanted = self.blocks.shape[:1] + (4, 4)
        if data.shape != wanted and self._skeleton is not None and data.shape == (self._skeleton[0], 4, 4):
            data = data[self._skeleton[1]]
        if data.shape != wanted:
            raise ValueError(f"expected blocks of shape {wanted} on the same pattern, got {data.shape}")
        return data

    def expectation(self, dH) -> np.ndarray:
        """(K,) complex ½ Σ_{(i,j) in pattern} tr(A_ji(ε) dH_ij) with A = spectral(), the conventions of
        `FermiMatrix.expectation`: ∫ f(ε)·expectation(dH) dε tends to `FermiMatrix.expectation(dH)` as Γ -> 0.  With
        dH = `correlation.current_operator(system, axis)` it is the spectral current; real up to round-off for
        Hermitian dH."""
        data = self._operator_blocks(dH)
        return 0.5 * np.einsum("keab,kba->e", self.spectral()[self._mirrors()], data)


def green_bonds(system, energies, sites=None, *, broadening=None, moments: int | None = None, digits: float = 12.0,
                scale: float | None = None, distance: int | None = None, samples: int = 1, seed: int = 0, signs=None,
                _all_columns: bool = False) -> GreenBonds:
    """G_ji(E + iΓ) on every skeleton block (j, i) of H with i among `sites` (see `Hamiltonian.green_bonds`);
    `distance`, `samples`, `seed` and `signs` probe as in `green_map`: block (j, i) picks up Σ ξ_i ξ_i' G_ji' over the
    other sites i' of the colour of i."""
    n = system.lattice.size
    if sites is None:
        columns_wanted = np.arange(n, dtype=np.int64)
    else:
        columns_wanted = np.array([system.lattice[tuple(site)] for site in sites], dtype=np.int64)
    if columns_wanted.size == 0:
        raise ValueError("green: sites is empty")
    energies, gamma, moments, scale = _series_arguments(system, energies, broadening, moments, digits, scale)

    full_indptr = np.asarray(system._matrix.indptr, dtype=np.int64)
    full_indices = np.asarray(system._matrix.indices, dtype=np.int64)
    full_rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(full_indptr))
    distinct = np.unique(columns_wanted)  # (a site is a source once, whatever the order of the list)
    wanted = np.zeros(n, dtype=bool)
    wanted[distinct] = True
    kept = np.flatnonzero(wanted[full_indices])  # the pattern: skeleton blocks with a source site for a column
    rows, cols = full_rows[kept], full_indices[kept]
    indptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    indices = cols.astype(np.int32)

    derive = not _all_columns and system.has_symmetric_spectrum(1e-12)
    columns = 2 if derive else 4
    if distance is not None:
        colour, n_colours, periods, signs, samples = _probe_arguments(system, distance, samples, seed, signs, wanted)
        weights = moment_weights(moments, scale, energies + 1j * gamma)
        blocks, stderr, perf = _probed_blocks(system._solver(), scale, weights, n, rows, cols, columns, colour, n_colours,
                                              signs)
        info = {"moments": moments, "scale": scale, "columns": columns, "hole_columns_derived": derive,
                "perf": perf[0] if len(perf) == 1 else perf, "distance": int(distance), "periods": periods,
                "colours": n_colours, "samples": samples, "seed": int(seed)}
        return GreenBonds(system.lattice, indptr, indices, blocks, energies, gamma, info, (full_indices.size, kept), stderr)
    solver = system._solver()
    weights = moment_weights(moments, scale, energies + 1j * gamma)
    # groups of source sites whose result (energies x blocks x 256 B) stays within the host limit
    per_site = np.bincount(cols, minlength=n)[distinct] * energies.size * 256
    blocks = np.empty((kept.size, energies.size, 4, 4), dtype=np.complex128)
    perf, lo = [], 0
    while lo < distinct.size:
        hi = lo + max(1, int(np.searchsorted(np.cumsum(per_site[lo:]), HOST_TABLE_LIMIT, side="right")))
        if hi < distinct.size and hi - lo > 64:
            hi -= (hi - lo) % 64  # (whole device batches)
        member = np.zeros(n, dtype=bool)
        member[distinct[lo:hi]] = True
        part = np.flatnonzero(member[cols])
        part_indptr = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(np.bincount(rows[part], minlength=n), out=part_indptr[1:])
        result = solver.green_bond_blocks(scale, weights, part_indptr, indices[part], columns)
        perf.append(solver.perf())
        blocks[part] = result.transpose(1, 0, 2, 3)
        lo = hi
    info = {"moments": moments, "scale": scale, "columns": columns, "hole_columns_derived": derive,
            "perf": perf[0] if len(perf) == 1 else perf}
    return GreenBonds(system.lattice, indptr, indices, blocks, energies, gamma, info, (full_indices.size, kept))


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
