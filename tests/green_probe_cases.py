"""Shared by tests/test_green_probe_host.py and tests/test_gpu_green_probe.py: the shapes at which colours hold several
sites, a numpy restatement of bdg_green_probe_blocks on sparse H (the probe vectors with signs in batches of whole
colours, one recurrence, the rows of every pattern block picked from the vectors of its column site's colour, the
hole-column rule, the weights in ascending n, the sign of the column site, Welford's update in the kernel's order) and
the probed dense sum - what the device must reproduce, which is not the true G.  Models, energies, Γ and the default
moments are those of green_bonds_cases.  The restatements are computed once and handed out read-only."""

import functools

import numpy as np
import scipy.sparse as sp

from bodge_amd import fermi
from bodge_amd import green as gr

import green_bonds_cases as cases

# name -> (builder, shape, distance, colour periods, colours, sites per colour)
SHAPES = {
    "dwave_9x8": (cases.dwave_open, (9, 8, 1), 3, (3, 4, 1), 12, 6),
    "dwave_8x6": (cases.dwave_open, (8, 6, 1), 4, (4, 6, 1), 24, 2),
    "peierls_8x6": (cases.peierls_disordered, (8, 6, 1), 4, (4, 6, 1), 24, 2),
    "cube_6x4x4": (cases.cube, (6, 4, 4), 3, (3, 4, 4), 48, 2),
}
IS_REAL = {"dwave_9x8": True, "dwave_8x6": True, "peierls_8x6": False, "cube_6x4x4": True}
SIGNS = ("plus", "z2")
SEED = 3
Z = cases.Z


def build(name):
    """A new system of the shape `name` (for a handle of its own)."""
    builder, shape = SHAPES[name][:2]
    return builder(shape)


@functools.lru_cache(maxsize=None)
def system_of(name):
    """The system for host-side use: built once, never modified."""
    return build(name)


def colours_of(system, distance, columns=None):
    """(colour (N,) int32, number of colours) as green_map / green_bonds(distance=...) pass them on: the colours of
    fermi.site_colours, -1 on the sites outside `columns`, the colours in use numbered from 0."""
    colour, _ = fermi.site_colours(system, distance)
    colour = np.array(colour, dtype=np.int32)
    if columns is not None:
        keep = np.zeros(colour.size, dtype=bool)
        keep[np.asarray(columns, dtype=np.int64)] = True
        colour[~keep] = -1
    used, compact = np.unique(colour[colour >= 0], return_inverse=True)
    colour[colour >= 0] = compact.astype(np.int32)
    return colour, int(used.size)


def signs_of(kind, n_sites, samples=1, seed=SEED):
    """(samples, N) int8: all +1 for "plus", the signs of green.z2_signs restated for "z2"."""
    if kind == "plus":
        return np.ones((samples, n_sites), dtype=np.int8)
    return np.stack([np.random.default_rng(seed + s).choice([-1, 1], n_sites) for s in range(samples)]).astype(np.int8)


# ------------------------------------------------------------------ the restatement
def probe_moments(h, indptr, indices, colour, n_colours, xi, moments, scale, columns=4, batch=None):
    """bdg_green_probe_blocks up to the contraction for one sample: the colours in batches of `batch` (default
    64 / columns); in a batch vector v = columns * c + b starts at Σ_{i: colour(i) = c} ξ_i e_{4i + b}, all vectors run
    one recurrence, and of every t_n the four rows of block row j are picked from the vectors of colour(i) for every
    pattern block (j, i) of the batch: (M, nnz, 4, columns), zero where the column site has no colour."""
    h = sp.csr_matrix(h)
    indices = np.asarray(indices, dtype=np.int64)
    rows = cases.block_rows(indptr)
    batch = batch or max(1, 64 // columns)
    of_block = colour[indices]
    mu = np.zeros((moments, indices.size, 4, columns), dtype=np.complex128)
    for c0 in range(0, n_colours, batch):
        n_own = min(batch, n_colours - c0)
        width = n_own * columns
        prev = np.zeros((h.shape[0], width), dtype=np.complex128)
        cur = prev.copy()
        for i in np.flatnonzero((colour >= c0) & (colour < c0 + n_own)):
            for b in range(columns):
                cur[4 * i + b, columns * (colour[i] - c0) + b] = xi[i]
        mine = np.flatnonzero((of_block >= c0) & (of_block < c0 + n_own))
        slot = of_block[mine] - c0
        pick_rows = 4 * rows[mine][:, None, None] + np.arange(4)[None, :, None]          # [k, a, .]
        pick_cols = columns * slot[:, None, None] + np.arange(columns)[None, None, :]   # [k, ., b]
        for n in range(moments):
            mu[n, mine] = cur[pick_rows, pick_cols]
            cur, prev = (1.0 if n == 0 else 2.0) * (h @ cur) / scale - prev, cur
    return mu


def restate_sample(system, indptr, indices, colour, n_colours, xi, z, moments, columns=4, batch=None):
    """One sample x_s as the device computes it, (nnz, K, 4, 4): the moments, the hole columns for columns = 2
    (green.hole_columns, term by term: the signs are real), the weights in ascending n, then the sign of the block's
    column site."""
    scale = cases.scale_of(system)
    mu = probe_moments(system.matrix("csr"), indptr, indices, colour, n_colours, xi, moments, scale, columns, batch)
    if columns == 2:
        mu = gr.hole_columns(mu)
    out = cases.contract(mu, gr.moment_weights(moments, scale, z))
    return out * np.asarray(xi, dtype=float)[np.asarray(indices, dtype=np.int64)][:, None, None, None]


def welford(samples):
    """(mean, standard error) of the arrays `samples` by the update of green_probe_accumulate, Re and Im apart:
    δ = x - mean; mean += δ / s; M2 += δ (x - mean); at the end sqrt(M2 / (S (S - 1))) (zeros for one sample)."""
    mean = np.zeros(samples[0].shape, dtype=np.complex128)
    m2 = np.zeros(samples[0].shape, dtype=np.complex128)
    for s, x in enumerate(samples, start=1):
        for part in ("real", "imag"):
            xs, m, q = getattr(x, part), getattr(mean, part), getattr(m2, part)
            delta = xs - m
            m += delta / s
            q += delta * (xs - m)
    count = len(samples)
    if count == 1:
        return mean, np.zeros_like(mean)
    return mean, np.sqrt(m2.real / (count * (count - 1))) + 1j * np.sqrt(m2.imag / (count * (count - 1)))


# ------------------------------------------------------------------ the probed dense sum
def dense_resolvent(system, z):
    """(K, N, 4, N, 4) V (z - E)^-1 V† from numpy.linalg.eigh."""
    n = system.lattice.size
    w, v = np.linalg.eigh(np.asarray(system.matrix("dense")))
    return np.stack([((v / (ze - w)[None, :]) @ v.conj().T).reshape(n, 4, n, 4) for ze in z])


def probed_dense(g, indptr, indices, colour, xi):
    """D[k = (j, i)] = Σ_{i': colour(i') = colour(i)} ξ_i ξ_i' G[j, i'] from the dense resolvent g of dense_resolvent,
    and the magnitude Σ_{i'} |G[j, i']| (entry by entry) of what is summed: ((nnz, K, 4, 4), (nnz, K, 4, 4)).  Zero
    where the column site has no colour.  With one site per colour it is G cut to the pattern."""
    rows = cases.block_rows(indptr)
    indices = np.asarray(indices, dtype=np.int64)
    xi = np.asarray(xi, dtype=float)
    total = np.zeros((indices.size, g.shape[0], 4, 4), dtype=np.complex128)
    size = np.zeros((indices.size, g.shape[0], 4, 4))
    for c in range(int(colour.max()) + 1):
        members = np.flatnonzero(colour == c)
        blocks = np.flatnonzero(colour[indices] == c)
        if blocks.size == 0:
            continue
        of_colour = g[:, :, :, members, :]                                  # [e, j, a, i', b]
        summed = np.einsum("ejaib,i->jeab", of_colour, xi[members])
        total[blocks] = summed[rows[blocks]] * xi[indices[blocks]][:, None, None, None]
        size[blocks] = np.abs(of_colour).sum(axis=3).transpose(1, 0, 2, 3)[rows[blocks]]
    return total, size


def readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def pattern(name):
    system = system_of(name)
    return readonly(*cases.pattern_of(system))


@functools.lru_cache(maxsize=None)
def colours(name):
    system = system_of(name)
    colour, count = colours_of(system, SHAPES[name][2])
    return readonly(colour), count


@functools.lru_cache(maxsize=None)
def restated(name, kind, columns=4):
    """restate_sample() of the whole skeleton at Z with the default moments and signs_of(kind)[0]: read-only."""
    system = system_of(name)
    colour, count = colours(name)
    xi = signs_of(kind, system.lattice.size)[0]
    return readonly(restate_sample(system, *pattern(name), colour, count, xi, Z, cases.moments_of(system), columns))


@functools.lru_cache(maxsize=None)
def dense(name):
    return readonly(dense_resolvent(system_of(name), Z))


@functools.lru_cache(maxsize=None)
def probed(name, kind):
    """(probed dense sum, magnitude of what is summed) for the whole skeleton and signs_of(kind)[0]: read-only."""
    system = system_of(name)
    xi = signs_of(kind, system.lattice.size)[0]
    return readonly(*probed_dense(dense(name), *pattern(name), colours(name)[0], xi))


def reference_magnitude(name, kind):
    """max(1, max over blocks of Σ_{i' in colour} |G_ji'|): the size of what the device actually sums."""
    return max(1.0, float(probed(name, kind)[1].max()))


# Distance (cases.distance) of restated(name, kind, C) from probed(name, kind)[0], the larger of C = 2 and 4, as measured
# on the CPU (test_green_probe_host.py prints them): the truncation of the series at the default moments and the
# rounding of the recurrence.  The yardstick of the device tolerance: 20 times the figure.
RESTATEMENT_ERROR = {
    ("dwave_9x8", "plus"): 6.95e-13, ("dwave_9x8", "z2"): 7.51e-13,
    ("dwave_8x6", "plus"): 7.10e-13, ("dwave_8x6", "z2"): 7.57e-13,
    ("peierls_8x6", "plus"): 5.71e-13, ("peierls_8x6", "z2"): 5.80e-13,
    ("cube_6x4x4", "plus"): 7.76e-13, ("cube_6x4x4", "z2"): 8.83e-13,
}
