"""Device-resident Hamiltonian: thin object wrapper over the C ABI handle.

`DeviceSolver` owns one `bdg_system*` (one BSR matrix in the HBM of one GPU).
`Communicator` owns one RCCL rank.  All numerics happen inside the library;
this module only marshals numpy buffers.
"""

from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from . import backend
from .backend import VEC_RADEMACHER, VEC_Z4  # noqa: F401  (re-exported)


def _default_device() -> int:
    device = int(os.environ.get("BODGE_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    return device % backend.device_count()


DENSE_LIBRARY_FROM = 2048  # 4N above which bdg_eigh_dense WITH all eigenvectors goes to rocSOLVER (kJacobiLimit in the library)


def prefetch_dense_library() -> None:
    """Start bringing the rocSOLVER / rocBLAS shared objects into the page cache in the background
    (`bdg_dense_prefetch`; file I/O only).  From cold storage the first dense eigensolve above
    4N = 2048 otherwise waits minutes for them."""
    backend.check(backend.load().bdg_dense_prefetch())


def prefetch_rccl_library() -> None:
    """The same for the RCCL shared object (573 MB) that the first `Communicator` loads."""
    backend.check(backend.load().bdg_rccl_prefetch())


def rccl_library_ready(timeout: float = 0.0) -> bool:
    ready = C.c_int32(0)
    backend.check(backend.load().bdg_rccl_prefetch_wait(float(timeout), C.byref(ready)))
    return bool(ready.value)


def dense_library_ready(timeout: float = 0.0) -> bool:
    """True once the background read started by `prefetch_dense_library` has finished; waits up
    to `timeout` seconds for it."""
    ready = C.c_int32(0)
    backend.check(backend.load().bdg_dense_prefetch_wait(float(timeout), C.byref(ready)))
    return bool(ready.value)


class DeviceSolver:
    def __init__(self, indptr, indices, data, device: int | None = None, n_cols: int | None = None,
                 row_offset: int = 0):
        """Upload a BSR matrix.  `n_cols` / `row_offset` describe a row slab (see `from_slab_plan`)."""
        lib = backend.load()
        backend.require_device()
        if device is None:
            device = _default_device()
        indptr = np.ascontiguousarray(indptr, dtype=np.int32)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.complex128)
        self.n_sites = int(indptr.size - 1)
        self.n_cols = self.n_sites if n_cols is None else int(n_cols)
        self.n_blocks = int(indices.size)
        self.dim = 4 * self.n_sites
        self.device = device
        if data.size != 16 * self.n_blocks:
            raise ValueError("block data does not match the index arrays")
        self._lib = lib
        self._handle = C.c_void_p()
        self._keepalive = None
        backend.check(
            lib.bdg_create_slab(
                device, self.n_sites, self.n_cols, self.n_blocks, backend.as_i32p(indptr),
                backend.as_i32p(indices), backend.as_f64p(data.view(np.float64)), int(row_offset),
                C.byref(self._handle),
            )
        )

    @classmethod
    def from_slab_plan(cls, plan, comm: "Communicator | None" = None, device: int | None = None):
        """One row slab (`bodge_amd.slab.SlabPlan`).  With `comm` the halo exchange uses RCCL
        send/recv between ranks; without it the handle must be put into a `SlabGroup`."""
        solver = cls(plan.indptr, plan.indices, plan.data, device=device, n_cols=plan.n_cols,
                     row_offset=plan.row0)
        n_peers = len(plan.peers)
        peer_rank = np.asarray(plan.peers, dtype=np.int32)
        send_count = np.asarray([rows.size for rows in plan.send_rows], dtype=np.int64)
        send_rows = (np.concatenate(plan.send_rows) if n_peers else np.zeros(0)).astype(np.int64)
        recv_col = np.asarray(plan.recv_offset, dtype=np.int64)
        recv_count = np.asarray(plan.recv_count, dtype=np.int64)
        backend.check(
            solver._lib.bdg_slab_set_exchange(
                solver._handle, comm._handle if comm is not None else None, n_peers,
                backend.as_i32p(peer_rank), backend.as_i64p(send_count), backend.as_i64p(send_rows),
                backend.as_i64p(recv_col), backend.as_i64p(recv_count),
            )
        )
        solver._keepalive = comm
        return solver

    @classmethod
    def from_hamiltonian(cls, system, device: int | None = None, drop_zero_blocks: bool = True):
        # (no read-ahead of the rocSOLVER object any more: from 4N > 512 on eigenvalues and eigenvectors come from
        # the library's own tridiagonalisation route; rocSOLVER is reached only through BODGE_AMD_EIGH)
        indptr, indices, data = system.bsr_arrays(drop_zero_blocks=drop_zero_blocks)
        solver = cls(indptr, indices, data, device=device)
        from .lattice import CubicLattice

        if isinstance(system.lattice, CubicLattice):
            solver.set_lattice_shape(system.lattice.shape)
        return solver

    def set_lattice_shape(self, shape) -> None:
        """Geometry hint (performance only): rows are numbered z + Lz*(y + Ly*x)."""
        lx, ly, lz = (int(v) for v in shape)
        backend.check(self._lib.bdg_set_lattice_shape(self._handle, lx, ly, lz))

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        if getattr(self, "_handle", None) is not None and self._handle:
            self._lib.bdg_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------- kernels
    def spmv(self, x: np.ndarray) -> np.ndarray:
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        x = np.ascontiguousarray(x, dtype=np.complex128).reshape(-1)
        if x.size != self.dim:
            raise ValueError(f"expected a vector of {self.dim} entries")
        y = np.empty_like(x)
        backend.check(
            self._lib.bdg_spmv(self._handle, backend.as_f64p(x.view(np.float64)),
                               backend.as_f64p(y.view(np.float64)))
        )
        return y

    def random_vector(self, seed: int, vec_id: int, kind: int = VEC_RADEMACHER) -> np.ndarray:
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        v = np.empty(self.dim, dtype=np.complex128)
        backend.check(
            self._lib.bdg_random_vector(self._handle, seed, vec_id, kind, backend.as_f64p(v.view(np.float64)))
        )
        return v

    def dots_random(self, scale, n_steps, n_vectors, seed=0, first_id=0, kind=VEC_RADEMACHER):
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        d = np.empty((n_steps, n_vectors))
        e = np.empty((n_steps, n_vectors))
        backend.check(
            self._lib.bdg_cheb_dots_random(
                self._handle, float(scale), n_steps, n_vectors, seed, first_id, kind,
                backend.as_f64p(d), backend.as_f64p(e),
            )
        )
        return d, e

    def dots_unit(self, scale, n_steps, rows):
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        d = np.empty((n_steps, rows.size))
        e = np.empty((n_steps, rows.size))
        backend.check(
            self._lib.bdg_cheb_dots_unit(
                self._handle, float(scale), n_steps, rows.size, backend.as_i64p(rows),
                backend.as_f64p(d), backend.as_f64p(e),
            )
        )
        return d, e

    def moments_random(self, scale, n_moments, n_vectors, seed=0, first_id=0, kind=VEC_RADEMACHER,
                       comm: "Communicator | None" = None) -> np.ndarray:
        """Σ_r <v_r|T_m(H/scale)|v_r> for m < n_moments (summed over ranks if `comm`)."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        mu = np.empty(n_moments)
        backend.check(
            self._lib.bdg_cheb_moments(
                self._handle, comm._handle if comm is not None else None, float(scale), n_moments,
                n_vectors, seed, first_id, kind, backend.as_f64p(mu),
            )
        )
        return mu

    def moments_unit(self, scale, n_moments, rows) -> np.ndarray:
        """(n_moments, len(rows)) array of <e_row|T_m(H/scale)|e_row>."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        mu = np.empty((n_moments, rows.size))
        backend.check(
            self._lib.bdg_cheb_diag_moments(
                self._handle, float(scale), n_moments, rows.size, backend.as_i64p(rows), backend.as_f64p(mu)
            )
        )
        return mu

    def fermi_blocks(self, scale, coef, site_colour, n_colours, n_components, indptr, indices) -> np.ndarray:
        """(nnzb, 4, 4) complex blocks of Σ_k coef[k] T_k(H/scale) on the pattern (indptr, indices) by probing with
        the colouring `site_colour` (bdg_fermi_blocks); n_components = 2 fills the columns 0, 1 only."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        site_colour = np.ascontiguousarray(site_colour, dtype=np.int32)
        indptr = np.ascontiguousarray(indptr, dtype=np.int32)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        if site_colour.shape != (self.n_sites,) or indptr.shape != (self.n_sites + 1,) or indices.size != indptr[-1]:
            raise ValueError("site colours and pattern must describe the handle's block rows")
        out = np.empty((indices.size, 4, 4), dtype=np.complex128)
        backend.check(self._lib.bdg_fermi_blocks(
            self._handle, float(scale), coef.size, backend.as_f64p(coef), int(n_colours), backend.as_i32p(site_colour),
            int(n_components), backend.as_i32p(indptr), backend.as_i32p(indices), backend.as_f64p(out.view(np.float64))))
        return out

    def apply_series(self, scale, coef, x) -> np.ndarray:
        """(V, F, 4N) complex y[v, f] = Σ_k coef[k, f] T_k(H/scale) x[v] for coefficients (M, F) and vectors (V, 4N),
        both complex, by Clenshaw's recurrence with a stored source on the device (bdg_apply_series)."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        coef = np.ascontiguousarray(coef, dtype=np.complex128)
        x = np.ascontiguousarray(x, dtype=np.complex128)
        if coef.ndim != 2 or coef.shape[0] < 1 or coef.shape[1] < 1:
            raise ValueError("apply_series: expected coefficients of shape (moments, functions)")
        if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] != self.dim:
            raise ValueError(f"apply_series: expected vectors of shape (count, {self.dim})")
        out = np.empty((x.shape[0], coef.shape[1], self.dim), dtype=np.complex128)
        backend.check(self._lib.bdg_apply_series(
            self._handle, float(scale), coef.shape[0], coef.shape[1], backend.as_f64p(coef.view(np.float64)),
            x.shape[0], backend.as_f64p(x.view(np.float64)), backend.as_f64p(out.view(np.float64))))
        return out

    def moment_matrix(self, scale, n_moments, a, b, rows=None, x=None) -> np.ndarray:
        """(M, M) complex μ[n, m] = Σ_v <v|T_n(H/scale) A T_m(H/scale) B|v> (bdg_moment_matrix).  `a`, `b`: BSR triples
        (indptr, indices, data (nnzb, 4, 4)) on this handle's block rows; the start vectors are the unit vectors of the
        scalar rows `rows`, or the rows of `x` (V, 4N) - exactly one of the two."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        if (rows is None) == (x is None):
            raise ValueError("moment_matrix: give exactly one of rows and x")
        if int(n_moments) < 1:
            raise ValueError("moment_matrix: expected at least one moment")
        keep, operators = [], []
        for name, (indptr, indices, data) in (("A", a), ("B", b)):
            indptr = np.ascontiguousarray(indptr, dtype=np.int32)
            indices = np.ascontiguousarray(indices, dtype=np.int32)
            data = np.ascontiguousarray(data, dtype=np.complex128)
            if indptr.shape != (self.n_sites + 1,) or data.shape != (indices.size, 4, 4):
                raise ValueError(f"moment_matrix: operator {name} does not describe the handle's {self.n_sites} block rows")
            keep.append((indptr, indices, data))
            operators.append(backend.Operator(indices.size, backend.as_i32p(indptr), backend.as_i32p(indices),
                                              backend.as_f64p(data.view(np.float64))))
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
            count, rows_p, x_p = rows.size, backend.as_i64p(rows), None
        else:
            x = np.ascontiguousarray(x, dtype=np.complex128)
            if x.ndim != 2 or x.shape[1] != self.dim:
                raise ValueError(f"moment_matrix: expected vectors of shape (count, {self.dim})")
            count, rows_p, x_p = x.shape[0], None, backend.as_f64p(x.view(np.float64))
        if count < 1:
            raise ValueError("moment_matrix: expected at least one start vector")
        mu = np.empty((int(n_moments), int(n_moments)), dtype=np.complex128)
        backend.check(self._lib.bdg_moment_matrix(
            self._handle, float(scale), int(n_moments), C.byref(operators[0]), C.byref(operators[1]), count, rows_p, x_p,
            backend.as_f64p(mu.view(np.float64))))
        return mu

    def response_map(self, scale, source_rows, a, coef, block_rows) -> np.ndarray:
        """(kernels, sites, 4, 4) complex blocks K_{q,j}[γ, δ] = Σ_nm c_q[n, m] Σ_αβ A[α, β] conj(X_m[(j, γ), β])
        X_n[(j, δ), α] with X_n = T_n(H/scale) on the unit columns of the S <= 32 distinct scalar rows `source_rows`
        (bdg_response_map): `a` (S, S) complex between those rows, `coef` (kernels, M, M) or (M, M) complex,
        `block_rows` the distinct target sites."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        source_rows = np.ascontiguousarray(source_rows, dtype=np.int64).reshape(-1)
        block_rows = np.ascontiguousarray(block_rows, dtype=np.int32).reshape(-1)
        a = np.ascontiguousarray(a, dtype=np.complex128)
        coef = np.ascontiguousarray(coef, dtype=np.complex128)
        if coef.ndim == 2:
            coef = coef[None]
        if coef.ndim != 3 or coef.shape[0] < 1 or coef.shape[1] < 1 or coef.shape[1] != coef.shape[2]:
            raise ValueError("response_map: expected coefficients of shape (kernels, moments, moments)")
        if source_rows.size < 1 or a.shape != (source_rows.size, source_rows.size):
            raise ValueError("response_map: expected at least one source row and A of shape (rows, rows)")
        if block_rows.size < 1:
            raise ValueError("response_map: expected at least one target block row")
        out = np.empty((coef.shape[0], block_rows.size, 4, 4), dtype=np.complex128)
        backend.check(self._lib.bdg_response_map(
            self._handle, float(scale), coef.shape[1], source_rows.size, backend.as_i64p(source_rows),
            backend.as_f64p(a.view(np.float64)), coef.shape[0], backend.as_f64p(coef.view(np.float64)), block_rows.size,
            backend.as_i32p(block_rows), backend.as_f64p(out.view(np.float64))))
        return out

    def green_moments(self, scale, n_moments, source_rows, target_block_rows) -> np.ndarray:
        """(n_moments, n_targets, 4, n_sources) complex moments <e_{4j+a}|T_n(H/scale)|e_row> for the scalar rows
        `source_rows` and the distinct block rows j of `target_block_rows` (bdg_green_moments)."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        source_rows = np.ascontiguousarray(source_rows, dtype=np.int64).reshape(-1)
        target_block_rows = np.ascontiguousarray(target_block_rows, dtype=np.int32).reshape(-1)
        if int(n_moments) < 1 or source_rows.size < 1 or target_block_rows.size < 1:
            raise ValueError("green_moments: expected at least one moment, one source row and one target block row")
        out = np.empty((int(n_moments), target_block_rows.size, 4, source_rows.size), dtype=np.complex128)
        backend.check(self._lib.bdg_green_moments(
            self._handle, float(scale), int(n_moments), source_rows.size, backend.as_i64p(source_rows),
            target_block_rows.size, backend.as_i32p(target_block_rows), backend.as_f64p(out.view(np.float64))))
        return out

    def green_local_moments(self, scale, n_moments, block_rows, n_components: int = 4) -> np.ndarray:
        """(n_moments, n_sites, 4, n_components) complex moments <e_{4j+a}|T_n(H/scale)|e_{4j+b}> on the distinct
        block rows j of `block_rows`, many sites per batch (bdg_green_local_moments)."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        block_rows = np.ascontiguousarray(block_rows, dtype=np.int32).reshape(-1)
        if int(n_moments) < 1 or block_rows.size < 1 or int(n_components) not in (2, 4):
            raise ValueError("green_local_moments: expected at least one moment, one block row and 2 or 4 components")
        out = np.empty((int(n_moments), block_rows.size, 4, int(n_components)), dtype=np.complex128)
        backend.check(self._lib.bdg_green_local_moments(
            self._handle, float(scale), int(n_moments), block_rows.size, backend.as_i32p(block_rows),
            int(n_components), backend.as_f64p(out.view(np.float64))))
        return out

    def green_bond_blocks(self, scale, weights, indptr, indices, n_components: int = 4) -> np.ndarray:
        """(n_weights, nnz, 4, 4) complex Σ_n weights[e, n] <e_{4j+a}|T_n(H/scale)|e_{4i+b}> on the blocks k = (j, i) of
        the BSR pattern (`indptr`, `indices`), every column site a source; the moments are contracted on the device
        (bdg_green_bond_blocks).  `weights` (n_weights, n_moments) complex; n_components = 2 derives the hole columns
        from the electron columns (particle-hole symmetric matrices only)."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        weights = np.ascontiguousarray(weights, dtype=np.complex128)
        indptr = np.ascontiguousarray(indptr, dtype=np.int32).reshape(-1)
        indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        if weights.ndim != 2 or weights.shape[0] < 1 or weights.shape[1] < 1:
            raise ValueError("green_bond_blocks: expected weights of shape (energies, moments)")
        if indptr.shape != (self.n_sites + 1,) or indices.size < 1 or int(indptr[-1]) != indices.size:
            raise ValueError(f"green_bond_blocks: the pattern does not describe the handle's {self.n_sites} block rows")
        if int(n_components) not in (2, 4):
            raise ValueError("green_bond_blocks: expected 2 or 4 components")
        out = np.empty((weights.shape[0], indices.size, 4, 4), dtype=np.complex128)
        backend.check(self._lib.bdg_green_bond_blocks(
            self._handle, float(scale), weights.shape[1], weights.shape[0], backend.as_f64p(weights.view(np.float64)),
            backend.as_i32p(indptr), backend.as_i32p(indices), int(n_components), backend.as_f64p(out.view(np.float64))))
        return out

    def green_probe_blocks(self, scale, weights, colours, n_colours: int, indptr, indices, n_components: int = 4,
                           signs=None, want_stderr: bool | None = None):
        """(mean, stderr) of the probed blocks on the BSR pattern (`indptr`, `indices`), each (n_weights, nnz, 4, 4)
        complex: one start vector per colour and Nambu column, `colours` (n_sites,) int32 below `n_colours` (negative:
        no source), `signs` (samples, n_sites) of ±1 or None for one sample of all +1 (bdg_green_probe_blocks).  stderr
        is None unless asked for (default: with two samples or more)."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        weights = np.ascontiguousarray(weights, dtype=np.complex128)
        colours = np.ascontiguousarray(colours, dtype=np.int32).reshape(-1)
        indptr = np.ascontiguousarray(indptr, dtype=np.int32).reshape(-1)
        indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        if weights.ndim != 2 or weights.shape[0] < 1 or weights.shape[1] < 1:
            raise ValueError("green_probe_blocks: expected weights of shape (energies, moments)")
        if indptr.shape != (self.n_sites + 1,) or indices.size < 1 or int(indptr[-1]) != indices.size:
            raise ValueError(f"green_probe_blocks: the pattern does not describe the handle's {self.n_sites} block rows")
        if colours.shape != (self.n_sites,):
            raise ValueError(f"green_probe_blocks: expected one colour for each of the {self.n_sites} sites")
        if int(n_components) not in (2, 4):
            raise ValueError("green_probe_blocks: expected 2 or 4 components")
        samples = 1
        if signs is not None:
            signs = np.ascontiguousarray(signs)
            if signs.ndim != 2 or signs.shape[0] < 1 or signs.shape[1] != self.n_sites:
                raise ValueError(f"green_probe_blocks: expected signs of shape (samples, {self.n_sites})")
            if not np.all(np.abs(signs) == 1):
                raise ValueError("green_probe_blocks: the signs must be +1 or -1")
            signs = np.ascontiguousarray(signs, dtype=np.int8)
            samples = signs.shape[0]
        if want_stderr is None:
            want_stderr = samples > 1
        mean = np.empty((weights.shape[0], indices.size, 4, 4), dtype=np.complex128)
        stderr = np.empty_like(mean) if want_stderr else None
        backend.check(self._lib.bdg_green_probe_blocks(
            self._handle, float(scale), weights.shape[1], weights.shape[0], backend.as_f64p(weights.view(np.float64)),
            int(n_colours), backend.as_i32p(colours), samples, None if signs is None else backend.as_i8p(signs),
            backend.as_i32p(indptr), backend.as_i32p(indices), int(n_components), backend.as_f64p(mean.view(np.float64)),
            None if stderr is None else backend.as_f64p(stderr.view(np.float64))))
        return mean, stderr

    def green_state_moments(self, scale, n_moments, amplitudes, n_components: int = 4) -> np.ndarray:
        """(n_moments, n_states, 4, n_components) complex moments <w_q a|T_n(H/scale)|w_q b> of the states
        `amplitudes` (n_states, n_sites): one complex amplitude per site, the same on every Nambu component
        (bdg_green_state_moments)."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        amplitudes = np.ascontiguousarray(amplitudes, dtype=np.complex128)
        if amplitudes.ndim != 2 or amplitudes.shape[0] < 1 or amplitudes.shape[1] != self.n_sites:
            raise ValueError(f"green_state_moments: expected amplitudes of shape (states, {self.n_sites})")
        if int(n_moments) < 1 or int(n_components) not in (2, 4):
            raise ValueError("green_state_moments: expected at least one moment and 2 or 4 components")
        out = np.empty((int(n_moments), amplitudes.shape[0], 4, int(n_components)), dtype=np.complex128)
        backend.check(self._lib.bdg_green_state_moments(
            self._handle, float(scale), int(n_moments), amplitudes.shape[0], backend.as_f64p(amplitudes.view(np.float64)),
            int(n_components), backend.as_f64p(out.view(np.float64))))
        return out

    def lanczos_begin(self, n_vectors: int, seed: int = 0, first_id: int = 0, kind: int = VEC_RADEMACHER,
                      max_iter: int = 10000) -> None:
        """Start n_vectors independent Lanczos processes on H^2 (see `lanczos_advance`)."""
        backend.check(self._lib.bdg_lanczos_begin(self._handle, n_vectors, seed, first_id, kind, max_iter))
        self._lanczos_vectors = n_vectors

    def lanczos_advance(self, n_iter: int):
        """Run n_iter more iterations; returns (alpha, beta) of shape (n_iter, n_vectors): diagonal and
        off-diagonal (beta_{j+1}) of the tridiagonal representation of H^2."""
        # (`_lanczos_vectors` sizes the output; the tests set it by hand after a run has ended to reach the library's
        # own refusal - keep the name, or change tests/test_gpu_parity.py and tests/test_gpu_lanczos.py with it)
        if not getattr(self, "_lanczos_vectors", 0):
            raise ValueError("bodge_hip: lanczos_begin has not been called on this handle")
        alpha = np.empty((n_iter, self._lanczos_vectors))
        beta = np.empty((n_iter, self._lanczos_vectors))
        backend.check(self._lib.bdg_lanczos_advance(self._handle, n_iter, backend.as_f64p(alpha), backend.as_f64p(beta)))
        return alpha, beta

    def lanczos_ritz_vectors(self, coef: np.ndarray) -> np.ndarray:
        """Second pass of a freshly begun Lanczos process: `coef[j, l, r]` are the coordinates of
        level l's Ritz vector of start vector r in the Lanczos basis; returns y[l, r, :] (4N complex)."""
        n_vectors = getattr(self, "_lanczos_vectors", 0)
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if not n_vectors or coef.ndim != 3 or coef.shape[2] != n_vectors:
            raise ValueError("bodge_hip: coefficients must be (iterations, levels, start vectors of lanczos_begin)")
        out = np.empty((coef.shape[1], n_vectors, self.dim), dtype=np.complex128)
        backend.check(self._lib.bdg_lanczos_ritz_vectors(self._handle, coef.shape[0], coef.shape[1], backend.as_f64p(coef),
                                                        backend.as_f64p(out.view(np.float64))))
        return out

    def lanczos_ritz_pairs(self, coef: np.ndarray, eps: np.ndarray, k: int, rank_tol: float = 1e-4):
        """Second pass + Rayleigh-Ritz on the device: the k lowest states found in the levels whose Ritz
        coordinates `coef[j, l, r]` and eigenvalue estimates `eps[l]` are given.  Returns
        (values (k',), vectors (k', 4N), n_found) with k' = min(k, n_found); only these cross PCIe."""
        n_vectors = getattr(self, "_lanczos_vectors", 0)
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        eps = np.ascontiguousarray(eps, dtype=np.float64)
        if not n_vectors or coef.ndim != 3 or coef.shape[2] != n_vectors or eps.shape != (coef.shape[1],):
            raise ValueError("bodge_hip: coefficients must be (iterations, levels, start vectors of lanczos_begin), eps (levels,)")
        values = np.empty(k)
        vectors = np.empty((k, self.dim), dtype=np.complex128)
        found = C.c_int32(0)
        backend.check(self._lib.bdg_lanczos_ritz_pairs(
            self._handle, coef.shape[0], coef.shape[1], backend.as_f64p(coef), backend.as_f64p(eps), float(rank_tol), k,
            C.byref(found), backend.as_f64p(values), backend.as_f64p(vectors.view(np.float64))))
        self._lanczos_vectors = 0  # (the library ended the run)
        kept = min(k, found.value)
        return values[:kept], vectors[:kept], found.value

    # ------------------------------------------------------------------ subspace block
    def subspace_begin(self, n_columns: int, seed: int = 0, first_id: int = 0) -> None:
        """Allocate a device-resident block of `n_columns` vectors (X, HX and a rotation target) and fill X with the
        Rademacher start vectors (seed, first_id + c) (bdg_subspace_begin).  A dense solve or a Lanczos run on the
        handle ends the block."""
        self._lanczos_vectors = 0  # (the library ends a Lanczos run: the block wants the memory)
        self._subspace_columns = 0
        backend.check(self._lib.bdg_subspace_begin(self._handle, int(n_columns), int(seed), int(first_id)))
        self._subspace_columns = int(n_columns)

    def subspace_end(self) -> None:
        self._subspace_columns = 0
        backend.check(self._lib.bdg_subspace_end(self._handle))

    def _subspace_width(self, name: str) -> int:
        # (`_subspace_columns` sizes the outputs.  A dense solve or a Lanczos run ends the block inside the library
        # and does not reset it here: the library's own refusal, with its message, is what the caller then gets)
        width = getattr(self, "_subspace_columns", 0)
        if not width:
            raise ValueError(f"bodge_hip: {name}: subspace_begin has not been called on this handle")
        return width

    def subspace_filter(self, scale, coef) -> None:
        """X <- Σ_k coef[k] T_k(H/scale) X for real coefficients (bdg_subspace_filter)."""
        self._subspace_width("subspace_filter")
        self._lanczos_vectors = 0
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.ndim != 1 or coef.size < 1:
            raise ValueError("subspace_filter: expected real coefficients of shape (moments,)")
        backend.check(self._lib.bdg_subspace_filter(self._handle, float(scale), coef.size, backend.as_f64p(coef)))

    def subspace_project(self):
        """HX <- H X; returns (S, G) = (X†X, X†HX), each (B, B) complex (bdg_subspace_project)."""
        width = self._subspace_width("subspace_project")
        self._lanczos_vectors = 0
        s = np.empty((width, width), dtype=np.complex128)
        g = np.empty((width, width), dtype=np.complex128)
        backend.check(self._lib.bdg_subspace_project(self._handle, backend.as_f64p(s.view(np.float64)),
                                                     backend.as_f64p(g.view(np.float64))))
        return s, g

    def subspace_rotate(self, q, theta) -> np.ndarray:
        """X <- X Q, HX <- HX Q for Q (B, r) complex; returns the r residual norms ‖HX_j − θ_j X_j‖
        (bdg_subspace_rotate).  Columns from r on are dead afterwards."""
        width = self._subspace_width("subspace_rotate")
        q = np.ascontiguousarray(q, dtype=np.complex128)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if q.ndim != 2 or q.shape[0] != width or not 1 <= q.shape[1] <= width or theta.shape != (q.shape[1],):
            raise ValueError(f"subspace_rotate: expected Q of shape ({width}, r <= {width}) and theta of shape (r,)")
        residual = np.empty(q.shape[1])
        backend.check(self._lib.bdg_subspace_rotate(self._handle, q.shape[1], backend.as_f64p(q.view(np.float64)),
                                                    backend.as_f64p(theta), backend.as_f64p(residual)))
        return residual

    def subspace_refill(self, first_column: int, count: int, seed: int = 0, first_id: int = 0) -> None:
        """X[first_column + c] <- start vector (seed, first_id + c) for c < count (bdg_subspace_refill)."""
        self._subspace_width("subspace_refill")
        backend.check(self._lib.bdg_subspace_refill(self._handle, int(first_column), int(count), int(seed), int(first_id)))

    def subspace_read(self, first_column: int, count: int) -> np.ndarray:
        """(count, 4N) complex: the columns of X from `first_column` on, one per row (bdg_subspace_read)."""
        width = self._subspace_width("subspace_read")
        if first_column < 0 or count < 1 or first_column + count > width:
            raise ValueError(f"subspace_read: columns [{first_column}, {first_column + count}) are not within the block's {width}")
        out = np.empty((int(count), self.dim), dtype=np.complex128)
        backend.check(self._lib.bdg_subspace_read(self._handle, int(first_column), int(count), backend.as_f64p(out.view(np.float64))))
        return out

    def subspace_write(self, first_column: int, x) -> None:
        """X[first_column + c] <- x[c] for the rows of x (count, 4N) (bdg_subspace_write)."""
        width = self._subspace_width("subspace_write")
        x = np.ascontiguousarray(x, dtype=np.complex128)
        if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] != self.dim or first_column < 0 or first_column + x.shape[0] > width:
            raise ValueError(f"subspace_write: expected (count, {self.dim}) vectors within the block's {width} columns")
        backend.check(self._lib.bdg_subspace_write(self._handle, int(first_column), x.shape[0], backend.as_f64p(x.view(np.float64))))

    def eigh(self, vectors: bool = True):
        """All eigenvalues ascending (and ALL eigenvectors as columns).  Eigenvalues alone: the library's own kernels
        at every size (Jacobi up to 4N = 512, tridiagonalisation + bisection above, through a band from 5000 rows for
        real matrices).  With vectors: own Jacobi kernels up to 4N = 2048, rocSOLVER above (dsyevd when imag(H) = 0,
        else zheevd) - `eigh_above` is the route `diagonalize()` takes and needs no library."""
        self._lanczos_vectors = 0  # any other use of the handle ends a Lanczos run (library: lanczos_free)
        w = np.empty(self.dim)
        if not vectors:
            backend.check(self._lib.bdg_eigh_dense(self._handle, backend.as_f64p(w), None))
            return w, None
        z = np.empty((self.dim, self.dim), dtype=np.complex128)  # column-major on return
        backend.check(
            self._lib.bdg_eigh_dense(self._handle, backend.as_f64p(w), backend.as_f64p(z.view(np.float64)))
        )
        return w, z.T

    def eigh_above(self, lower_bound: float = 0.0):
        """All eigenvalues ascending, and the eigenvectors (as columns) of those above `lower_bound` - what
        `diagonalize()` keeps.  From 4N > 512 on the library's own tridiagonalisation route (no rocSOLVER)."""
        self._lanczos_vectors = 0
        w = np.empty(self.dim)
        count = C.c_int64(0)
        capacity = self.dim // 2 + 8
        for _ in range(2):
            z = np.empty((capacity, self.dim), dtype=np.complex128)
            status = self._lib.bdg_eigh_dense_above(self._handle, float(lower_bound), capacity, backend.as_f64p(w),
                                                    C.byref(count), backend.as_f64p(z.view(np.float64)))
            if status == 0 or count.value <= capacity:
                break
            capacity = count.value  # (an asymmetric spectrum: more than half of the eigenvalues above the bound)
        backend.check(status)
        return w, z[: count.value].T

    def hermiticity_defect(self) -> float:
        """max |H - H^†| over the stored entries of the uploaded matrix (device-side twin of the
        check at reference hamiltonian.py:121-122)."""
        out = np.zeros(1)
        backend.check(self._lib.bdg_hermiticity_defect(self._handle, backend.as_f64p(out)))
        return float(out[0])

    def set_lanes_per_row(self, lanes: int) -> None:
        backend.check(self._lib.bdg_set_lanes_per_row(self._handle, lanes))

    def perf(self) -> dict:
        rec = backend.Perf()
        backend.check(self._lib.bdg_perf_query(self._handle, C.byref(rec)))
        return {name: getattr(rec, name) for name, _ in backend.Perf._fields_}


# ---------------------------------------------------------------------------
class SlabGroup:
    """Several row slabs of one matrix driven in lock step by this process.

    The slabs may sit on one GPU (how the slab path is validated on a single-GPU box) or on
    several GPUs of the node (`devices`); halo rows move by device-to-device copies.
    """

    def __init__(self, indptr, indices, data, n_slabs: int, granule: int = 1, devices=None, lattice_shape=None):
        from . import slab

        n_rows = len(indptr) - 1
        self.bounds = slab.partition_rows(n_rows, n_slabs, granule)
        self.plans = [slab.build_plan(indptr, indices, data, self.bounds, r) for r in range(n_slabs)]
        devices = [None] * n_slabs if devices is None else list(devices)
        self.members = [DeviceSolver.from_slab_plan(p, device=d) for p, d in zip(self.plans, devices)]
        if lattice_shape is not None and granule == lattice_shape[1] * lattice_shape[2]:
            # geometry hint per slab (a stack of whole x-planes): lets a 3-D slab run the stencil kernel that
            # reads its neighbours' boundary planes in place instead of exchanging halo rows
            for member, plan in zip(self.members, self.plans):
                member.set_lattice_shape((plan.n_own // granule, lattice_shape[1], lattice_shape[2]))
        self._lib = backend.load()
        self._handle = C.c_void_p()
        handles = (C.c_void_p * n_slabs)(*[m._handle for m in self.members])
        backend.check(self._lib.bdg_group_create(handles, n_slabs, C.byref(self._handle)))
        self.dim = 4 * n_rows

    @classmethod
    def from_hamiltonian(cls, system, n_slabs: int, devices=None):
        from . import slab

        indptr, indices, data = system.bsr_arrays()
        shape = getattr(system.lattice, "shape", None)
        return cls(indptr, indices, data, n_slabs, slab.lattice_granule(system.lattice), devices,
                   lattice_shape=tuple(shape) if shape is not None and len(shape) == 3 else None)

    def dots_random(self, scale, n_steps, n_vectors, seed=0, first_id=0, kind=VEC_RADEMACHER):
        d = np.empty((n_steps, n_vectors))
        e = np.empty((n_steps, n_vectors))
        backend.check(
            self._lib.bdg_group_dots_random(
                self._handle, float(scale), n_steps, n_vectors, seed, first_id, kind,
                backend.as_f64p(d), backend.as_f64p(e),
            )
        )
        return d, e

    def dots_unit(self, scale, n_steps, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        d = np.empty((n_steps, rows.size))
        e = np.empty((n_steps, rows.size))
        backend.check(
            self._lib.bdg_group_dots_unit(
                self._handle, float(scale), n_steps, rows.size, backend.as_i64p(rows),
                backend.as_f64p(d), backend.as_f64p(e),
            )
        )
        return d, e

    def close(self) -> None:
        if getattr(self, "_handle", None) is not None and self._handle:
            self._lib.bdg_group_destroy(self._handle)
            self._handle = C.c_void_p()
            for member in self.members:
                member.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _StdoutToStderr:
    """RCCL prints a version banner on stdout at communicator creation; programs that emit
    machine-readable stdout (bench.py's single JSON line) must not see it."""

    def __enter__(self):
        import sys

        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        os.dup2(self._saved, 1)
        os.close(self._saved)


class Communicator:
    """One RCCL rank.  The 128-byte unique id travels through `bodge_amd.rendezvous` (TCP)."""

    def __init__(self, rank: int, n_ranks: int, device: int, unique_id: bytes):
        lib = backend.load()
        self._lib = lib
        self.rank, self.n_ranks, self.device = rank, n_ranks, device
        self._handle = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        with _StdoutToStderr():
            backend.check(lib.bdg_comm_init(device, buf, n_ranks, rank, C.byref(self._handle)))

    @staticmethod
    def new_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        with _StdoutToStderr():
            backend.check(backend.load().bdg_comm_unique_id(buf))
        return bytes(buf)

    _sequence = 0  # communicators created by this process through `from_environment`

    @classmethod
    def from_environment(cls, timeout: float = 300.0) -> "Communicator | None":
        """Build the communicator of a `torch.distributed.run`-style launch.

        Uses RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT.  Rank 0 publishes the
        RCCL unique id through the launch's TCP rendezvous (`bodge_amd.rendezvous`: no files, a
        per-launch nonce on every message); the others block on it.  Returns None for a
        single-process run.
        """
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if world <= 1 and os.environ.get("BODGE_AMD_FORCE_COMM") != "1":
            return None  # (the override builds a one-rank communicator: exercises the RCCL path on one GPU)
        rank = int(os.environ.get("RANK", "0"))
        local = int(os.environ.get("LOCAL_RANK", rank))
        # The RCCL object is 573 MB; from cold storage its first read takes minutes.  Every rank
        # streams it into the page cache (shared: one read serves all) BEFORE the id exchange, so
        # that the exchange's timeout covers the exchange and not rank 0's library load.
        prefetch_rccl_library()
        waited = 0
        while not rccl_library_ready(30.0):
            waited += 30
            if rank == 0:
                print(f"[bodge_amd] reading the RCCL library from cold storage ... {waited} s", file=sys.stderr, flush=True)
            if waited >= 1800:
                raise RuntimeError("the RCCL shared object could not be read within 30 minutes")
        if world <= 1:
            uid = cls.new_unique_id()
        else:
            from .rendezvous import store_from_environment

            store = store_from_environment(timeout)
            key = f"rccl_unique_id/{cls._sequence}"
            cls._sequence += 1
            if rank == 0:
                uid = cls.new_unique_id()
                store.set(key, uid)
            else:
                uid = store.get(key, timeout)
            if len(uid) != 128:
                raise RuntimeError(f"rank {rank}: rendezvous returned {len(uid)} bytes instead of an RCCL id")
        # one process per GPU; more ranks than GPUs wrap around.  RCCL refuses two ranks on one device ("invalid usage"),
        # but only after its bootstrap and topology search - tens of seconds per rank: the ranks compare (host, device)
        # over the rendezvous store first and give the same answer at once
        count = backend.device_count()
        device = local % count if count > 0 else local
        if world > 1:
            import socket

            places = [blob.decode() for blob in store.gather(f"{socket.gethostname()}/{device}".encode())]
            clash = sorted({place for place in places if places.count(place) > 1})
            if clash:
                raise RuntimeError(f"rank {rank}: {world} ranks but some share a GPU ({', '.join(clash)}): RCCL refuses duplicate devices")
        comm = cls(rank, world, device, uid)
        comm.barrier()
        return comm

    def info(self) -> dict:
        """{'n_ranks': ncclCommCount, 'rank', 'device', 'pci_bus_id'} as the library and RCCL report them."""
        n_ranks, rank, device = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        bus = C.create_string_buffer(32)
        backend.check(self._lib.bdg_comm_info(self._handle, C.byref(n_ranks), C.byref(rank), C.byref(device), bus))
        return {"n_ranks": n_ranks.value, "rank": rank.value, "device": device.value,
                "pci_bus_id": bus.value.decode("ascii", "replace")}

    def allreduce_sum(self, values: np.ndarray) -> np.ndarray:
        out = np.ascontiguousarray(values, dtype=np.float64).copy()
        backend.check(self._lib.bdg_comm_allreduce_sum(self._handle, backend.as_f64p(out), out.size))
        return out

    def allreduce_max(self, values: np.ndarray) -> np.ndarray:
        out = np.ascontiguousarray(values, dtype=np.float64).copy()
        backend.check(self._lib.bdg_comm_allreduce_max(self._handle, backend.as_f64p(out), out.size))
        return out

    def barrier(self) -> None:
        self.allreduce_sum(np.zeros(1))

    def close(self) -> None:
        if getattr(self, "_handle", None) is not None and self._handle:
            self._lib.bdg_comm_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
