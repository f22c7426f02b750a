"""Host arithmetic of the composed three-step sweep (csrc/composed.hpp through bdg_host_composed_dots): no GPU.

A composed run steps by T_3: sweep k starts from u = t_{3k} and makes w_1 = H~u, w_2 = 2H~w_1 - u, w_3 = 2H~w_2 - w_1,
then u_{k+1} = 2 w_3 - u_{k-1} (u_1 = w_3).  Its six dot products per sweep are not d_n, e_n; the exported function turns
them back.  Here the sweeps are restated with scipy on the oracle's start block, their dots are fed to the function, and
d_n, e_n must agree with the plain recurrence of `cheb_ref.recurrence_dots` to the project's 1e-12 * 4N - with d_{3k}
handed through bit for bit."""

import numpy as np
import pytest

from oracle import cheb_ref

STEPS = [1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 255]
N_VECTORS = 3


def _system(api, kind):
    lattice = api.CubicLattice((12, 13, 1))
    system = api.Hamiltonian(lattice)
    with system as (H, Δ):
        H.set_sites(3.0 * api.σ0 - 0.05 * api.σ3)
        Δ.set_sites(-0.1 * api.jσ2)
        if kind == "swave":
            H.set_bonds(-1.0 * api.σ0)
        else:  # Peierls phases on the x bonds: a genuinely complex matrix
            pairs = lattice.bond_array(axis=0, coords=True)
            phase = np.where(pairs[:, 1, 0] > pairs[:, 0, 0], np.exp(0.3j), np.exp(-0.3j))
            H.set_bonds(-phase[:, None, None] * api.σ0, axis=0)
            H.set_bonds(-1.0 * api.σ0, axis=1)
    return system


def _composed_raw(bsr, scale, steps, start):
    """Rows n = 3k + j of a composed run's dot table: (<w_j|w_j>, Re <w_{j+1}|w_j>) per vector, interleaved."""
    dots = cheb_ref._column_dots
    raw = np.zeros((steps, 2 * start.shape[1]))
    u, u_before = np.array(start, dtype=np.complex128), None
    for c in range(0, steps, 3):
        w = [u, (bsr @ u) / scale]
        w.append((bsr @ w[1]) * (2.0 / scale) - w[0])
        w.append((bsr @ w[2]) * (2.0 / scale) - w[1])
        for j in range(min(3, steps - c)):
            raw[c + j, 0::2] = dots(w[j], w[j])
            raw[c + j, 1::2] = dots(w[j + 1], w[j])
        u, u_before = (w[3] if u_before is None else 2.0 * w[3] - u_before), u
    return raw


@pytest.fixture(scope="module", params=["swave", "peierls"])
def case(request, api):
    """One model: matrix, scale, start block, the plain recurrence at the longest run, composed tables per run length."""
    bsr = _system(api, request.param).matrix("bsr")
    scale = cheb_ref.spectral_bound(bsr)
    kind = cheb_ref.VEC_Z4 if request.param == "peierls" else cheb_ref.VEC_RADEMACHER
    start = cheb_ref.random_block(bsr.shape[0], 3, range(N_VECTORS), kind)
    d, e = cheb_ref.recurrence_dots(bsr, scale, 2 * max(STEPS), start)
    raw = _composed_raw(bsr, scale, max(STEPS), start)
    return bsr.shape[0], d, e, raw


def _turn_back(hip_library, raw, steps, pad=0):
    from bodge_amd import backend

    table = np.full((steps, raw.shape[1] + pad), np.nan)  # (a row stride wider than the vectors, as the device table has)
    table[:, : raw.shape[1]] = raw[:steps]
    d = np.full((steps, N_VECTORS + 1), np.nan)
    e = np.full((steps, N_VECTORS + 1), np.nan)
    backend.check(hip_library.bdg_host_composed_dots(steps, N_VECTORS, backend.as_f64p(table), table.shape[1],
                                                     backend.as_f64p(d), backend.as_f64p(e), N_VECTORS + 1))
    assert np.isnan(d[:, N_VECTORS]).all() and np.isnan(e[:, N_VECTORS]).all()  # nothing written beyond the vectors
    return d[:, :N_VECTORS], e[:, :N_VECTORS]


@pytest.mark.parametrize("steps", STEPS)
def test_composed_dots_give_the_plain_recurrence(hip_library, case, steps):
    n, d_ref, e_ref, raw = case
    d, e = _turn_back(hip_library, raw, steps, pad=2)
    err_d, err_e = np.abs(d - d_ref[:steps]).max(), np.abs(e - e_ref[:steps]).max()
    print(f"steps {steps}: max |d - d_ref| = {err_d / n:.2e} * 4N, max |e - e_ref| = {err_e / n:.2e} * 4N")
    assert err_d <= 1e-12 * n and err_e <= 1e-12 * n
    assert np.array_equal(d[0::3], raw[:steps:3, 0::2])  # d_{3k} is the sweep's own <u|u>, bit for bit
    assert np.array_equal(d[0], np.full(N_VECTORS, float(n)))  # d_0 = 4N exactly (entries of modulus 1)


def test_composed_dots_reject_bad_arguments(hip_library):
    from bodge_amd import backend

    buf = np.zeros(8)
    p = backend.as_f64p(buf)
    assert hip_library.bdg_host_composed_dots(0, 1, p, 2, p, p, 1) == -1
    assert hip_library.bdg_host_composed_dots(1, 2, p, 3, p, p, 2) == -1  # row stride below 2 * vectors
    assert hip_library.bdg_host_composed_dots(1, 2, p, 4, p, p, 1) == -1  # ld below the vectors
    assert hip_library.bdg_host_composed_dots(1, 1, None, 2, p, p, 1) == -1
