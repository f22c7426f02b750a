"""What tests/test_gpu_family_tiles.py rests on, without a GPU: the two Green recurrences restated in numpy
(family_tile_cases.picked_moments, local_moments) against the Chebyshev polynomials of the dense eigenpairs, and the tile
arithmetic that makes a workgroup of the Clenshaw-family kernels walk several tiles on the 67 x 63 lattice."""

import numpy as np
import pytest

import bodge_amd as ba

import apply_cases
import family_tile_cases as cases

MODELS = {
    "uniform": lambda: apply_cases.uniform_swave((9, 8, 1)),
    "disordered": lambda: apply_cases.disordered_swave((9, 8, 1), onsite=ba.σ2),
}


# ------------------------------------------------------------------ 8. the restatements against dense eigh
@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("matrix", ["sparse", "dense"])
def test_green_restatements_match_the_chebyshev_polynomials_of_the_dense_eigenpairs(name, matrix):
    """μ_n = V cos(n arccos(E / scale)) V† on the picked rows and columns, M = 24, the models of the GPU tests at
    9 x 8 sites.  The distances printed here (restatement to dense) are the figures a device bound would fall back on."""
    system = MODELS[name]()
    n = system.lattice.size
    assert n == 72
    scale = cases.scale_of(system)
    dense = np.asarray(system.matrix("dense"))
    assert (np.abs(dense.imag).max() == 0) == (name == "uniform")
    h = system.matrix("csr") if matrix == "sparse" else dense
    w, v = np.linalg.eigh(dense)
    everything = cases.dense_chebyshev_moments(w, v, scale, cases.M, np.arange(4 * n), np.arange(4 * n))  # (M, 4N, 4N)

    sources, targets = cases.green_sources(n), cases.green_targets(n)
    assert sources.size == 8 and targets.size == 64 == np.unique(targets).size
    picked = cases.picked_moments(h, scale, cases.M, sources, targets)
    rows = (4 * targets.astype(np.int64)[:, None] + np.arange(4)[None, :]).reshape(-1)
    exact = everything[:, rows][:, :, sources].reshape(cases.M, targets.size, 4, sources.size)
    distance = np.abs(picked - exact).max()
    print(name, matrix, "picked_moments - dense", distance)
    assert picked.shape == exact.shape and np.abs(exact).max() > 0.1 and distance <= 1e-12
    assert np.array_equal(picked[0, :, :, 0], (rows == sources[0]).reshape(-1, 4).astype(float))  # t_0 is the unit vector

    sites = cases.local_sites(n)
    local = cases.local_moments(h, scale, cases.M, sites, chunk=32)  # 32 + 32 + 8 sites
    blocks = everything.reshape(cases.M, n, 4, n, 4)[:, sites, :, sites, :]  # (advanced indices first: (S, M, 4, 4))
    exact = blocks.transpose(1, 0, 2, 3)
    distance = np.abs(local - exact).max()
    print(name, matrix, "local_moments - dense", distance)
    assert local.shape == exact.shape == (cases.M, n, 4, 4) and distance <= 1e-12
    assert np.array_equal(local[0], np.broadcast_to(np.eye(4), (n, 4, 4)))
    # a column does not see its neighbours: another chunking, fewer columns, a sample of the sites
    assert np.array_equal(cases.local_moments(h, scale, cases.M, sites, chunk=5), local)
    assert np.array_equal(cases.local_moments(h, scale, cases.M, sites[3:11], columns=2), local[:, 3:11, :, :2])
    if name == "uniform" and matrix == "sparse":
        # in float64, as cases.restated runs a real matrix: its own roundings, the same pin
        assert np.abs(cases.local_moments(h.real, scale, cases.M, sites) - exact).max() <= 1e-12
    # the picked recurrence on the four rows of a site is that site's local recurrence
    j = int(sites[5])
    own = cases.picked_moments(h, scale, cases.M, 4 * j + np.arange(4), [j])
    assert np.array_equal(own[:, 0], local[:, 5])


# ------------------------------------------------------------------ 9. the tile arithmetic
def test_the_lattice_gives_every_workgroup_several_tiles():
    """The figures the GPU tests rest on, for the 256 CUs of an MI355X (they assert theirs from perf): another lattice or
    lane width must not turn the multi-tile cases into one-tile cases unnoticed."""
    n = int(np.prod(cases.SHAPE))
    assert n == 4221 and cases.SHAPE[0] % 2 == cases.SHAPE[1] % 2 == 1
    for name in ("uniform", "disordered"):
        assert cases.system_of(name).lattice.size == n

    expected = {  # lanes: (tiles, block rows of the last tile, fewest and most tiles of a workgroup at one workgroup per CU)
        16: (264, 13, 1, 2),
        32: (528, 5, 2, 3),
        64: (1056, 1, 4, 5),
    }
    for lanes, (tiles, ragged, fewest, most) in expected.items():
        assert cases.tiles_of(n, lanes) == tiles and cases.last_tile_rows(n, lanes) == ragged
        grid = cases.grid_of(tiles, 1)
        assert grid == 256 and tiles > grid
        shares = cases.tile_shares(tiles, grid)
        assert shares.sum() == tiles and (shares.min(), shares.max()) == (fewest, most), (lanes, shares.min(), shares.max())
        assert (tiles > 2 * grid) == (lanes >= 32)  # (16 lanes: only some workgroups take a second tile)
        one_tile = cases.grid_of(tiles, 8)  # the reference run
        assert one_tile >= tiles and cases.tile_shares(tiles, one_tile).max() == 1
    # 32 lanes, the last tile: two rows per wave, so waves 0 and 1 are full, wave 2 is half valid, wave 3 wholly past the end
    assert 64 // 32 == 2 and cases.last_tile_rows(n, 32) == 2 + 2 + 1
    # two workgroups per CU at 32 lanes: a second tile for a few workgroups only
    shares = cases.tile_shares(528, cases.grid_of(528, 2))
    assert cases.grid_of(528, 2) == 512 and shares.sum() == 528 and shares.max() == 2 and (shares == 2).sum() == 16
    # the cube: 7 blocks per row, more than two tiles per workgroup at 32 lanes
    cube = cases.system_of("cube")
    assert cube.lattice.size == 4352 and int(np.diff(cube._matrix.indptr).max()) == 7
    assert int(np.diff(cases.system_of("uniform")._matrix.indptr).max()) == 5
    assert cases.tiles_of(4352, 32) == 544 > 2 * cases.grid_of(544, 1)
    # the XCD split itself: every tile once, whatever the grid
    for tiles, grid in ((528, 256), (1056, 256), (7, 8), (529, 264), (1, 8)):
        seen = np.zeros(tiles, dtype=int)
        for b in range(grid):
            lo, hi = tiles * (b & 7) // 8, tiles * ((b & 7) + 1) // 8
            seen[lo + (b >> 3) : hi : grid // 8] += 1
        assert np.all(seen == 1), (tiles, grid)
        assert cases.tile_shares(tiles, grid).sum() == tiles


def test_the_sample_of_the_local_moments_is_near_every_site():
    """family_tile_cases.local_sample: no site of the lattice is more than 8 bonds from a sampled one, the sample holds
    the ragged last tile and every offset within a tile; local_positions finds the sample in the permuted site list."""
    n = int(np.prod(cases.SHAPE))
    sample = cases.local_sample()
    assert sample.size == 63  # (8 x 7 and the last eight, one of which is on the grid)
    assert set(range(n - 8, n)) <= set(sample.tolist())
    assert set((sample % 8).tolist()) == set(range(8))
    coordinates = cases.system_of("uniform").lattice.site_array()
    assert np.array_equal(coordinates[:, 1] + cases.SHAPE[1] * coordinates[:, 0], np.arange(n))  # rows number y + Ly x
    distance = np.abs(coordinates[:, None, :] - coordinates[sample][None, :, :]).sum(axis=2).min(axis=1)
    print("farthest site from the sample:", distance.max(), "bonds")
    assert distance.max() <= 8
    assert np.array_equal(cases.local_sites(n)[cases.local_positions()], sample)
