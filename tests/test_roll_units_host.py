"""The rolling kernel's equal-length units without a GPU: the restatements of roll_unit_cases.py (launch shape and
unit-to-pieces loop) tile every launch of every case exactly once, reproduce the figures the code documents, and every
case of the table still exercises what it was chosen for."""

import numpy as np
import pytest

import roll_unit_cases as rc


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_pieces_cover_every_window_and_plane_of_every_launch_exactly_once(name):
    plan = rc.plan_of(name)
    chunked = 0
    for x_lo, x_hi, _, chunk in rc.launches(name):
        if chunk == 0:
            continue
        chunked += 1
        span = x_hi - x_lo
        cut = rc.units(plan.n_cols, x_lo, x_hi, chunk)
        assert len(cut) == (plan.n_cols * span + chunk - 1) // chunk  # the kernel's n_units
        seen = np.zeros((plan.n_cols, plan.lx), dtype=np.int64)
        for u, pieces in enumerate(cut):
            assert 1 <= len(pieces) <= 2, (u, pieces)
            for col, x0, x1 in pieces:
                assert 0 <= col < plan.n_cols and x_lo <= x0 < x1 <= x_hi, (u, pieces)  # no empty piece, inside the band
                seen[col, x0:x1] += 1
                for reverse in (False, True):  # a reversed march visits the same planes, last to first
                    assert sorted(rc.act_planes(x0, x1, reverse)) == list(range(x0, x1))
                assert rc.act_planes(x0, x1, True)[0] == x1 - 1
            if len(pieces) == 2:  # the run goes on at the bottom of the next column
                assert pieces[0][2] == x_hi and pieces[1][:2] == (pieces[0][0] + 1, x_lo)
            if u < len(cut) - 1:
                assert sum(x1 - x0 for _, x0, x1 in pieces) == chunk
        assert np.all(seen[:, x_lo:x_hi] == 1) and seen.sum() == plan.n_cols * span
    assert chunked > 0


def test_restatement_gives_the_figures_the_code_documents():
    """100^3 (BASELINE config 4) on 2048 wave slots: 715 windows of 14 positions, 35 planes per unit (sweep.hpp, RollArgs.chunk;
    DESIGN.md §9 (6)); two lane groups side by side get half the slots each; with 2 lanes per site the 334 x 6 = 2004
    whole-column segments fill the slots well enough; a slab of 12 or 13 planes is too short to cut."""
    four = rc.windows((100, 100, 100), 4)
    assert four == 715
    assert rc.RollPlan(four, 100, 2048, 1).chunk_for(100) == 35
    assert rc.RollPlan(four, 100, 2048, 2).chunk_for(100) == 70
    two = rc.RollPlan(rc.windows((100, 100, 100), 2), 100, 2048, 1)
    assert (two.n_cols, two.whole_segs, two.chunk_for(100)) == (334, 6, 0)
    assert int(0.92 * 2048) <= 2004 <= 2048
    for planes in (12, 13):
        assert rc.RollPlan(four, planes, 2048, 1).chunk_for(planes) == 0
    # the suite's other 3-D shapes never chunk, whatever the device: the coverage gap the cases close
    for shape in ((12, 30, 4), (9, 7, 13), (10, 6, 8), (40, 12, 14), (30, 30, 30)):
        for lanes in (2, 4):
            for waves in (1024, 2048):
                assert rc.RollPlan(rc.windows(shape, lanes), shape[0], waves, 1).chunk_for(shape[0]) == 0


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_every_case_has_the_properties_its_row_claims(name):
    case, plan = rc.CASES[name], rc.plan_of(name)
    x_lo, x_hi, _, chunk = rc.launches(name)[-1]
    assert chunk == case.chunk and chunk > 0
    cut = rc.units(plan.n_cols, x_lo, x_hi, chunk)
    lengths = [x1 - x0 for pieces in cut for _, x0, x1 in pieces]
    assert len(cut) == case.n_units
    assert sum(len(pieces) == 2 for pieces in cut) == case.two_piece > 0
    assert min(lengths) == case.shortest
    assert sum(x1 - x0 for _, x0, x1 in cut[-1]) == case.last_unit
    assert len(cut) <= rc.WAVES // case.share  # one unit per wave slot of the launch's part of the device
    assert plan.n_cols == rc.windows(case.shape, case.lanes) == {4: 386, 2: 180}[case.lanes]


def test_band_launches_of_the_unit_start_case_change_their_shape_from_launch_to_launch():
    got = rc.launches("F14")
    assert [(lo, hi) for lo, hi, _, _ in got[:3]] == [(11, 14), (10, 15), (9, 16)]
    assert [chunk for _, _, _, chunk in got] == [0] * 8 + [8, 8, 9, 10, 10, 10]
    assert got[8][:2] == (3, 22) and got[-1][:2] == (0, 24)  # x_lo > 0 with chunk > 0, then the whole lattice
    assert rc.launches("F9") == got[:9]
    low = rc.launches("F16-low")
    assert [chunk for _, _, _, chunk in low] == [0] * 12 + [8, 8, 8, 9]
    assert [(lo, hi) for lo, hi, _, _ in low[12:]] == [(0, 19), (0, 20), (0, 21), (0, 22)]  # off-centre: x_lo + x_hi != lx
    rows = rc.unit_rows("F9")
    sites = rows // 4
    assert len(set(rows % 4)) == 4 and len(set(sites % 75)) == 8 and len(set(sites // 75 % 72)) == 8
    assert set(sites // (72 * 75)) == {12}


def test_palette_systems_are_hermitian_inhomogeneous_and_small_enough_for_every_table():
    import scipy.sparse as sp

    for kind, distinct, real in (("real", 20, True), ("peierls", 24, False)):
        bsr, scale = rc.matrix_of((8, 24, 25), kind)  # (the palettes do not depend on the shape: a small one is enough here)
        assert bsr.shape == (4 * 4800, 4 * 4800) and scale > 0
        blocks = np.unique(bsr.data.reshape(len(bsr.data), 16), axis=0)
        assert len(blocks) == distinct <= 96  # (ComplexMode: 272 B per block of a 32 KiB table)
        assert (np.abs(bsr.data.imag).max() == 0) == real
        csr = sp.csr_matrix(bsr)
        assert abs(csr - csr.getH()).max() == 0
        # not translation invariant: neighbouring planes carry different diagonal blocks
        diag = bsr.diagonal().reshape(8, -1)
        assert all(not np.array_equal(diag[x], diag[x + 1]) for x in range(7))
