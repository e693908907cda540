"""CPU: ``SectorTables.ladder_rows`` (pymes_amd/solver/sectors.py), the two tables the direct particle ladder reads in place of
the ``abcd`` lists (include/pymes_amd.h, pymes_sector_ladder_direct): they must reproduce ``block_pqrs("abcd")``
element by element, empty sectors included."""
import numpy as np
import pytest

from pymes_amd.solver.sectors import SectorTables
from tests._sector_lattices import line_lattice


def ueg_tables(nel, cutoff):
    from pymes_amd.model.ueg import UEG
    m = UEG(nel, nel // 2, nel // 2, 1.0)
    m.init_single_basis(cutoff)
    return m.sector_tables()


def lattice_tables(no, nv):
    k, no = line_lattice(no, nv)
    return SectorTables(k, no)


CASES = {"ueg-14-2": lambda: ueg_tables(14, 2), "ueg-14-5": lambda: ueg_tables(14, 5), "ueg-54-5": lambda: ueg_tables(54, 5),
         "line-3-40": lambda: lattice_tables(3, 40)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_ladder_rows_reproduce_the_abcd_lists(case):
    tab = CASES[case]()
    rows, first = tab.ladder_rows()
    nsec = len(tab.P_keys)
    assert rows.dtype == np.int32 and rows.shape == (len(tab.vv_pairs), 2)
    assert first.dtype == np.int64 and first.shape == (nsec,)
    assert rows.min() >= tab.no and rows.max() < tab.n
    if case in ("ueg-14-2", "ueg-54-5"):
        assert (tab.n_vv == 0).any()
    want = tab.block_pqrs("abcd")
    off = tab.block_offsets("abcd")
    assert len(want) == off[-1] and off[-1] > 0
    got = np.empty_like(want)
    for s in range(nsec):                       # every element of sector s, row r, column c
        v = int(tab.n_vv[s])
        assert first[s] + v <= len(rows)
        r, c = np.divmod(np.arange(v * v), max(v, 1))
        got[off[s]:off[s + 1], :2] = rows[first[s] + r]
        got[off[s]:off[s + 1], 2:] = rows[first[s] + c]
    assert np.array_equal(got, want)
    # a sector's rows are its own: consecutive sectors do not share a row
    assert np.array_equal(first, np.concatenate(([0], np.cumsum(tab.n_vv)))[:-1])
