"""Synthetic orbital lists for the sector path.  TEST INFRASTRUCTURE ONLY: SectorTables / TriplesTables and the numpy
restatements take any list of distinct integer vectors, so the orbital counts of a test need not be those of an electron gas."""
import numpy as np


def line_lattice(no, nv):
    """(k_int [no + nv, 3], no): the vectors (x, 0, 0), x = 0 ... no + nv - 1.  Occupied (listed first, ascending x): nv // 2 <=
    x < nv // 2 + no; the virtuals are the rest in ascending x.  The lookup box has extent 1 on two axes, and K - k_a - k_b
    leaves it on both sides of the first."""
    x = np.arange(no + nv)
    occ = (x >= nv // 2) & (x < nv // 2 + no)
    k = np.zeros((no + nv, 3), dtype=np.int64)
    k[:, 0] = np.concatenate((x[occ], x[~occ]))
    return k, no
