"""``clean_counts`` and ``clean_gos`` (scde_amd/prep.py) on hand-made inputs where each strict
``>`` decides, and where the order of the three filters decides.  No GPU."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def P():
    from scde_amd import prep
    return prep


#            c0  c1  c2  c3
COUNTS = [[5,  1,  1,  9],   # g0
          [0,  2,  2,  9],   # g1
          [1,  3,  0,  0],   # g2
          [1,  0,  4,  0],   # g3
          [0,  0,  0,  9]]   # g4


def test_each_strict_comparison_decides(P):
    a = np.array(COUNTS)
    # detected genes per cell: 3, 3, 3, 3
    assert P.clean_counts(a, min_lib_size=3, min_reads=0, min_detected=0).shape == (0, 0)  # 3 > 3 is false
    assert P.clean_counts(a, min_lib_size=2, min_reads=0, min_detected=0).shape == (5, 4)
    # reads per gene over all cells: 16, 13, 4, 5, 9
    got = P.clean_counts(a, min_lib_size=0, min_reads=5, min_detected=0)
    assert np.array_equal(got, a[[0, 1, 4]])  # 5 > 5 is false: g3 goes
    got = P.clean_counts(a, min_lib_size=0, min_reads=4, min_detected=0)
    assert np.array_equal(got, a[[0, 1, 3, 4]])  # 4 > 4 is false: g2 goes
    # cells a gene is seen in: 4, 3, 2, 2, 1
    got = P.clean_counts(a, min_lib_size=0, min_reads=0, min_detected=2)
    assert np.array_equal(got, a[[0, 1]])
    got = P.clean_counts(a, min_lib_size=0, min_reads=0, min_detected=1)
    assert np.array_equal(got, a[[0, 1, 2, 3]])


def test_filter_order_matters(P):
    #            c0  c1  c2
    a = np.array([[9, 1, 1],    # g0
                  [9, 1, 0],    # g1
                  [0, 1, 1],    # g2
                  [0, 0, 1]])   # g3
    # cell c0 has 2 detected genes and is dropped first (2 > 2 is false); c1 and c2 have 3.
    # Only then the reads are counted: g0 2, g1 1, g2 2, g3 1; with min_reads = 1, g0 and g2 stay.
    # Genes first would have kept g1 (10 reads over all cells).
    got = P.clean_counts(a, min_lib_size=2, min_reads=1, min_detected=1)
    assert np.array_equal(got, np.array([[1, 1], [1, 1]]))
    # and the third filter sees what the second left, in the remaining cells: g1 is seen in one
    got = P.clean_counts(a, min_lib_size=2, min_reads=0, min_detected=1)
    assert np.array_equal(got, np.array([[1, 1], [1, 1]]))
    got = P.clean_counts(a, min_lib_size=2, min_reads=0, min_detected=0)
    assert np.array_equal(got, a[:, 1:])


def test_dataframe_keeps_labels(P):
    import pandas as pd
    df = pd.DataFrame(COUNTS, index=[f"g{i}" for i in range(5)], columns=[f"c{i}" for i in range(4)])
    got = P.clean_counts(df, min_lib_size=0, min_reads=5, min_detected=1)
    assert list(got.index) == ["g0", "g1"] and list(got.columns) == ["c0", "c1", "c2", "c3"]
    assert np.array_equal(got.values, np.array(COUNTS)[[0, 1]])


def test_defaults_are_the_reference_s(P):
    a = np.ones((1802, 7), dtype=np.int64)
    assert P.clean_counts(2 * a).shape == (1802, 7)  # 1802 > 1800 genes, 14 > 10 reads, 7 > 5 cells
    assert P.clean_counts(a).shape == (0, 7)         # 7 reads > 10 is false
    a2 = a.copy()
    a2[:3, 0] = 0                                    # cell 0 now has 1799 genes
    assert P.clean_counts(2 * a2).shape == (1802, 6)  # 12 reads > 10, 6 cells > 5
    assert P.clean_counts(2 * a2[:, :6]).shape == (0, 5)  # ... and 10 reads > 10 is false


def test_clean_gos(P):
    go = {"five": list(range(5)), "six": list(range(6)), "nine": list(range(9)), "ten": list(range(10))}
    assert list(P.clean_gos(go, min_size=5, max_size=10)) == ["six", "nine"]
    assert list(P.clean_gos(go, min_size=4, max_size=11)) == ["five", "six", "nine", "ten"]
    assert list(P.clean_gos(go)) == ["six", "nine", "ten"]  # the defaults: 5 and 5000
    assert P.clean_gos(go)["six"] == list(range(6))
    with pytest.raises(NotImplementedError):
        P.clean_gos(go, annot=True)
