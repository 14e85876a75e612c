"""The packed-caption row plan (tests/text_varlen_ref.py, the host restatement of vtp_text_row_plan) against brute force."""
import numpy as np

from text_varlen_ref import packed_rows, row_plan


def _brute(ids):
    eot, cu, acc = [], [0], 0
    for row in ids:
        best, bi = row[0], 0
        for t, v in enumerate(row):
            if v > best:  # strict: the first maximum wins
                best, bi = v, t
        eot.append(bi)
        acc += bi + 1
        cu.append(acc)
    return eot, cu, acc


def test_row_plan_matches_brute_force_on_random_captions():
    rng = np.random.default_rng(0)
    for B, T in ((1, 1), (1, 77), (5, 77), (32, 77), (7, 16)):
        ids = rng.integers(0, 50, size=(B, T))
        eot, cu, rows = row_plan(ids)
        b_eot, b_cu, b_rows = _brute(ids.tolist())
        assert eot.tolist() == b_eot and cu.tolist() == b_cu and rows == b_rows
        assert eot.dtype == np.int32 and cu.dtype == np.int32 and cu.shape == (B + 1,)


def test_row_plan_edge_cases():
    T = 9
    ids = np.zeros((6, T), dtype=np.int64)
    ids[0] = 0                                   # an all-zero caption: every position ties, the first wins -> length 1
    ids[1, [2, 5, 7]] = 40                       # ties in the arg-max: the first maximum (position 2)
    ids[2, 0] = 99                               # EOT at position 0
    ids[3, T - 1] = 99                           # EOT at position T - 1
    ids[4] = np.arange(T)[::-1] + 1              # decreasing: position 0
    ids[5] = np.arange(T) + 1                    # increasing: position T - 1
    eot, cu, rows = row_plan(ids)
    assert eot.tolist() == [0, 2, 0, T - 1, 0, T - 1]
    assert cu.tolist() == [0, 1, 4, 5, 5 + T, 6 + T, 6 + 2 * T] and rows == 6 + 2 * T
    b_eot, b_cu, b_rows = _brute(ids.tolist())
    assert eot.tolist() == b_eot and cu.tolist() == b_cu and rows == b_rows
    # the packed order visits caption after caption, token after token
    pr = packed_rows(cu, T)
    assert pr.shape == (rows,) and pr.tolist()[:6] == [0, T, T + 1, T + 2, 2 * T, 3 * T]
    assert all(pr[cu[b + 1] - 1] == b * T + eot[b] for b in range(6))  # the pooled (EOT) row is the last of every caption
