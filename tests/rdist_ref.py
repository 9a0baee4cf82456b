"""A numpy restatement of R's ``stats::dist`` as include/scde_hip.h states it: vectorised over the
pairs, sequential over the columns, every operation a separate float64 rounding.  The reference of
tests/test_rdist.py and tests/test_gpu_rdist.py."""
import numpy as np

METHODS = ("euclidean", "manhattan", "maximum")


def rdist(x, method="euclidean"):
    """The n x n matrix of distances between the rows of the n x p ``x``."""
    if method not in METHODS:
        raise ValueError(method)
    x = np.asarray(x, dtype=np.float64)
    n, p = x.shape
    s = np.zeros((n, n))
    count = np.zeros((n, n), np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(p):  # the columns in increasing order
            d = x[:, k][:, None] - x[:, k][None, :]
            part = ~np.isnan(d)  # a NaN on either side, or Inf - Inf, drops the column
            if method == "euclidean":
                t = d * d
            else:
                t = np.abs(d)
            if method == "maximum":
                s = np.where(part & (t > s), t, s)
            else:
                s = np.where(part, s + t, s)
            count += part
        if method != "maximum":
            scale = count.astype(np.float64) / np.float64(p if p else 1)
            s = np.where(count != p, s / scale, s)
        if method == "euclidean":
            s = np.sqrt(s)  # correctly rounded
        s = np.where(count == 0, np.nan, s)
    s[np.arange(n), np.arange(n)] = 0.0
    return s
