"""Inputs shared by the cross-fit tests: synthetic cell pairs with a set number of rows, and the
cells of the ES/MEF fixture the GPU tests use."""
import numpy as np

ROWS = (1, 63, 64, 65, 255, 256, 257)
# Chosen on the CPU, with the restatement alone: all 25 pairs fit with status 0 and keep their
# number of rounds under gene permutations (cell 0's pairs with 5 and 7 lose a component; the
# pair (22, 24) stops a round earlier or later depending on the order of its sums).
ES_CELLS, MEF_CELLS = (1, 2, 3, 4, 5, 6), (20, 21, 22, 23, 25)


def synthetic_pair(n, seed, N=None):
    """Two cells over N genes whose first n genes have a count in either cell (the rest are zero):
    a shared log-normal magnitude, NB counts around it, each cell dropping out independently."""
    rng = np.random.default_rng(seed)
    N = n if N is None else N
    out = np.zeros((N, 2), np.int32)
    mag = np.exp(rng.normal(2.5, 1.3, n))
    for k in range(2):
        th = 1.5 + k
        y = rng.negative_binomial(th, th / (th + mag * (0.8 + 0.4 * k)))
        drop = rng.random(n) < 1 / (1 + np.exp(-1.0 + 0.9 * np.log(mag)))
        y[drop] = rng.poisson(0.1, int(drop.sum()))
        out[:n, k] = y
    both = out[:n].sum(axis=1) == 0
    out[:n, 0][both] = 1  # (every one of the n genes is a row)
    return out


def many_cells(seed=11, N=40, C=26):
    rng = np.random.default_rng(seed)
    mag = np.exp(rng.normal(2.5, 1.2, (N, 1)))
    y = rng.negative_binomial(2.0, 2.0 / (2.0 + mag * rng.uniform(0.6, 1.5, (1, C))))
    drop = rng.random((N, C)) < 1 / (1 + np.exp(-1.0 + 0.9 * np.log(mag)))
    y[drop] = rng.poisson(0.1, int(drop.sum()))
    return np.asfortranarray(y.astype(np.int32))
