"""The 2-D t-SNE embedding of a cell-to-cell distance matrix on the GPU (csrc/tsne.hip; the
contract is in include/scde_hip.h).

  * ``tsne_embedding``                    the whole run, the step the PAGODA walkthrough takes
                                          with ``Rtsne(cell.clustering$distance, is_distance =
                                          TRUE, perplexity = 10)`` (vignettes/pagoda.md:230-250)
  * ``tsne_affinities`` / ``tsne_iterate``  the same in two steps on a state that stays in HBM: a
                                          run can be extended or resumed without redoing the
                                          affinities

This is van der Maaten's exact t-SNE, the method ``Rtsne(theta = 0)`` wraps, written from the
published algorithm.  The vignette's call uses Rtsne's default Barnes-Hut approximation
(``theta = 0.5``), of which this is the exact limit.  Nothing here was checked against a run of
Rtsne.  Two things are this project's own choice because Rtsne's are not known here: a distance
is squared before the affinities are formed unless ``squared=True`` says it already is, and
the seeded start is ``1e-4 * rnorm(2 n)`` of R's stream after ``set.seed(seed)``, filled point by
point.

Only the strict lower triangle of the matrix is read (what ``as.dist`` reads, as ``hclust``
does), and every value there must be finite and not negative.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import api
from ._lib import check, lib

#: Rtsne's defaults
DEFAULTS = dict(eta=200.0, exaggeration=12.0, stop_lying_iter=250, mom_switch_iter=250, momentum=0.5,
                final_momentum=0.8)


def _square(d, perplexity):
    """(Fortran-ordered float64 square matrix, labels or None), the Python-side argument checks."""
    labels = [str(x) for x in d.index] if hasattr(d, "index") and hasattr(d, "columns") else None
    a = np.asarray(d.values if labels is not None else d)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError("d must be a square distance matrix")
    n = a.shape[0]
    if n < 4:
        raise ValueError(f"at least 4 objects are needed (n = {n})")
    if not perplexity >= 1 or not 3 * perplexity <= n - 1:
        raise ValueError(f"perplexity must be at least 1 and 3 * perplexity at most n - 1 "
                         f"(perplexity = {perplexity}, n = {n})")
    return np.asfortranarray(a, dtype=np.float64), labels


def _y_init(Y_init, n):
    if Y_init is None:
        return None
    y = np.ascontiguousarray(np.asarray(Y_init, dtype=np.float64))
    if y.shape != (n, 2):
        raise ValueError(f"Y_init must be {n} x 2")
    return y


def _params(kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown argument(s): {', '.join(sorted(unknown))}")
    p = dict(DEFAULTS, **kw)
    return (float(p["eta"]), float(p["exaggeration"]), int(p["stop_lying_iter"]), int(p["mom_switch_iter"]),
            float(p["momentum"]), float(p["final_momentum"]))


def initial_Y(n, seed=1):
    """The seeded start: ``Y0[i, c] = 1e-4 * z[2 i + c]``, ``z = rnorm(2 n)`` after
    ``set.seed(seed)`` (host code; no device is touched)."""
    L = lib()
    st = np.zeros(625, np.uint32)
    check(L.scde_r_set_seed(int(seed) & 0xFFFFFFFF, api._p(st)))
    z = np.zeros(2 * n)
    check(L.scde_r_norm_rand(api._p(st), 2 * n, api._p(z)))
    return (1e-4 * z).reshape(n, 2)


def _labelled(Y, labels):
    if labels is None:
        return Y
    import pandas as pd
    return pd.DataFrame(Y, index=labels, columns=["tSNE1", "tSNE2"])


def tsne_embedding(d, perplexity=30, max_iter=1000, seed=1, Y_init=None, squared=False, return_details=False,
                   ctx: api.Context | None = None, **kw):
    """Exact t-SNE of the distance matrix ``d`` (a square array, or a DataFrame whose labels
    are kept: the result is then a DataFrame with that index) into two dimensions, in one call:
    upload, affinities at ``perplexity``, ``max_iter`` iterations, cost.  ``Y_init``: an n x 2
    start instead of the seeded one.  ``squared``: ``d`` holds squared distances.  Further
    keywords, with Rtsne's defaults: ``eta`` 200, ``exaggeration`` 12, ``stop_lying_iter`` 250,
    ``mom_switch_iter`` 250, ``momentum`` 0.5, ``final_momentum`` 0.8.

    Returns the n x 2 embedding; with ``return_details`` {"Y", "costs" (per point; their sum
    is the Kullback-Leibler divergence), "beta" (per point, the precision the perplexity search
    ended on), "P" (n x n), "labels"}.  ``max_iter=0`` returns the start.

    This is the exact method (the limit theta = 0 of the Barnes-Hut approximation that the
    vignette's Rtsne call uses by default), written from the published algorithm; nothing was
    checked against Rtsne.  Results repeat bit for bit."""
    a, labels = _square(d, perplexity)
    n = a.shape[0]
    y0 = _y_init(Y_init, n)
    prm = _params(kw)
    if int(max_iter) < 0:
        raise ValueError("max_iter must not be negative")
    Y = np.zeros((n, 2))
    costs, beta = np.zeros(n), np.zeros(n)
    P = np.zeros((n, n), order="F") if return_details else None
    check(lib().scde_tsne_host(ctx.handle if ctx else None, api._p(a), n, n, float(perplexity), int(bool(squared)),
                               *prm, int(max_iter), int(seed) & 0xFFFFFFFF, api._p(y0), api._p(Y), api._p(costs),
                               api._p(beta), api._p(P)))
    if return_details:
        return {"Y": _labelled(Y, labels), "costs": costs, "beta": beta, "P": P, "labels": labels}
    return _labelled(Y, labels)


class TsneState:
    """A run resident in HBM: P, Y, uY, gains and the workspace; ``iter`` iterations done.
    ``Y()``, ``uY()``, ``gains()``, ``P()`` and ``costs()`` read it back; ``set(Y, uY, gains,
    iter)`` replaces the state; ``close()`` frees the device memory (also done on collection)."""

    def __init__(self, ctx, n, labels, beta, params):
        self.ctx, self.n, self.labels, self.beta, self.params = ctx, n, labels, beta, params
        self.iter = 0
        self._ptrs = {}

    def _alloc(self, name, nbytes):
        p = ctypes.c_void_p()
        check(lib().scde_dev_alloc(self.ctx.handle, int(nbytes), ctypes.byref(p)))
        self._ptrs[name] = p
        return p

    def _get(self, name, shape, order="C"):
        out = np.zeros(shape, order=order)
        check(lib().scde_d2h(self.ctx.handle, api._p(out), self._ptrs[name], out.nbytes))
        return out

    def _put(self, name, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (self.n, 2):
            raise ValueError(f"{name} must be {self.n} x 2")
        check(lib().scde_h2d(self.ctx.handle, self._ptrs[name], api._p(a), a.nbytes))

    def Y(self):
        return _labelled(self._get("Y", (self.n, 2)), self.labels)

    def uY(self):
        return self._get("uY", (self.n, 2))

    def gains(self):
        return self._get("gains", (self.n, 2))

    def P(self):
        return self._get("P", (self.n, self.n), order="F")

    def set(self, Y, uY, gains, iter):
        arrays = [np.ascontiguousarray(x, dtype=np.float64) for x in (Y, uY, gains)]
        if any(x.shape != (self.n, 2) for x in arrays) or int(iter) < 0:
            raise ValueError(f"Y, uY and gains must be {self.n} x 2 and iter not negative")
        for name, x in zip(("Y", "uY", "gains"), arrays):
            self._put(name, x)
        self.iter = int(iter)

    def costs(self):
        out = np.zeros(self.n)
        check(lib().scde_tsne_cost_dev(self.ctx.handle, self._ptrs["P"], self.n, self._ptrs["Y"], api._p(out),
                                       self._ptrs["ws"], self.ws_bytes))
        return out

    def close(self):
        ptrs, self._ptrs = self._ptrs, {}
        for p in ptrs.values():
            lib().scde_dev_free(self.ctx.handle, p)

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def tsne_affinities(d, perplexity=30, seed=1, Y_init=None, squared=False, ctx: api.Context | None = None, **kw):
    """The first half of ``tsne_embedding``: ``d`` is uploaded, the affinities P are formed and
    stay in HBM with the start (``Y_init`` or the seeded one), zero ``uY`` and unit gains.
    Returns the ``TsneState`` that ``tsne_iterate`` advances; the keywords of ``tsne_embedding``
    (``eta`` ...) are fixed here for the run."""
    a, labels = _square(d, perplexity)
    n = a.shape[0]
    y0 = _y_init(Y_init, n)
    prm = _params(kw)
    if y0 is None:
        y0 = initial_Y(n, seed)
    ctx = ctx or api.default_context()
    L = lib()
    wsb = ctypes.c_int64()
    check(L.scde_tsne_ws_bytes(n, ctypes.byref(wsb)))
    beta = np.zeros(n)
    st = TsneState(ctx, n, labels, beta, prm)
    st.ws_bytes = wsb.value
    try:
        dp = st._alloc("d", a.nbytes)
        st._alloc("P", a.nbytes)
        for name in ("Y", "uY", "gains"):
            st._alloc(name, 16 * n)
        st._alloc("ws", wsb.value)
        check(L.scde_h2d(ctx.handle, dp, api._p(a), a.nbytes))
        check(L.scde_tsne_affinities_dev(ctx.handle, dp, n, n, float(perplexity), int(bool(squared)), st._ptrs["P"],
                                         api._p(beta), st._ptrs["ws"], wsb.value))
        check(L.scde_dev_free(ctx.handle, st._ptrs.pop("d")))
        st.set(y0, np.zeros((n, 2)), np.ones((n, 2)), 0)
    except Exception:
        st.close()
        raise
    return st


def tsne_iterate(state: TsneState, n_iter):
    """``n_iter`` more iterations on ``state`` (in place; ``state.iter`` counts them, and the
    exaggeration and momentum switches follow it).  Splitting a run anywhere gives the bits of
    the unsplit run.  A refused call leaves the state as it was."""
    n_iter = int(n_iter)
    if n_iter < 0:
        raise ValueError("n_iter must not be negative")
    p = state._ptrs
    check(lib().scde_tsne_iterate_dev(state.ctx.handle, p["P"], state.n, *state.params, state.iter, n_iter, p["Y"],
                                      p["uY"], p["gains"], p["ws"], state.ws_bytes))
    state.iter += n_iter
    return state
