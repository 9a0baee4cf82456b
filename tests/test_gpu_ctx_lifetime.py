"""A context that has used every workspace family is destroyed and replaced, twice.

The context's device buffers free themselves when the context goes (engine_internal.h, Buf), so
teardown is no longer a list somebody keeps.  This test is the one that destroys a context after
more than the differential-expression pipeline has run on it: per round, a fresh explicit context,
one tiny call of each family that owns workspace -- differential expression (the smoke() input),
a distance measure, hclust, optimal leaf ordering, t-SNE, the aspects' t renormalisation, a
weighted-PCA batch -- then scde_ctx_destroy.  Every call succeeds, the second round repeats the
first bit for bit (same seeds, a new context), and the default context still works afterwards.
Free device memory is not looked at: the card is shared.
"""
import ctypes

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu


def _inputs():
    from oracle import oracle as O
    g = golden("esmef500.npz")
    rng = np.random.default_rng(3)
    de = dict(models={c: g["models"][:, j] for j, c in enumerate(O.MODEL_COLUMNS)
                      if not np.all(np.isnan(g["models"][:, j]))},
              counts=np.ascontiguousarray(g["counts"][:64]), prior={"x": g["prior_x"], "y": g["prior_y"]},
              groups=list(g["groups"]))
    x = rng.normal(size=(8, 4))                      # a distance measure: 8 genes x 4 cells
    u = rng.uniform(0.2, 1.0, size=(8, 4))
    p5 = rng.normal(size=(5, 3))                     # hclust / order.optimal: 5 objects
    d5 = np.sqrt(((p5[:, None, :] - p5[None, :, :]) ** 2).sum(-1))
    p8 = rng.normal(size=(8, 3))                     # t-SNE: 8 objects
    d8 = np.sqrt(((p8[:, None, :] - p8[None, :, :]) ** 2).sum(-1))
    r3 = np.asfortranarray(rng.uniform(-0.9, 0.9, size=(3, 3)))  # t renormalisation: m = 3
    n3 = np.asfortranarray(rng.integers(5, 40, size=(3, 3)), dtype=np.int32)
    n, G = 120, 90                                   # weighted PCA: tests/test_gpu_wpca.py's batch shape
    m = rng.normal(size=(n, G))
    w = rng.uniform(0.05, 1.0, size=(n, G))
    m = m - (m * w).sum(0) / w.sum(0)
    cols = np.arange(12)
    starts = rng.uniform(size=2 * len(cols))
    return dict(de=de, x=x, u=u, d5=d5, d8=d8, r3=r3, n3=n3, m=m, w=w, cols=cols, starts=starts)


def _round(inp):
    """One context's life; every output as bytes, in call order.  A failing call raises ScdeError."""
    from scde_amd import api, hclust, order_optimal, tsne_embedding
    from scde_amd import pagoda as PG
    from scde_amd._lib import check, lib
    from scde_amd.distance import weighted_correlation
    out = []

    def keep(*arrays):
        out.extend(np.ascontiguousarray(a).tobytes() for a in arrays)

    ctx = api.Context(0)
    try:
        de = inp["de"]
        got = api.scde_expression_difference(de["models"], de["counts"], de["prior"], groups=de["groups"],
                                             n_randomizations=20, n_cores=1, return_posteriors=True, ctx=ctx)
        keep(got["joint.posteriors"][0], got["joint.posteriors"][1], got["difference.posterior"].values,
             *(got["results"][k].to_numpy() for k in ("lb", "mle", "ub", "ce", "Z", "cZ")))
        keep(weighted_correlation(inp["x"], inp["u"], ctx=ctx))
        hc = hclust(inp["d5"], method="average", ctx=ctx)
        keep(hc.merge, hc.height, hc.order)
        oo, length = order_optimal(hc, inp["d5"], ctx=ctx, return_length=True)
        keep(oo.merge, oo.order, np.float64(length))
        ts = tsne_embedding(inp["d8"], perplexity=2, max_iter=5, seed=1, return_details=True, ctx=ctx)
        keep(ts["Y"], ts["costs"], ts["beta"], ts["P"])
        cr = np.zeros((3, 3), order="F")
        check(lib().scde_t_renorm_host(ctx.handle, api._p(inp["r3"]), api._p(inp["n3"]), 3, 10.0, api._p(cr)))
        keep(cr)
        dev = PG.DeviceMatrixPair(ctx, inp["m"].T, inp["w"].T)
        try:
            b = PG.WpcaBatch()
            b.add(inp["cols"], 2, 1, inp["starts"])
            res = b.run(dev, want_iterations=True)[0]
        finally:
            dev.free()
        keep(res["rotation"], res["scores"], res["scoreweights"], res["var"], np.float64(res["totvar"]),
             res["iterations"])
    finally:
        ctx.close()
    return out


def test_contexts_that_used_every_family_are_destroyed_and_replaced():
    from scde_amd import api, hclust
    from scde_amd._lib import lib
    kind = api.get_rand_kind()
    api.set_rand("glibc")
    try:
        inp = _inputs()
        first = _round(inp)
        second = _round(inp)
    finally:
        lib().scde_set_rand_kind(kind)
    assert len(first) == len(second) and len(first) > 20
    differing = [i for i, (a, b) in enumerate(zip(first, second)) if a != b]
    assert not differing, f"outputs {differing} of {len(first)} differ between the two contexts"
    assert all(len(a) > 0 for a in first)
    # the default context (a null ctx at the C ABI) after two explicit ones came and went
    hc = hclust(inp["d5"], method="average")
    assert hc.merge.tobytes() == first[10] and hc.height.tobytes() == first[11]
    h = ctypes.c_void_p()
    assert lib().scde_ctx_create(0, ctypes.byref(h)) == 0  # and a third explicit one can still be made
    lib().scde_ctx_destroy(h)
