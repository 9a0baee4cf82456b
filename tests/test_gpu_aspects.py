"""GPU tests of PAGODA's aspect redundancy reduction (csrc/aspects.hip, scde_amd/aspects.py)
against the CPU restatement in tests/aspects_ref.py.

The tolerance rule (DESIGN.md sections 4.4, 4.6, 4.9): the GPU's maximum error against a
high-precision evaluation (mpmath at 40 digits or more, or np.longdouble) is at most 16 x the
float64 restatement's own maximum error on the same case plus 8 ulp of the result's scale, and
NaN appears exactly where the restatement has NaN.  Every test prints the two figures before it
asserts.
"""
import functools

import numpy as np
import pytest

import aspects_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    from scde_amd import aspects
    return aspects


@pytest.fixture()
def dev(A):
    from scde_amd import api
    d = A._Dev(api.default_context())
    yield d
    d.free()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_rule(got, exact, ref64, what, scale=None):
    """The tolerance rule on arrays; exact may be longdouble."""
    got = np.asarray(got, np.float64)
    ref64 = np.asarray(ref64, np.float64)
    exact = np.asarray(exact)
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern differs from the restatement's"
    ok = ~nan
    if not ok.any():
        return 0.0, 0.0
    e_gpu = float(np.abs(got.astype(np.longdouble) - exact)[ok].max())
    e_ref = float(np.abs(ref64.astype(np.longdouble) - exact)[ok].max())
    if scale is None:
        scale = float(np.abs(exact[ok]).max())
    print(f"{what}: gpu max err {e_gpu:.3g}, restatement's own {e_ref:.3g}, bar {R.bar(e_ref, scale):.3g}")
    assert e_gpu <= R.bar(e_ref, scale), (what, e_gpu, e_ref, scale)
    return e_gpu, e_ref


# ------------------------------------------------------------------ 1. the renormalisation
def grid_pairs():
    return [(s * r, n) for n in R.GRID_N for r in R.GRID_R for s in (1.0, -1.0)]


EXACT_R = [(0.3, 0), (0.3, 1), (-0.3, 2), (1.0, 50), (-1.0, 50), (float("nan"), 50), (1.0, 2)]


def gpu_renorm(dev, r, n, target=100.0):
    m = r.shape[0]
    rd = dev.put(np.asfortranarray(r, dtype=np.float64))
    nd = dev.put(np.asfortranarray(n, dtype=np.int32))
    cd = dev.alloc(8 * m * m)
    from scde_amd._lib import check
    check(dev.L.scde_t_renorm_dev(dev.ctx.handle, rd, nd, m, float(target), cd))
    return dev.get(cd, (m, m))


@functools.lru_cache(maxsize=None)
def renorm_refs():
    """Per grid pair: (exact, float64 restatement, the restatement's log p); computed once."""
    return {(r, n): (R.t_renorm_exact(abs(r), n) * np.sign(r) if r else r, R.t_renorm64(r, n), R.t_renorm_logp(r, n))
            for r, n in grid_pairs()}


@pytest.mark.parametrize("m", [2, 3, 64, 65, 130])
def test_renorm_grid(dev, m):
    pairs = grid_pairs() + EXACT_R
    rng = np.random.default_rng(m)
    iu = np.triu_indices(m, 1)
    npairs = len(iu[0])
    if npairs >= len(pairs):
        pick = np.concatenate([np.arange(len(pairs)), rng.integers(0, len(pairs), npairs - len(pairs))])
        pick = rng.permutation(pick)
    else:  # the small matrices walk the list in several calls
        pick = None
    refs = renorm_refs()
    e_gpu = e_ref = e_deep = 0.0
    calls = [pick] if pick is not None else [np.arange(s, s + npairs) % len(pairs)
                                             for s in range(0, len(pairs), npairs)]
    for pk in calls:
        r = np.eye(m)
        n = np.zeros((m, m), np.int32)
        r[iu] = [pairs[i][0] for i in pk]
        n[iu] = [pairs[i][1] for i in pk]
        # what lies below the diagonal is not read
        r[(iu[1], iu[0])] = 7.0
        n[(iu[1], iu[0])] = 5
        cr = gpu_renorm(dev, r, n)
        assert np.array_equal(bits(cr), bits(cr.T)), "the mirrored output is not symmetric bit for bit"
        assert np.array_equal(np.diag(cr), np.ones(m))
        for (i, j), p in zip(zip(*iu), pk):
            rr, nn = pairs[p]
            g = cr[i, j]
            if (rr, nn) in refs:
                ex, f64, lp = refs[(rr, nn)]
                if rr == 0:
                    assert g == 0
                elif np.isfinite(lp):
                    e_gpu, e_ref = max(e_gpu, abs(g - ex)), max(e_ref, abs(f64 - ex))
                else:
                    e_deep = max(e_deep, abs(g - ex))
            else:  # the exact-r cases
                assert bits(np.array([g]))[0] == bits(np.array([rr]))[0], (rr, nn, g)
    print(f"renorm m={m}: gpu max err {e_gpu:.3g}, restatement's own {e_ref:.3g}, deep points {e_deep:.3g}, "
          f"bar {R.bar(e_ref):.3g}")
    assert e_gpu <= R.bar(e_ref)
    assert e_deep <= R.bar(e_ref)


def test_renorm_deep_tail_and_the_deviation(dev):
    """n = 40000 at r = 0.9 has log p near -33000: the restatement's p has underflowed, the
    log-space map has not.  On the negative side R's double evaluation keeps r; the odd map is
    used instead."""
    r = np.eye(3)
    n = np.zeros((3, 3), np.int32)
    r[0, 1], n[0, 1] = 0.9, 40000
    r[0, 2], n[0, 2] = -0.9, 2000
    r[1, 2], n[1, 2] = 0.9, 2000
    cr = gpu_renorm(dev, r, n)
    assert not np.isfinite(R.t_renorm_logp(0.9, 40000))
    assert abs(cr[0, 1] - R.t_renorm_exact(0.9, 40000)) <= R.bar(renorm_grid_ref_err())
    assert R.t_renorm_R(-0.9, 2000) == -0.9            # R falls back to r here
    assert cr[0, 2] == -cr[1, 2] and cr[0, 2] < -0.999  # the odd map does not
    assert abs(cr[1, 2] - R.t_renorm_exact(0.9, 2000)) <= R.bar(renorm_grid_ref_err())


def renorm_grid_ref_err():
    return max(abs(f64 - ex) for ex, f64, lp in renorm_refs().values() if np.isfinite(lp))


def test_renorm_same_ndf_and_host_form(A):
    """n = target_ndf gives r back to rounding; the host form equals the resident one."""
    from scde_amd import api
    from scde_amd._lib import ScdeError, check, lib
    rs = np.array([1e-8, 0.1, -0.5, 0.9, 0.999999])
    m = 6
    r = np.eye(m, order="F")
    n = np.zeros((m, m), np.int32, order="F")
    r[0, 1:] = rs
    n[0, 1:] = 100
    cr = np.zeros((m, m), order="F")
    check(lib().scde_t_renorm_host(None, api._p(r), api._p(n), m, 100.0, api._p(cr)))
    print("n = target_ndf: max |cr - r| / |r| =", np.max(np.abs(cr[0, 1:] - rs) / np.abs(rs)))
    assert np.all(np.abs(cr[0, 1:] - rs) <= 8 * R.U * np.abs(rs))
    n[0, 1:] = 102
    check(lib().scde_t_renorm_host(None, api._p(r), api._p(n), m, 102.0, api._p(cr)))
    assert np.all(np.abs(cr[0, 1:] - rs) <= 8 * R.U * np.abs(rs))
    with pytest.raises(ScdeError, match="target_ndf"):
        check(lib().scde_t_renorm_host(None, api._p(r), api._p(n), m, 2.0, api._p(cr)))


# ------------------------------------------------------------------ 2. distances
def gpu_distances(dev, x, w, cr, ab, power):
    from scde_amd._lib import check
    m, ncells = x.shape
    xd, wd = dev.put(np.ascontiguousarray(x)), dev.put(np.ascontiguousarray(w))
    crd = dev.put(np.asfortranarray(cr)) if cr is not None else None
    out = dev.alloc(8 * m * m)
    check(dev.L.scde_aspect_distance_dev(dev.ctx.handle, xd, ncells, m, crd, int(ab), float(power), out))
    d = dev.get(out, (m, m))
    check(dev.L.scde_matWCorr_distance_dev(dev.ctx.handle, xd, wd, ncells, m, int(ab), out))
    return d, dev.get(out, (m, m))


@pytest.mark.parametrize("ncells", [2, 3, 63, 65, 257])
@pytest.mark.parametrize("m", [2, 3, 63, 64, 65, 130])
def test_distances(dev, m, ncells):
    rng = np.random.default_rng(1000 * m + ncells)
    x = rng.normal(size=(m, ncells))
    w = rng.uniform(0.2, 1.0, size=(m, ncells))
    cr = rng.uniform(-1, 1, size=(m, m))
    cr = np.triu(cr, 1) + np.triu(cr, 1).T + np.eye(m)
    ld = np.longdouble
    for ab in (True, False):
        wex, w64 = R.matwcorr_distance(x, w, ab, ld), R.matwcorr_distance(x, w, ab)
        for power, use_cr in ((1, True), (4, True), (1, False)):
            c = cr if use_cr else None
            d, dwc = gpu_distances(dev, x, w, c, ab, power)
            assert np.array_equal(bits(d), bits(d.T)) and not np.diag(d).any()
            check_rule(d, R.aspect_distance(x, c, ab, power, ld), R.aspect_distance(x, c, ab, power),
                       f"aspect distance m={m} cells={ncells} abs={ab} power={power} cr={use_cr}", scale=1.0)
        assert np.array_equal(bits(dwc), bits(dwc.T)) and not np.diag(dwc).any()
        check_rule(dwc, wex, w64, f"matWCorr distance m={m} cells={ncells} abs={ab}", scale=1.0)


def test_constant_row_is_nan_and_hclust_refuses_it(dev, A):
    from scde_amd import cluster
    from scde_amd._lib import ScdeError
    rng = np.random.default_rng(5)
    x = rng.normal(size=(7, 33))
    x[3] = 0.1
    d, _ = gpu_distances(dev, x, np.ones_like(x), None, True, 1)
    ref = R.aspect_distance(x, None, True)
    assert np.array_equal(np.isnan(d), np.isnan(ref)) and np.isnan(d[3, 0]) and d[3, 3] == 0
    with pytest.raises(ScdeError, match="non-finite distance"):
        cluster.hclust(d, "complete")
    tam = {"xv": x, "xvw": np.ones_like(x), "names": [f"#PC1# s{i}" for i in range(7)]}
    with pytest.raises(ScdeError, match="non-finite distance"):
        A.pagoda_reduce_redundancy(tam, weighted_correlation=False)


# ------------------------------------------------------------------ 3. collapse
SIZES = (1, 2, 3, 17, 64, 65)


def planted_rows(rng, k, ncells):
    """k rows sharing one pattern: sigma_1 / sigma_2 of the centred block is far above 2."""
    s = rng.normal(size=ncells)
    a = rng.uniform(0.5, 1.5, size=k)
    return np.outer(a, s) + 0.05 * rng.normal(size=(k, ncells)) + rng.normal(size=(k, 1))


def gpu_collapse(dev, x, w, ct, names, scale=True, pick_top=False, seed=1):
    m, ncells = x.shape
    from scde_amd import aspects
    dd, dw, rn, members, info = aspects._collapse_dev(dev, dev.put(np.ascontiguousarray(x)),
                                                      dev.put(np.ascontiguousarray(w)), ncells, m, ct, names, scale,
                                                      pick_top, seed)
    k = len(rn)
    return dev.get(dd, (k, ncells), "C"), dev.get(dw, (k, ncells), "C"), rn, info


@pytest.mark.parametrize("ncells", [2, 5, 65, 257])
def test_collapse_sizes(dev, ncells):
    rng = np.random.default_rng(40 + ncells)
    sizes = SIZES + ((9,) if ncells == 5 else ())
    blocks = [planted_rows(rng, k, ncells) for k in sizes]
    x = np.vstack(blocks)
    m = x.shape[0]
    perm = rng.permutation(m)  # the members of a cluster are scattered over the rows
    ct = np.empty(m, np.int32)
    ct[perm] = np.repeat(np.arange(1, len(sizes) + 1), sizes)
    xs = np.empty_like(x)
    xs[perm] = x
    w = rng.uniform(0.2, 1.0, size=(m, ncells))
    names = [f"#PC1# set{i}" for i in range(m)]
    d, dw, rn, info = gpu_collapse(dev, xs, w, ct, names)
    ref = R.collapse(xs, w, ct, names)
    ex = R.collapse(xs, w, ct, names, exact=True)
    assert rn == ref["names"]
    assert [names[t] for t in info["top"]] == ref["names"]
    assert not info["fallback"].any()
    for c, k in enumerate(sizes):
        if k > 1:
            assert ref["gap"][c] >= 2, (k, ref["gap"][c])  # the bound on a singular vector needs the gap
            assert info["orientation"][c] >= 0
            assert abs(info["orientation"][c] - ref["orientation"][c]) < 1e-9
        else:
            assert np.array_equal(d[c], xs[ct == c + 1][0])
        check_rule(d[c], ex["d"][c], ref["d"][c], f"collapse cells={ncells} k={k} pattern")
        check_rule(dw[c], ex["w"][c], ref["w"][c], f"collapse cells={ncells} k={k} weights")


def test_collapse_pick_top_and_unscaled(dev):
    rng = np.random.default_rng(7)
    x = np.vstack([planted_rows(rng, 4, 33), planted_rows(rng, 3, 33)])
    x[5] = x[4]  # two rows of equal variance: the first maximum is taken
    w = rng.uniform(0.2, 1.0, size=x.shape)
    ct = np.array([1, 1, 1, 1, 2, 2, 2])
    names = [f"#PC1# s{i}" for i in range(7)]
    d, dw, rn, info = gpu_collapse(dev, x, w, ct, names, pick_top=True)
    ref = R.collapse(x, w, ct, names, pick_top=True)
    assert rn == ref["names"] and np.array_equal(d, ref["d"])
    d, dw, rn, info = gpu_collapse(dev, x, w, ct, names, scale=False)
    ref, ex = R.collapse(x, w, ct, names, scale=False), R.collapse(x, w, ct, names, scale=False, exact=True)
    for c in range(2):
        check_rule(d[c], ex["d"][c], ref["d"][c], f"unscaled pattern {c}")


def lib_rnorm(seed, n):
    from scde_amd import api
    from scde_amd._lib import check, lib
    from scde_amd.pagoda import RState
    st = RState(seed)
    out = np.empty(n)
    check(lib().scde_r_norm_rand(api._p(st.w), n, api._p(out)))
    return out


def test_collapse_fallback_rows_follow_the_seeded_stream(dev):
    rng = np.random.default_rng(9)
    ncells = 21
    x = np.vstack([np.full((3, ncells), 2.0),       # an all-equal cluster
                   planted_rows(rng, 3, ncells),
                   np.zeros((2, ncells))])            # two identical constant rows
    w = rng.uniform(0.2, 1.0, size=x.shape)
    ct = np.array([1, 1, 1, 2, 2, 2, 3, 3])
    names = [f"#PC1# s{i}" for i in range(8)]
    for seed in (1, 5):
        d, dw, rn, info = gpu_collapse(dev, x, w, ct, names, seed=seed)
        z = np.abs(lib_rnorm(seed, 2 * ncells)) * 1e-6
        assert list(info["fallback"]) == [1, 0, 1]
        assert np.array_equal(bits(d[0]), bits(z[:ncells]))
        assert np.array_equal(bits(d[2]), bits(z[ncells:]))  # a later fallback cluster continues the stream
        assert rn[0] == names[0] and rn[2] == names[6]
    # the restatement's stream (numpy's MT19937 behind R's seeding) is the library's
    assert np.allclose(lib_rnorm(5, 40), R.r_rnorm(5, 40), rtol=1e-13, atol=0)


def test_collapse_orientation_not_finite_raises(A):
    # a pattern that is not finite leaves cor() NA, where R stops; a singleton passes through
    rng = np.random.default_rng(2)
    x = planted_rows(rng, 4, 12)
    x[1, 3] = np.inf
    names = [f"#PC1# s{i}" for i in range(4)]
    with pytest.raises(ValueError, match="not finite"):
        A.collapse_aspect_clusters(x, np.ones_like(x), [1, 1, 1, 2], names)
    out = A.collapse_aspect_clusters(x, np.ones_like(x), [1, 2, 1, 1], names)
    assert np.array_equal(out["d"][1], x[1])


def test_collapse_second_call_shows_no_stale_value(A):
    from scde_amd import api
    rng = np.random.default_rng(11)
    big = np.vstack([planted_rows(rng, 40, 120), planted_rows(rng, 30, 120)])
    small = np.vstack([planted_rows(rng, 3, 17), planted_rows(rng, 1, 17), planted_rows(rng, 5, 17)])
    ctb = np.repeat([1, 2], [40, 30])
    cts = np.repeat([1, 2, 3], [3, 1, 5])
    nb, ns = [f"#PC1# b{i}" for i in range(70)], [f"#PC1# s{i}" for i in range(9)]
    A.collapse_aspect_clusters(big, np.ones_like(big), ctb, nb)
    second = A.collapse_aspect_clusters(small, np.ones_like(small), cts, ns)
    ctx = api.Context(0)
    fresh = A.collapse_aspect_clusters(small, np.ones_like(small), cts, ns, ctx=ctx)
    assert second["names"] == fresh["names"]
    assert np.array_equal(bits(second["d"]), bits(fresh["d"])) and np.array_equal(bits(second["w"]), bits(fresh["w"]))


def test_collapse_alone_equals_inside_a_batch_of_300(dev):
    rng = np.random.default_rng(13)
    ncells = 40
    sizes = rng.integers(1, 6, size=300)
    sizes[137] = 23
    x = np.vstack([planted_rows(rng, int(k), ncells) for k in sizes])
    w = rng.uniform(0.2, 1.0, size=x.shape)
    ct = np.repeat(np.arange(1, 301), sizes)
    names = [f"#PC1# s{i}" for i in range(len(ct))]
    d, dw, rn, info = gpu_collapse(dev, x, w, ct, names)
    sel = ct == 138
    d1, dw1, rn1, info1 = gpu_collapse(dev, x[sel], w[sel], np.ones(23, np.int32), [n for n, s in zip(names, sel) if s])
    assert rn1[0] == rn[137]
    assert np.array_equal(bits(d1[0]), bits(d[137])) and np.array_equal(bits(dw1[0]), bits(dw[137]))
    assert info1["orientation"][0] == info["orientation"][137]


def test_collapse_argument_errors(dev):
    from scde_amd import api
    from scde_amd._lib import ScdeError, check
    x = np.zeros((3, 4))
    xd = dev.put(x)
    out = dev.alloc(8 * 4 * 2)
    top, fb, oc = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2)

    def call(off, idx, ncells=4, m=3):
        off, idx = np.array(off, np.int64), np.array(idx, np.int32)
        check(dev.L.scde_collapse_aspects_dev(dev.ctx.handle, xd, xd, ncells, m, len(off) - 1, api._p(off),
                                              api._p(idx), 1, 0, out, out, api._p(top), api._p(fb), api._p(oc)))
    with pytest.raises(ScdeError, match=r"cluster 1: row index 3 outside \[0, 3\)"):
        call([0, 1, 3], [0, 1, 3])
    with pytest.raises(ScdeError, match="cluster 0 has no rows"):
        call([0, 0, 3], [0, 1, 2])
    with pytest.raises(ScdeError, match="at least 2 cells"):
        call([0, 1, 3], [0, 1, 2], ncells=1)


# ------------------------------------------------------------------ 4. end to end
def planted_aspects(seed=3, ngroups=38, ncells=96):
    """A synthetic pwpca with planted duplicate sets: per group a gene set of its own (no gene
    is shared between groups) and a cell pattern orthogonal to every other group's; within a
    group three near-duplicates (the same genes with slightly different loadings, one of them
    with two genes exchanged for new ones) whose patterns differ by a little noise.  Six groups
    also carry a second component.  About 120 aspects x 96 cells."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(np.column_stack([np.ones(ncells), rng.normal(size=(ncells, 2 * ngroups))]))
    base = q[:, 1:].T * np.sqrt(ncells)                     # orthogonal, zero-mean patterns
    pwpca, names, xv = {}, [], []
    gene = 0
    for g in range(ngroups):
        ng = int(rng.integers(12, 30))
        genes = [f"g{gene + i}" for i in range(ng)]
        gene += ng + 2
        load = rng.normal(size=ng)
        amp = 1.0 + 0.05 * g
        for v in range(3):
            gs = list(genes)
            if v == 2:
                gs[-2:] = [f"g{gene - 2}", f"g{gene - 1}"]
            order = rng.permutation(ng)                     # rotation rows in an order of their own
            rot = (load + 0.03 * rng.normal(size=ng))[:, None]
            pat = amp * (base[g] + 0.03 * rng.normal(size=ncells))
            key = f"GO:{g:04d}.{v} set # {g}"               # (a set name may itself contain '#')
            if v == 0 and g < 6:
                rot = np.column_stack([rot[:, 0], rng.normal(size=ng)])
                names.append(f"#PC2# {key}")
                xv.append(0.7 * amp * base[ngroups + g])
            pwpca[key] = {"xp": {"rotation": rot[order], "rotation_names": [gs[i] for i in order]}}
            names.append(f"#PC1# {key}")
            xv.append(pat)
    order = rng.permutation(len(names))
    xv = np.array(xv)[order]
    names = [names[i] for i in order]
    xvw = rng.uniform(0.8, 1.0, size=xv.shape)
    return {"xv": xv, "xvw": xvw, "names": names, "df": 7.0}, pwpca


def assert_separated(dist, h):
    off = dist[np.triu_indices_from(dist, 1)]
    assert np.all((off < h / 4) | (off > 4 * h)), "the planted inputs do not keep the cut clear of the threshold"
    assert (off < h / 4).any() and (off > 4 * h).any()


def exact_patterns(tam, ct):
    return R.collapse(tam["xv"], tam["xvw"], ct, list(tam["names"]), exact=True)


def test_reduce_loading_redundancy_end_to_end(A):
    tam, pwpca = planted_aspects()
    names = tam["names"]
    m = len(names)
    assert 110 <= m <= 130
    ref = R.reduce_loading_redundancy(tam, pwpca)
    assert_separated(ref["distance"], 0.01)
    got = A.pagoda_reduce_loading_redundancy(tam, pwpca, return_details=True)
    # the distance: loadings in longdouble, the renormalisation at 50 digits, the rest in longdouble
    ld = np.longdouble
    rl, nl = R.pl_cor(R.loading_lists(pwpca, names)[1], ld)
    cr_ex = R.t_renorm_matrix(rl, nl, 100, R.t_renorm_exact)
    check_rule(got["distance"], R.aspect_distance(tam["xv"], cr_ex, True, 4, ld), ref["distance"],
               "loading redundancy distance", scale=1.0)
    assert np.array_equal(got["ct"], ref["ct"])
    assert got["names"] == ref["names"] and got["cnam"] == ref["cnam"]
    assert got["df"] == 7.0
    assert len(got["names"]) < m
    ex = exact_patterns(tam, ref["ct"])
    for c in range(len(ref["names"])):
        check_rule(got["xv"][c], ex["d"][c], ref["xv"][c], f"pattern {c}")
        check_rule(got["xvw"][c], ex["w"][c], ref["xvw"][c], f"weights {c}")
    # the distance helper on its own
    d = A.pathway_pc_correlation_distance(pwpca, names, target_ndf=100)
    pclc_ex = 1 - np.abs(cr_ex.astype(ld))
    pclc_ex[pclc_ex < 0] = 0
    np.fill_diagonal(pclc_ex, 0)
    check_rule(d, pclc_ex, R.pc_distance(pwpca, names, 100), "pathway.pc.correlation.distance", scale=1.0)
    d0 = A.pathway_pc_correlation_distance(pwpca, names)
    assert np.max(np.abs(d0 - R.pc_distance(pwpca, names))) <= 8 * R.U


@pytest.mark.parametrize("weighted,ab", [(True, False), (True, True), (False, False), (False, True)])
def test_reduce_redundancy_end_to_end(A, weighted, ab):
    tam, _ = planted_aspects()
    ref = R.reduce_redundancy(tam, 0.2, weighted, ab)
    assert_separated(ref["distance"], 0.2)
    got = A.pagoda_reduce_redundancy(tam, weighted_correlation=weighted, abs=ab, return_details=True)
    ld = np.longdouble
    dex = R.matwcorr_distance(tam["xv"], tam["xvw"], ab, ld) if weighted else R.aspect_distance(tam["xv"], None, ab,
                                                                                               dtype=ld)
    check_rule(got["distance"], dex, ref["distance"], f"redundancy distance weighted={weighted} abs={ab}", scale=1.0)
    assert np.array_equal(got["ct"], ref["ct"])
    assert got["names"] == ref["names"] and got["cnam"] == ref["cnam"]
    ex = exact_patterns(tam, ref["ct"])
    order = R.variance_order(np.array(ex["d"], np.float64))
    for c, o in enumerate(order):
        check_rule(got["xv"][c], ex["d"][o], ref["xv"][c], f"pattern {c}")
        check_rule(got["xvw"][c], ex["w"][o], ref["xvw"][c], f"weights {c}")
    v = np.var(got["xv"], axis=1, ddof=1)
    assert np.all(np.diff(v) <= 0)


@pytest.mark.parametrize("method", ["single", "average", "mcquitty", "ward.D", "ward.D2"])
def test_other_linkages_are_accepted(A, method):
    """The cut of the three linkages whose heights are distances equals scipy's on the planted
    inputs; the two Ward linkages (heights on another scale) run."""
    tam, pwpca = planted_aspects()
    got = A.pagoda_reduce_redundancy(tam, cluster_method=method, return_details=True)
    assert got["clustering"].method == method
    if not method.startswith("ward"):
        scipy_name = {"mcquitty": "weighted"}.get(method, method)
        ref = R.reduce_redundancy(tam, 0.2, True, False, method=scipy_name)
        assert np.array_equal(got["ct"], ref["ct"]) and got["names"] == ref["names"]
    got = A.pagoda_reduce_loading_redundancy(tam, pwpca, cluster_method=method)
    assert len(got["names"]) == len(got["cnam"]) <= len(tam["names"])


def test_reduce_redundancy_trim_top_and_the_chain(A):
    from scde_amd import cluster
    tam, pwpca = planted_aspects()
    tam["cnam"] = {n: [n + "/a", n + "/b"] for n in tam["names"]}
    ref = R.reduce_redundancy(tam, 0.2, True, False, top=5, trim=1.1 / 96)
    got = A.pagoda_reduce_redundancy(tam, top=5, trim=1.1 / 96)
    assert got["xv"].shape == (5, 96) and got["names"] == ref["names"] and got["cnam"] == ref["cnam"]
    full = R.reduce_redundancy(tam, 0.2, True, False)
    ex = exact_patterns(tam, full["ct"])
    exw = R.winsorize_rows(np.array(ex["d"], np.float64), 1.1 / 96)  # (the exact patterns rounded to float64 first)
    order = R.variance_order(exw, 5)
    for c, o in enumerate(order):
        check_rule(got["xv"][c], exw[o].astype(np.longdouble), ref["xv"][c], f"trimmed pattern {c}")
    # first function into the second, and the result into pagoda.cluster.cells
    t1 = A.pagoda_reduce_loading_redundancy(tam, pwpca)
    t2 = A.pagoda_reduce_redundancy(t1, distance_threshold=0.9)
    assert set(t2["cnam"]) == set(t2["names"]) and sum(len(v) for v in t2["cnam"].values()) == 2 * len(tam["names"])
    rng = np.random.default_rng(1)
    genes = [f"g{i}" for i in range(30)]
    varinfo = {"mat": rng.normal(size=(30, 96)), "matw": rng.uniform(0.5, 1, size=(30, 96)), "genes": genes,
               "arv": np.full(30, 2.0)}
    t2["gw"] = {g: 1.0 for g in genes}
    hc = cluster.pagoda_cluster_cells(t2, varinfo, include_aspects=True)
    assert sorted(hc.order) == list(range(1, 97))
