"""CPU restatement of PAGODA's aspect redundancy reduction, for tests/test_aspects.py and
tests/test_gpu_aspects.py: plain numpy / scipy / mpmath, written from R/functions.R:2490-2526,
2559-2610, 5126-5198 and src/pagoda.cpp:41-117.  Nothing here touches the library.

Every numerical function takes ``dtype``: ``np.float64`` is the float64 restatement, whose own
error the tolerance rule scales; ``np.longdouble`` is the high-precision evaluation where a
formula allows one.  The Student-t renormalisation has a 50-digit mpmath evaluation instead
(``t_renorm_exact``), and the first principal component one refined by mpmath power steps
(``pc1_exact``).
"""
import functools
import re

import numpy as np

U = 2.0 ** -52          # ulp(1)
_PC = re.compile(r"^#PC(\d+)# ")

GRID_N = (3, 4, 5, 12, 101, 102, 2000, 40000)
GRID_R = (0.0, 1e-300, 1e-8, 0.1, 0.5, 0.9, 0.999999, 1 - 2.0 ** -53)


def bar(ref_err, scale=1.0):
    """The tolerance rule (DESIGN.md sections 4.4, 4.6): 16 x the float64 restatement's own
    maximum error on the case plus 8 ulp of the result's scale."""
    return 16.0 * ref_err + 8.0 * U * scale


# ------------------------------------------------------------------ names, loading lists
def parse_names(names):
    out = []
    for nam in names:
        m = _PC.match(nam)
        out.append((nam[m.end():], int(m.group(1))))
    return out


def loading_lists(pcc, names):
    parsed = parse_names(names)
    rotn = []
    seen = set()
    for pnam, _ in parsed:
        for g in pcc[pnam]["xp"]["rotation_names"]:
            if g not in seen:
                seen.add(g)
                rotn.append(g)
    pos = {g: i for i, g in enumerate(rotn)}
    pl = []
    for pnam, pn in parsed:
        rt = np.asarray(pcc[pnam]["xp"]["rotation"], np.float64)[:, pn - 1]
        mi = np.array([pos[g] for g in pcc[pnam]["xp"]["rotation_names"]])
        mo = np.argsort(mi, kind="stable")
        pl.append((mi[mo], (rt - rt.mean())[mo]))
    return rotn, pl


def pl_cor(pl, dtype=np.float64):
    """plSemicompleteCor2 (src/pagoda.cpp:67-117): r over the shared genes, n the union sizes."""
    m = len(pl)
    r = np.eye(m, dtype=dtype)
    n = np.zeros((m, m), np.int64)
    for i in range(m):
        i1, v1 = pl[i][0], pl[i][1].astype(dtype)
        for j in range(i + 1, m):
            i2, v2 = pl[j][0], pl[j][1].astype(dtype)
            _, a, b = np.intersect1d(i1, i2, assume_unique=True, return_indices=True)
            l12 = l11 = l22 = dtype(0)
            for x, y in zip(v1[a], v2[b]):  # in the order of the first list, as the merge join runs
                l12 += y * x
                l11 += y * y
                l22 += x * x
            cv = l11 * l22
            if cv > 0:
                cv = l12 / np.sqrt(cv)
            r[i, j] = r[j, i] = cv
            n[i, j] = n[j, i] = len(i1) + len(i2) - len(a)
    return r, n


# ------------------------------------------------------------------ the renormalisation
def t_renorm_R(r, n, target_ndf=100):
    """R/functions.R:5148-5152 literally, in float64 (scipy's Student t): one pair."""
    from scipy.stats import t as st
    r = float(r)
    with np.errstate(all="ignore"):
        tv = r * np.sqrt((n - 2) / (1 - r * r)) if n - 2 >= 0 else np.nan
        z = st.logsf(tv, n - 2) if n > 2 else np.nan
        nr = st.isf(np.exp(z), target_ndf - 2)
        nr = nr / np.sqrt(target_ndf - 2 + nr * nr)
    return r if np.isnan(nr) else float(nr)


def _tail64(r, n):
    from scipy.special import betainc
    return float(betainc((n - 2) / 2, 0.5, (1 - r) * (1 + r)))


def t_renorm_logp(r, n):
    """The restatement's log p at |r| (-inf once p has underflowed, NaN for the exact cases)."""
    r = abs(float(r))
    if n <= 2 or not r < 1:
        return np.nan
    with np.errstate(all="ignore"):
        return float(np.log(0.5 * _tail64(r, n)))


def t_renorm64(r, n, target_ndf=100):
    """The float64 restatement of the contract in correlation space (scipy.special's regularised
    incomplete beta function and its inverse): 2 p = I_{1 - r^2}(nu / 2, 1/2) is matched when it
    is at most 1/2, its complement I_{r^2}(1/2, nu / 2) otherwise; sign(cr) = sign(r)."""
    from scipy.special import betainc, betaincinv
    r = float(r)
    x = abs(r)
    if n <= 2 or not x < 1 or x == 0:
        return r
    a, at = (n - 2) / 2, (target_ndf - 2) / 2
    F = _tail64(x, n)
    if F > 0.5:
        cr = np.sqrt(betaincinv(0.5, at, betainc(0.5, a, x * x)))
    else:
        cr = np.sqrt(1 - betaincinv(at, 0.5, F))
    return float(np.copysign(cr, r))


@functools.lru_cache(maxsize=None)
def t_renorm_exact(r, n, target_ndf=100):
    """The contract at 50 digits, rounded to float64: p = I_{1 - r^2}(nu / 2, 1/2) / 2 and |cr|
    solving I_{1 - cr^2}((target_ndf - 2) / 2, 1/2) / 2 = p, matched in log space on the smaller
    of the tail and the centre."""
    import mpmath as mp
    r = float(r)
    if n <= 2 or not abs(r) < 1 or r == 0:
        return r
    with mp.workdps(50):
        half = mp.mpf(1) / 2
        x = abs(mp.mpf(r))
        a, at = mp.mpf(n - 2) / 2, mp.mpf(target_ndf - 2) / 2
        F = mp.betainc(a, half, 0, 1 - x * x, regularized=True)
        if F > half:
            lG = mp.log(mp.betainc(half, a, 0, x * x, regularized=True))
            v0 = 2 * (lG + mp.log(mp.beta(at, half) / 2))
            v = mp.findroot(lambda v: mp.re(mp.log(mp.betainc(half, at, 0, mp.e ** v, regularized=True))) - lG, v0)
            cr = mp.e ** (v / 2)
        else:
            lF = mp.re(mp.log(F))
            u0 = min((lF + mp.log(at) + mp.log(mp.beta(at, half))) / at, mp.mpf(-1) / 1000)
            u = mp.findroot(lambda u: mp.re(mp.log(mp.betainc(at, half, 0, mp.e ** u, regularized=True))) - lF, u0)
            cr = mp.sqrt(1 - mp.e ** u)
        return float(mp.sign(r) * mp.re(cr))  # (betainc leaves imaginary dust of 1e-50)


def t_renorm_matrix(r, n, target_ndf, f=t_renorm64):
    """The matrix form: pairs above the diagonal transformed and mirrored, the diagonal kept."""
    m = r.shape[0]
    cr = np.array(r, dtype=np.float64)
    for j in range(m):
        for i in range(j):
            cr[i, j] = cr[j, i] = f(float(r[i, j]), int(n[i, j]), target_ndf)
    return cr


def pc_distance(pcc, names, target_ndf=None, f=t_renorm64):
    _, pl = loading_lists(pcc, names)
    r, n = pl_cor(pl)
    cr = t_renorm_matrix(r, n, target_ndf, f) if target_ndf is not None else r
    d = 1 - np.abs(cr)
    d[d < 0] = 0
    np.fill_diagonal(d, 0)
    return d


# ------------------------------------------------------------------ distances
def cor_rows(x, dtype=np.float64):
    """cor(t(x)) (two-pass Pearson); NaN where a row is constant."""
    x = np.asarray(x, dtype)
    xc = x - x.mean(axis=1, keepdims=True)
    ss = (xc * xc).sum(axis=1)
    const = np.all(x == x[:, :1], axis=1)
    with np.errstate(all="ignore"):
        c = (xc @ xc.T) / np.sqrt(np.outer(ss, ss))
    c[const, :] = np.nan
    c[:, const] = np.nan
    return c


def aspect_distance(x, cr=None, ab=True, power=4, dtype=np.float64):
    """scde_aspect_distance_dev's contract (R/functions.R:2491-2499, 2571-2575)."""
    c = cor_rows(x, dtype)
    with np.errstate(all="ignore"):
        if cr is None:
            d = 1 - np.abs(c) if ab else 1 - c
        else:
            cda = np.abs(c) if ab else np.where(c < 0, dtype(0), c)
            cda = 1 - cda
            pclc = 1 - np.abs(np.asarray(cr, dtype))
            pclc = np.where(pclc < 0, dtype(0), pclc)
            d = (1 - np.sqrt((1 - pclc) * (1 - cda))) ** dtype(power)
    np.fill_diagonal(d, 0)
    return d


def matwcorr_distance(x, w, ab=False, dtype=np.float64):
    """1 - matWCorr(t(x), t(w)) (src/pagoda.cpp:41-65), both triangles, zero diagonal."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    m = x.shape[0]
    d = np.zeros((m, m), dtype)
    for i in range(m):
        for j in range(i + 1, m):
            jw = np.sqrt(w[i] * w[j])
            jw = jw / jw.sum()
            a, b = x[i] - (x[i] * jw).sum(), x[j] - (x[j] * jw).sum()
            with np.errstate(all="ignore"):
                c = (a * b * jw).sum() / np.sqrt((a * a * jw).sum() * (b * b * jw).sum())
            d[i, j] = d[j, i] = 1 - abs(c) if ab else 1 - c
    return d


# ------------------------------------------------------------------ clustering
def cut_complete(d, h, method="complete"):
    """cutree(hclust(as.dist(d), method), h = h): labels numbered by first observation."""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    lab = fcluster(linkage(squareform(np.asarray(d, np.float64), checks=False), method=method), t=h,
                   criterion="distance")
    first = {}
    return np.array([first.setdefault(v, len(first) + 1) for v in lab], np.int32)


# ------------------------------------------------------------------ collapse
def r_var(x):
    return np.var(x, ddof=1)


def pc1_exact(rows):
    """(v1, X v1) for X the k x C rows transposed with each column centred, all in 40-digit
    mpmath from the float64 rows: numpy's top right singular vector refined by six power steps.
    Returned as longdouble arrays; the sign is numpy's."""
    import mpmath as mp
    rows = np.asarray(rows, np.float64)
    k, C = rows.shape
    v = np.linalg.svd((rows - rows.mean(axis=1, keepdims=True)).T, full_matrices=False)[2][0]
    with mp.workdps(40):
        R = [[mp.mpf(float(t)) for t in row] for row in rows]
        R = [[t - mp.fsum(row) / C for t in row] for row in R]       # R[i][c]: X[c, i]
        vm = [mp.mpf(float(t)) for t in v]
        for _ in range(6):
            w = [mp.fsum(R[i][c] * vm[i] for i in range(k)) for c in range(C)]
            vm = [mp.fsum(R[i][c] * w[c] for c in range(C)) for i in range(k)]
            nrm = mp.sqrt(mp.fsum(t * t for t in vm))
            vm = [t / nrm for t in vm]
        sc = [mp.fsum(R[i][c] * vm[i] for i in range(k)) for c in range(C)]
        ld = np.longdouble

        def down(vals):
            return np.array([ld(float(t)) + ld(float(t - mp.mpf(float(t)))) for t in vals], ld)
        return down(vm), down(sc)


def collapse_cluster(rows, dtype=np.float64, scale=True, pick_top=False, exact=False):
    """One cluster of collapse.aspect.clusters: (pattern or None for a fallback, top row,
    orientation correlation or None, sigma_1 / sigma_2 or None).  rows: k x C.  With ``exact`` the
    principal component is ``pc1_exact``'s and the rest runs in longdouble."""
    rows = np.asarray(rows, np.float64)
    k, C = rows.shape
    var = np.array([r_var(r.astype(dtype)) for r in rows])
    top = int(np.argmax(var))
    if k == 1:
        return rows[0].astype(dtype), 0, None, None
    if pick_top:
        return rows[top].astype(dtype), top, None, None
    mu = rows.astype(np.longdouble).mean(axis=1) if exact else rows.astype(dtype).mean(axis=1)
    X = (rows.astype(mu.dtype) - mu[:, None]).T  # C x k
    s = np.linalg.svd(X.astype(np.float64), compute_uv=False)
    gap = s[0] / s[1] if len(s) > 1 and s[1] > 0 else np.inf
    if exact:
        v1, xv = pc1_exact(rows)
        dtype = np.longdouble
    else:
        v1 = np.linalg.svd(X, full_matrices=False)[2][0]
        xv = X @ v1
    if np.abs(np.diff(xv)).sum() == 0:
        return None, top, None, gap
    a = (rows.astype(dtype) * np.abs(v1)[:, None]).mean(axis=0)
    xc, ac = xv - xv.mean(), a - a.mean()
    with np.errstate(all="ignore"):
        cor = (xc * ac).sum() / np.sqrt((xc * xc).sum() * (ac * ac).sum())
    if not np.isfinite(cor):
        raise ValueError("missing value where TRUE/FALSE needed")
    if cor < 0:
        xv, cor = -xv, -cor
    if scale:
        xv = xv * np.sqrt(var.max()) / np.sqrt(r_var(xv))
    if np.abs(xv).sum() == 0:
        return None, top, None, gap
    return xv, top, cor, gap


def collapse_weights(rows, wrows, dtype=np.float64):
    rows, wrows = np.asarray(rows, dtype), np.asarray(wrows, dtype)
    sd = np.sqrt(np.array([r_var(r) for r in rows]))
    w = (wrows * sd[:, None]).sum(axis=0)
    with np.errstate(all="ignore"):  # (rows of zero variance: 0 / 0, as in R)
        return w / w.sum()


def r_rnorm(seed, n):
    """The first n values of rnorm() after set.seed(seed) (Mersenne-Twister, Inversion): numpy's
    MT19937 seeded with R's scrambling, unif_rand's fix-up, the 2^27 combination, scipy's ppf."""
    from scipy.stats import norm
    s = np.uint32(seed)
    with np.errstate(over="ignore"):
        for _ in range(50):
            s = np.uint32(69069) * s + np.uint32(1)
        key = np.zeros(624, np.uint32)
        for j in range(625):
            s = np.uint32(69069) * s + np.uint32(1)
            if j > 0:
                key[j - 1] = s
    bg = np.random.MT19937()
    st = bg.state
    st["state"]["key"], st["state"]["pos"] = key, 624
    bg.state = st
    u = bg.random_raw(2 * n).astype(np.float64) * 2.3283064365386963e-10
    u = np.clip(u, 0.5 * 2.328306437080797e-10, 1 - 0.5 * 2.328306437080797e-10)
    big = 134217728.0
    return norm.ppf((np.floor(big * u[0::2]) + u[1::2]) / big)


def collapse(d, dw, ct, names, scale=True, pick_top=False, seed=1, dtype=np.float64, exact=False):
    """collapse.aspect.clusters: {"d", "w", "names", "fallback", "orientation", "gap"}."""
    d = np.asarray(d, np.float64)
    labels = np.unique(ct)
    out = {"d": [], "w": [], "names": [], "fallback": [], "orientation": [], "gap": []}
    nfb = 0
    for c in labels:
        ii = np.nonzero(np.asarray(ct) == c)[0]
        xv, top, cor, gap = collapse_cluster(d[ii], dtype, scale, pick_top, exact)
        if xv is None:
            nfb += 1
            xv = np.abs(r_rnorm(seed, nfb * d.shape[1])[-d.shape[1]:] * 1e-6)
        out["d"].append(xv)
        out["w"].append(collapse_weights(d[ii], np.asarray(dw)[ii], np.longdouble if exact else dtype))
        out["names"].append(names[ii[top]])
        out["fallback"].append(cor is None and len(ii) > 1 and not pick_top)
        out["orientation"].append(cor)
        out["gap"].append(gap)
    out["d"], out["w"] = np.array(out["d"]), np.array(out["w"])
    out["members"] = [np.nonzero(np.asarray(ct) == c)[0] for c in labels]
    return out


def cnam(tam_cnam, names, members, rn):
    out = {}
    for key, ii in zip(rn, members):
        xn = [names[i] for i in ii]
        out[key] = [g for n in xn for g in tam_cnam.get(n, [])] if tam_cnam is not None else xn
    return out


def winsorize_rows(x, trim):
    """winsorize.matrix (R/functions.R:1109-1115; src/pagoda.cpp:6-31)."""
    x = np.array(x, np.float64)
    n = x.shape[1]
    if trim > 0.5:
        trim = trim / n
    ntr = int(np.floor(n * trim + 0.5))
    if ntr == 0:
        return x
    for row in x:
        s = np.sort(row)
        lo, hi = s[ntr], s[n - ntr - 1]
        np.clip(row, lo, hi, out=row)
    return x


def variance_order(d, top=np.inf):
    var = np.var(np.asarray(d, np.float64), axis=1, ddof=1)
    return np.argsort(-var, kind="stable")[:int(min(len(var), top))]


def reduce_loading_redundancy(tam, pcc, threshold=0.01, power=4, ab=True, seed=1, method="complete"):
    names = list(tam["names"])
    pclc_cr = t_renorm_matrix(*pl_cor(loading_lists(pcc, names)[1]), 100)
    dist = aspect_distance(tam["xv"], pclc_cr, ab, power)
    ct = cut_complete(dist, threshold, method)
    col = collapse(tam["xv"], tam["xvw"], ct, names, seed=seed)
    return {"xv": col["d"], "xvw": col["w"], "names": col["names"], "distance": dist, "ct": ct,
            "cnam": cnam(tam.get("cnam"), names, col["members"], col["names"])}


def reduce_redundancy(tamr, threshold=0.2, weighted=True, ab=False, top=np.inf, trim=0, seed=1, method="complete"):
    names = list(tamr["names"])
    dist = (matwcorr_distance(tamr["xv"], tamr["xvw"], ab) if weighted
            else aspect_distance(tamr["xv"], None, ab))
    ct = cut_complete(dist, threshold, method)
    col = collapse(tamr["xv"], tamr["xvw"], ct, names, seed=seed)
    cn = cnam(tamr.get("cnam"), names, col["members"], col["names"])
    d = winsorize_rows(col["d"], trim) if trim > 0 else col["d"]
    vi = variance_order(d, top)
    rn = [col["names"][i] for i in vi]
    return {"xv": d[vi], "xvw": col["w"][vi], "names": rn, "distance": dist, "ct": ct,
            "cnam": {k: cn[k] for k in rn}}
