"""Plain numpy restatement of knn.error.models' per-cell mixture fit: this project's contract for
fit.nb2gth.mixture.model + get.compressed.v1.model (R/functions.R:3653-3660, 4058-4187,
3422-3434), stated in DESIGN.md section 4.15.  The reference of tests/test_knn_fit.py and
tests/test_gpu_knn_fit.py.

Everything is float64 and one cell at a time.  The densities are R's saddle-point forms
(nmath dbinom_raw / stirlerr / bd0), written out here, so that a log-likelihood can be compared
to 1e-12; the curve minimiser is the project's own projected Levenberg-Marquardt, step by step
as DESIGN.md states it (no SciPy minimiser).  Sums are numpy's; the GPU's fixed-order sums
differ from them by rounding.
"""
import collections
import functools
import math

import numpy as np
from scipy.special import gammaln

LOG_FAIL = math.log(0.1)  # fail.r
LN10 = math.log(10.0)
LN2PI = 1.837877066409345483560659472811
LNSQRT2PI = 0.918938533204672741780329736406
DBL_MIN = np.finfo(np.float64).tiny
BOX_LO = np.array([-100.0, -10.0, -100.0, -100.0, 0.1])
BOX_HI = np.array([10.0, 100.0, 100.0, 0.0, 20.0])
COLUMNS = ["conc.b", "conc.a", "fail.r", "corr.b", "corr.a", "corr.theta", "corr.ltheta.b", "corr.ltheta.t",
           "corr.ltheta.m", "corr.ltheta.s", "corr.ltheta.r", "conc.a2"]

OK, TOO_FEW, NO_WEIGHT, NOT_FINITE = 0, 1, 2, 3

#: genes visited by each kind of pass since the last clear() (tools/bench_knn_fit.py's work count)
PASSES = collections.Counter()

_SFERR = np.array([
    0.0, 0.1534264097200273452913848, 0.0810614667953272582196702, 0.0548141210519176538961390,
    0.0413406959554092940938221, 0.03316287351993628748511048, 0.02767792568499833914878929,
    0.02374616365629749597132920, 0.02079067210376509311152277, 0.01848845053267318523077934,
    0.01664469118982119216319487, 0.01513497322191737887351255, 0.01387612882307074799874573,
    0.01281046524292022692424986, 0.01189670994589177009505572, 0.01110455975820691732662991,
    0.010411265261972096497478567, 0.009799416126158803298389475, 0.009255462182712732917728637,
    0.008768700134139385462952823, 0.008330563433362871256469318, 0.007934114564314020547248100,
    0.007573675487951840794972024, 0.007244554301320383179543912, 0.006942840107209529865664152,
    0.006665247032707682442354394, 0.006408994188004207068439631, 0.006171712263039457647532867,
    0.005951370112758847735624416, 0.005746216513010115682023589, 0.005554733551962801371038690])


# ------------------------------------------------------------------ R's densities
def stirlerr(n):
    n = np.asarray(n, np.float64)
    out = np.empty_like(n)
    small = n <= 15.0
    nn = n + n
    tab = small & (nn == np.floor(nn))
    out[tab] = _SFERR[nn[tab].astype(np.int64)]
    lg = small & ~tab
    if lg.any():
        v = n[lg]
        out[lg] = gammaln(v + 1.0) - (v + 0.5) * np.log(v) + v - LNSQRT2PI
    big = ~small
    if big.any():
        v = n[big]
        v2 = v * v
        s0, s1, s2, s3, s4 = (0.083333333333333333333, 0.00277777777777777777778, 0.00079365079365079365079365,
                              0.000595238095238095238095238, 0.0008417508417508417508417508)
        r = np.where(v > 500, (s0 - s1 / v2) / v,
                     np.where(v > 80, (s0 - (s1 - s2 / v2) / v2) / v,
                              np.where(v > 35, (s0 - (s1 - (s2 - s3 / v2) / v2) / v2) / v,
                                       (s0 - (s1 - (s2 - (s3 - s4 / v2) / v2) / v2) / v2) / v)))
        out[big] = r
    return out


def bd0(x, m):
    """x log(x / m) + m - x, by its series where x is near m (R's bd0)."""
    x, m = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(m, np.float64))
    with np.errstate(all="ignore"):
        out = x * np.log(x / m) + m - x
        ser = np.abs(x - m) < 0.1 * (x + m)
    out = np.array(out)
    out[~np.isfinite(x) | ~np.isfinite(m) | (m == 0.0)] = np.nan
    if ser.any():
        xs, ms = x[ser], m[ser]
        v = (xs - ms) / (xs + ms)
        s = (xs - ms) * v
        ej = 2 * xs * v
        v = v * v
        done = np.abs(s) < DBL_MIN
        for j in range(1, 1000):
            ej = ej * v
            s1 = s + ej / (2 * j + 1)
            newly = ~done & (s1 == s)
            s = np.where(done, s, s1)
            done |= newly
            if done.all():
                break
        out[ser] = s
    return out


def dbinom_raw_log(x, n, p, q):
    """R's dbinom_raw(give_log = TRUE) for x > 0 and 0 < p <= 1 (what dnbinom_log sends it)."""
    x, n, p, q = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (x, n, p, q)))
    out = np.empty(x.shape)
    with np.errstate(all="ignore"):
        q0 = q == 0
        out[q0] = np.where(x[q0] == n[q0], 0.0, -np.inf)
        full = ~q0 & (x == n)
        if full.any():
            nf, pf, qf = n[full], p[full], q[full]
            out[full] = np.where(qf < 0.1, -bd0(nf, nf * pf) - nf * qf, nf * np.log(pf))
        rest = ~q0 & ~full
        if rest.any():
            xr, nr, pr, qr = x[rest], n[rest], p[rest], q[rest]
            lc = stirlerr(nr) - stirlerr(xr) - stirlerr(nr - xr) - bd0(xr, nr * pr) - bd0(nr - xr, nr * qr)
            lf = LN2PI + np.log(xr) + np.log1p(-xr / nr)
            out[rest] = lc - 0.5 * lf
    return out


def dnbinom_log(y, size, prob):
    """log dnbinom(y; size, prob) for size > 0, as csrc/device_math.h states R's."""
    y, size, prob = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (y, size, prob)))
    ans = dbinom_raw_log(size, y + size, prob, 1 - prob)
    return np.log(size / (size + y)) + ans


def dpois_log(y, lam):
    y = np.asarray(y, np.float64)
    out = np.full(y.shape, -lam)
    pos = y > lam * DBL_MIN
    if pos.any():
        v = y[pos]
        out[pos] = -0.5 * np.log(2 * math.pi * v) + (-stirlerr(v) - bd0(v, lam))
    return out


# ------------------------------------------------------------------ small dense solves
def chol_solve(A, g):
    """x with A x = g by an unpivoted Cholesky factorisation written out (the kernel's own);
    NaN when a pivot is not positive."""
    n = len(g)
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j]
        for k in range(j):
            d -= L[j, k] * L[j, k]
        if not d > 0:
            return np.full(n, np.nan)
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, n):
            s = A[i, j]
            for k in range(j):
                s -= L[i, k] * L[j, k]
            L[i, j] = s / L[j, j]
    z = np.zeros(n)
    for i in range(n):
        s = g[i]
        for k in range(i):
            s -= L[i, k] * z[k]
        z[i] = s / L[i, i]
    x = np.zeros(n)
    for i in reversed(range(n)):
        s = z[i]
        for k in range(i + 1, n):
            s -= L[k, i] * x[k]
        x[i] = s / L[i, i]
    return x


# ------------------------------------------------------------------ concomitant
def log_sigmoid(eta):
    return np.minimum(eta, 0.0) - np.log1p(np.exp(-np.abs(eta)))


def conc_objective(beta, l, p2):
    PASSES["concomitant_objective"] += len(l)
    eta =beta[0] + beta[1] * l + beta[2] * l * l
    return float(np.sum(p2 * log_sigmoid(eta) + (1 - p2) * log_sigmoid(-eta)))


def concomitant(l, p2):
    """beta maximising sum p2 log sigma(eta) + (1 - p2) log(1 - sigma(eta)): Newton from 0, a
    step halved (at most 30 times) while it lowers the objective by more than rounding.  NaN when
    the Hessian cannot be factorised or the stopping rule is not met within 50 steps."""
    beta = np.zeros(3)
    z = np.stack([np.ones_like(l), l, l * l])
    f = conc_objective(beta, l, p2)
    for _ in range(50):
        PASSES["concomitant_newton"] += len(l)
        eta = z.T @ beta
        lsp, lsn = log_sigmoid(eta), log_sigmoid(-eta)
        # p2 - sigma and sigma (1 - sigma) without cancellation, so that saturated genes keep a
        # smooth, positive curvature (1 - sigma in floating point is 0 from eta = 37 on)
        g = z @ (p2 * np.exp(lsn) - (1 - p2) * np.exp(lsp))
        H = (z * np.exp(lsp + lsn)) @ z.T
        d = chol_solve(H, g)
        if not np.all(np.isfinite(d)):
            return np.full(3, np.nan)
        t = 1.0
        for _h in range(30):
            fb = conc_objective(beta + t * d, l, p2)
            if np.isfinite(fb) and fb >= f - 1e-10 * (abs(f) + 1.0):
                break
            t *= 0.5
        else:
            return np.full(3, np.nan)
        step = t * d
        beta = beta + step
        f = fb
        if np.max(np.abs(step)) / (1 + np.max(np.abs(beta))) < 1e-10:
            return beta
    return np.full(3, np.nan)  # no maximiser within 50 steps (separable data: it lies at infinity)


# ------------------------------------------------------------------ correlated component
def theta_sums(th, y, mu, w, ylog):
    """The moment equation's left side minus its right side, and its derivative, at theta."""
    PASSES["theta"] += len(y)
    r = (y + th) / (mu + th)
    lr = np.log(r)
    g = np.sum(w * 2.0 * (ylog - (y + th) * lr)) - (np.sum(w) - 1.0)
    d = np.sum(w * 2.0 * (r - 1.0 - lr))
    return float(g), float(d)


def theta_root(y, mu, w, lo, hi):
    """The root in [lo, hi] of sum w 2 [y log(max(1, y) / mu) - (y + th) log((y + th) / (mu + th))]
    = sum w - 1 (MASS::theta.md's equation); the bound on the side the sign indicates when there
    is none.  Newton kept inside a bracket (a step that leaves it is replaced by the bracket's
    geometric mean), from sqrt(lo hi), until |step| <= 1e-14 theta, at most 100 steps."""
    with np.errstate(all="ignore"):
        ylog = np.where(y > 0, y * np.log(np.maximum(1.0, y) / mu), 0.0)
        g_lo = theta_sums(lo, y, mu, w, ylog)[0]
        g_hi = theta_sums(hi, y, mu, w, ylog)[0]
        if not (np.isfinite(g_lo) and np.isfinite(g_hi)):
            return np.nan
        if g_lo >= 0:
            return lo
        if g_hi <= 0:
            return hi
        a, b = lo, hi
        t = math.sqrt(lo * hi)
        for _ in range(100):
            g, d = theta_sums(t, y, mu, w, ylog)
            if g == 0:
                break
            if g < 0:
                a = t
            else:
                b = t
            tn = t - g / d
            if not (tn > a and tn < b):
                tn = math.sqrt(a * b)
            done = abs(tn - t) <= 1e-14 * t
            t = tn
            if done:
                break
        return t


def curve_parts(par, l):
    """P = (1 + 10^((m - l) s))^-r through the stable softplus, with softplus and z."""
    z = (par[2] - l) * par[3] * LN10
    sp = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
    return np.exp(-par[4] * sp), sp, z


def curve(par, l):
    """f(l) = b + (t - b) / (1 + 10^((m - l) s))^r, the fitted log alpha = -log theta."""
    P = curve_parts(par, l)[0]
    return par[0] + (par[1] - par[0]) * P


def curve_objective(par, l, la, W):
    e = la - curve(par, l)
    return float(np.sum(W * e * e))


def lm_eval(par, l, la, W):
    """Objective, J'WJ and J'We at par."""
    PASSES["curve"] += len(l)
    P, sp, z = curve_parts(par, l)
    b, t, m, s, r = par
    e = la - (b + (t - b) * P)
    q = np.exp(z - sp)  # 10^z' / (1 + 10^z')
    c = (t - b) * (-r) * P * q * LN10
    J = np.stack([1.0 - P, P, c * s, c * (m - l), (t - b) * (-P * sp)])
    JW = J * W
    return float(np.sum(W * e * e)), JW @ J.T, JW @ e


def quantile7_sorted(v, p):
    h = (len(v) - 1) * p
    lo = int(math.floor(h))
    hi = min(lo + 1, len(v) - 1)
    return v[lo] + (h - lo) * (v[hi] - v[lo])


def curve_start(l, la):
    """R's start: quantiles of log alpha below and above the mid-range of l, the mid-range, -1,
    0.5; clipped to the box.  NaN where a half holds no gene."""
    mid = (np.min(l) + np.max(l)) / 2
    low = l < mid
    bot = quantile7_sorted(np.sort(la[low]), 0.025) if low.any() else np.nan
    top = quantile7_sorted(np.sort(la[~low]), 0.975) if (~low).any() else np.nan
    return np.clip(np.array([bot, top, mid, -1.0, 0.5]), BOX_LO, BOX_HI)


def lm_fit(l, la, W, start, max_steps=100):
    """Projected Levenberg-Marquardt in the box (DESIGN.md section 4.15 states this rule)."""
    par = np.array(start, np.float64)
    if not np.all(np.isfinite(par)):
        return np.full(5, np.nan), np.nan, 0
    with np.errstate(all="ignore"):
        f, A, g = lm_eval(par, l, la, W)
    if not np.isfinite(f):
        return np.full(5, np.nan), np.nan, 0
    lam = 1e-3
    steps = 0
    for steps in range(1, max_steps + 1):
        dg = np.diag(A)
        hold = ((par <= BOX_LO) & (g < 0)) | ((par >= BOX_HI) & (g > 0)) | ~(dg > 0)
        if hold.all():
            break
        accepted = False
        for _trial in range(12):
            M = A.copy()
            gg = g.copy()
            for i in range(5):
                if hold[i]:
                    M[i, :] = 0.0
                    M[:, i] = 0.0
                    M[i, i] = 1.0
                    gg[i] = 0.0
                else:
                    M[i, i] = A[i, i] * (1.0 + lam)
            d = chol_solve(M, gg)
            pt = np.minimum(np.maximum(par + d, BOX_LO), BOX_HI)
            with np.errstate(all="ignore"):
                ft, At, gt = (np.nan, None, None) if not np.all(np.isfinite(par + d)) else lm_eval(pt, l, la, W)
            if np.isfinite(ft) and ft < f:
                accepted = True
                lam /= 10.0
                break
            lam *= 10.0
        if not accepted:
            break
        dec = f - ft
        par, f_old, f, A, g = pt, f, ft, At, gt
        if dec <= 1e-14 * f_old:
            break
    return par, f, steps


# ------------------------------------------------------------------ the EM
def alpha_of(y, mu, theta_range):
    with np.errstate(all="ignore"):
        al = (y / mu - 1.0) ** 2 - 1.0 / mu
    return np.minimum(np.maximum(al, 1.0 / theta_range[1]), 1.0 / theta_range[0])  # (a NaN stays)


def cell_theta(row_theta, par, l, local_theta, theta_range):
    if not local_theta:
        return np.full(l.shape, row_theta)
    with np.errstate(all="ignore"):
        th = np.exp(-curve(par, l))
    th = np.minimum(np.maximum(th, theta_range[0]), theta_range[1])
    th[np.isnan(th)] = theta_range[0]
    return th


def m_step(y, x, l, p2, local_theta, theta_range, awp):
    """(beta, a, theta, par, status) from the posteriors p2."""
    nanp = np.full(5, np.nan)
    beta = concomitant(l, p2)
    swx = float(np.sum(p2 * x))
    if not swx > 0:
        return beta, np.nan, np.nan, nanp, NO_WEIGHT
    a = float(np.sum(p2 * y)) / swx
    if not (a > 0 and np.isfinite(a)):
        return beta, a, np.nan, nanp, NOT_FINITE
    mu = a * x
    al = alpha_of(y, mu, theta_range)
    theta = theta_root(y, mu, p2, theta_range[0], theta_range[1])
    par = nanp
    if local_theta:
        la = np.log(al)
        W = p2 * al ** awp
        par = lm_fit(l, la, W, curve_start(l, la))[0]
    vals = np.r_[beta, a, theta, par if local_theta else []]
    return beta, a, theta, par, (OK if np.all(np.isfinite(vals)) else NOT_FINITE)


def e_step(y, x, l, beta, a, theta, par, local_theta, theta_range):
    """(p1, p2, llh) of the parameters."""
    PASSES["e_step"] += len(l)
    eta =beta[0] + beta[1] * l + beta[2] * l * l
    th = cell_theta(theta, par, l, local_theta, theta_range)
    mu = a * x
    a1 = log_sigmoid(-eta) + dpois_log(y, 0.1)
    a2 = log_sigmoid(eta) + dnbinom_log(y, th, th / (th + mu))
    m = np.maximum(a1, a2)
    lse = m + np.log(np.exp(a1 - m) + np.exp(a2 - m))
    return np.exp(a1 - lse), np.exp(a2 - lse), float(np.sum(lse))


def fit_cell(y, x, fp, local_theta=True, theta_range=(1e-2, 1e2), alpha_weight_power=0.5, iter=50):
    """One cell's fit.  y: counts of the valid genes, x: their fpm (> 0), fp: the starting
    failed-component posteriors.  Returns a dict: ``row`` (12 values in COLUMNS' order, NaN where
    the status is not 0), ``iterations``, ``llh``, ``status``, ``clusters`` (1 / 2), ``p1``."""
    y = np.asarray(y, np.float64)
    x = np.asarray(x, np.float64)
    n = len(y)
    row = np.full(12, np.nan)
    out = {"row": row, "iterations": 0, "llh": np.nan, "status": OK, "clusters": np.zeros(n, np.int32),
           "p1": np.full(n, np.nan)}
    if n < 3:
        out["status"] = TOO_FEW
        return out
    l = np.log(x)
    p1 = np.asarray(fp, np.float64).copy()
    p2 = 1.0 - p1
    llh_old = -np.inf
    status = OK
    its = 0
    llh = np.nan
    for its in range(1, int(iter) + 1):
        beta, a, theta, par, status = m_step(y, x, l, p2, local_theta, theta_range, alpha_weight_power)
        if status != OK:
            break
        p1, p2, llh = e_step(y, x, l, beta, a, theta, par, local_theta, theta_range)
        if not np.isfinite(llh):
            status = NOT_FINITE
            break
        if abs(llh - llh_old) / (abs(llh) + 0.1) < 1e-6:
            break
        llh_old = llh
    out["iterations"], out["status"] = its, status
    if status != OK:
        return out
    row[:] = [beta[0], beta[1], LOG_FAIL, math.log(a), 1.0, theta, *par, beta[2]]
    out["llh"] = llh
    out["clusters"] = np.where(p2 > p1, 2, 1).astype(np.int32)
    out["p1"] = p1
    return out


def fit_cells(counts, fpm, fail_prior, cells=None, **kw):
    """fit_cell over the columns of genes x cells matrices (fail_prior NaN outside the valid
    genes), as the library's entry takes them."""
    counts = np.asarray(counts)
    cells = range(counts.shape[1]) if cells is None else cells
    res = []
    for i in cells:
        g = np.flatnonzero(~np.isnan(fail_prior[:, i]))
        res.append(fit_cell(counts[g, i], fpm[g, i], fail_prior[g, i], **kw))
    return res


def neighbourhood_inputs(counts, cells, k, thr, min_nonfailed=5, min_size_entries=2000, trim=0.25):
    """(count, fpm, fail prior) of the valid genes of each of ``cells``: the neighbourhood stage
    by tests/knn_ref.py, the trimmed means taken on sorted rows (knn_ref.trimmed_mean's values)."""
    import knn_ref as K
    counts = np.asarray(counts)
    ls = K.estimate_library_sizes(counts, min_size_entries, thr)
    nb = K.neighbours(K.similarity(counts, thr), k)
    out = []
    for i in cells:
        oc = nb[i][nb[i] >= 0]
        sub = counts[:, oc]
        nabove = (sub > thr).sum(axis=1)
        val = np.sort(np.where(sub >= thr, sub / ls[oc], np.inf), axis=1)
        cnt = (sub >= thr).sum(axis=1)
        fpm = np.full(counts.shape[0], np.nan)
        for g in np.flatnonzero(nabove >= min_nonfailed):
            lo = int(math.floor(cnt[g] * trim)) + 1
            fpm[g] = np.mean(val[g, lo - 1:cnt[g] + 1 - lo])
        vi = K.valid_genes(fpm[:, None], nabove[:, None], min_nonfailed, 0)
        cc = counts[:, [i]]
        fp = K.fail_prior(cc, fpm[:, None], vi, thr)[:, 0]
        g = np.flatnonzero(vi[:, 0])
        out.append((counts[g, i], fpm[g], fp[g]))
    return out


# ------------------------------------------------------------------ distances between model rows
def log_theta_curve(row, lgrid, theta_range=(1e-2, 1e2)):
    par = row[6:11]
    with np.errstate(all="ignore"):
        lt = -curve(par, lgrid)
    lt = np.minimum(np.maximum(lt, math.log(theta_range[0])), math.log(theta_range[1]))
    lt[np.isnan(lt)] = math.log(theta_range[0])
    return lt


def curve_distance(row_a, row_b, l, theta_range=(1e-2, 1e2)):
    """Largest |log theta_a - log theta_b| (theta clamped to the range) on 101 points spanning the
    type-7 5 % to 95 % quantiles of l."""
    ls = np.sort(l)
    grid = np.linspace(quantile7_sorted(ls, 0.05), quantile7_sorted(ls, 0.95), 101)
    return float(np.max(np.abs(log_theta_curve(row_a, grid, theta_range) - log_theta_curve(row_b, grid, theta_range))))


def row_distances(row, ref, l):
    """corr.b absolute, corr.theta relative, curve distance, largest relative conc.* difference."""
    conc = [0, 1, 11]
    return {"corr.b": abs(row[3] - ref[3]), "theta": abs(row[5] - ref[5]) / abs(ref[5]),
            "curve": curve_distance(row, ref, l),
            "conc": float(np.max(np.abs(row[conc] - ref[conc]) / np.abs(ref[conc])))}


# ------------------------------------------------------------------ synthetic cells
TRUE_CURVE = np.array([-2.0, 1.0, 2.0, -0.5, 0.8])  # the generator's log alpha curve
TRUE_CONC = (-1.0, 1.2, 0.0)                        # its drop-out: conc.b, conc.a, conc.a2


def synthetic_cell(n, seed, drop=True, theta_kind="curve", truth=False):
    """One cell of the generator the tests use: log-normal fpm, an NB correlated component whose
    theta depends on the magnitude (TRUE_CURVE), a logistic drop-out (TRUE_CONC), and the starting
    posteriors by R's rule (threshold.prior where the count is at most 1 and fpm is at least the
    median fpm of such genes).  (count, fpm, fail prior), and the planted slope with ``truth``."""
    rng = np.random.default_rng(seed)
    x = np.exp(rng.normal(2.0, 1.6, n))
    l = np.log(x)
    a = math.exp(rng.normal(0.0, 0.3))
    if theta_kind == "curve":
        th = np.exp(-curve(TRUE_CURVE, l))
    elif theta_kind == "poisson":
        th = np.full(n, 1e6)
    else:  # "wild"
        th = np.full(n, 2e-3)
    mu = a * x
    y = rng.negative_binomial(th, th / (th + mu)).astype(np.float64)
    if drop:
        fail = rng.random(n) < 1 / (1 + np.exp(TRUE_CONC[0] + TRUE_CONC[1] * l))
        y[fail] = rng.poisson(0.1, int(fail.sum()))
    lowc = y <= 1
    med = np.median(x[lowc]) if lowc.any() else np.nan
    with np.errstate(invalid="ignore"):
        fp = np.where(lowc & (x >= med), 1 - 1e-6, 1e-6)
    y = np.minimum(y, 2.0 ** 30).astype(np.int32)
    return (y, x, fp, a) if truth else (y, x, fp)


def curve_grid(x):
    """101 points spanning the type-7 5 % to 95 % quantiles of log x."""
    ls = np.sort(np.log(x))
    return np.linspace(quantile7_sorted(ls, 0.05), quantile7_sorted(ls, 0.95), 101)


@functools.lru_cache(maxsize=None)
def reference(n, seed, local_theta=True, iter=50, drop=True, theta_kind="curve", permutations=0):
    """The generator's cell (n, seed) and its fit, computed once per session and shared by the
    tests.  With ``permutations``, the fits of that many gene permutations too, and the
    restatement's own spread over them: ``spread`` (the curve on curve_grid, and the relative
    moves of a, theta and beta) and ``llh_spread``."""
    cell = synthetic_cell(n, seed, drop=drop, theta_kind=theta_kind)
    with np.errstate(all="ignore"):
        fit = fit_cell(*cell, local_theta=local_theta, iter=iter)
        perms = permuted_fits(*cell, seeds=tuple(range(1, permutations + 1)), local_theta=local_theta, iter=iter)
    out = {"cell": cell, "fit": fit, "perms": perms, "curve_spread": 0.0, "spread": 0.0, "llh_spread": 0.0}
    if perms and fit["status"] == 0 and all(p["status"] == 0 for p in perms):
        grid = curve_grid(cell[1])
        r = fit["row"]
        sc = [0.0]
        for p in perms:
            q = p["row"]
            if local_theta:
                out["curve_spread"] = max(out["curve_spread"],
                                          float(np.max(np.abs(curve(q[6:11], grid) - curve(r[6:11], grid)))))
            sc += [abs(q[3] - r[3]), abs(q[5] - r[5]) / abs(r[5])]
            sc += [abs(q[j] - r[j]) / max(1.0, abs(r[j])) for j in (0, 1, 11)]
        out["spread"] = max(max(sc), out["curve_spread"])
        ll = [fit["llh"]] + [p["llh"] for p in perms]
        out["llh_spread"] = max(ll) - min(ll)
    return out


def permuted_fits(y, x, fp, seeds=(1, 2, 3), **kw):
    """fit_cell on gene permutations of one cell: the restatement's own sensitivity to rounding."""
    out = []
    for s in seeds:
        o = np.random.default_rng(s).permutation(len(y))
        out.append(fit_cell(y[o], x[o], fp[o], **kw))
    return out
