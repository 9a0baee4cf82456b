"""Plain float64 numpy/scipy restatement of pagoda.varnorm after its weights stage and of
pagoda.subtract.aspect, written from the reference's lines (R/functions.R:1511-1811, 1850-1862,
4039-4056, 5062-5093).  Test support for tests/test_varnorm.py and tests/test_gpu_varnorm.py and
the CPU baseline of tools/bench_varnorm.py; whole matrices at a time, as the R code works.

It takes the stage-1 outputs (avmodes, modes, matw, bmatw) as inputs, so a comparison measures
the later stages only.  The trend is an input too (``trend``: predicted cv2 per gene): the
smoother is tested on its own.  Nothing here calls the library under test.
"""
import numpy as np
from scipy.interpolate import CubicSpline
from scipy.optimize import brentq
from scipy.stats import chi2, norm


class EdfSpline:
    """predict(scde.edff, lt): the natural cubic spline through the table, linear outside it."""

    def __init__(self, lt, log_edf):
        self.lt = np.asarray(lt, np.float64)
        self.y = np.asarray(log_edf, np.float64)
        self.cs = CubicSpline(self.lt, self.y, bc_type="natural")
        self.d0 = float(self.cs(self.lt[0], 1))
        self.d1 = float(self.cs(self.lt[-1], 1))

    def log_edf(self, x):
        x = np.asarray(x, np.float64)
        xc = np.clip(x, self.lt[0], self.lt[-1])
        s = self.cs(xc)
        s = np.where(x < self.lt[0], self.y[0] + self.d0 * (x - self.lt[0]), s)
        return np.where(x > self.lt[-1], self.y[-1] + self.d1 * (x - self.lt[-1]), s)

    def edf(self, theta):
        theta = np.asarray(theta, np.float64)
        with np.errstate(all="ignore"):
            e = np.exp(self.log_edf(np.log(theta)))
        return np.where(theta > 1e3, 1.0, e)          # 1525


def corr_theta(models, i, lfpm, theta_range):
    """get.corr.theta (4039-4056) for cell i."""
    with np.errstate(all="ignore"):
        if "corr.ltheta.b" in models:
            b, t, m, s, r = (models["corr.ltheta." + k][i] for k in "btmsr")
            th = np.exp(-1 * (b + (t - b) / (1 + 10 ** ((m - lfpm) * s)) ** r))
        else:
            th = np.full(np.shape(lfpm), models["corr.theta"][i], np.float64)
    th = np.array(th, np.float64)
    nan = np.isnan(th)
    with np.errstate(invalid="ignore"):
        th[th < theta_range[0]] = theta_range[0]
        th[th > theta_range[1]] = theta_range[1]
    th[nan] = theta_range[0]
    return th


def moments(models, cd, edf, avmodes, matw, modes=None, bmatw=None, codes=None, weight_df_power=1.0,
            theta_range=(1e-2, 1e2)):
    """1511-1619: edf, wvar, rowSums(matw); with a batch bedf, bwvar, rowSums(bmatw), bwvar.ratio."""
    cd = np.asarray(cd, np.float64)
    N, C = cd.shape
    batched = codes is not None

    def per_cell(i, lfpm):
        with np.errstate(all="ignore"):
            mu = np.exp(lfpm * models["corr.a"][i] + models["corr.b"][i])
        th = corr_theta(models, i, lfpm, theta_range)
        return mu, th

    with np.errstate(all="ignore"):
        lf = np.log(avmodes)
        edf_mat = np.empty((N, C))
        mat = np.empty((N, C))
        for i in range(C):
            mu, th = per_cell(i, lf)
            edf_mat[:, i] = (matw[:, i] * edf.edf(th)) ** weight_df_power        # 1534
            lam = np.exp(models["fail.r"][i])
            mat[:, i] = edf_mat[:, i] * (cd[:, i] - mu) ** 2 / (mu + mu ** 2 / th + lam)   # 1580
        out = {"edf": edf_mat.sum(1) + 1, "wvar": mat.sum(1) / edf_mat.sum(1), "rowsum_matw": matw.sum(1)}
        if batched:
            bedf_mat = np.empty((N, C))
            bmat = np.empty((N, C))
            for i in range(C):
                mu, th = per_cell(i, np.log(modes[codes[i]]))
                bedf_mat[:, i] = (bmatw[:, i] * edf.edf(th)) ** weight_df_power  # 1556
                lam = np.exp(models["fail.r"][i])
                bmat[:, i] = edf_mat[:, i] * (cd[:, i] - mu) ** 2 / (mu + mu ** 2 / th + lam)  # 1601: edf.mat
            out["bedf"] = bedf_mat.sum(1) + 1
            out["bwvar"] = bmat.sum(1) / bedf_mat.sum(1)
            out["rowsum_bmatw"] = bmatw.sum(1)
            out["bwvar_ratio"] = out["bwvar"] / out["wvar"]
    return out


def qchisq_upper_log(lq, df):
    """qchisq(lq, df, lower.tail = FALSE, log.p = TRUE) by root finding on chi2.logsf."""
    if lq >= 0:
        return 0.0
    if np.isneginf(lq):
        return np.inf
    hi = max(1.0, float(df))
    while chi2.logsf(hi, df) > lq:
        hi *= 2
        if hi > 1e300:
            return np.inf
    return brentq(lambda x: chi2.logsf(x, df) - lq, 0.0, hi, xtol=1e-300, rtol=4 * np.finfo(float).eps, maxiter=500)


def adjusted_variance(zval, edf, C, max_adj_var):
    """1701-1706 for the valid genes."""
    with np.errstate(all="ignore"):
        qv = chi2.logsf(zval * (edf - 1), edf)
    qv = np.where(edf <= 1, 0.0, qv)
    qv = np.where(np.abs(qv) < 1e-10, 0.0, qv)
    x = np.array([qchisq_upper_log(q, C - 1) for q in qv])
    return np.minimum(max_adj_var, x / C)


def statistics(avmodes, mom, C, trend, fit_mask=None, max_adj_var=10.0):
    """1610-1706 with the trend's predictions given: vi, zval, arv (NaN outside vi)."""
    batched = "bwvar" in mom
    wvar = mom["bwvar"] if batched else mom["wvar"]
    rsw = mom["rowsum_bmatw"] if batched else mom["rowsum_matw"]
    vi = (rsw > 0) & np.isfinite(wvar) & (wvar > 0)
    fvi = vi & fit_mask if fit_mask is not None else vi
    if not fvi.any():
        raise ValueError("unable to find a set of valid genes to establish the variance fit")
    with np.errstate(all="ignore"):
        cv2 = np.log10(wvar / avmodes ** 2)
        zval = 10 ** (cv2[vi] - np.asarray(trend)[vi])
        if batched:
            r = mom["bwvar_ratio"][vi]
            zval = zval * np.minimum(r, 1 / r)                                    # 1697
    arv = np.full(avmodes.size, np.nan)
    arv[vi] = adjusted_variance(zval, mom["edf"][vi], C, max_adj_var)
    z = np.full(avmodes.size, np.nan)
    z[vi] = zval
    return {"vi": vi, "zval": z, "arv": arv, "wvar": wvar}


def wsu(k, n, z):
    p = k / n
    return np.minimum(1, (2 * n * p + z ** 2 + (z * np.sqrt(z ** 2 - 1 / n + 4 * n * p * (1 - p) - (4 * p - 2)) + 1)) /
                      (2 * (n + z ** 2)))


def weighted_mat_center(mat, matw):
    return mat - ((mat * matw).sum(1) / matw.sum(1))[:, None]


def matrix(models, cd, matw, arv, codes=None, weight_k=0.9):
    """1725-1804: (mat, matw).  matw is the weight matrix in use (bmatw with a batch)."""
    cd = np.asarray(cd, np.float64)
    N, C = cd.shape
    with np.errstate(all="ignore"):
        w = 1 - weight_k * (1 - matw)
        w = w / w.sum(1)[:, None]
        mat = np.log10(np.exp((np.log(cd) - models["corr.b"][None, :]) / models["corr.a"][None, :]) + 1)
        c = weighted_mat_center(mat, w)
        ov = (c * c * w).sum(1) / w.sum(1)
        vr = arv / ov
        vr[ov <= 0] = 0
        if codes is not None:
            levels = sorted(set(codes.tolist()))
            z = norm.ppf(1 - 1e-2)
            ub = np.stack([wsu((mat[:, codes == lv] > 0).sum(1), np.sum(codes == lv), z) for lv in levels], 1)
            nbub = ub.min(1)
            nbo = np.empty_like(w)
            for lv in levels:
                ii = codes == lv
                nbo[:, ii] = w[:, ii] * np.minimum(1, np.ceil(nbub * ii.sum()) / (mat[:, ii] > 0).sum(1))[:, None]
            w = nbo
            nr = C / w.sum(1)
            av = (mat * w).mean(1) * nr
            amat = np.empty_like(mat)
            for lv in levels:
                ii = codes == lv
                amat[:, ii] = mat[:, ii] - (mat[:, ii] * w[:, ii] * nr[:, None]).mean(1)[:, None]
            mat = amat + av[:, None]
        mat = weighted_mat_center(mat, w)
        mat = mat * np.sqrt(vr)[:, None]
    return mat, w


def trim_counts(models, cd, trim):
    """1372-1386 (the Winsorization by the CPU oracle's winsorizeMatrix)."""
    from oracle import pagoda as OP
    with np.errstate(all="ignore"):
        fpm = (np.log(np.asarray(cd, np.float64)) - models["corr.b"][None, :]) / models["corr.a"][None, :]
        tfpm = OP.winsorize_matrix(fpm, trim)
        back = np.round(np.exp(tfpm * models["corr.a"][None, :] + models["corr.b"][None, :]))
    back[back < 0] = 0
    keep = back.sum(1) > 0
    return back[keep].astype(np.int32), np.where(keep)[0]


def varnorm(models, cd, edf, stage1, codes, trend, fit_mask=None, weight_k=0.9, weight_df_power=1.0,
            max_adj_var=10.0, theta_range=(1e-2, 1e2)):
    """Stages 2-4 from the stage-1 outputs ``stage1`` (avmodes, modes, matw, bmatw)."""
    C = cd.shape[1]
    mom = moments(models, cd, edf, stage1["avmodes"], stage1["matw"], stage1.get("modes"), stage1.get("bmatw"),
                  codes, weight_df_power, theta_range)
    st = statistics(stage1["avmodes"], mom, C, trend, fit_mask, max_adj_var)
    w = stage1["bmatw"] if codes is not None else stage1["matw"]
    mat, mw = matrix(models, cd, w, st["arv"], codes, weight_k)
    return {"mom": mom, "mat": mat, "matw": mw, **st}


def subtract_aspect(mat, matw, aspect, center=True):
    """1850-1862."""
    v = np.asarray(aspect, np.float64)
    v = v - v.mean()
    v = v / np.sqrt((v ** 2).sum())
    nr = ((mat * matw) @ v) / (matw @ v ** 2)
    out = mat - np.outer(nr, v)
    return weighted_mat_center(out, matw) if center else out
