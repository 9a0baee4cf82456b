"""Write tests/golden/pollen_knn.npz: the pollen counts after clean.counts' defaults
(R/functions.R:127-135: cells with more than 1800 detected genes, genes with more than 10 reads
seen in more than 5 cells), as int32, the cell names, and R's own stored result of

    knn.error.models(clean.counts(pollen), k = ncol/4, min.count.threshold = 2, min.nonfailed = 5)

(data/knn.rda, 64 x 12, in scde_amd.models.MODEL_COLUMNS' order).  Both files are parsed with
tools/rdata.py, which executes nothing from them.  Data only.

Usage:  python tools/make_pollen_fixture.py --data <the scde package's data/ directory>
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rdata  # noqa: E402
from scde_amd.models import MODEL_COLUMNS  # noqa: E402


def clean_counts(X, min_lib_size=1.8e3, min_reads=10, min_detected=5):
    keep_c = (X > 0).sum(0) > min_lib_size
    X = X[:, keep_c]
    keep_g = np.flatnonzero(X.sum(1) > min_reads)
    X = X[keep_g]
    k2 = (X > 0).sum(1) > min_detected
    return X[k2], keep_g[k2], keep_c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True, help="directory holding pollen.rda and knn.rda")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pollen_knn.npz"))
    args = ap.parse_args()

    obj = rdata.read_rda(os.path.join(args.data, "pollen.rda"))["pollen"]
    dims = obj.attrs["dim"].value
    dn = obj.attrs["dimnames"].value
    X = np.asarray(obj.value).reshape(tuple(dims), order="F").astype(np.int64)
    cells = list(dn[1].value)
    X, _, keep_c = clean_counts(X)
    cells = [c for c, k in zip(cells, keep_c) if k]
    _, mrows, mcols = rdata.data_frame(rdata.read_rda(os.path.join(args.data, "knn.rda"))["knn"])
    if list(mrows) != cells:
        raise SystemExit("the stored models' cells are not the cleaned counts' cells, in order")
    models = np.stack([np.asarray(mcols[c], np.float64) for c in MODEL_COLUMNS], 1)
    np.savez_compressed(args.out, counts=X.astype(np.int32), cells=np.array(cells), models=models)
    print("wrote", args.out, X.shape, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
