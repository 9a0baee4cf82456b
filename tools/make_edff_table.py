"""Turn scde's `data/scde.edff.rda` into the edf table `pagoda_varnorm` takes.

    python tools/make_edff_table.py PATH_TO_scde.edff.rda OUT.npz

`scde.edff` is an `mgcv::gam` with one thin-plate smooth `s(lt)` fitted on 1,000 evenly
spaced points `lt` = log(theta) from log(1e-2) to log(1e3).  A one-dimensional thin-plate
smooth (m = 2) is a natural cubic spline whose knots are its data points, so the gam's
predictions are the natural cubic spline through the stored pairs (lt, fitted.values);
those two vectors are all the table holds:

    lt       1,000 ascending values
    log_edf  the gam's fitted.values in the same order (log of the effective d.f.)

The file is only parsed (tools/rdata.py); nothing in it is executed.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rdata  # noqa: E402


def edff_table(path):
    """(lt, log_edf) of the gam saved in `path`, ordered by lt."""
    gam = rdata.read_rda(path)["scde.edff"]
    names = gam.attrs["names"].value
    fitted = np.asarray(gam.value[names.index("fitted.values")].value, np.float64)
    model = gam.value[names.index("model")]
    lt = np.asarray(model.value[model.attrs["names"].value.index("lt")].value, np.float64)
    if lt.shape != fitted.shape or lt.ndim != 1:
        raise ValueError("scde.edff: model$lt and fitted.values differ in length")
    o = np.argsort(lt, kind="stable")
    return lt[o], fitted[o]


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        raise SystemExit(__doc__)
    lt, log_edf = edff_table(argv[0])
    np.savez(argv[1], lt=lt, log_edf=log_edf)
    print(f"{argv[1]}: {lt.size} points, lt in [{lt[0]:.6g}, {lt[-1]:.6g}], "
          f"edf in [{np.exp(log_edf.min()):.4g}, {np.exp(log_edf.max()):.4g}]")


if __name__ == "__main__":
    main()
