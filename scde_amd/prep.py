"""The first call of both walkthroughs: ``clean.counts`` (R/functions.R:127-135) and ``clean.gos``
(R/functions.R:90-93).  Host code; nothing here touches the GPU."""
from __future__ import annotations

import numpy as np


def clean_counts(counts, min_lib_size=1.8e3, min_reads=10, min_detected=5):
    """``clean.counts``: genes x cells ``counts`` (a DataFrame, whose labels are kept, or an
    array) filtered in R's order, each step on what the previous one left, every comparison a
    strict ``>``:

      1. cells with more than ``min_lib_size`` detected genes (``colSums(counts > 0)``);
      2. genes with more than ``min_reads`` reads in those cells (``rowSums(counts)``);
      3. genes detected in more than ``min_detected`` of those cells (``rowSums(counts > 0)``).
    """
    frame = hasattr(counts, "iloc")
    a = counts.values if frame else np.asarray(counts)
    if a.ndim != 2:
        raise ValueError("counts must be a genes x cells matrix")
    cells = np.nonzero((a > 0).sum(axis=0) > min_lib_size)[0]
    a1 = a[:, cells]
    g1 = np.nonzero(a1.sum(axis=1) > min_reads)[0]
    a2 = a1[g1]
    g2 = np.nonzero((a2 > 0).sum(axis=1) > min_detected)[0]
    if frame:
        return counts.iloc[g1[g2], cells]
    return a2[g2]


def clean_gos(go_env, min_size=5, max_size=5000, annot=False):
    """``clean.gos``: the gene sets of ``go_env`` ({name: genes}) with
    ``min_size < len(genes) < max_size``, both strict, in their original order.  ``annot=True``
    (appending GO.db's term to each name) is not built."""
    if annot:
        raise NotImplementedError("clean_gos: annot=True needs GO.db's term table, which is not built")
    return {k: v for k, v in dict(go_env).items() if len(v) > min_size and len(v) < max_size}
