"""scde_amd -- MI355X-native (gfx950) implementation of scde's Bayesian
differential-expression hot path (logBootPosterior / jpmatLogBoot / matSlideMult
behind scde.posteriors() and scde.expression.difference()).

The numeric work runs in ``libscde_hip.so`` (hand-written HIP kernels, C ABI in
``include/scde_hip.h``); this package is the host-side mirror of the R API.
"""
from .api import (Context, DeviceCounts, RatioPosterior, ScdeError, bh_cz, calculate_ratio_posterior,  # noqa: F401
                  expectation_column, jpmatLogBatchBoot, jpmatLogBoot, logBootBatchPosterior, logBootPosterior,
                  marginals, matSlideMult, quick_distribution_summary, ratio_columns, scde_expression_difference,
                  scde_posteriors, scde_test_gene_expression_difference, set_rand)
from .aspects import (collapse_aspect_clusters, pagoda_reduce_loading_redundancy,  # noqa: F401
                      pagoda_reduce_redundancy, pathway_pc_correlation_distance)
from .cluster import (HClust, cutree, dist, hclust, hclust_batch, hclust_dist, leaf_order_length, order_optimal,  # noqa: F401
                      pagoda_cluster_cells, pagoda_gene_cluster_samples, pagoda_gene_clusters,
                      pagoda_gene_clusters_observed)
from .distance import (direct_dropout_distance, mode_relative_distance, reciprocal_distance,  # noqa: F401
                       weighted_correlation)
from .embedding import TsneState, tsne_affinities, tsne_embedding, tsne_iterate  # noqa: F401
from .error_models import (crossfit_models, crossfit_pairs, error_model_inputs, nb2_fit_models,  # noqa: F401
                           scde_error_models, scde_fit_models_to_reference)
from .knn import (estimate_library_sizes, knn_cell_data, knn_cell_similarity, knn_error_models,  # noqa: F401
                  knn_expected_magnitudes, knn_fit_models, knn_model_inputs, knn_neighbours, tmm_norm_factors)
from .prep import clean_counts, clean_gos  # noqa: F401
from .prior import expression_prior  # noqa: F401
from .spearman import rank_columns, spearman_cell_similarity  # noqa: F401
from .top_aspects import pagoda_effective_cells, pagoda_top_aspects, top_aspects_table  # noqa: F401
from .views import pagoda_show_pathways, pagoda_view_aspects, view_pathway_genes  # noqa: F401
from .varnorm import (EdfTable, fit_trend, load_edf_table, pagoda_subtract_aspect, pagoda_varnorm)  # noqa: F401

__version__ = "0.1.0"
