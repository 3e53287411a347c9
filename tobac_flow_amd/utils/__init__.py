"""Helpers of the hot path that do not depend on the other modules of the package.

The reference gathers its helper modules the same way (tobac_flow/utils/__init__.py); only the helpers the
hot path and its recipes touch exist here, and what the package namespace exposes is spelled out.
"""
from tobac_flow_amd.utils.datetime_utils import get_datetime_from_coord, get_time_diff_from_coord, time_diff
from tobac_flow_amd.utils.flow_utils import select_border_mode, select_interp_mode, select_of_model, warp_flow
from tobac_flow_amd.utils.label_utils import (apply_func_to_labels, find_overlapping_labels, flat_label,
                                              get_step_labels_for_label, labeled_comprehension, make_step_labels,
                                              relabel_objects, remap_labels, slice_labels)
from tobac_flow_amd.utils.normalisation_utils import (inverse_log_norm, linear_norm, linearise_field, local_linear_norm,
                                                      log_norm, select_normalisation_method, to_8bit, uniform_norm, z_norm)
from tobac_flow_amd.utils.stats_utils import (argmax_groupby, argmin_groupby, calc_combined_mean, calc_combined_std,
                                              combined_mean_groupby, combined_std_groupby, cooling_rate_groupby, counts_groupby,
                                              find_overlap_mode, get_weighted_proportions, idxmax_cooling_rate_groupby,
                                              idxmax_groupby, idxmin_groupby, mse, n_unique_along_axis, weighted_average_and_std,
                                              weighted_average_groupby, weighted_average_uncertainty,
                                              weighted_average_uncertainty_groupby, weighted_stats,
                                              weighted_stats_and_uncertainties, weighted_uncertainties)
from tobac_flow_amd.utils.xarray_utils import get_coord_bin_edges, isel_anvil, isel_core, sel_anvil, sel_core

__all__ = (
    "get_datetime_from_coord", "get_time_diff_from_coord", "time_diff",
    "select_border_mode", "select_interp_mode", "select_of_model", "warp_flow",
    "apply_func_to_labels", "find_overlapping_labels", "flat_label", "get_step_labels_for_label",
    "labeled_comprehension", "make_step_labels", "relabel_objects", "remap_labels", "slice_labels",
    "inverse_log_norm", "linear_norm", "linearise_field", "local_linear_norm", "log_norm",
    "select_normalisation_method", "to_8bit", "uniform_norm", "z_norm",
    "mse", "find_overlap_mode", "n_unique_along_axis", "weighted_average_and_std", "weighted_stats", "weighted_average_uncertainty",
    "weighted_uncertainties", "weighted_stats_and_uncertainties", "get_weighted_proportions",
    "calc_combined_mean", "calc_combined_std", "combined_mean_groupby", "combined_std_groupby", "weighted_average_groupby",
    "weighted_average_uncertainty_groupby", "argmax_groupby", "argmin_groupby", "counts_groupby", "idxmin_groupby",
    "idxmax_groupby", "cooling_rate_groupby", "idxmax_cooling_rate_groupby",
    "get_coord_bin_edges", "sel_anvil", "isel_anvil", "sel_core", "isel_core",
)
