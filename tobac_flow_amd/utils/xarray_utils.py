"""Coordinate helpers of the gridding recipes (reference: utils/xarray_utils.py:25-31; no xarray needed)."""
import numpy as np


def get_coord_bin_edges(coord):
    """The size + 1 bin edges around the points of a one-dimensional coordinate: the midpoints of neighbouring points
    inside, the first and the last point themselves at the ends.  `coord` is an array or anything with `.data`; the sum
    and the halving are taken in float64 whatever the coordinate's dtype, as the reference does."""
    data = np.asarray(getattr(coord, "data", coord))
    bins = np.zeros(data.size + 1)
    bins[:-1] += data
    bins[1:] += data
    bins[1:-1] /= 2
    return bins


__all__ = ("get_coord_bin_edges",)
