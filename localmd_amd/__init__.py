"""
localmd_amd -- MI355X (gfx950) implementation of localmd's blockwise-PMD hot path.

Public surface mirrors /root/reference/localmd/__init__.py:1-7.
"""
from .decomposition import localmd_decomposition, compute_lowrank_factorized_svd, projected_svd
from .pmdarray import PMDArray, save_npz, load_npz
from .dataset import TiffArray, lazy_data_loader, ArrayDataset
from .projection import project_movie
from .diagnostic_images import make_pmd_diagnostic_images
from .export import export_movie
from .traces import extract_traces
from .maps import regressor_maps, event_regressors
from .summary import summary_images
from .quantiles import quantile_images
from .baseline import Baseline, rolling_baseline, dff_movie, trace_baseline
from .demix import Demixed, demix
from .superpixels import Superpixels, superpixels
from .grow import Grown, Merged, Refined, grow_rois, merge_rois, refine_demix
from .deconvolve import (Deconvolved, deconvolve, estimate_decay, estimate_ar2, ar2_from_roots,
                         ar2_from_time_constants)
from .register import Registration, RegisteredMovie, register_movie, apply_shifts, subpixel_peak
from .piecewise import PiecewiseRegistration, WarpedMovie, register_piecewise, apply_field, warp_frames
from .spatial import SpatialFilter, spatial_filter, filter_frames, filter_movie

PMDDataset = lazy_data_loader  # the name the reference's README uses (README.md:67)

__all__ = [
    "localmd_decomposition", "compute_lowrank_factorized_svd", "projected_svd", "PMDArray", "TiffArray",
    "lazy_data_loader", "PMDDataset", "ArrayDataset", "save_npz", "load_npz",
    "project_movie", "make_pmd_diagnostic_images", "export_movie", "extract_traces",
    "regressor_maps", "event_regressors", "summary_images", "quantile_images",
    "Baseline", "rolling_baseline", "dff_movie", "trace_baseline", "Demixed", "demix",
    "Superpixels", "superpixels", "Grown", "Merged", "Refined", "grow_rois", "merge_rois", "refine_demix", "Deconvolved", "deconvolve", "estimate_decay",
    "estimate_ar2", "ar2_from_roots", "ar2_from_time_constants",
    "Registration", "RegisteredMovie", "register_movie", "apply_shifts", "subpixel_peak",
    "PiecewiseRegistration", "WarpedMovie", "register_piecewise", "apply_field", "warp_frames",
    "SpatialFilter", "spatial_filter", "filter_frames", "filter_movie",
]
