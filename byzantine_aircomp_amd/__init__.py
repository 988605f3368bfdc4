"""MI355X-native geometric-median aggregation (Byzantine_AirComp hot path).

Drop-in replacements for the reference's aggregators, backed by hand-written
HIP kernels for gfx950 behind a C ABI (include/gmagg.h, libgmagg.so):

    from byzantine_aircomp_amd import gm2, gm, OMA

See DESIGN.md for the kernels and INTEGRATION.md for swapping them into the
reference's training loop.
"""
from .aggregators import (GMResult, Krum, OMA, arc, bucketed, bucketing, bulyan, caf,  # noqa: F401
                          cclip, clip, clipped, context, dnc, fltrust, gm, gm2, meamed, mean, median,
                          mixed, multi_krum, nnm, pair_distances, trimmed_mean)
from .attacks import alie, ipm, minmax, minsum, z_max  # noqa: F401
from .panels import ClientPanels, panel_width  # noqa: F401

__version__ = "0.1.0"
