"""clearsky.jl_amd -- MI355X-native (gfx950, HIP) line-by-line radiative-transfer core behind ClearSky.jl's
operator surface for ONE hot path: Voigt line sums -> layer optical depth -> Planck/multi-stream fluxes -> band
integrals (reference src/absorption/line_shapes.jl, src/core/discretized.jl, src/core/shared.jl, src/fluxes.jl).

The directory name is not a Python identifier; import it as `clearsky_jl_amd` through the shim at the repo root.
"""
from . import constants
from ._lib import ClearSkyHIPError, build_native, lib, check, dptr, as_f64, SHAPES, LIB_PATH, SIGNATURES, HEADER, HEADER_DEV, WORK_COUNT, DISPATCH_FLAGS, TUNING
from .hitran import MOLPARAM, TMIN, TMAX, ISOINDEX, MolParam, SpectralLines, readpar
from .cia import CIATables, Continuum, cia, radiation_term, readcia
from .core import (interp_plan, phco2_plan, phco2_wide_regions, MultiContext, balanced_ranges, rebalance_ranges, CIA, AcceleratedAbsorber, Sigma, update_, checkpressures, pressurelimits, temperaturelimits, shape_points, AtmosphericDomain, AtmosphericProfile, Column, Gas, reconcentrate, Context, DirectGas, Discretized, HIPDiscretized, FluxPack, GrayGas, SemiGrayGas, UnifiedAbsorber, hipfluxes, hipnetfluxes, opacityerror,
                   PHCO2, PHCO2_, chebygrid, default_context, doppler, doppler_, dtaudP, faddeeva, device_function, fluxes, formprofile,
                   lobattoevaluations, lobattonodes, logrange, lorentz, lorentz_, monochromaticfluxes,
                   monochromaticfluxes_, netfluxes, nodepressures, nodevalues, opticaldepth, ozonelayer, planck,
                   pressuregrid, psatH2O, radiate, radiate_, shape_batch, stefanboltzmann, streamnodes, transmittance,
                   tile_ranges, band_fluxes, band_transmittance, tau_mode, trapz, trapz_weights, unifyabsorbers, voigt, voigt_, voigtCKD, voigtCKD_,
                   voigtVVH, voigtVVH_, voigtCKDVVH, voigtCKDVVH_, voigtLBL, voigtLBL_)

__version__ = "0.1.0"
