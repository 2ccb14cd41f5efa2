#!/usr/bin/env python3
"""H2O lines in the MT_CKD convention (pedestal-removed Voigt, cut at 25 cm^-1) plus a self and a foreign continuum held on the device.

    THE CONTINUUM COEFFICIENTS BELOW ARE MADE UP.  They have the shape of a water-vapour continuum (falling with wavenumber, the self
    part falling with temperature) and nothing else: use them to see the calls, not for numbers.  Real coefficients (MT_CKD's tables)
    are not part of this library; bring your own, on a spacing for which ln C linear in wavenumber is good enough.

Needs a GPU:  python examples/h2o_continuum.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clearsky_jl_amd as cs
import workloads as W

H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "hitran")
nu = np.linspace(1.0, 2500.0, 50_000)                        # wavenumber grid [cm^-1]
P = cs.pressuregrid(1.0, 1e5, 41)                            # 40 layers, top of atmosphere first
T = W.earth_temperature(P)
h2o = cs.DirectGas(cs.SpectralLines(os.path.join(H, "H2O.par")), W.fC_h2o, nu, shape="voigtCKD")


def made_up_coefficients(v, T_):
    """C(nu, T) [cm^2 molecule^-1 per cm^-1] -- MADE UP, see above"""
    return 1e-22 * np.exp(-v / 350.0) * (296.0 / T_) ** 4.2


grid = np.linspace(0.0, 2600.0, 261)                         # the continuum's own samples, 10 cm^-1 apart
self_c = cs.Continuum([dict(nu=grid, T=T_, C=made_up_coefficients(grid, T_)) for T_ in (180.0, 220.0, 260.0, 296.0, 340.0)], h2o, "self")
foreign_c = cs.Continuum({296.0: 2e-3 * made_up_coefficients(grid, 296.0)}, h2o, "foreign", nu=grid)      # one temperature: no T dependence

core = cs.Discretized(nstream=5, nlobatto=2)
F0 = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, h2o, core=core)
F1 = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, h2o, self_c, foreign_c, core=core)
print(f"OLR, H2O lines alone (pedestals removed)       = {F0.Fup[0]:.3f} W/m^2")
print(f"OLR, with the MADE-UP self + foreign continuum = {F1.Fup[0]:.3f} W/m^2")
