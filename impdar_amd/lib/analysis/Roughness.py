"""Bed roughness of a picked layer (the reference's ``analysis/Roughness.py``) by Kirchhoff theory, Christianson et al.
(2016), eqs. C1 and C2.  SciPy's ``medfilt``, ``detrend`` and ``i0`` on O(tnum) vectors on the host, the reference's
arithmetic operation for operation: the results are its bits."""
import numpy as np
from scipy.signal import detrend, medfilt
from scipy.special import i0

from .geometric_power_corrections import pick_depths


def kirchhoff_roughness(dat, picknum, freq, filt_n=101, eps=3.15):
    """RMS roughness of the bed within the first Fresnel zone around every trace, and the power reduction it causes.

    Parameters
    ----------
    picknum: int
        the pick of the bed
    freq: float
        antenna frequency (Hz)
    filt_n: int, optional
        traces of the median filter over the bed elevation
    eps: float, optional
        relative permittivity of ice

    Returns
    -------
    ED1, pn: per trace, the RMS deviation from the detrended bed (m; NaN within a Fresnel half-width of the ends and where
    fewer than 2 values are picked) and the normalised power
    """
    if 'interp' not in vars(dat.flags):
        raise KeyError('dat.flags has no interp attribute: roughness needs evenly spaced traces, interpolate first')
    eps0 = 8.8541878128e-12
    mu0 = 1.25663706212e-6
    u = 1./np.sqrt(eps*eps0*mu0)
    lam = u/freq
    Z = pick_depths(dat, u)
    # half the traces across the first Fresnel zone
    D1 = np.sqrt(2.*lam*(np.nanmean(Z)/np.sqrt(eps)))
    dx = dat.trace_int[0]
    N = int(round(D1/(2.*dx)))

    bed = medfilt(dat.elev - Z[picknum], filt_n)
    ED1 = np.nan*np.empty((len(bed),))
    for n in range(N, len(bed)-N+1):
        b = bed[n-N:n+N].copy()
        b = b[np.where(~np.isnan(b))]
        if len(b) > 1:
            flat = detrend(b)
            total = 0.
            for v in flat:
                total += (v)**2.
            ED1[n] = np.sqrt((1/(len(b)-1.))*total)

    g = 4.*np.pi*ED1/lam
    pn = np.exp(-(g**2.))*(i0((g**2.)/2.))**2.
    return ED1, pn
