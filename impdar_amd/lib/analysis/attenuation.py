"""The empirical attenuation framework of Hills et al. (2020) (the reference's ``analysis/attenuation.py``): one-way
attenuation rates in dB/km from picked, geometrically corrected power (``dat.picks.corrected_power``, see
``geometric_power_corrections.power_correction``) and pick depths (``dat.picks.z``, else the pick time at the velocity ``u``).

Methods 2, 5, 6a and 7 are O(picks) NumPy / SciPy on the host, the reference's arithmetic operation for operation: their
results are its bits, and -- as there -- methods 5 and 7 turn the caller's ``picks.z`` into kilometres in place when any depth
exceeds 10, methods 6a and 6b the caller's ``att_ds``.  Methods 3 and 6b are growing-window searches over candidate
rates; the search of every trace (method 3) or depth (method 6b) runs in one launch on the MI355X
(``impdar_amd.attsearch``, ``csrc/attsearch.hip``), with NumPy where no GPU is visible.
"""
import numpy as np
from scipy import stats

from ... import attsearch
from .geometric_power_corrections import pick_depths


def _line_fit(z, pc, sigZ, sigPc, Cint):
    """The slope of power (dB) against depth (km) as a two-way rate and its confidence half-width: least squares where both
    errors are 0 (after Jacobel et al. 2009), else Deming regression with Gleser's modification (Casella and Berger 2002,
    eqs. 12.2.16 and 12.2.22)."""
    Szz = np.sum((z-np.mean(z))**2.)
    Spp = np.sum((pc-np.mean(pc))**2.)
    Szp = np.sum((z-np.mean(z))*(pc-np.mean(pc)))
    dof = len(z)-2
    if sigZ == 0 and sigPc == 0:
        N = -(Szp)/Szz
        alpha = np.mean(pc) + N*np.mean(z)
        misfit = np.sum((pc - ((-N)*z + alpha))**2.)
        sigN = np.sqrt(misfit/Szz/dof)
        return N, stats.t.ppf(1.-(1.-Cint)/2., dof)*sigN
    lam = (sigZ**2.)/(sigPc**2.)
    N = -(-Szz+lam*Spp+np.sqrt((Szz-lam*Spp)**2.+4.*lam*Szp**2.))/(2.*lam*Szp)
    sigN = np.sqrt(((1.+lam*N**2.)**2.*(Szz*Spp-Szp**2.))/((Szz-lam*Spp)**2.+4.*lam*Szp**2.))
    return N, stats.t.ppf(1.-(1.-Cint)/2., dof)*sigN/(np.sqrt(dof))


def _one_pick(dat, picknum, u):
    """Depth and power (dB) of one pick where both are numbers, the depth in km (copies: the caller's arrays stay)."""
    Z = pick_depths(dat, u)
    Pc = 10.*np.log10(dat.picks.corrected_power[picknum])
    Z = Z[picknum]
    keep = ~np.isnan(Pc) & ~np.isnan(Z)
    Pc, Z = Pc[keep], Z[keep]
    if np.any(Z > 10.):
        Z /= 1000.
    return Z, Pc


def _pooled_picks(dat, picknums, u):
    """Depth (km) and power (dB) of all listed picks in one array each, where both are numbers."""
    Z = pick_depths(dat, u)
    Pc = 10.*np.log10(dat.picks.corrected_power[picknums].flatten())
    Z = Z[picknums].flatten()
    keep = ~np.isnan(Pc) & ~np.isnan(Z)
    Pc, Z = Pc[keep], Z[keep]
    if np.any(Z > 10.):
        Z /= 1000.
    return Z, Pc


def attenuation_method2(dat, picknum, sigPc=0., sigZ=0., Cint=.95, u=1.69e8, *args, **kwargs):
    """Method 2 (method 1 where the pick is the bed): a line through the power of one reflector against its depth; the rate
    is the average over the depths the reflector spans.

    Parameters
    ----------
    picknum: int
        the pick
    sigPc, sigZ: float, optional
        standard deviation of power and of depth (above 0.1 taken as metres); both 0: simple regression
    Cint: float, optional
        confidence level of the returned error
    u: float, optional
        wave speed in ice

    Returns
    -------
    N, Nerr: one-way rate and its error (dB/km)
    """
    Z, Pc = _one_pick(dat, picknum, u)
    if sigZ > .1:
        sigZ /= 1000.
    N, Nerr = _line_fit(Z, Pc, sigZ, sigPc, Cint)
    N *= 1/2.
    Nerr *= 1/2.
    return N, Nerr


def attenuation_method3(dat, picknum, Ns=np.arange(30.), Nh_target=1., Cw=0.1, win_init=100, win_step=100, u=1.69e8):
    """Method 3 (after Schroeder et al. 2016): around every trace, the rate that decorrelates the attenuation-corrected
    power from the depth of one reflector, in a window of traces widened until the rates below the correlation
    threshold span no more than ``Nh_target``.

    Parameters
    ----------
    picknum: int
        the pick
    Ns: array, optional
        candidate one-way rates (dB/km); must hold 0 once
    Nh_target: float, optional
        radiometric resolution to reach
    Cw: float, optional
        correlation threshold
    win_init, win_step: int, optional
        first window width and its increment, in traces (>= 2 and >= 1)
    u: float, optional
        wave speed in ice

    Returns
    -------
    N_result, win_result: per trace, the rate (dB/km) and the window width the search ended on
    """
    Z, Pc = _one_pick(dat, picknum, u)
    Ns = np.asarray(Ns)
    N_result = np.zeros((dat.tnum,))
    win_result = np.zeros((dat.tnum,))
    traces = range(win_init//2, dat.tnum-win_init//2)
    rates, widths = attsearch.settle(Ns, *attsearch.search(attsearch.INDEX, Z, Pc, Ns, Cw, Nh_target, win_init, win_step, traces))
    if len(traces):
        N_result[traces.start:traces.stop] = rates
        win_result[traces.start:traces.stop] = widths
    return N_result, win_result


def attenuation_method5(dat, picknums, win=1, sigPc=0, sigZ=0, Cint=.95, u=1.69e8, *args, **kwargs):
    """Method 5 (after MacGregor et al. 2014, Matsuoka et al. 2010): at every trace a line through the power of several
    internal reflectors against depth, over ``win`` traces; NaN where fewer than 5 values are picked.

    Parameters
    ----------
    picknums: array
        the picks
    win: int, optional
        traces per regression
    sigPc, sigZ, Cint, u:
        as in method 2

    Returns
    -------
    N_result, Nerr_result: per trace, the one-way rate and its error (dB/km)
    """
    Z = pick_depths(dat, u)
    if np.any(Z > 10.):
        Z /= 1000.
    if sigZ > .1:
        sigZ /= 1000.
    N_result = np.nan*np.empty((dat.tnum,))
    Nerr_result = np.nan*np.empty((dat.tnum,))
    for tr in np.arange(win//2, dat.tnum-win//2):
        pc = np.squeeze(10.*np.log10(dat.picks.corrected_power[picknums, tr-win//2:tr+win//2+1]))
        z = np.squeeze(Z[picknums, tr-win//2:tr+win//2+1])
        keep = ~np.isnan(pc) & ~np.isnan(z)
        pc, z = pc[keep], z[keep]
        if len(pc) >= 5:
            N, Nerr = _line_fit(z, pc, sigZ, sigPc, Cint)
            N_result[tr] = N*.5
            Nerr_result[tr] = Nerr*.5
    return N_result, Nerr_result


def attenuation_method6a(dat, picknums, att_ds, win=500., sigPc=0, sigZ=0, Cint=.95, u=1.69e8, *args, **kwargs):
    """Method 6a: the picks of all traces pooled; at every depth of ``att_ds`` a line through the power of all values
    within ``win`` of depth around it; NaN where fewer than 5 fall inside.

    Parameters
    ----------
    picknums: array
        the picks
    att_ds: array
        the depths (above 10 taken as metres and converted in place)
    win: float
        depth window (above 10 taken as metres)
    sigPc, sigZ, Cint, u:
        as in method 2

    Returns
    -------
    N_result, Nerr_result: per depth, the one-way rate and its error (dB/km)
    """
    Z, Pc = _pooled_picks(dat, picknums, u)
    if np.any(att_ds > 10.):
        att_ds /= 1000.
    if win > 10.:
        win /= 1000.
    N_result = np.zeros_like(att_ds).astype(float)
    Nerr_result = np.zeros_like(att_ds).astype(float)
    for i, att_d in enumerate(att_ds):
        inside = np.logical_and(Z > (att_d-win/2), Z < (att_d+win/2))
        z, pc = Z[inside], Pc[inside]
        if len(z) < 5:
            N_result[i] = np.nan
            Nerr_result[i] = np.nan
            continue
        N, Nerr = _line_fit(z, pc, sigZ, sigPc, Cint)
        N_result[i] = .5*N
        Nerr_result[i] = .5*Nerr
    return N_result, Nerr_result


def attenuation_method6b(dat, picknums, att_ds, Ns=np.arange(30.), Nh_target=1., Cw=0.1, win_init=100., win_step=100., u=1.69e8,
                         *args, **kwargs):
    """Method 6b: the search of method 3 in the vertical -- the picks of all traces pooled, and around every depth of
    ``att_ds`` a depth window widened until the rates below the correlation threshold span no more than
    ``2 Nh_target``.

    Parameters
    ----------
    picknums: array
        the picks
    att_ds: array
        the depths (above 10 taken as metres and converted in place)
    Ns, Nh_target, Cw, u:
        as in method 3
    win_init, win_step: float, optional
        first window and its increment in depth (``win_init`` above 10: both taken as metres)

    Returns
    -------
    N_result, win_result: per depth, the rate (dB/km) and the window (m) the search ended on
    """
    Z, Pc = _pooled_picks(dat, picknums, u)
    if np.any(att_ds > 10.):
        att_ds /= 1000.
    if win_init > 10.:
        win_init /= 1000.
        win_step /= 1000.
    Ns = np.asarray(Ns)
    N_result = np.zeros_like(att_ds)
    win_result = np.zeros_like(att_ds)
    order = np.argsort(Z, kind='stable')
    centres = np.array([att_d for att_d in att_ds], dtype=np.float64)
    if len(centres) and Z.size == 0:
        raise ValueError('no picked value with both a depth and a power: the depth range of an empty array')
    rates, widths = attsearch.settle(Ns, *attsearch.search(attsearch.DEPTH, Z[order], Pc[order], Ns, Cw, Nh_target, win_init, win_step,
                                                           centres))
    N_result[:] = rates
    win_result[:] = widths*1000.
    return N_result, win_result


def attenuation_method7(dat, primary_picknum, secondary_picknum, Rib=-.22, Rfa=-17, u=1.69e8, *args, **kwargs):
    """Method 7 (after MacGregor 2011, Christianson et al. 2016, eq. A4): the rate from the bed reflection and its
    multiple, which has crossed the ice twice more and been reflected once more at the bed and at the surface.

    Parameters
    ----------
    primary_picknum, secondary_picknum: int
        the bed pick and the pick of its multiple (about twice as deep, ``ValueError`` otherwise)
    Rib: float, optional
        reflectivity of the ice-bed interface (dB); the default is ice over sea water
    Rfa: float, optional
        reflectivity of the firn-air interface (dB)
    u: float, optional
        wave speed in ice

    Returns
    -------
    mean and standard deviation of the per-trace rates (dB/km)
    """
    Z = pick_depths(dat, u)
    if np.any(Z > 10.):
        Z /= 1000.
    P1 = dat.picks.corrected_power[primary_picknum]
    P2 = dat.picks.corrected_power[secondary_picknum]
    Z1, Z2 = Z[primary_picknum], Z[secondary_picknum]
    keep = ~np.isnan(P1) & ~np.isnan(P2) & ~np.isnan(Z1) & ~np.isnan(Z2)
    P1, P2, Z1, Z2 = P1[keep], P2[keep], Z1[keep], Z2[keep]
    if not abs(np.nanmean(Z1)*2. - np.nanmean(Z2)) < .1*np.nanmean(Z1):
        raise ValueError('pick %r is no multiple of pick %r: its mean depth is not within 10 %% of twice the primary\'s'
                         % (secondary_picknum, primary_picknum))
    Rfa = 10**(Rfa/10.)
    Rib = 10**(Rib/10.)
    La = -2.*Z1/np.log((4./(Rib*Rfa))*(P2/P1))
    N = 10.*np.log10(np.e)/La
    return np.nanmean(N), np.nanstd(N)
