"""Geometric corrections of picked power (the reference's ``analysis/geometric_power_corrections.py``): spherical
spreading and, through a layered firn or from an aircraft, refractive focusing (Bogorodsky et al. 1985, eq. 3.8).  O(picks)
NumPy on the host, the reference's arithmetic operation for operation: the results are its bits."""
import numpy as np


def pick_depths(dat, u):
    """``dat.picks.z`` where the user has set it, else the depth of the two-way pick time at the constant velocity ``u``
    (with the reference's warning)."""
    if 'z' in vars(dat.picks):
        return dat.picks.z
    print('Warning: setting pick depth for constant velocity in ice.')
    return dat.picks.time*u/2/1e6


def power_correction(dat, eps=[], d_eps=[], u=1.69e8, h_aircraft=0.):
    """Write ``dat.picks.corrected_power``: ``dat.picks.power`` times the spreading loss ``(2 z)^2`` of a spherical wave,
    divided by the refractive focusing gains.

    Parameters
    ----------
    eps: array, optional
        relative permittivity of the firn layers, top down
    d_eps: array, optional
        depth of the top of every layer; the first must be 0 (``KeyError`` otherwise)
    u: float, optional
        wave speed in ice, used where ``dat.picks.z`` is not set
    h_aircraft: float, optional
        height of the aircraft above the surface; > 0 adds the focusing from air into the first layer
    """
    Z = pick_depths(dat, u)
    spreading = (2.*Z)**2.
    gain = np.ones_like(Z)
    if len(d_eps) > 0:
        if d_eps[0] != 0:
            raise KeyError('d_eps[0] must be 0: the first permittivity layer starts at the surface')
        if h_aircraft > 0.:
            gain *= refractive_focusing(h_aircraft, 2.*(Z+h_aircraft), 1., eps[0])
        for k in range(len(eps)-1):
            gain *= refractive_focusing(d_eps[k], 2.*Z, eps[k], eps[k+1])
    dat.picks.corrected_power = dat.picks.power * spreading/gain


def refractive_focusing(z1, z2, eps1, eps2):
    """The focusing coefficient of an interface with ``z1`` (permittivity ``eps1``) above and ``z2`` (``eps2``) below it;
    1 where ``z2 <= z1``.  Scalars or arrays."""
    q = ((z1+z2)/(z1+z2*np.sqrt(eps1/eps2)))**2.
    if hasattr(q, '__len__'):
        q[z2 <= z1] = 1.
    elif z2 <= z1:
        q = 1.
    return q
