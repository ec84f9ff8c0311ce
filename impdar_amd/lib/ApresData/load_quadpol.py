"""The four polarizations of a quad-polarized ApRES acquisition as an :class:`ApresQuadPol`
(behaviour of ``src/impdar/lib/ApresData/load_quadpol.py``)."""
import datetime

import numpy as np
from scipy.io import loadmat

from . import ApresQuadPol
from ._acquisitions import files_of_site, profile, require_same_axis, take
from .ApresFlags import QuadPolFlags

POLARIZATIONS = ('HH', 'HV', 'VH', 'VV')
_VECTORS = ('shh', 'shv', 'svh', 'svv')
_SHARED = (('snum', 'snum'), ('decday', 'decday'), ('range', 'Rcoarse'), ('dt', 'dt'), ('travel_time', 'travel_time'))


def load_quadpol(fn, ftype='mat', load_single_pol=True, *args, **kwargs):
    """``fn`` names the four files: a string ``s`` with exactly one file matching each of ``s_HH.*``, ``s_HV.*``,
    ``s_VH.*``, ``s_VV.*``, or the four names in that order.  Each acquisition is stacked and converted to range where
    it is not yet; all must agree with the first in ``snum`` and ``travel_time``.  With ``load_single_pol`` false,
    ``fn`` is a file that :meth:`ApresQuadPol.save` wrote."""
    if not load_single_pol:
        return ApresQuadPol(fn)
    if isinstance(fn, str):
        names = files_of_site(fn, ['_%s.*' % pol for pol in POLARIZATIONS], 'Need exactly one file matching each polarization')
    elif len(fn) == 4:
        names = [str(name) for name in fn]
    else:
        raise ValueError('fn must be a glob for files with _HH, _HV, etc., or a 4-tuple')
    profiles = [profile(name, i + 1) for i, name in enumerate(names)]
    for other in profiles[1:]:
        require_same_axis(profiles[0], other)

    quad = ApresQuadPol(None)
    take(quad, profiles[0], _SHARED)
    for vector, acq in zip(_VECTORS, profiles):
        setattr(quad, vector, acq.data.flatten().astype(np.cdouble))
    quad.data = quad.shh.copy()                  # so that the object saves like the other two
    quad.data_dtype = quad.data.dtype
    # flags of its own with the first acquisition's read code; the first acquisition's header
    quad.flags = QuadPolFlags()
    quad.flags.file_read_code = profiles[0].flags.file_read_code
    quad.header = profiles[0].header
    return quad


def load_quadpol_fujita(model_name):
    """An :class:`ApresQuadPol` of a modelled acquisition.  ``model_name`` is an object with the vectors ``shh``,
    ``shv``, ``svh``, ``svv`` and ``range`` and the scalars ``c`` and ``epsr``, or a ``.mat`` file of those; the travel
    time follows from the range at the wave speed ``c / sqrt(epsr)``, and ``decday`` is now (a Matlab datenum)."""
    if type(model_name) is str:
        values = {k: np.squeeze(v) for k, v in loadmat(model_name).items() if not k.startswith('__')}
    else:
        values = vars(model_name)
    quad = ApresQuadPol(None)
    for name in _VECTORS + ('range',):
        setattr(quad, name, values[name])
    quad.snum = len(quad.shh)
    quad.data_dtype = quad.shh.dtype
    quad.travel_time = quad.range / (values['c'] / np.sqrt(values['epsr']))
    quad.dt = np.mean(np.gradient(quad.travel_time))
    since = datetime.datetime.now() - datetime.datetime(1, 1, 1)
    quad.decday = since.days + since.seconds / 86400. + 366.
    return quad
