"""What the pair loader and the quad loader share: finding the files of a site, bringing each acquisition to one
stacked, range-converted profile, and checking that two profiles lie on one axis."""
import glob
from copy import deepcopy

import numpy as np

from ..ImpdarError import ImpdarError
from .load_apres import load_apres


def files_of_site(stem, patterns, message):
    """For each glob pattern (``stem`` + pattern) the one file that matches it; ``FileNotFoundError(message)`` unless
    every pattern has exactly one match."""
    found = [glob.glob(stem + pattern) for pattern in patterns]
    if any(len(hits) != 1 for hits in found):
        raise FileNotFoundError(message)
    return [hits[0] for hits in found]


def profile(source, number):
    """A private copy of acquisition ``number`` (a file name, or an ``ApresData`` already loaded) as one stacked chirp
    in range: stacked over everything first, then converted at pad factor 2 if its flags say it has not been -- the
    reference's order, with its progress lines."""
    acq = load_apres([source]) if isinstance(source, str) else source
    try:
        acq.stacking()
        print('Restacked acquisition #{:d} to a 1-d array.'.format(number))
    except ImpdarError:
        print('Acquisition #{:d} is already stacked to shape: {:s}'.format(number, str(np.shape(acq.data))))
    if acq.flags.range == 0:
        print('Acquisition #', number, 'has not been converted to range. Range conversion now...')
        acq.apres_range(2)
    return deepcopy(acq)


def require_same_axis(first, other):
    if first.snum != other.snum:
        raise ValueError('Need the same number of vertical samples in each file')
    if not np.all(first.travel_time == other.travel_time):
        raise ValueError('Need matching travel time vectors')


def take(target, source, names):
    """``target.<to> = source.<from>`` for every ``(to, from)`` of ``names``."""
    for to, frm in names:
        setattr(target, to, getattr(source, frm))
