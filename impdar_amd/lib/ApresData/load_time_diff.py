"""Two ApRES acquisitions of one site as an :class:`ApresTimeDiff`, ready for differencing
(behaviour of ``src/impdar/lib/ApresData/load_time_diff.py``)."""
from . import ApresTimeDiff
from ._acquisitions import files_of_site, profile, require_same_axis, take
from .ApresFlags import TimeDiffFlags

_SHARED = (('snum', 'snum'), ('decday', 'decday'), ('range', 'Rcoarse'), ('dt', 'dt'), ('travel_time', 'travel_time'))


def load_time_diff(fn, load_single_acquisitions=True, *args, **kwargs):
    """``fn`` names the pair: a string ``s`` with exactly one file matching each of ``s_time1*`` and ``s_time2*``, or
    two file names, or two loaded ``ApresData`` objects.  Each acquisition is stacked and converted to range where it
    is not yet; they must agree in ``snum`` and ``travel_time``.  With ``load_single_acquisitions`` false, ``fn`` is a
    file that :meth:`ApresTimeDiff.save` wrote.

    (In the glob form the reference passes its lists of matches on as if they were loaded objects and fails on them;
    here the matched files are loaded.)"""
    if not load_single_acquisitions:
        return ApresTimeDiff(fn)
    if isinstance(fn, str):
        sources = files_of_site(fn, ('_time1*', '_time2*'), 'Need exactly one file matching each time acqusition')
    elif len(fn) == 2:
        sources = list(fn)
    else:
        raise ValueError('fn must be a glob for files with _time1, _time2, or a 2-tuple')
    first, second = (profile(source, i + 1) for i, source in enumerate(sources))
    require_same_axis(first, second)

    pair = ApresTimeDiff(None)
    take(pair, first, _SHARED)
    pair.data = first.data.flatten().astype(complex)
    pair.data2 = second.data.flatten().astype(complex)
    pair.data_dtype = pair.data.dtype
    pair.fn1, pair.fn2 = first.header.fn, second.header.fn
    pair.fn = pair.fn1 + '_diff_' + pair.fn2
    for name, acq in (('unc1', first), ('unc2', second)):      # phase uncertainties, where they were computed
        if hasattr(acq, 'uncertainty'):
            setattr(pair, name, acq.uncertainty)
    # flags of its own with the first acquisition's read code; the first acquisition's header
    pair.flags = TimeDiffFlags()
    pair.flags.file_read_code = first.flags.file_read_code
    pair.header = first.header
    return pair
