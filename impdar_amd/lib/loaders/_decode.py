"""Where a loader's samples become the radargram: on the host (``resident=None``: ``dat.data`` in the reference's
dtype) or in HBM (``resident='float32' | 'float64'``: the file's bytes go up as they are, ``dat._dev`` holds the result
and ``dat.data`` is None, as after ``to_device()``)."""
import numpy as np

from ... import rawload

RESIDENT_DTYPES = {'float32': np.float32, 'float64': np.float64}


def install(dat, raw, layout, resident):
    """Decode ``raw`` by ``layout`` into ``dat``; sets ``snum``, ``tnum`` and ``data_dtype`` with it."""
    dat.snum, dat.tnum = int(layout.snum), int(layout.tnum)
    dat.data_dtype = rawload.native_dtype(layout)
    if resident is None:
        dat.data = rawload.decode_host(raw, layout)
        return dat
    if isinstance(resident, str) and resident in RESIDENT_DTYPES:
        out_dtype = RESIDENT_DTYPES[resident]
    else:
        raise ValueError("resident must be None, 'float32' or 'float64', got %r" % (resident,))
    dat._dev = rawload.decode_dev(raw, layout, out_dtype)
    dat._dev_widen = False
    dat.data = None
    return dat
