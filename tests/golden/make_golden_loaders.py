#!/usr/bin/env python3
"""Generate the ``LD_*`` fixtures of the instrument loaders by running the REFERENCE's ``load_gssi``, ``load_pe``,
``load_ramac`` and ``load_tek`` (``src/impdar/lib/load``), imported -- never copied, with the ``h5py`` stand-in and the
``np.NaN`` alias of ``make_golden_apres_io.py`` -- on the reference's sample files kept in this folder (``ten_col.*``,
``ten_col_nogps.*``, ``test_tek.DAT``, ``test_pe.HD`` / ``.GPS``, ``test_gssi.DZG`` and the header and first 64 traces of
``test_gssi.DZT``) and on the files that the writers of ``tests/rawload_ref.py`` make from its case tables:

  LD_<case>.npz     every attribute of what the loader returned (``rawload_ref.flatten_object``), dtype of ``data`` included
  LD_Z_errors.npz   exception type and message of every ``rawload_ref.error_cases`` file
  LD_<type>_raw.mat what the reference's ``save`` writes for one object per format (``rawload_ref.RAW_MAT_CASES``)
  LD_P_impdar.json  what the reference's ``impdarexec`` parser makes of ``load <type> a b -o x`` for the four types

Usage:  python tests/golden/make_golden_loaders.py <root of the reference's source tree>
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('IMPDAR_REFERENCE_ROOT')
if not REF:
    sys.exit(__doc__)
sys.path.insert(0, os.path.join(REF, 'src'))
try:
    import h5py          # noqa: F401
except ImportError:
    sys.modules['h5py'] = types.ModuleType('h5py')
if not hasattr(np, 'NaN'):
    np.NaN = np.nan

import rawload_ref as ref                                                            # noqa: E402
from impdar.lib.load import load_gssi, load_pulse_ekko, load_ramac, load_tek           # noqa: E402

LOADERS = {'gssi': load_gssi.load_gssi, 'pe': load_pulse_ekko.load_pe, 'ramac': load_ramac.load_ramac,
           'tek': load_tek.load_tek}


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def save(name, g):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **g)
    assert os.path.getsize(path) < 1 << 20, (name, os.path.getsize(path))
    print('%-36s %7d bytes' % (name, os.path.getsize(path)))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        loaded = {}
        for name, (filetype, fn) in ref.loader_cases(tmp, HERE).items():
            with quiet(), np.errstate(all='ignore'):
                dat = LOADERS[filetype](fn)
            loaded[name] = dat
            save(name, ref.flatten_object(dat))
        errors = {}
        for name, (filetype, fn) in ref.error_cases(tmp, HERE).items():
            try:
                with quiet(), np.errstate(all='ignore'):
                    LOADERS[filetype](fn)
            except Exception as e:                      # noqa: BLE001  (the type is what is recorded)
                errors[name + '.type'] = type(e).__name__
                errors[name + '.message'] = str(e).replace(tmp, '<tmp>')
            else:
                raise AssertionError('%s: nothing raised' % name)
        save('LD_Z_errors', errors)
        for filetype, name in ref.RAW_MAT_CASES.items():
            path = os.path.join(HERE, 'LD_%s_raw.mat' % filetype)
            loaded[name].fn = os.path.basename(loaded[name].fn)          # (no folder in what is saved)
            loaded[name].save(path)
            assert os.path.getsize(path) < 1 << 20, path
            print('%-36s %7d bytes' % (os.path.basename(path), os.path.getsize(path)))
    try:
        from impdar.bin import impdarexec
        parser, how = impdarexec._get_args(), 'the reference parser'
    except Exception as e:                              # noqa: BLE001
        parser, how = None, 'restated by hand (%s: %s)' % (type(e).__name__, e)
    parsed = {'_how': how}
    for filetype in ('gssi', 'pe', 'ramac', 'tek'):
        if parser is not None:
            ns = vars(parser.parse_args(['load', filetype, 'a', 'b', '-o', 'x']))
            ns['func'] = ns['func'].__name__
        else:
            ns = {'func': 'load_and_exit', 'filetype': filetype, 'fns_in': ['a', 'b'], 'channel': 'processed',
                  'gps_offset': 0.0, 't_srs': None, 's_srs': None, 'o': 'x', 'nans': None, 'dname': 'data'}
        parsed[filetype] = ns
    with open(os.path.join(HERE, 'LD_P_impdar.json'), 'w') as f:
        json.dump(parsed, f, indent=1, sort_keys=True)
    print('LD_P_impdar.json: %s' % how)


if __name__ == '__main__':
    main()
