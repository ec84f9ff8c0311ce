"""NumPy restatement of the Stolt velocity scan (impdar_amd/velscan.py over csrc/stolt.hip: impdar_stolt_scan).

The images come from ``oracle.mig_oracle.stolt``; the sums and the varimax are restated here twice: in float64 as the
library computes them (``ref_sums`` -- what the CPU tests put in the kernels' place) and in longdouble as the yardstick
(``exact_sums``, ``exact_varimax``).

Error bound of a sum of n terms (``sum_bound``): every term of ``sum x^2`` carries one float64 rounding, every term of
``sum x^4 = sum (x^2)^2`` two, and adding n non-negative terms in ANY order (serial, pairwise, the kernel's lanes-waves
tree) costs at most (n - 1) u relative, u = 2^-53.  So |s - exact| <= ((1 + u)^(n + 1) - 1) exact < (n + 4) u exact for
every n the tests use; the yardstick's own longdouble error (n 2^-64) is inside the slack.
"""
import numpy as np

from oracle import mig_oracle

U = 2.0 ** -53


def sum_bound(n):
    return (n + 4) * U


def images(data, geo, vels, htaper, vtaper):
    """The oracle's Stolt image at every velocity: list of (2 * (snum // 2), tnum) arrays."""
    return [mig_oracle.stolt(data, geo['dt'], geo['trace_int'], geo['dist'], float(v), htaper, vtaper) for v in vels]


def ref_sums(imgs, t0, t1):
    """(nv, nout, 3) float64: sum |x|, sum x^2, sum (x^2)^2 over traces t0 <= j < t1, in float64."""
    out = np.empty((len(imgs), imgs[0].shape[0], 3))
    for b, im in enumerate(imgs):
        x = np.asarray(im, dtype=np.float64)[:, t0:t1]
        x2 = x * x
        out[b, :, 0] = np.abs(x).sum(axis=1)
        out[b, :, 1] = x2.sum(axis=1)
        out[b, :, 2] = (x2 * x2).sum(axis=1)
    return out


def exact_sums(imgs, t0, t1):
    """The same in longdouble from the images' exact values."""
    out = np.empty((len(imgs), imgs[0].shape[0], 3), dtype=np.longdouble)
    for b, im in enumerate(imgs):
        x = np.asarray(im, dtype=np.longdouble)[:, t0:t1]
        x2 = x * x
        out[b, :, 0] = np.abs(x).sum(axis=1)
        out[b, :, 1] = x2.sum(axis=1)
        out[b, :, 2] = (x2 * x2).sum(axis=1)
    return out


def exact_varimax(imgs, t0, t1, s0, s1):
    """n sum x^4 / (sum x^2)^2 over rows s0 <= k < s1 and traces t0 <= j < t1, longdouble; NaN without energy."""
    out = np.empty(len(imgs), dtype=np.longdouble)
    for b, im in enumerate(imgs):
        x = np.asarray(im, dtype=np.longdouble)[s0:s1, t0:t1]
        x2 = x * x
        e2, e4 = x2.sum(), (x2 * x2).sum()
        out[b] = np.nan if e2 == 0 else x.size * e4 / (e2 * e2)
    return out


def fake_scan(geo_of=None):
    """Stand-ins for ``velscan.scan_host`` / ``scan_dev`` built on the oracle: ``(scan_host, calls)``; every call's
    arguments are appended to ``calls``.  ``geo_of(data)`` gives the geometry dict the oracle needs (dt, trace_int,
    dist) -- the library's functions get kx and ws instead, which the stand-in only records."""
    calls = []

    def scan_host(data, kx, ws, vels, htaper, vtaper, t0, t1, keep=-1, max_batch=0):
        calls.append(dict(data=np.array(data), kx=np.array(kx), ws=np.array(ws), vels=np.array(vels), htaper=htaper,
                          vtaper=vtaper, t0=t0, t1=t1, keep=keep, max_batch=max_batch))
        geo = geo_of(data)
        if htaper != htaper:                 # NaN: the caller has tapered (integer data) -- a taper that does nothing
            htaper = vtaper = 1e-300
        imgs = images(data, geo, vels, htaper, vtaper)
        return ref_sums(imgs, t0, t1), (imgs[keep] if keep >= 0 else None)

    return scan_host, calls
