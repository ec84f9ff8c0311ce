"""What the reference's ``plot_radargram`` and ``plot_traces`` (``src/impdar/lib/plot.py:102-283, 368-445``) read from
the radargram before they draw, taken from where it is -- resident or on the host: the percentiles of a window (their
colour and axis limits), a window as a dense host array (the image, the traces) and the image distorted so that a picked
layer lies flat.  From a resident radargram only those results cross PCIe.
"""
import numpy as np

from ... import display
from ._resident import data_shape


def percentiles(self, q, y_range=(0, -1), x_range=(0, -1), skip_nan=True):
    """``np.percentile`` of rows ``y_range``, traces ``x_range`` of the radargram (``(0, -1)``: all of them) at the
    percentages ``q`` -- of the values that are no NaN, or with ``skip_nan=False`` NaN as soon as the window holds one.
    float64, bit for bit NumPy's."""
    dev = getattr(self, '_dev', None)
    if dev is not None:
        return display.percentile_dev(dev, q, y_range, x_range, skip_nan)
    return display.percentile_host(self.data, q, y_range, x_range, skip_nan)


def window(self, y_range=(0, -1), x_range=(0, -1)):
    """Rows ``y_range``, traces ``x_range`` of the radargram as a host array of their own."""
    dev = getattr(self, '_dev', None)
    if dev is not None:
        return display.window_dev(dev, y_range, x_range)
    return display.window_host(self.data, y_range, x_range)


def flattened(self, picknum, x_range=(0, -1)):
    """Traces ``x_range`` of the radargram, every trace shifted so that pick ``picknum`` lies on its mean row
    (``plot.get_offset``): the (snum, x1 - x0) host image of ``plot_radargram(flatten_layer=picknum)``, NaN where a
    shifted trace has no sample and on the traces the pick misses."""
    from ..plot import get_offset
    offset, _ = get_offset(self, picknum)
    snum, tnum = data_shape(self)
    x0, x1 = display.resolve_range(x_range, tnum, 'x_range')
    shift = display.shifts_from_offset(np.asarray(offset, dtype=np.float64)[x0:x1], snum)
    dev = getattr(self, '_dev', None)
    if dev is not None:
        return display.flatten_dev(dev, shift, (x0, x1))
    return display.flatten_host(self.data, shift, (x0, x1))
