"""Where a RadarData's radargram lives: the resident array ``_dev`` (``to_device``) or the host array ``data``.
The processing and filtering steps ask for its shape and dtype and run their device or host form through here."""
import numpy as np


def data_shape(self):
    dev = getattr(self, '_dev', None)
    return dev.shape if dev is not None else np.shape(self.data)


def data_dtype(self):
    dev = getattr(self, '_dev', None)
    return dev.dtype if dev is not None else np.asarray(self.data).dtype


def update_data(self, on_dev, on_host):
    """Run a step that keeps shape and dtype: ``on_dev`` rewrites the resident array where it is, ``on_host``
    returns the new host array."""
    dev = getattr(self, '_dev', None)
    if dev is not None:
        on_dev(dev)
    else:
        self.data = on_host(self.data)


def replace_data(self, on_dev, on_host):
    """Install the result of a step that changes shape or dtype: a new resident array (the old one is freed,
    unless the step handed the same one back) or a new host array."""
    dev = getattr(self, '_dev', None)
    if dev is not None:
        new_dev = on_dev(dev)
        if new_dev is not dev:
            dev.free()
            self._dev = new_dev
            self.data = None
    else:
        self.data = on_host(self.data)
