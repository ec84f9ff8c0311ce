"""Host side of the instrument-file decode.  A GSSI ``.DZT``, pulseEKKO ``.DT1``, RAMAC ``.rd3`` or Tek ``.DAT`` file is
``tnum`` trace-major records of ``snum`` integer (or float32) samples; a :class:`Layout` says where they sit in the
file's bytes and which of the reference readers' touches the samples get.  ``decode_dev`` sends the bytes up as they are
and makes the ``(snum, tnum)`` sample-major radargram in HBM (``csrc/rawload.hip`` through the C ABI); ``decode_host`` is
the same in vectorised NumPy and needs no GPU.  Both equal the reference's ``data`` bit for bit.

Reference: ``src/impdar/lib/load/load_gssi.py:200-211``, ``load_pulse_ekko.py:225-239``, ``load_ramac.py:132-137``,
``load_tek.py:56-74``.
"""
import collections
import ctypes as C

import numpy as np

from . import _hip

I16, I32, F32 = 0, 1, 2                                  # in_kind (unsigned counts are the same bits as signed)
NONE, GSSI_TOP, TEK_BIAS, PE_DEMEAN = 0, 1, 2, 3         # op
NATIVE, OUT_F32, OUT_F64 = 0, 1, 2                       # out_kind
MEAN_WINDOW = 100                                        # samples of a trace that PE_DEMEAN averages at most

IN_DTYPES = {I16: np.dtype('<i2'), I32: np.dtype('<i4'), F32: np.dtype('<f4')}
TEK_SNUM, TEK_HEAD = 1000, 20
PE_HEAD = 128
GSSI_HEADER_WORDS = 32768

Layout = collections.namedtuple('Layout', 'base stride head snum tnum in_kind op')


def native_dtype(layout):
    """dtype of the reference's ``data`` for this layout."""
    return np.dtype(IN_DTYPES[layout.in_kind].name)


def gssi_layout(snum, tnum, bits):
    """``.DZT``: a file header of ``32768 * bits / 8`` bytes, then ``snum`` counts of 16 or 32 bits per trace."""
    if bits not in (16, 32):
        raise ValueError('GSSI samples are 16 or 32 bits, got %r' % (bits,))
    el = bits // 8
    return Layout(GSSI_HEADER_WORDS * el, snum * el, 0, snum, tnum, I16 if bits == 16 else I32, GSSI_TOP)


def pe_layout(snum, tnum, first_generation):
    """``.DT1``: per trace a 128-byte header, then ``snum`` int16 (header version 1.0) or float32 samples."""
    el = 2 if first_generation else 4
    return Layout(0, PE_HEAD + snum * el, PE_HEAD, snum, tnum, I16 if first_generation else F32, PE_DEMEAN)


def ramac_layout(snum, tnum):
    """``.rd3``: ``snum`` int16 per trace, nothing else."""
    return Layout(0, 2 * snum, 0, snum, tnum, I16, NONE)


def tek_layout(tnum):
    """Tek ``.DAT``: per trace a 20-byte header, then 1000 uint16."""
    return Layout(0, TEK_HEAD + 2 * TEK_SNUM, TEK_HEAD, TEK_SNUM, tnum, I16, TEK_BIAS)


def out_kind_of(layout, out_dtype):
    if out_dtype is None or np.dtype(out_dtype) == native_dtype(layout):
        return NATIVE, native_dtype(layout)
    out_dtype = np.dtype(out_dtype)
    if out_dtype == np.float32:
        return OUT_F32, out_dtype
    if out_dtype == np.float64:
        return OUT_F64, out_dtype
    raise TypeError('a decoded radargram is %s, float32 or float64, not %s' % (native_dtype(layout), out_dtype))


def plan(nbytes, layout, out_kind=NATIVE):
    """Bytes of the result for ``layout`` on a buffer of ``nbytes`` bytes, from the library's own check
    (``impdar_rawload_plan``: no device needed).  ``ValueError`` / ``NotImplementedError`` for a layout it rejects."""
    out = C.c_longlong(0)
    rc = _hip.load().impdar_rawload_plan(int(nbytes), int(layout.base), int(layout.stride), int(layout.head),
                                         int(layout.snum), int(layout.tnum), int(layout.in_kind), int(layout.op),
                                         int(out_kind), C.byref(out))
    _hip.check(rc, 'impdar_rawload_plan')
    return out.value


def _check_host(nbytes, L):
    """The descriptor checks of ``csrc/rawload_route.h`` for the host decode (Python integers do not overflow)."""
    if L.in_kind not in IN_DTYPES or L.op not in (NONE, GSSI_TOP, TEK_BIAS, PE_DEMEAN):
        raise NotImplementedError('rawload: unknown in_kind or op')
    if (L.op == GSSI_TOP and L.in_kind == F32) or (L.op == TEK_BIAS and L.in_kind != I16) or \
            (L.op == PE_DEMEAN and L.in_kind == I32):
        raise NotImplementedError('rawload: op %d does not take in_kind %d' % (L.op, L.in_kind))
    el = IN_DTYPES[L.in_kind].itemsize
    if L.snum < 1 or L.tnum < 1:
        raise ValueError('rawload: snum and tnum must be at least 1')
    if L.op == GSSI_TOP and L.snum < 3:
        raise ValueError('rawload: GSSI_TOP needs snum >= 3')
    if min(nbytes, L.base, L.stride, L.head) < 0:
        raise ValueError('rawload: a negative size or offset')
    if L.head + L.snum * el > L.stride:
        raise ValueError('rawload: head + snum * elem exceeds the record stride')
    if L.base + (L.tnum - 1) * L.stride + L.head + L.snum * el > nbytes:
        raise ValueError('rawload: the last record ends past the raw buffer')


def _as_bytes(raw):
    if isinstance(raw, np.ndarray):
        return np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
    return np.frombuffer(raw, dtype=np.uint8)


def records(raw, layout):
    """``(tnum, snum)`` view-like array of the samples as they are in the records (native dtype)."""
    buf = _as_bytes(raw)
    _check_host(buf.size, layout)
    L = layout
    el = IN_DTYPES[L.in_kind].itemsize
    rows = np.lib.stride_tricks.as_strided(buf[L.base + L.head:], shape=(L.tnum, L.snum * el), strides=(L.stride, 1),
                                           writeable=False)
    return np.ascontiguousarray(rows).view(IN_DTYPES[L.in_kind]).astype(native_dtype(L), copy=False)


def window_nanmean(rec):
    """``np.nanmean`` of every row of the float64 ``(tnum, n)`` array ``rec``, n <= 128, in the order NumPy sums one
    contiguous vector: NaN as 0 and out of the count; n < 8 in sequence, else eight running sums over the first
    ``n - n % 8`` elements, combined pairwise, the rest added in order."""
    nan = np.isnan(rec)
    a = np.where(nan, 0.0, rec)
    n = a.shape[1]
    if n < 8:
        res = np.zeros((a.shape[0],))
        for i in range(n):
            res = res + a[:, i]
    else:
        r = a[:, :8].copy()
        body = n - n % 8
        for i in range(8, body, 8):
            r += a[:, i:i + 8]
        res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
        for i in range(body, n):
            res = res + a[:, i]
    with np.errstate(invalid='ignore', divide='ignore'):
        return res / (n - nan.sum(axis=1)).astype(np.float64)


def decode_host(raw, layout):
    """The reference's ``data`` for ``layout`` on the file's bytes: ``(snum, tnum)``, native dtype, no GPU."""
    rec = records(raw, layout)
    native = native_dtype(layout)
    if layout.op == GSSI_TOP:
        rec = rec.copy()
        rec[:, 0] = rec[:, 2]
        rec[:, 1] = rec[:, 2]
    elif layout.op == TEK_BIAS:
        rec = (rec.view(np.uint16) - np.uint16(512)).view(np.int16)
    elif layout.op == PE_DEMEAN:
        wide = rec.astype(np.float64)
        diff = wide - window_nanmean(wide[:, :MEAN_WINDOW])[:, None]
        if native == np.int16:
            # NumPy's float64 -> int16 store: truncated through int32, the low 16 bits kept
            rec = np.trunc(diff).astype(np.int64).astype(np.int16)
        else:
            with np.errstate(over='ignore', invalid='ignore'):
                rec = diff.astype(np.float32)
    return np.ascontiguousarray(rec.T)


def decode_dev(raw, layout, out_dtype=None, ctx=None):
    """The same in HBM: ``raw`` is the file's bytes on the host (``bytes`` / a NumPy array; they go up as they are) or a
    :class:`impdar_amd._hip.DeviceArray` of them.  Returns a ``(snum, tnum)`` :class:`DeviceArray` of ``out_dtype``
    (None: the native dtype; float32 / float64: the native value converted as ``astype`` does)."""
    out_kind, out_dtype = out_kind_of(layout, out_dtype)
    lib = _hip.load()
    L = layout
    if isinstance(raw, _hip.DeviceArray):
        ctx = raw.ctx
        nbytes = raw.nbytes
    else:
        ctx = ctx if ctx is not None else _hip.context()
        raw = _as_bytes(raw)
        nbytes = raw.size
    plan(nbytes, layout, out_kind)                       # a rejected layout allocates nothing
    desc = (int(nbytes), int(L.base), int(L.stride), int(L.head), int(L.snum), int(L.tnum), int(L.in_kind), int(L.op), out_kind)
    with _hip.new_device_array(ctx, (L.snum, L.tnum), out_dtype) as d_out:
        if isinstance(raw, _hip.DeviceArray):
            rc = lib.impdar_rawload_dev(ctx, raw.ptr, *(desc + (d_out.ptr,)))
        else:
            rc = lib.impdar_rawload(ctx, raw.ctypes.data_as(C.c_void_p), *(desc + (d_out.ptr,)))
        _hip.check(rc, 'impdar_rawload')
    return d_out
