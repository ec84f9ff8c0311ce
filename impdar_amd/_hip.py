"""ctypes binding of ``libimpdar_hip.so`` (the C ABI in ``include/impdar_hip.h``).

There is deliberately no CPU fallback: if the library is missing or no GPU
is visible the migration entry points raise.
"""
import contextlib
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('IMPDAR_HIP_LIB') or os.path.join(_HERE, 'csrc', 'libimpdar_hip.so')

F32, F64 = 0, 1
KIRCH_AUTO, KIRCH_EXACT, KIRCH_FAST = 0, 1, 2
UNIQUE_ID_BYTES = 128

ERR_ARG, ERR_HIP, ERR_FFT, ERR_COMM, ERR_NODEV, ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6


class HipUnavailableError(RuntimeError):
    """The HIP extension could not be loaded or no GPU is usable."""


_lib = None
_lock = threading.Lock()
_ctx = {}

_p = C.c_void_p
_dp = C.POINTER(C.c_double)
_i = C.c_int
_d = C.c_double
_ip = C.POINTER(C.c_int)
_ll = C.c_longlong

# name -> (restype, argtypes); must list every symbol of include/impdar_hip.h
SIGNATURES = {
    'impdar_last_error': (C.c_char_p, []),
    'impdar_device_count': (_i, []),
    'impdar_ctx_create': (_i, [_i, C.POINTER(_p)]),
    'impdar_ctx_destroy': (None, [_p]),
    'impdar_ctx_sync': (_i, [_p]),
    'impdar_ctx_last_ms': (_i, [_p, C.POINTER(C.c_float)]),
    'impdar_ctx_last_kernel_ms': (_i, [_p, C.POINTER(C.c_float)]),
    'impdar_ctx_last_metrics': (_i, [_p, C.c_char_p, C.c_size_t]),
    'impdar_dev_alloc': (_i, [_p, C.c_size_t, C.POINTER(_p)]),
    'impdar_dev_free': (_i, [_p, _p]),
    'impdar_dev_upload': (_i, [_p, _p, _p, C.c_size_t]),
    'impdar_dev_download': (_i, [_p, _p, _p, C.c_size_t]),
    'impdar_dev_memset': (_i, [_p, _p, _i, C.c_size_t]),
    'impdar_dev_download_f64': (_i, [_p, _dp, _p, _i, C.c_size_t]),
    'mig_kirch_loop': (None, [_dp, _i, _i, _dp, _dp, _dp, _dp, _d, _dp, _d, _i]),
    'impdar_kirchhoff': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _d, _i, _i, _d, _dp, _dp, _dp, _i, _dp]),
    'impdar_kirch_plan_create': (_i, [_p, _i, _i, _i, _dp, _dp, _d, _i, _i, _d, _dp, _dp, _dp, _i, _i,
                                      C.POINTER(_p)]),
    'impdar_kirch_plan_destroy': (None, [_p]),
    'impdar_kirch_plan_mode': (_i, [_p]),
    'impdar_kirch_plan_tnum_pad': (_i, [_p]),
    'impdar_kirch_plan_xnoise': (_d, [_p]),
    'impdar_kirch_plan_kernel': (_i, [_p]),
    'impdar_kirch_queue_policy': (_i, [_i, _i]),
    'impdar_kirch_window_policy': (_i, [_i]),
    'impdar_kirch_plan_window': (_i, [_p]),
    'impdar_kirch_prep': (_i, [_p, _p, _i, _i, _i]),
    'impdar_kirch_allgather': (_i, [_p]),
    'impdar_kirch_exchange': (_i, [_p, _i, _ip, _ip, _ip, _i, _ip, _ip, _ip]),
    'impdar_kirch_migrate': (_i, [_p, _p, _i, _i]),
    'impdar_kirch_last_ms': (_i, [_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    'impdar_kirch_history_ms': (_i, [_p, _i, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    'impdar_kirch_count_pairs': (C.c_longlong, [_p, _i, _i]),
    'impdar_stolt': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _d, _d, _d, _p]),
    'impdar_stolt_dev': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _d, _d, _d, _p]),
    'impdar_stolt_scan_dev': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _dp, _i, _d, _d, _i, _i, _i, _dp, _i, _p]),
    'impdar_stolt_scan': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _dp, _i, _d, _d, _i, _i, _i, _dp, _i, _p]),
    'impdar_fk_fan': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _d, _d, _d, _i, _i, _p]),
    'impdar_fk_fan_dev': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _d, _d, _d, _i, _i, _p]),
    'impdar_fk_power': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _dp]),
    'impdar_fk_power_dev': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _p]),
    'impdar_decon': (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _d, _i, _p, _dp]),
    'impdar_decon_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _d, _i, _p, _p]),
    'impdar_acorr': (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _dp]),
    'impdar_acorr_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    'impdar_attr': (_i, [_p, _p, _i, _i, _i, _i, _i, _d, _p]),
    'impdar_attr_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _d, _p]),
    'impdar_attr_route_probe': (_i, [_i, _i, _i, _i, _ip]),
    'impdar_slope': (_i, [_p, _p, _i, _i, _i, _i, _d, _d, _d, _dp]),
    'impdar_slope_dev': (_i, [_p, _p, _i, _i, _i, _i, _d, _d, _d, _p]),
    'impdar_dipsmooth': (_i, [_p, _p, _i, _i, _i, _i, _dp, _d, _d, _d, _p]),
    'impdar_dipsmooth_dev': (_i, [_p, _p, _i, _i, _i, _i, _p, _d, _d, _d, _p]),
    'impdar_slope_route_probe': (_i, [_i, _i, _d, _d, _i, _ip]),
    'impdar_fft_rows_dev':(_i, [_p, _i, _i, _i, _i, _p, _p, _d]),
    'impdar_fft_rows_any_dev': (_i, [_p, _i, _i, _i, _i, _p, _p, _d]),
    'impdar_phaseshift': (_i, [_p, _p, _i, _i, _i, _i, _dp, _dp, _d, _dp, _d, _dp, _i, _d, _d, _p]),
    'impdar_phaseshift_dev': (_i, [_p, _p, _i, _i, _i, _i, _dp, _dp, _d, _dp, _d, _dp, _i, _d, _d, _p]),
    'impdar_phaseshift_tk_dev': (_i, [_p, _p, _i, _i, _i, _i, _dp, _dp, _d, _dp, _d, _dp, _i, _d, _d, _i, _i, _p]),
    'impdar_ps_alltoall_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), _p]),
    'impdar_phaseshift_finish_dev': (_i, [_p, _p, _i, _i, _i, _p]),
    'impdar_phaseshift_ffd': (_i, [_p, _dp, _i, _i, _i, _dp, _dp, _d, _dp, _dp, _d, _d, _d, _dp]),
    'impdar_taper': (_i, [_p, _p, _i, _i, _i, _d, _d]),
    'impdar_filtfilt': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _i, _dp]),
    'impdar_filtfilt_dev': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _i, _dp]),
    'impdar_fir_shift': (_i, [_p, _p, _i, _i, _i, _dp, _i]),
    'impdar_fir_shift_dev': (_i, [_p, _p, _i, _i, _i, _dp, _i]),
    'impdar_trace_lerp': (_i, [_p, _p, _i, _i, _i, _ip, _ip, _dp, _dp, _i, _p]),
    'impdar_cast_dev': (_i, [_p, _p, _i, _p, _i, C.c_size_t]),
    'impdar_trace_lerp_dev': (_i, [_p, _p, _i, _i, _i, _ip, _ip, _dp, _dp, _i, _p]),
    'impdar_hfilt': (_i, [_p, _p, _i, _i, _i, _i, _i, _dp]),
    'impdar_hfilt_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _dp]),
    'impdar_ahfilt': (_i, [_p, _p, _i, _i, _i, _ip, _ip, _dp]),
    'impdar_ahfilt_dev': (_i, [_p, _p, _i, _i, _i, _ip, _ip, _dp]),
    'impdar_wiener': (_i, [_p, _p, _i, _i, _i, _i, _i, _d, _i, _dp, _dp]),
    'impdar_wiener_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _d, _i, _p, _dp]),
    'impdar_median': (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    'impdar_median_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    'impdar_hfiltfilt': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _i, _dp, _dp]),
    'impdar_hfiltfilt_dev': (_i, [_p, _p, _i, _i, _i, _dp, _dp, _i, _dp, _p]),
    'impdar_row_lerp': (_i, [_p, _p, _i, _i, _i, _ip, _ip, _dp, _dp, _i, _p]),
    'impdar_row_lerp_dev': (_i, [_p, _p, _i, _i, _i, _ip, _ip, _dp, _dp, _i, _p]),
    'impdar_col_shift': (_i, [_p, _p, _i, _i, _i, _ip, _i, _p]),
    'impdar_col_shift_dev': (_i, [_p, _p, _i, _i, _i, _ip, _i, _p]),
    'impdar_winavg': (_i, [_p, _p, _i, _i, _i, _ip, _ip, _dp]),
    'impdar_winavg_dev': (_i, [_p, _p, _i, _i, _i, _ip, _ip, _dp]),
    'impdar_rangegain': (_i, [_p, _p, _i, _i, _i, _dp, _ip]),
    'impdar_rangegain_dev': (_i, [_p, _p, _i, _i, _i, _dp, _ip]),
    'impdar_agc': (_i, [_p, _p, _i, _i, _i, _i, _d]),
    'impdar_agc_dev': (_i, [_p, _p, _i, _i, _i, _i, _d]),
    'impdar_row_absmax': (_i, [_p, _p, _i, _i, _i, _dp]),
    'impdar_restack': (_i, [_p, _p, _i, _i, _i, _i, _p]),
    'impdar_restack_dev': (_i, [_p, _p, _i, _i, _i, _i, _p]),
    'impdar_reverse_dev': (_i, [_p, _p, _i, _i, _i]),
    'impdar_hcrop_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    'impdar_qp_rotate': (_i, [_p, _dp, _dp, _dp, _dp, _i, _dp, _dp, _dp, _i, _dp, _dp, _dp, _dp]),
    'impdar_qp_rotate_dev': (_i, [_p, _p, _p, _p, _p, _i, _dp, _dp, _dp, _i, _p, _p, _p, _p]),
    'impdar_qp_coherence': (_i, [_p, _dp, _dp, _i, _i, _i, _i, _i, _dp]),
    'impdar_qp_coherence_dev': (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    'impdar_qp_phase_gradient': (_i, [_p, _dp, _i, _i, _i, _d, _dp, _dp, _dp, _dp, _dp, _i, _dp, _dp]),
    'impdar_qp_phase_gradient_dev': (_i, [_p, _p, _i, _i, _i, _d, _dp, _dp, _dp, _dp, _dp, _i, _dp, _p]),
    'impdar_qp_power_anomaly': (_i, [_p, _dp, _i, _i, _dp]),
    'impdar_qp_power_anomaly_dev': (_i, [_p, _p, _i, _i, _p]),
    'impdar_qp_find_cpe': (_i, [_p, _dp, _i, _i, _dp, _dp, _i, _dp, _i, _i, _ip, _dp]),
    'impdar_qp_find_cpe_dev': (_i, [_p, _p, _i, _i, _dp, _dp, _i, _dp, _i, _i, _p, _p]),
    'impdar_qp_find_cpe_last_ms': (_i, [_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    'impdar_qp_cpe_gather': (_i, [_p, _dp, _i, _i, _i, _ip, _dp]),
    'impdar_qp_cpe_gather_dev': (_i, [_p, _p, _i, _i, _i, _p, _p]),
    'impdar_apres_range': (_i, [_p, _dp, _i, _i, _i, _i, _dp, _dp, _dp, _d, _d, _i, _d, _i, _dp, _dp, _dp]),
    'impdar_apres_range_dev': (_i, [_p, _p, _i, _i, _i, _i, _dp, _dp, _dp, _d, _d, _i, _d, _i, _p, _p, _p]),
    'impdar_apres_range_last_ms': (_i, [_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    'impdar_apres_stack': (_i, [_p, _dp, _i, _i, _i, _i, _i, _dp]),
    'impdar_apres_stack_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    'impdar_apres_phase_diff': (_i, [_p, _dp, _dp, _i, _i, _i, _dp]),
    'impdar_apres_phase_diff_dev': (_i, [_p, _p, _p, _i, _i, _i, _p]),
    'impdar_apres_decode': (_i, [_p, _p, _i, C.c_longlong, _d, _dp]),
    'impdar_apres_decode_dev': (_i, [_p, _p, _i, C.c_longlong, _d, _p]),
    'impdar_apres_decode_pieces_dev': (_i, [_p, _p, _i, C.c_longlong, _d, _p, C.c_longlong]),
    'impdar_rawload_plan': (_i, [_ll, _ll, _ll, _ll, _i, _i, _i, _i, _i, C.POINTER(_ll)]),
    'impdar_rawload_dev': (_i, [_p, _p, _ll, _ll, _ll, _ll, _i, _i, _i, _i, _i, _p]),
    'impdar_rawload': (_i, [_p, _p, _ll, _ll, _ll, _ll, _i, _i, _i, _i, _i, _p]),
    'impdar_gps_cc_plan': (_i, [_ll, _ll, _ll, _i, C.POINTER(_ll)]),
    'impdar_gps_cc': (_i, [_p, _dp, _dp, _dp, _ll, _dp, _dp, _dp, _ll, _d, _dp, _ll, _i, _dp, C.POINTER(_ll), _ll, _dp, _dp]),
    'impdar_att_search_plan': (_i, [_i, _ll, _ll, _ll, _d, _d, _ll, _ll, C.POINTER(_ll)]),
    'impdar_att_search': (_i, [_p, _i, _dp, _dp, _ll, _dp, _ll, _ll, _dp, _ll, _ll, _d, _d, _d, _d, C.POINTER(_ll), _dp, _ip, _ll, _dp, _ll,
                               C.POINTER(_ll)]),
    'impdar_auto_pick': (_i, [_p, _p, _i, _i, _i, _i, _ip, _ip, _i, _i, _i, _i, _dp, _ip]),
    'impdar_auto_pick_dev': (_i, [_p, _p, _i, _i, _i, _i, _ip, _ip, _i, _i, _i, _i, _dp, _ip]),
    'impdar_pick_guided': (_i, [_p, _p, _i, _i, _i, _i, _i, _ip, _i, _i, _i, _i, _dp, _ip]),
    'impdar_pick_guided_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _ip, _i, _i, _i, _i, _dp, _ip]),
    'impdar_continuity': (_i, [_p, _p, _i, _i, _i, _ip, _ip, _i, _d, _dp]),
    'impdar_continuity_dev': (_i, [_p, _p, _i, _i, _i, _ip, _ip, _i, _d, _dp]),
    'impdar_mean_spectrum': (_i, [_p, _p, _i, _i, _i, _i, _dp]),
    'impdar_mean_spectrum_dev': (_i, [_p, _p, _i, _i, _i, _i, _dp]),
    'impdar_periodogram': (_i, [_p, _p, _i, _i, _i, _dp, _d, _p]),
    'impdar_periodogram_dev': (_i, [_p, _p, _i, _i, _i, _dp, _d, _p]),
    'impdar_spec_route_probe': (_i, [_i, C.c_longlong, _ip]),
    'impdar_order_stats': (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _dp, _i, _i, C.POINTER(C.c_longlong), _p]),
    'impdar_order_stats_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _dp, _i, _i, C.POINTER(C.c_longlong), _p]),
    'impdar_flatten': (_i, [_p, _p, _i, _i, _i, _i, _i, _ip, _p]),
    'impdar_flatten_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _ip, _p]),
    'impdar_window_dev': (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    'impdar_comm_unique_id':(_i, [C.c_char_p]),
    'impdar_comm_init': (_i, [_p, C.c_char_p, _i, _i]),
    'impdar_comm_rank': (_i, [_p]),
    'impdar_comm_size': (_i, [_p]),
    'impdar_comm_info': (_i, [_p, _ip, _ip, _ip, _ip]),
    'impdar_comm_barrier': (_i, [_p]),
}

# the reference's native hooks that carry no prefix of this library (mig_kirch_loop is listed above)
HOOKS = {
    'coherence2d': (None, [_dp, _dp, _dp, _i, _i, _i, _i]),
}


def load():
    """Load the shared library (once) and declare every prototype."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise HipUnavailableError(
                'HIP extension %s not built; run `python -c "import __graft_entry__ as g; g.build()"` '
                'or `python -m impdar_amd.build`' % LIB_PATH)
        try:
            lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        except OSError as exc:
            raise HipUnavailableError('cannot load %s: %s' % (LIB_PATH, exc))
        for name, (res, args) in list(SIGNATURES.items()) + list(HOOKS.items()):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def mapped_rccl():
    """Paths of every librccl mapped into this process (there must be one, and it must be the ROCm install's:
    a torch wheel ships its own older librccl.so under the same SONAME, and whichever is loaded first serves
    both)."""
    paths = set()
    try:
        with open('/proc/self/maps') as fi:
            for line in fi:
                if 'librccl' in line:
                    paths.add(line.split()[-1])
    except OSError:
        pass
    return sorted(paths)


def require_system_rccl():
    load()
    foreign = [p for p in mapped_rccl() if not os.path.realpath(p).startswith(os.path.realpath('/opt/rocm') + os.sep)
               and '/opt/rocm' not in p]
    if foreign and os.environ.get('IMPDAR_ALLOW_FOREIGN_RCCL') != '1':
        raise HipUnavailableError(
            'librccl was already mapped from %s before libimpdar_hip.so was loaded (import torch after '
            'impdar_amd._hip.load(), or not at all): the library is linked against /opt/rocm\'s RCCL; set '
            'IMPDAR_ALLOW_FOREIGN_RCCL=1 to run anyway' % ', '.join(foreign))


def last_error():
    msg = load().impdar_last_error()
    return msg.decode('utf-8', 'replace') if msg else ''


def check(rc, what=''):
    """Map a C status to the exception type the reference raises."""
    if rc == 0:
        return
    msg = '%s%s' % (what + ': ' if what else '', last_error())
    if rc == ERR_ARG:
        raise ValueError(msg)
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == ERR_NODEV:
        raise HipUnavailableError(msg)
    raise RuntimeError('impdar HIP error %d: %s' % (rc, msg))


def apply_queue_policy():
    """Hand $IMPDAR_KIRCH_ORDER (chunk | packed) and $IMPDAR_KIRCH_G (1 | 2 | 4) to the library before a Kirchhoff plan is
    created (impdar_kirch_queue_policy: the library itself does not read them).  Unset, or anything else: its own choice."""
    order = {'chunk': 1, 'packed': 2}.get(os.environ.get('IMPDAR_KIRCH_ORDER', ''), 0)
    gang = {'1': 1, '2': 2, '4': 4}.get(os.environ.get('IMPDAR_KIRCH_G', ''), 0)
    check(load().impdar_kirch_queue_policy(order, gang), 'impdar_kirch_queue_policy')
    # ... and $IMPDAR_KIRCH_WINDOW (slide | quad), the output window of the float32 ring kernel's tiles
    window = {'slide': 1, 'quad': 2}.get(os.environ.get('IMPDAR_KIRCH_WINDOW', ''), 0)
    check(load().impdar_kirch_window_policy(window), 'impdar_kirch_window_policy')


def device_count():
    return load().impdar_device_count()


def context(device=None):
    """Per-process context for ``device`` (default: $IMPDAR_DEVICE, else $LOCAL_RANK, else 0).  A rank whose
    device does not exist is an error -- two ranks must never end up sharing GPU 0 silently."""
    lib = load()
    if device is None:
        device = int(os.environ.get('IMPDAR_DEVICE', os.environ.get('LOCAL_RANK', '0')))
        ndev = lib.impdar_device_count()
        if device < 0 or device >= max(ndev, 1):
            raise HipUnavailableError('rank wants GPU %d but only %d device(s) are visible (LOCAL_RANK / '
                                      'IMPDAR_DEVICE / IMPDAR_NGPUS larger than the node)' % (device, ndev))
    with _lock:
        if device in _ctx:
            return _ctx[device]
    h = _p()
    check(lib.impdar_ctx_create(device, C.byref(h)), 'impdar_ctx_create')
    with _lock:
        _ctx[device] = h
    return h


def as_dp(a):
    """float64 C-contiguous array -> (array, double*)."""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def dtype_code(dt):
    dt = np.dtype(dt)
    if dt == np.float32:
        return F32
    if dt == np.float64:
        return F64
    raise TypeError('device kernels take float32 or float64 data, got %s' % dt)


def work_array(data, what, copy):
    """float32 / float64 C-contiguous (snum, tnum) array for a host-buffer entry point (integers and bools
    widened to float64).  ``what`` opens the ``TypeError`` for complex data, subject and verb; ``copy`` asks for
    a fresh array whatever the input, because the C call works in place."""
    data = np.asarray(data)
    if data.ndim != 2:
        raise ValueError('data must be (snum, tnum)')
    if np.iscomplexobj(data):
        raise TypeError('%s not supported by the MI355X engine' % what)
    dtype = data.dtype if data.dtype in (np.float32, np.float64) else np.float64
    return np.array(data, dtype=dtype, order='C') if copy else np.ascontiguousarray(data, dtype=dtype)


class DeviceArray(object):
    """A (rows, cols) row-major array resident in HBM (an empty one still owns a one-byte allocation)."""

    def __init__(self, ctx, shape, dtype):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = _p()
        check(load().impdar_dev_alloc(ctx, max(self.nbytes, 1), C.byref(self.ptr)), 'impdar_dev_alloc')

    @classmethod
    def from_host(cls, ctx, a):
        a = np.ascontiguousarray(a)
        d = cls(ctx, a.shape, a.dtype)
        check(load().impdar_dev_upload(ctx, d.ptr, a.ctypes.data_as(_p), d.nbytes), 'impdar_dev_upload')
        return d

    def to_host(self):
        out = np.empty(self.shape, dtype=self.dtype)
        check(load().impdar_dev_download(self.ctx, out.ctypes.data_as(_p), self.ptr, self.nbytes),
              'impdar_dev_download')
        return out

    def to_host_f64(self):
        """float64 host copy (widened on several host threads when the array is float32)."""
        out = np.empty(self.shape, dtype=np.float64)
        n = int(np.prod(self.shape))
        check(load().impdar_dev_download_f64(self.ctx, out.ctypes.data_as(_dp), self.ptr, dtype_code(self.dtype), n),
              'impdar_dev_download_f64')
        return out

    def free(self):
        if self.ptr:
            load().impdar_dev_free(self.ctx, self.ptr)
            self.ptr = _p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


@contextlib.contextmanager
def new_device_array(ctx, shape, dtype):
    """A fresh :class:`DeviceArray` for the result of a ``*_dev`` call: freed if the body raises, else the
    caller's."""
    d = DeviceArray(ctx, shape, dtype)
    try:
        yield d
    except Exception:
        d.free()
        raise
