// The host-side check of a raw-record descriptor (rawload.hip): is it a layout the decode kernels may run on, and how many
// bytes does its (snum, tnum) result take -- plain C++, no HIP include; impdar_rawload_plan answers from it without a device.
// No kernel is launched on a descriptor that rawload_route() rejects, so the kernels test nothing but their tile edges.
//
// A raw buffer of `nbytes` bytes holds `tnum` records: record t starts at byte base + t stride, its `snum` samples of
// `in_kind` at byte `head` of it.  v[s, t] is sample s of record t; the native result of `op` is
//   NONE       v
//   GSSI_TOP   rows 0 and 1 take row 2's values (snum >= 3)
//   TEK_BIAS   v - 512 in int16, wrapping (I16)
//   PE_DEMEAN  v minus the trace's np.nanmean over its first min(100, snum) samples, formed in float64 and stored as
//              NumPy stores a float64 into the native type (I16: truncated through int32, low 16 bits; F32: to nearest even)
// and `out_kind` keeps the native type (int16, int32, float32) or converts it to float32 / float64 as astype does.
#pragma once
#include <cstddef>
#include "../../include/impdar_hip.h"

enum { RAWLOAD_MEAN_WINDOW = 100 };   // samples of a trace that PE_DEMEAN averages at most

struct RawloadDesc {
    long long nbytes = 0, base = 0, stride = 0, head = 0;
    int snum = 0, tnum = 0;
    int in_kind = 0, op = 0, out_kind = 0;
};

struct RawloadRoute {
    int status = IMPDAR_ERR_ARG;
    const char *why = "";
    int in_bytes = 0;             // bytes of a sample in the record
    int out_bytes = 0;            // ... and of an element of the result
    int native_kind = 0;          // IMPDAR_RAW_I16 / I32 / F32: what out_kind NATIVE keeps
    long long total_bytes = 0;    // snum tnum out_bytes
    long long last_end = 0;       // one past the last byte the kernels read
};

static inline bool rawload_mul(long long a, long long b, long long *r) { return !__builtin_mul_overflow(a, b, r); }
static inline bool rawload_add(long long a, long long b, long long *r) { return !__builtin_add_overflow(a, b, r); }

static inline RawloadRoute rawload_route(const RawloadDesc &d)
{
    RawloadRoute R;
    const auto fail = [&](int status, const char *why) {
        R.status = status;
        R.why = why;
        return R;
    };
    if (d.in_kind != IMPDAR_RAW_I16 && d.in_kind != IMPDAR_RAW_I32 && d.in_kind != IMPDAR_RAW_F32)
        return fail(IMPDAR_ERR_UNSUPPORTED, "in_kind is none of I16, I32, F32");
    if (d.out_kind != IMPDAR_RAW_OUT_NATIVE && d.out_kind != IMPDAR_RAW_OUT_F32 && d.out_kind != IMPDAR_RAW_OUT_F64)
        return fail(IMPDAR_ERR_UNSUPPORTED, "out_kind is none of NATIVE, F32, F64");
    switch (d.op) {
    case IMPDAR_RAW_NONE:
        break;
    case IMPDAR_RAW_GSSI_TOP:
        if (d.in_kind == IMPDAR_RAW_F32) return fail(IMPDAR_ERR_UNSUPPORTED, "GSSI_TOP takes integer counts (I16, I32)");
        break;
    case IMPDAR_RAW_TEK_BIAS:
        if (d.in_kind != IMPDAR_RAW_I16) return fail(IMPDAR_ERR_UNSUPPORTED, "TEK_BIAS takes I16");
        break;
    case IMPDAR_RAW_PE_DEMEAN:
        if (d.in_kind == IMPDAR_RAW_I32) return fail(IMPDAR_ERR_UNSUPPORTED, "PE_DEMEAN takes I16 or F32");
        break;
    default:
        return fail(IMPDAR_ERR_UNSUPPORTED, "op is none of NONE, GSSI_TOP, TEK_BIAS, PE_DEMEAN");
    }
    R.in_bytes = d.in_kind == IMPDAR_RAW_I16 ? 2 : 4;
    R.native_kind = d.in_kind;
    R.out_bytes = d.out_kind == IMPDAR_RAW_OUT_F64 ? 8 : (d.out_kind == IMPDAR_RAW_OUT_F32 ? 4 : R.in_bytes);
    if (d.snum < 1 || d.tnum < 1) return fail(IMPDAR_ERR_ARG, "snum and tnum must be at least 1");
    if (d.op == IMPDAR_RAW_GSSI_TOP && d.snum < 3) return fail(IMPDAR_ERR_ARG, "GSSI_TOP needs snum >= 3");
    if (d.nbytes < 0 || d.base < 0 || d.stride < 0 || d.head < 0) return fail(IMPDAR_ERR_ARG, "a negative size or offset");
    long long samples, rec_end, span, last, end, total;
    // head + snum elem <= stride
    if (!rawload_mul(d.snum, R.in_bytes, &samples) || !rawload_add(d.head, samples, &rec_end))
        return fail(IMPDAR_ERR_ARG, "head + snum * elem overflows 64 bits");
    if (rec_end > d.stride) return fail(IMPDAR_ERR_ARG, "head + snum * elem exceeds the record stride");
    // base + (tnum - 1) stride + head + snum elem <= nbytes (stride * tnum itself must fit: the kernels form byte offsets below it)
    if (!rawload_mul(d.stride, d.tnum, &span) || !rawload_mul(d.stride, (long long)d.tnum - 1, &last) ||
        !rawload_add(d.base, last, &last) || !rawload_add(last, rec_end, &end) || !rawload_add(d.base, span, &span))
        return fail(IMPDAR_ERR_ARG, "base + stride * tnum overflows 64 bits");
    if (end > d.nbytes) return fail(IMPDAR_ERR_ARG, "the last record ends past the raw buffer");
    if (!rawload_mul(d.snum, d.tnum, &total) || !rawload_mul(total, R.out_bytes, &total))
        return fail(IMPDAR_ERR_ARG, "snum * tnum * sizeof(out) overflows 64 bits");
    R.total_bytes = total;
    R.last_end = end;
    R.status = IMPDAR_OK;
    R.why = "";
    return R;
}
