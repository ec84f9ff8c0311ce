// What fft.h declares and every unit with transforms shares: the once-per-process rocFFT setup, the lock its plans are created
// under, and the C entry points of the library's own row transforms (own_fft.h).
#include "fft.h"
#include "own_fft.h"
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <unistd.h>

static std::once_flag g_fft_once;
static int g_fft_rc = IMPDAR_OK;

int impdar_fft_global_setup()
{
    std::call_once(g_fft_once, [] {
        // rocFFT keeps the kernels of the plans it has built in a small user database; without one every new process
        // fetches them again from the 1.8 GB system database (0.25 s per plan with that file in the page cache, up to
        // 1.7 s from a cold disk: profiles/r05_first_call.txt) instead of 25 ms.  Where the user has not chosen a place
        // (ROCFFT_RTC_CACHE_PATH) and rocFFT's own default is not writable ($HOME on a batch node), give it one.
        if (!getenv("ROCFFT_RTC_CACHE_PATH")) {
            std::string dir;
            const char *xdg = getenv("XDG_CACHE_HOME"), *home = getenv("HOME");
            auto usable = [](const std::string &d) {
                if (d.empty()) return false;
                (void)mkdir(d.c_str(), 0700);
                return access(d.c_str(), W_OK | X_OK) == 0;
            };
            if (xdg && *xdg && usable(xdg)) dir = std::string(xdg) + "/impdar_amd";
            else if (home && *home && usable(std::string(home) + "/.cache")) dir = std::string(home) + "/.cache/impdar_amd";
            else dir = "/tmp/impdar_amd-" + std::to_string((long)getuid());
            if (usable(dir)) {
                const std::string path = dir + "/rocfft_kernel_cache.db";
                (void)setenv("ROCFFT_RTC_CACHE_PATH", path.c_str(), 0);
                impdar_trace("rocFFT user kernel cache: %s", path.c_str());
            }
        }
        impdar_trace("rocfft_setup: start");
        if (rocfft_setup() != rocfft_status_success) {
            g_fft_rc = IMPDAR_ERR_FFT;
        }
        impdar_trace("rocfft_setup: done");
    });
    if (g_fft_rc) impdar_set_error("rocfft_setup failed");
    return g_fft_rc;
}

std::mutex &impdar_fft_plan_mutex()
{
    static std::mutex mu;
    return mu;
}

// any: lengths 2^a 3^b 5^c 7^d too (impdar_fft_rows_any_dev)
static int fft_rows_dev(impdar_ctx *ctx, bool any, int mode, int dtype, int n, int batch, const void *d_in, void *d_out, double scale)
{
    IMPDAR_ARG_CHECK(ctx && d_in && d_out, "null argument");
    IMPDAR_ARG_CHECK(mode >= 0 && mode <= 4 && (dtype == IMPDAR_F32 || dtype == IMPDAR_F64) && batch >= 1, "bad mode / dtype / batch");
    const bool real = mode == OWN_R2C || mode == OWN_C2R;
    const int M = real ? n / 2 : n;
    const bool pow2 = n >= 2 && (n & (n - 1)) == 0 && own_fft_len_ok(M);
    if (any)
        IMPDAR_ARG_CHECK(pow2 || (n >= 2 && !(real && n % 2) && own_fft_mixed_len_ok(M)),
                         "length %d: the complex length must be 16 .. 8192 with no prime factor above 7 (a real length even)", n);
    else
        IMPDAR_ARG_CHECK(pow2, "length %d is not a power of two in range", n);
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    OwnTwiddles tw;
    int rc;
    const size_t cin = mode == OWN_R2C ? (size_t)n : (mode == OWN_C2R ? (size_t)M + 1 : (size_t)n);
    const size_t cout = mode == OWN_R2C ? (size_t)M + 1 : (size_t)n;
    if (dtype == IMPDAR_F32) {
        if ((rc = tw.ensure<float>(n, ctx->stream))) return rc;
        rc = own_fft_launch<float>(mode, n, (size_t)batch, d_in, d_out, cin, cout, scale, tw, ctx->stream);
    } else {
        if ((rc = tw.ensure<double>(n, ctx->stream))) return rc;
        rc = own_fft_launch<double>(mode, n, (size_t)batch, d_in, d_out, cin, cout, scale, tw, ctx->stream);
    }
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // (the table is this call's)
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_fft_rows_dev(impdar_ctx *ctx, int mode, int dtype, int n, int batch, const void *d_in, void *d_out, double scale)
{
    return fft_rows_dev(ctx, false, mode, dtype, n, batch, d_in, d_out, scale);
}

extern "C" int impdar_fft_rows_any_dev(impdar_ctx *ctx, int mode, int dtype, int n, int batch, const void *d_in, void *d_out, double scale)
{
    return fft_rows_dev(ctx, true, mode, dtype, n, batch, d_in, d_out, scale);
}
