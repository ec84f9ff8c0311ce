// The cached plan of the phase shift: transform plans, twiddles and every device buffer a call of ps_run may need, kept
// from call to call (g_ps_plan in phaseshift.hip owns the one instance).
#pragma once
#include "fft.h"                // FftPlan, DevBuf
#include "own_fft.h"            // OwnTwiddles
#include "ps_path_plan.h"       // PsMfmaRun
#include "ps_series_plan.h"     // SrHostPlan

struct PsPlan {
    // A device buffer of the plan is a Buf{this}: it enrols itself in dev_, which release_device() walks.
    std::vector<DevBuf *> dev_;
    struct Buf : DevBuf {
        explicit Buf(PsPlan *pl) { pl->dev_.push_back(this); }
    };
    OwnTwiddles tw_time, tw_trace;       // the library's own row transforms (own_fft.h): what the first call of a size runs on
    Buf d_taper{this};                     // [tnum + snum] float64 taper weights (the transform over the traces taken first: P.fhalf)
    int own_calls = 0;                   // ... calls of this size that did
    int dtype = -1, snum = 0, tnum = 0, nt = 0;
    const impdar_ctx *owner = nullptr;   // plans and buffers live on this context's device and stream
    FftPlan f_time, f_trace, b_trace;
    // launch order of the runs kernels (ps_order_rows) and what it was made from: kept for the next call
    std::vector<double> rm_kx, rm_ws, rm_v;
    int rm_state = -1;                   // -1 none, 0 natural order, 1 d_rowmap holds the order
    bool rows_form = true;               // b_trace / r_trace / b_slab run on contiguous rows of transposed arrays (else rocFFT's strided plans)
    FftPlan r_time, r_trace;             // Hermitian walk: real-to-complex along time (nt/2 + 1 rows), then over the traces
    bool r_ready = false, c_ready = false;
    Buf Xr{this};                        // ... its real input [tnum][nt]
    FftPlan b_slab;                      // kx-sharded run: inverse transform over k of this rank's depth rows
    int slab_key[3] = {-1, -1, -1};
    const impdar_ctx *slab_owner = nullptr;
    Buf d_sendbuf{this}, d_slab{this};   // ... packed blocks of the all-to-all; the transposed slab
    Buf d_blocks{this}, d_edge{this}, d_runtab{this};   // matrix-core path: row-block table; boundary-frequency counts + lists; per-run phases
    Buf d_pr_runs{this}, d_pr_stages{this}, d_rw{this}; // many-runs matrix-core path (ps_runs.h): runs, stages, 1 / w
    Buf d_mcount{this};                  // matrix-core paths: MFMA instructions the kernel issued (one 64-bit counter)
    Buf d_pn_pieces{this}, d_pn_corr{this}, d_pn_e1{this};    // transform path (ps_nufft.h): pieces, the window's correction tables, the first-order sums
    SrHostPlan sr_plan;                  // series path (ps_series.h): the pieces of the last velocity profile, and on the device
    Buf d_sr_pieces{this}, d_sr_ev{this};
    bool sr_dev = false;                 // ... the device copies are those of sr_plan
    OwnTwiddles pn_tw[14];               // ... twiddles of the grid lengths 2^l
    std::vector<float> h_pn_corr;        // ... the tables on the host (made once per padded length)
    std::vector<double> h_pn_corr64;
    int pn_corr_off[2][13] = {{-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}};     // [float32, float64]
    int pn_corr_dev = -1;                // which of the two tables the device buffer holds
    double mfma_instructions = -1.0;     // ... of the last call (-1: not a matrix-core call)
    // a (kx, runs) geometry whose boundary-frequency lists overflowed in a matrix-core path: not tried again
    std::vector<double> ovf_kx;
    std::vector<PsMfmaRun> ovf_runs;
    Buf X{this}, TK{this}, d_kx{this}, d_w{this}, d_vz{this}, d_thr{this}, d_sched{this}, d_rowmap{this}, d_eps{this}, d_sm{this}, d_part{this};
    std::vector<double> h_sm_step, h_sm_tile;
    bool b_ready = false;
    // another device / stream: drop everything bound to the old one (tw_time / tw_trace rebuild themselves)
    void release_device()
    {
        for (DevBuf *b : dev_) b->release();
        for (OwnTwiddles &t : pn_tw) {
            t.buf.release();
            t.nt = 0;
        }
        pn_corr_dev = -1;
        sr_dev = false;
    }
};
