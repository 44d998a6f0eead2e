// pmi_common.h — shared host/device helpers for libpicasso_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>

#include "../../include/picasso_hip.h"

#define PMI_WAVE 64

namespace pmi {

// Launch-shape and debugging variables (PMI_IDENTIFY_*, PMI_FIT_*, PMI_LQ_*, ...) are honoured only by a tuning build
// (make TUNING=1 -> -DPMI_TUNING): the shipped library reads none of them, so nothing in the environment can make it
// skip work or take another kernel.  (PMI_MLE_MODE, documented in picasso_hip.h, is the one variable it reads.)
#ifdef PMI_TUNING
inline const char *tuning_env(const char *name) { return getenv(name); }
#else
inline const char *tuning_env(const char *) { return nullptr; }
#endif

void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define PMI_HIP(call)                                                          \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) return pmi::hip_fail(e_, #call, __FILE__, __LINE__); \
    } while (0)

// Library state that lives in device memory or belongs to a device — scratch banks, unit-vector tables, the opt-in to more
// than 64 KB of dynamic LDS per kernel, FFT plans, side streams — is keyed by the device current in the calling thread
// (hipGetDevice), so that ONE process can drive several GPUs from one host thread each (localize_streamed(devices=...),
// INTEGRATION.md).  Settings (the modes, the number of frame ranges) stay process-wide.
constexpr int PMI_MAX_DEVICES = 16;
int current_device();                 // the calling thread's device, 0 if it cannot be asked; pmi_set_device refuses >= PMI_MAX_DEVICES
int checked_device(int *device);      // the same with a status: PMI_ERR_HIP / PMI_ERR_ARG (a device the library keeps no state for) instead of device 0
int device_cu_count();                // compute units of that device (cached per device)

// Grow-only scratch arena per device.  slot = purpose id.
//
// The rule.  A slot that grows is freed, so a pointer into it taken before is stale.  Hence: ONE carve per slot per call
// (scratch(), carve() or Staged::place()), and the slots of a host form are disjoint from those of every _dev form or
// helper it calls.  Who carves from which slot (host forms stage through Staged, further down):
//   SCR_STAGE_A   host  pmi_zfit, pmi_avgroi, pmi_gaussmle, pmi_get_spots, pmi_gausslq, pmi_identify, pmi_net_gradient,
//                       pmi_xcorr, pmi_rcc_pair_list / pmi_rcc_pairs / pmi_rcc_shifts (rcc_pair_list_impl: the fit windows
//                       stay resident here for rcc_fit_peaks), pmi_radial_sum, and the image layer's host forms
//                       (render_common.h)
//                 _dev  pmi_aim_partition_dev, pmi_aim_table_create_dev (aim::table_create), pmi_link_groups_dev,
//                       pmi_link_combine_dev, pmi_nena_hist_dev, pmi_cluster_counts_dev / _smlm_dev / _dbscan_dev,
//                       pmi_knn_order_dev, pmi_pairs_order_dev / _density_dev / _distance_hist_dev, pmi_picks_circle_dev /
//                       _shape_dev, pmi_similar_shift_dev, pmi_centers_order_dev / _stats_dev / _hull_dev,
//                       pmi_kinetics_dark_order_dev / _stats_dev, pmi_combine_order_dev / _stats_dev / _mindist_dev,
//                       pmi_fiducials_drift_dev, pmi_cumexp_fit_dev, pmi_frc_curve_dev, pmi_g5m_fit_dev / _fit_fixed_dev
//                       (the search state and one round's records), pmi_g5m_assign_dev
//   SCR_STAGE_B   host  none
//                 _dev  every rocPRIM temporary (rows::two_pass: the sorts and scans of the row, group, block and image
//                       layers, pmi_cumexp_fit_dev's segmented sort) and pmi_frc_curve_dev's spectra (it sorts nothing),
//                       pmi_g5m_fit_dev / _fit_fixed_dev's responsibilities beyond LDS (they sort nothing)
//   SCR_STAGE_C   host  pmi_cumexp_fit, pmi_frc_curve, pmi_aim_roi_cc, pmi_g5m_fit, pmi_g5m_fit_fixed, pmi_g5m_assign (inputs)
//                 _dev  the cut spots of a fit from the movie (fit_impl: pmi_gaussmle_movie_dev, pmi_localize_mle_dev;
//                       lq::launch: pmi_gausslq_movie_dev, pmi_localize_lq_dev), pmi_cluster_smlm_dev and
//                       pmi_cluster_frame_analysis_dev, the Gaussian renders (render_common.h)
//   SCR_STAGE_D   host  pmi_peak_fit, pmi_g5m_assign (outputs)
//                 _dev  the work arrays of every MLE and least-squares fit (fit_impl, lq::launch), pmi_blur_dev
//   SCR_FIT       host  pmi_rcc_shifts (rcc_fit_peaks, behind rcc_pair_list_impl's SCR_STAGE_A)
//                 _dev  every MLE fit (fit_impl)
//   SCR_RECORDS, SCR_RECORDS2, SCR_FRAME_COUNT, SCR_COUNTERS, SCR_NARROW, SCR_GATES
//                 _dev  identify_impl: pmi_identify_dev, every chunk of pmi_identify, the fused calls; SCR_RECORDS also the
//                       tile lists of the Gaussian renders (render_common.h)
//   SCR_IDS, SCR_ROWS, SCR_DEFER_PRIOR
//                 _dev  the fused calls pmi_localize_mle_dev and pmi_localize_lq_dev (fused_ranges, defer_prior_begin)
//   SCR_STATS, SCR_LQ_STATS
//                 _dev  every MLE fit and every least-squares fit: the 64 bytes LastFitStats reads later
enum ScratchSlot {
    SCR_RECORDS = 0,      // unordered identification records
    SCR_RECORDS2,         // frame-grouped records
    SCR_FRAME_COUNT,      // per-frame counts + cursors + bases
    SCR_COUNTERS,         // small counters
    SCR_IDS,              // frame/y/x/ng for the fused pipeline
    SCR_FIT,              // thetas/crlbs/ll/it for the fused pipeline
    SCR_STAGE_A,          // host-API staging (movie chunks)
    SCR_STAGE_B,
    SCR_STAGE_C,
    SCR_STAGE_D,
    SCR_ROWS,             // rows the fit stages of the fused pipelines may touch
    SCR_NARROW,           // uint16 copy of a chunk of a 32-bit movie (identify)
    SCR_GATES,            // per-chunk flags of that copy
    SCR_STATS,            // flag statistics of the last MLE fit (re-fit count, count per criterion)
    SCR_LQ_STATS,         // the same of the last least-squares fit (spots fitted again, count per reason)
    SCR_DEFER_PRIOR,      // accept-rate prior of the deferring scans and their per-range counts (DeferWords)
    SCR_NUM
};
int scratch(int slot, size_t bytes, void **ptr);

// one scratch slot cut into 256-byte aligned pieces; without a base it only measures
struct Arena {
    char *base = nullptr;
    size_t used = 0;
    template <typename T>
    T *take(size_t count)
    {
        T *p = base ? (T *)(base + used) : nullptr;
        used += (count * sizeof(T) + 255) & ~size_t(255);
        return p;
    }
};

// layout(Arena &) takes every piece of a call, in one order: it runs once to measure and once on the slot's buffer,
// so the size asked for is the size used.  The pieces start at the first one taken and span *used bytes.
template <typename Layout>
static int carve(int slot, Layout &&layout, size_t *used = nullptr)
{
    Arena measure;
    layout(measure);
    void *base = nullptr;
    const int rc = scratch(slot, measure.used, &base);
    if (rc != PMI_OK) return rc;
    Arena place;
    place.base = (char *)base;
    layout(place);
    if (used) *used = place.used;
    return PMI_OK;
}

// What a host form keeps on the device, in one slot: every piece is named once, with the host array it is filled from
// (`up`) or copied back to (`down`), or with neither (a work buffer); place() carves them all and uploads, fetch()
// downloads.  A piece of zero bytes is carved and never copied.
struct Staged {
    struct Piece { void **dev; size_t bytes; const void *up; void *down; };
    Piece pieces[12];
    int n = 0;
    const int slot;
    explicit Staged(int slot_) : slot(slot_) {}
    template <typename T>
    void add(T *&dev, size_t count, const void *up = nullptr, void *down = nullptr)
    {
        pieces[n++] = Piece{(void **)&dev, count * sizeof(T), up, down};
    }
    int place()
    {
        const int rc = carve(slot, [&](Arena &a) {
            for (int k = 0; k < n; k++) *pieces[k].dev = a.take<char>(pieces[k].bytes);
        });
        if (rc != PMI_OK) return rc;
        for (int k = 0; k < n; k++)
            if (pieces[k].up && pieces[k].bytes) PMI_HIP(hipMemcpy(*pieces[k].dev, pieces[k].up, pieces[k].bytes, hipMemcpyHostToDevice));
        return PMI_OK;
    }
    int fetch()
    {
        for (int k = 0; k < n; k++)
            if (pieces[k].down && pieces[k].bytes) PMI_HIP(hipMemcpy(pieces[k].down, *pieces[k].dev, pieces[k].bytes, hipMemcpyDeviceToHost));
        return PMI_OK;
    }
};

int scratch_release_all();
int scratch_enter_inner();           // -> the bank to hand back to scratch_leave_inner
void scratch_leave_inner(int was);
unsigned scratch_generation(int slot);      // of the current device and the calling thread's bank; bumped whenever a buffer of that slot (the bank or its inner bank) is released: pointers into it taken before are stale
unsigned scratch_generation_of(int device, int user_bank, int slot);
int scratch_user_bank();                    // the bank pmi_scratch_bank selected for the calling thread (its inner bank counts as the same)
// The side stream a fused call runs its second frame range on, with the events that join it to the caller's stream, and the
// events recorded behind the statistics kernels of a fit.  Process-wide, one per device, user bank and pipeline
// (0: MLE, 1: least squares), created on first use with that device current and kept for the life of the process: host
// threads come and go (localize_streamed starts lane threads per call), what belongs to a device does not.  Two threads on
// one device and bank are serialised by the caller (picasso_amd/_lib.py lock()), as for the scratch buffers.
struct SideLane { hipStream_t s2 = nullptr; hipEvent_t ev_start = nullptr, ev_scan_a = nullptr, ev_b = nullptr, stats_done[2] = {nullptr, nullptr}; };
int side_lane(int pipeline, SideLane **lane);

// Statistics of the calling thread's last fit of one pipeline (0: MLE, SCR_STATS: [0] spots re-fitted, [1..] spots flagged per
// criterion; 1: least squares, SCR_LQ_STATS: [0] spots fitted again, [1..8] why): a 64-byte device buffer per frame range of
// the call, read behind the event recorded after its statistics kernel (the stream the fit ran on may be gone by then) and
// only while the scratch generation it was taken from stands.
struct LastFitStats {
    int device = 0, bank = 0, slot = 0;
    unsigned generation = 0;
    const unsigned *buf[2] = {nullptr, nullptr};     // [1]: the second frame range of a fused call
    hipEvent_t done[2] = {nullptr, nullptr};         // the events belong to the device's side lane, not to this thread
    // after the statistics kernel of frame range `range` (0: a whole call, or the first range) is queued on s
    int record(int pipeline, int range, const unsigned *stats, hipStream_t s);
    bool valid() const;
    int read(unsigned (&h)[16]) const;               // the ranges' sums; zeros when there is no fit or its buffers are gone
};

// The schedule of the fused calls (pmi_localize_mle_dev, pmi_localize_lq_dev): identify, fit, table, with the frames cut in
// two ranges when that pays (runtime.hip).  The caller supplies its parts; `ids` is one range's SCR_IDS buffer of ids_bytes.
struct FusedRanges {
    unsigned *defer_words = nullptr;   // DeferWords of a call whose scan may defer (else nullptr): fit_rows_kernel folds a range's counts into the prior
    size_t ids_bytes;
    int64_t capc;          // rows of a range's identification / fit arrays: the candidates it may hold
    int64_t cap;           // rows of the table
    bool rejects;          // the fit may reject candidates: `accepted` counts those it kept (else accepted == candidates)
    std::function<int(void *ids, int64_t f_lo, int64_t f_hi, int64_t *d_cnt, int range, hipStream_t st)> scan;
    std::function<int(void *ids, const int64_t *d_rows, int range, hipStream_t st)> fit;
    std::function<const unsigned *(void *ids)> accepted;
    std::function<int(void *ids, const int64_t *d_rows, const int64_t *d_row0, hipStream_t st)> table;
};
int fused_ranges(const FusedRanges &c, int pipeline, int64_t F, int64_t Y, int64_t X, int64_t f_lo, int64_t f_hi,
                 int64_t *d_out_n, hipStream_t s);

// Accept-rate prior of the deferring scan (identify_fast.hip): 16 words of device memory per (device, user bank), in the outer
// bank's SCR_DEFER_PRIOR.  A scan of frame range r reads the prior pair and adds its own counts to the statistics words of r;
// the one-thread kernel queued behind it (fit_rows_kernel) folds them into the prior, keeps them for
// pmi_localize_last_scan_decisions and clears them.  Range B's scan starts behind that kernel of range A (ev_scan_a) and the
// next call's scan A behind both ranges: every scan reads a settled prior that nobody writes while it runs.
enum DeferWords {
    DW_PRIOR = 0,         // (seen, kept): candidates earlier scans decided in exact rounds, and how many of them they kept
    DW_STATS = 4,         // + 4 * range: (decided, kept, emitted undecided, -) of the scan in flight
    DW_LAST = 12,         // + 2 * range: (decided, emitted undecided) of the last call's scans
    DW_NUM = 16
};
// The pair is halved while it holds more than this: a scan that decides a few tens of thousands of candidates outweighs what
// the calls before it saw within a few calls (a movie whose density drifts), and the sums stay far from 2^32.
constexpr unsigned DEFER_PRIOR_BOUND = 1u << 18;
// Everything the accept rate depends on besides the pixels: a call with another key starts without a prior.
struct DeferKey {
    int dtype = -1, box = 0;
    int64_t Y = 0, X = 0, roi[4] = {0, 0, 0, 0};
    double min_ng = 0.0;
    bool operator==(const DeferKey &o) const {
        return dtype == o.dtype && box == o.box && Y == o.Y && X == o.X && roi[0] == o.roi[0] && roi[1] == o.roi[1] &&
               roi[2] == o.roi[2] && roi[3] == o.roi[3] && min_ng == o.min_ng;
    }
};
// The words of the calling thread's device and bank for a deferring call with this key, cleared on `s` when the key, the
// buffer or the reset epoch is not what the last call left (no prior).  Call with the OUTER bank selected.
int defer_prior_begin(const DeferKey &key, unsigned **words, hipStream_t s);
void defer_prior_none();             // the calling thread's fused call does not defer: pmi_localize_last_scan_decisions reports zeros
void defer_prior_reset();            // every (device, bank) starts its next call without a prior

int identify_impl(const void *d_movie, int dtype, int64_t F, int64_t Y, int64_t X, int box, double min_ng,
                  const int64_t *roi4, int64_t f_lo, int64_t f_hi, int64_t label_offset,
                  int32_t *d_frame, int32_t *d_y, int32_t *d_x, float *d_ng, int64_t cap, int64_t *d_out_n,
                  bool defer_exact, hipStream_t s, const unsigned *prior_in = nullptr, unsigned *stats_out = nullptr);

struct Record {   // one identification, 16 B
    int32_t frame;
    uint32_t yx;      // y << 16 | x (frames are at most 65535 x 65535 on this path)
    int32_t pad;      // 0: keeps a record one 16-byte store
    float ng;
};
__host__ __device__ __forceinline__ uint32_t pack_yx(int y, int x) { return ((uint32_t)y << 16) | (uint32_t)(x & 0xffff); }
// A fused pipeline may ask the packed scan to leave the exact stage (float32 net gradient in the reference's order,
// first-argmax rule: picasso/localize.py:97-134, 202-244, 288) to the fit's start-value kernel, which reads the very
// rows it needs: the scan then emits CANDIDATES whose net gradient is this NaN pattern (an accepted identification's
// net gradient is never NaN: it passed `ng > min_ng`), and the start-value kernel decides them (gaussmle_g8.hip).
constexpr uint32_t NG_DEFERRED_BITS = 0x7fc0d1feu;
// the scan kernel the calling thread launched last, as rocprofv3 names it (+ " defer" when it may leave its exact stage to
// the fit): pmi_last_scan_kernel, so that a benchmark can tell which kernel a committed counter file belongs to
extern thread_local char g_last_scan_kernel[128];
extern int g_localize_ranges;        // frame ranges a fused call keeps in flight (pmi_localize_set_ranges)

// pixel load as float32 (the reference's np.float32(frame), localize.py:332)
template <typename T>
__device__ __forceinline__ float px_f32(const T *p, int64_t i) { return (float)p[i]; }

struct KernelTimes { float scan_ms, fit_ms; };
extern bool g_kernel_timing;
extern KernelTimes g_last_times;

struct ScopedKernelTimer {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s;
    float *dst;
    ScopedKernelTimer(hipStream_t stream, float *dst_) : s(stream), dst(dst_) {
        if (g_kernel_timing) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, s); }
    }
    void stop() {
        if (a) { (void)hipEventRecord(b, s); }
    }
    ~ScopedKernelTimer() {
        if (a) {
            (void)hipEventSynchronize(b);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, a, b);
            *dst = ms;
            (void)hipEventDestroy(a); (void)hipEventDestroy(b);
        }
    }
};

}  // namespace pmi
