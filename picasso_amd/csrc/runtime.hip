// runtime.hip — library state: errors, device selection, memory, scratch, events.
#include <stdarg.h>

#include <mutex>

#include "pmi_common.h"

namespace pmi {

static thread_local char g_err[512] = "";
bool g_kernel_timing = false;
KernelTimes g_last_times = {0.f, 0.f};
int g_localize_ranges = 2;          // pmi_localize_set_ranges (gaussmle.hip); read by both fused calls
thread_local char g_last_scan_kernel[128] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char *what, const char *file, int line)
{
    set_error("HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    return PMI_ERR_HIP;
}

struct ScratchBuf { void *p = nullptr; size_t bytes = 0; };
// Two banks: a caller that keeps two pipelines in flight on two streams (frame range A fitting while range B is
// scanned) gives each its own scratch (pmi_scratch_bank); everything else lives in bank 0.
constexpr int SCR_USER_BANKS = 2;                 // what pmi_scratch_bank selects
constexpr int SCR_BANKS = 2 * SCR_USER_BANKS;      // + one inner bank each: the second frame range a fused call keeps in flight
static ScratchBuf g_scratch_banks[PMI_MAX_DEVICES][SCR_BANKS][SCR_NUM];      // [device]: a buffer belongs to the device it was allocated on
// the bank is a property of the calling thread: two host threads that drive two streams select a bank each
// (pmi_scratch_bank) and never see each other's records or fit state
static thread_local int g_scratch_bank = 0;
static std::mutex g_scratch_mu[PMI_MAX_DEVICES];      // one per device: growth on one device (a device-wide synchronise) does not stall the others' lanes
// per device, USER bank (a bank and its inner bank count as one) and slot: a record in one slot outlives the growth of
// another, and the statistics of a lane on bank 0 outlive growth in the other lane of the same device
static unsigned g_scratch_generation[PMI_MAX_DEVICES][SCR_USER_BANKS][SCR_NUM] = {};
int scratch_user_bank() { return g_scratch_bank % SCR_USER_BANKS; }
unsigned scratch_generation_of(int device, int user_bank, int slot)
{
    std::lock_guard<std::mutex> lk(g_scratch_mu[device]);
    return g_scratch_generation[device][user_bank % SCR_USER_BANKS][slot];
}
unsigned scratch_generation(int slot) { return scratch_generation_of(current_device(), scratch_user_bank(), slot); }

int current_device()
{
    // pmi_set_device refuses devices >= PMI_MAX_DEVICES; a thread put on one behind the library's back (hipSetDevice, torch)
    // is refused by checked_device() at the head of every scratch() call instead of being aliased to device 0's state
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= PMI_MAX_DEVICES) return 0;
    return dev;
}
int checked_device(int *device)
{
    int dev = 0;
    PMI_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= PMI_MAX_DEVICES) {
        set_error("the calling thread is on device %d: the library keeps state for devices 0 ... %d", dev, PMI_MAX_DEVICES - 1);
        return PMI_ERR_ARG;
    }
    *device = dev;
    return PMI_OK;
}
int device_cu_count()
{
    static int cus[PMI_MAX_DEVICES] = {};
    const int dev = current_device();
    int n = __atomic_load_n(&cus[dev], __ATOMIC_RELAXED);
    if (!n) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        __atomic_store_n(&cus[dev], n, __ATOMIC_RELAXED);
    }
    return n;
}

int scratch(int slot, size_t bytes, void **ptr)
{
    int dev = 0;
    const int rc = checked_device(&dev);
    if (rc != PMI_OK) return rc;
    std::lock_guard<std::mutex> lk(g_scratch_mu[dev]);
    ScratchBuf &b = g_scratch_banks[dev][g_scratch_bank][slot];
    if (b.bytes < bytes) {
        if (b.p) { PMI_HIP(hipDeviceSynchronize()); PMI_HIP(hipFree(b.p)); b.p = nullptr; b.bytes = 0; g_scratch_generation[dev][scratch_user_bank()][slot]++; }
        size_t want = bytes + bytes / 4 + 4096;   // headroom so repeated calls stop reallocating
        PMI_HIP(hipMalloc(&b.p, want));
        b.bytes = want;
    }
    *ptr = b.p;
    return PMI_OK;
}

int scratch_release_all()
{
    // every device's buffers: each is synchronised and freed with its own device current, the caller's device is restored
    const int was = current_device();
    int rc = PMI_OK;
    for (int dev = 0; dev < PMI_MAX_DEVICES; dev++) {
        std::lock_guard<std::mutex> lk(g_scratch_mu[dev]);
        bool any = false;
        for (auto &bank : g_scratch_banks[dev])
            for (auto &b : bank) any = any || b.p;
        for (auto &bank : g_scratch_generation[dev])
            for (unsigned &g : bank) g++;
        if (!any) continue;
        if (hipSetDevice(dev) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { rc = PMI_ERR_HIP; set_error("pmi_release_scratch: device %d cannot be synchronised", dev); continue; }
        for (auto &bank : g_scratch_banks[dev])
            for (auto &b : bank)
                if (b.p) { if (hipFree(b.p) != hipSuccess) rc = PMI_ERR_HIP; b.p = nullptr; b.bytes = 0; }
    }
    (void)hipSetDevice(was);
    return rc;
}
int scratch_select_bank(int bank)
{
    if (bank < 0 || bank >= SCR_USER_BANKS) { set_error("scratch bank %d out of range", bank); return PMI_ERR_ARG; }
    g_scratch_bank = bank;
    return PMI_OK;
}
// the inner bank of the calling thread's bank (and back): scratch of the second frame range of a fused call
int scratch_enter_inner() { const int was = g_scratch_bank; g_scratch_bank = was % SCR_USER_BANKS + SCR_USER_BANKS; return was; }
void scratch_leave_inner(int was) { g_scratch_bank = was; }

static SideLane g_side_lanes[PMI_MAX_DEVICES][SCR_USER_BANKS][2];
static std::mutex g_side_mu;
int side_lane(int pipeline, SideLane **lane)
{
    int dev = 0;
    const int rc = checked_device(&dev);
    if (rc != PMI_OK) return rc;
    std::lock_guard<std::mutex> lk(g_side_mu);
    SideLane &sd = g_side_lanes[dev][scratch_user_bank()][pipeline ? 1 : 0];
    if (!sd.s2) {
        hipStream_t s2 = nullptr;
        PMI_HIP(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
        PMI_HIP(hipEventCreateWithFlags(&sd.ev_start, hipEventDisableTiming));
        PMI_HIP(hipEventCreateWithFlags(&sd.ev_scan_a, hipEventDisableTiming));
        PMI_HIP(hipEventCreateWithFlags(&sd.ev_b, hipEventDisableTiming));
        PMI_HIP(hipEventCreateWithFlags(&sd.stats_done[0], hipEventDisableTiming));
        PMI_HIP(hipEventCreateWithFlags(&sd.stats_done[1], hipEventDisableTiming));
        sd.s2 = s2;                        // last: a lane with a stream is complete
    }
    *lane = &sd;
    return PMI_OK;
}

// ---- the accept-rate prior of the deferring scans (pmi_common.h DeferWords) -------------------------------------------------
// Host side: per (device, user bank) the key of the call that left the words, the generation of their buffer and the reset epoch.
struct DeferPriorState { bool has_key = false, last = false; DeferKey key; unsigned generation = 0, epoch = 0; const unsigned *words = nullptr; };
static DeferPriorState g_defer_prior[PMI_MAX_DEVICES][SCR_USER_BANKS];
static std::mutex g_defer_mu;
static unsigned g_defer_epoch = 0;       // bumped by defer_prior_reset
int defer_prior_begin(const DeferKey &key, unsigned **words, hipStream_t s)
{
    int dev = 0;
    int rc = checked_device(&dev);
    if (rc != PMI_OK) return rc;
    void *ptr = nullptr;
    if ((rc = scratch(SCR_DEFER_PRIOR, DW_NUM * sizeof(unsigned), &ptr)) != PMI_OK) return rc;
    const unsigned gen = scratch_generation_of(dev, scratch_user_bank(), SCR_DEFER_PRIOR);
    bool cold;
    {
        std::lock_guard<std::mutex> lk(g_defer_mu);
        DeferPriorState &st = g_defer_prior[dev][scratch_user_bank()];
        cold = !st.has_key || !(st.key == key) || st.generation != gen || st.epoch != g_defer_epoch || st.words != ptr;
        st.has_key = true; st.last = true; st.key = key; st.generation = gen; st.epoch = g_defer_epoch; st.words = (const unsigned *)ptr;
    }
    if (cold) PMI_HIP(hipMemsetAsync(ptr, 0, DW_NUM * sizeof(unsigned), s));
    *words = (unsigned *)ptr;
    return PMI_OK;
}
void defer_prior_none()
{
    std::lock_guard<std::mutex> lk(g_defer_mu);
    g_defer_prior[current_device()][scratch_user_bank()].last = false;
}
void defer_prior_reset()
{
    std::lock_guard<std::mutex> lk(g_defer_mu);
    g_defer_epoch++;
}
// (decided in the scan, emitted undecided) per range of the calling thread's last fused MLE call; zeros when it did not defer or
// its words are gone
static int defer_last_decisions(int64_t *out4, hipStream_t s)
{
    for (int i = 0; i < 4; i++) out4[i] = 0;
    const unsigned *words = nullptr;
    {
        const int dev = current_device(), bank = scratch_user_bank();
        const unsigned gen = scratch_generation_of(dev, bank, SCR_DEFER_PRIOR);
        std::lock_guard<std::mutex> lk(g_defer_mu);
        const DeferPriorState &st = g_defer_prior[dev][bank];
        if (st.has_key && st.last && st.generation == gen) words = st.words;
    }
    if (!words) return PMI_OK;
    PMI_HIP(hipStreamSynchronize(s));        // the call has joined its side stream to s before it returned
    unsigned h[4];
    PMI_HIP(hipMemcpy(h, words + DW_LAST, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; i++) out4[i] = h[i];
    return PMI_OK;
}

int LastFitStats::record(int pipeline, int range, const unsigned *stats, hipStream_t s)
{
    SideLane *lane = nullptr;
    const int rc = side_lane(pipeline, &lane);
    if (rc != PMI_OK) return rc;
    PMI_HIP(hipEventRecord(lane->stats_done[range], s));
    if (range == 0) buf[1] = nullptr;
    buf[range] = stats;
    done[range] = lane->stats_done[range];
    slot = pipeline ? SCR_LQ_STATS : SCR_STATS;
    device = current_device();
    bank = scratch_user_bank();
    generation = scratch_generation_of(device, bank, slot);
    return PMI_OK;
}
bool LastFitStats::valid() const { return buf[0] && generation == scratch_generation_of(device, bank, slot); }
int LastFitStats::read(unsigned (&h)[16]) const
{
    for (unsigned &v : h) v = 0;
    if (!valid()) return PMI_OK;      // no fit yet, or its buffers are gone
    for (int k = 0; k < 2; k++) {
        if (!buf[k]) continue;
        unsigned part[16];
        PMI_HIP(hipEventSynchronize(done[k]));
        PMI_HIP(hipMemcpy(part, buf[k], 64, hipMemcpyDeviceToHost));
        for (int i = 0; i < 16; i++) h[i] += part[i];
    }
    return PMI_OK;
}

// ---- the fused calls' frame ranges -----------------------------------------------------------------------------
// rows: [0] rows of A to fit, [1] rows of B to fit, [2] rows of A for the table, [3] rows of B for the table, [4] row offset of B.
// A range whose candidates overflow its arrays (their columns were not written) fits none of them.
// A deferring scan (dw: its DeferWords, pmi_common.h) has added its counts to the statistics words of its range: they are folded
// into the prior pair here, behind the scan and in front of whatever starts next — scan B waits for this kernel of range A,
// the next call's scan A for both — kept for pmi_localize_last_scan_decisions, and cleared for the next scan of the range.
__global__ void fit_rows_kernel(const int64_t *__restrict__ n_cand, int64_t capc, int64_t *__restrict__ rows_fit,
                                unsigned *__restrict__ dw, int range)
{
    *rows_fit = *n_cand > capc ? 0 : *n_cand;
    if (dw) {
        unsigned *st = dw + DW_STATS + 4 * range;
        unsigned seen = dw[DW_PRIOR] + st[0], kept = dw[DW_PRIOR + 1] + st[1];
        while (seen > DEFER_PRIOR_BOUND) { seen >>= 1; kept >>= 1; }       // old evidence fades
        dw[DW_PRIOR] = seen; dw[DW_PRIOR + 1] = kept;
        dw[DW_LAST + 2 * range] = st[0]; dw[DW_LAST + 2 * range + 1] = st[2];
        if (range == 0) dw[DW_LAST + 2] = dw[DW_LAST + 3] = 0;             // (a call of one range)
        st[0] = st[1] = st[2] = 0;
    }
}
// The table rows once every count is known (cand_b == nullptr: one range; acc_* == nullptr: every candidate was kept).  A
// range that overflowed its arrays: *d_out_n is the candidates' number, an upper bound of the rows; more rows than the
// table holds: *d_out_n is theirs.  Either way no table row is written.
__global__ void table_rows_kernel(const int64_t *__restrict__ cand_a, const unsigned *__restrict__ acc_a,
                                  const int64_t *__restrict__ cand_b, const unsigned *__restrict__ acc_b, int64_t capc,
                                  int64_t cap, int64_t *__restrict__ rows, int64_t *__restrict__ d_out_n)
{
    const int64_t ca = *cand_a, cb = cand_b ? *cand_b : 0;
    const bool overflow = ca > capc || cb > capc;
    const int64_t a = overflow ? 0 : (acc_a ? (int64_t)*acc_a : ca);
    const int64_t b = overflow ? 0 : (acc_b ? (int64_t)*acc_b : cb);
    const bool fits = !overflow && a + b <= cap;
    rows[2] = fits ? a : 0;
    rows[3] = fits ? b : 0;
    rows[4] = a;
    *d_out_n = overflow ? ca + cb : a + b;
}

// The scan is bound by memory requests, the fit by VALU issue: the scan of frame range B beside the fit of range A takes
// less than the two one after the other.  A large call therefore cuts its frames in two: stream s runs
// scan A, fit A; the side stream of the device's lane runs scan B (started when scan A is done) and fit B, with scratch from
// the inner bank; the table is written once both counts are known (A's rows, then B's), so the capacity contract holds for
// the sum.  A fit that keeps every candidate lets the last range fit its table rows, so that the counts need one kernel.
int fused_ranges(const FusedRanges &c, int pipeline, int64_t F, int64_t Y, int64_t X, int64_t f_lo, int64_t f_hi,
                 int64_t *d_out_n, hipStream_t s)
{
    const int64_t lo = f_lo < 0 ? 0 : f_lo, hi = f_hi > F - 1 ? F - 1 : f_hi, nf = hi - lo + 1;
    // two ranges pay when each keeps the chip busy for a while (below ~1e8 pixels a range is a few tens of microseconds)
    const bool two = g_localize_ranges == 2 && !g_kernel_timing && nf >= 16 && (double)nf * (double)Y * (double)X >= 2.5e8;
    void *ptr = nullptr, *cptr = nullptr;
    int rc;
    // the counts of the ranges and the row bookkeeping live in the OUTER bank (both streams read them)
    if ((rc = scratch(SCR_ROWS, 8 * sizeof(int64_t), &cptr)) != PMI_OK) return rc;
    int64_t *n = (int64_t *)cptr, *rows = n + 2;              // n[r]: candidates of range r
    if ((rc = scratch(SCR_IDS, c.ids_bytes, &ptr)) != PMI_OK) return rc;
    void *ids[2] = {ptr, nullptr};
    auto table_rows = [&](hipStream_t st) {
        hipLaunchKernelGGL(table_rows_kernel, dim3(1), dim3(1), 0, st, (const int64_t *)n, c.rejects ? c.accepted(ids[0]) : nullptr,
                           (const int64_t *)(two ? n + 1 : nullptr), c.rejects && two ? c.accepted(ids[1]) : nullptr, c.capc,
                           c.cap, rows, d_out_n);
    };
    // the rows range r fits: its candidates, or, when the fit keeps every candidate, the last range its table rows
    auto fit_rows = [&](int r, hipStream_t st) -> const int64_t * {
        if (!c.rejects && r == (two ? 1 : 0)) {
            table_rows(st);
            return rows + 2 + r;
        }
        hipLaunchKernelGGL(fit_rows_kernel, dim3(1), dim3(1), 0, st, (const int64_t *)(n + r), c.capc, rows + r, c.defer_words, r);
        return rows + r;
    };
    if (!two) {
        if ((rc = c.scan(ids[0], f_lo, f_hi, n, 0, s)) != PMI_OK) return rc;
        if ((rc = c.fit(ids[0], fit_rows(0, s), 0, s)) != PMI_OK) return rc;
    } else {
        SideLane *side_p = nullptr;
        if ((rc = side_lane(pipeline, &side_p)) != PMI_OK) return rc;
        SideLane &side = *side_p;
        const int64_t mid = lo + nf / 2 - 1;                  // A = [lo, mid], B = [mid + 1, hi]
        PMI_HIP(hipEventRecord(side.ev_start, s));           // the side stream joins the caller's stream order here
        PMI_HIP(hipStreamWaitEvent(side.s2, side.ev_start, 0));
        // From here on work may be queued on the side stream: whatever happens, the caller's stream is ordered after it
        // before this call returns (a caller that frees or reuses its buffers on an error must not race kernels on s2).
        struct Join {
            SideLane &sd; hipStream_t st; bool done = false;
            ~Join() { if (!done) { (void)hipEventRecord(sd.ev_b, sd.s2); (void)hipStreamWaitEvent(st, sd.ev_b, 0); } }
        } join{side, s};
        // ---- range A on the caller's stream
        if ((rc = c.scan(ids[0], lo, mid, n, 0, s)) != PMI_OK) return rc;
        const int64_t *rows_a = fit_rows(0, s);
        PMI_HIP(hipEventRecord(side.ev_scan_a, s));
        if ((rc = c.fit(ids[0], rows_a, 0, s)) != PMI_OK) return rc;
        // ---- range B on the side stream, scratch from the inner bank; its scan starts when scan A is done
        PMI_HIP(hipStreamWaitEvent(side.s2, side.ev_scan_a, 0));
        const int outer = scratch_enter_inner();
        rc = scratch(SCR_IDS, c.ids_bytes, &ids[1]);
        if (rc == PMI_OK) rc = c.scan(ids[1], mid + 1, hi, n + 1, 1, side.s2);
        if (rc == PMI_OK) rc = c.fit(ids[1], fit_rows(1, side.s2), 1, side.s2);
        scratch_leave_inner(outer);
        if (rc != PMI_OK) return rc;
        PMI_HIP(hipEventRecord(side.ev_b, side.s2));
        PMI_HIP(hipStreamWaitEvent(s, side.ev_b, 0));
        join.done = true;
    }
    // ---- the table, once every count is known: A's rows, then B's
    if (c.rejects) table_rows(s);
    if ((rc = c.table(ids[0], rows + 2, nullptr, s)) != PMI_OK) return rc;
    if (two && (rc = c.table(ids[1], rows + 3, rows + 4, s)) != PMI_OK) return rc;
    PMI_HIP(hipGetLastError());
    return PMI_OK;
}

void release_fft_plans();   // xcorr.hip

}  // namespace pmi

extern "C" {

int pmi_version(void) { return 126; }   // 0.1.26: + pmi_g5m_* (G5M molecular mapping in 2-D); 0.1.25: + pmi_rotate_locs / pmi_render_hist_rot / pmi_render_gaussian_rot and their _dev forms (rotated views); 0.1.24: + pmi_cumexp_fit_dev / pmi_cumexp_fit (kinetic rates of picks); 0.1.23: + pmi_blur_dev / pmi_blur / pmi_render_blurred (image blur); 0.1.22: + pmi_similar_shift_dev / pmi_similar_filter (pick_similar); 0.1.21: + pmi_fiducials_* (fiducial undrift); 0.1.20: + pmi_picks_* (picked localizations); 0.1.19: + pmi_frc_* / pmi_radial_sum (Fourier ring correlation); 0.1.18: + pmi_average_* (particle averaging); 0.1.17: + pmi_localize_reset_defer_prior / pmi_localize_last_scan_decisions (accept-rate prior of the deferring scan); 0.1.16: + pmi_areas_* (cluster areas and volumes); 0.1.15: + pmi_combine_* (cluster combine and its nearest-cluster distances); 0.1.14: + pmi_knn_* (nearest-neighbour distances); 0.1.13: + pmi_kinetics_* (dark times, group properties); 0.1.12: + pmi_centers_* (cluster centers); 0.1.11: + pmi_pairs_* (local density, distance histogram); 0.1.10: + pmi_cluster_* (DBSCAN, the SMLM clusterer); 0.1.9: + pmi_link_* / pmi_nena_hist_dev (link, NeNA); 0.1.8: - the pixel hand-off from the scan to the fit and its setter; 0.1.7: + pmi_aim_* (AIM undrift); 0.1.6: round 6 (32-bit integer movies on the key scan, side lanes per (device, bank); + pmi_mle_set_libm / pmi_mle_get_libm / pmi_libm_eval_dev)

const char *pmi_last_error(void) { return pmi::g_err; }

int pmi_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pmi_set_device(int device)
{
    // the calling THREAD's device (HIP keeps it per thread); everything the library keeps on a device is keyed by it
    if (device < 0 || device >= pmi::PMI_MAX_DEVICES || device >= pmi_device_count()) {
        pmi::set_error("pmi_set_device: no device %d (%d visible, at most %d supported)", device, pmi_device_count(), pmi::PMI_MAX_DEVICES);
        return PMI_ERR_ARG;
    }
    PMI_HIP(hipSetDevice(device));
    return PMI_OK;
}

int pmi_last_scan_kernel(char *name, size_t name_len)
{
    if (name && name_len) { strncpy(name, pmi::g_last_scan_kernel, name_len - 1); name[name_len - 1] = 0; }
    return PMI_OK;
}

int pmi_get_device(int *device)
{
    int dev = 0;
    PMI_HIP(hipGetDevice(&dev));
    if (device) *device = dev;
    return PMI_OK;
}

int pmi_device_info(char *name, size_t name_len, int *compute_units, size_t *total_mem_bytes)
{
    int dev = 0;
    PMI_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    PMI_HIP(hipGetDeviceProperties(&prop, dev));
    if (name && name_len) { strncpy(name, prop.gcnArchName, name_len - 1); name[name_len - 1] = 0; }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (total_mem_bytes) *total_mem_bytes = prop.totalGlobalMem;
    return PMI_OK;
}

int pmi_malloc(void **dptr, size_t bytes) { PMI_HIP(hipMalloc(dptr, bytes)); return PMI_OK; }
int pmi_free(void *dptr) { PMI_HIP(hipFree(dptr)); return PMI_OK; }
int pmi_memcpy_h2d(void *d, const void *h, size_t bytes) { PMI_HIP(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)); return PMI_OK; }
int pmi_memcpy_d2h(void *h, const void *d, size_t bytes) { PMI_HIP(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost)); return PMI_OK; }
int pmi_stream_synchronize(void *stream) { PMI_HIP(hipStreamSynchronize((hipStream_t)stream)); return PMI_OK; }
int pmi_stream_create(void **stream)
{
    // non-blocking: work on it does not order against the default stream, so a host thread's blocking upload of the
    // next frame chunk runs beside this stream's kernels and row copies
    hipStream_t s;
    PMI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *)s;
    return PMI_OK;
}
int pmi_stream_destroy(void *stream) { PMI_HIP(hipStreamDestroy((hipStream_t)stream)); return PMI_OK; }
int pmi_memcpy_d2h_async(void *h, const void *d, size_t bytes, void *stream)
{
    PMI_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return PMI_OK;
}
int pmi_release_scratch(void) { pmi::release_fft_plans(); return pmi::scratch_release_all(); }
int pmi_scratch_bank(int bank) { return pmi::scratch_select_bank(bank); }
int pmi_localize_last_scan_decisions(int64_t *out4, void *stream)
{
    if (!out4) { pmi::set_error("pmi_localize_last_scan_decisions: null pointer"); return PMI_ERR_ARG; }
    return pmi::defer_last_decisions(out4, (hipStream_t)stream);
}

int pmi_event_create(void **event)
{
    hipEvent_t e;
    PMI_HIP(hipEventCreate(&e));
    *event = (void *)e;
    return PMI_OK;
}
int pmi_event_record(void *event, void *stream) { PMI_HIP(hipEventRecord((hipEvent_t)event, (hipStream_t)stream)); return PMI_OK; }
int pmi_event_elapsed_ms(void *start, void *stop, float *ms)
{
    PMI_HIP(hipEventSynchronize((hipEvent_t)stop));
    PMI_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return PMI_OK;
}
int pmi_event_destroy(void *event) { PMI_HIP(hipEventDestroy((hipEvent_t)event)); return PMI_OK; }

int pmi_set_kernel_timing(int enabled) { pmi::g_kernel_timing = enabled != 0; return PMI_OK; }
int pmi_last_kernel_ms(float *scan_ms, float *fit_ms)
{
    if (scan_ms) *scan_ms = pmi::g_last_times.scan_ms;
    if (fit_ms) *fit_ms = pmi::g_last_times.fit_ms;
    return PMI_OK;
}

}  // extern "C"
