/*
 * picasso_hip.h — C ABI of libpicasso_hip.so, the MI355X (gfx950) backend for
 * Picasso's localization hot path.
 *
 * Conventions follow the one native binding the reference already has
 * (picasso/ext/pygpufit/gpufit.py:40-76,338-366, Gpufit's C interface):
 *   - the caller owns every buffer; arrays are C-contiguous;
 *   - every call returns an int status, 0 = ok; pmi_last_error() gives the text;
 *   - no torch / numpy types cross this boundary, only pointers and sizes.
 *
 * Two families of entry points:
 *   pmi_<op>        host buffers in, host buffers out (what a ctypes/cffi/cgo
 *                   binding of the reference would call; does H2D/D2H inside);
 *   pmi_<op>_dev    device pointers + a HIP stream (void* = hipStream_t, NULL =
 *                   default stream); asynchronous; used to keep a movie
 *                   resident in HBM and to chain identify -> fit without a
 *                   host round trip.
 *
 * Reference interfaces replaced (paths relative to jungmannlab/picasso v0.10.3):
 *   pmi_identify*      picasso/localize.py:639-749 identify (-> :247-292
 *                      identify_in_image, :97-134 _local_maxima, :202-244
 *                      _net_gradient, :295-337 ROI crop, :395-401 frame bounds)
 *   pmi_net_gradient   picasso/localize.py:202-244 _net_gradient (+ :153-181
 *                      _gradient_at) on one frame with the caller's unit vectors
 *   pmi_get_spots*     picasso/localize.py:1115-1145 get_spots (-> :917-931
 *                      _cut_spots_numba, :1101-1112 _to_photons)
 *   pmi_gaussmle*      picasso/gaussmle.py:409-475 gaussmle / :478-530
 *                      gaussmle_async (-> :533-742 sigma, :745-954 sigmaxy)
 *   pmi_locs_from_fits_dev  picasso/gaussmle.py:957-1037 locs_from_fits
 *   pmi_zfit*          picasso/zfit.py:327-382 _fit_z (per-localization loop)
 *   pmi_avgroi*        picasso/avgroi.py:45-65 fit_spots
 *   pmi_gausslq*       picasso/gausslq.py:206-300 fit_spot / fit_spots /
 *                      fit_spots_parallel (scipy.optimize.leastsq = MINPACK lmdif
 *                      on the residuals of :151-203, start values of :95-112)
 *   pmi_locs_from_fits_lq_dev  picasso/gausslq.py:404-484 locs_from_fits
 *                      (+ :547-589 localization_precision)
 *   pmi_localize_lq_dev     picasso/localize.py:1682-1815 localize with
 *                      fitting_method="gausslq"
 *   pmi_render_*       picasso/render.py:37-175 render -> :798-853 _render_hist,
 *                      :1020-1070 _render_gaussian (ang=None), :177-232, :451-467, :494-575
 *   pmi_rotate_locs, pmi_render_*_rot  picasso/render.py:1571-1637 locs_rotation and the same renders with ang
 *                      (:578-679 _draw_gaussian_rot_loc)
 *   pmi_blur*, pmi_render_blurred  picasso/render.py:1413-1460 _fftconvolve under :1349-1410
 *                      _render_smooth and :1249-1319 _render_convolve
 *   pmi_xcorr, pmi_rcc_pairs   picasso/imageprocess.py:27-50 xcorr, :53-161
 *                      get_image_shift (up to its curve_fit), :164-217 rcc
 *   pmi_localize_mle_dev    picasso/localize.py:1682-1815 localize with
 *                      fitting_method="gaussmle" (identify -> get_spots -> fit
 *                      -> table) as one asynchronous device pipeline
 *   pmi_aim_*          picasso/aim.py:517-659 intersection_max, :662-773
 *                      intersection_max_z (-> :89-126 _count_intersections,
 *                      :206-250 _run_intersections_multithread, :275-320
 *                      _point_intersect_2d, :349-397 _point_intersect_3d): the
 *                      roi_cc counts of AIM undrift (:776-950 aim)
 *   pmi_link_*, pmi_nena_*  picasso/postprocess.py:2441-2552 _get_link_groups,
 *                      :2555-2661 _link_group_* as :2680-2821 _link_loc_groups
 *                      uses them, :1212-1272 _nfndh / _fill_dnfl
 *   pmi_cluster_*      picasso/clusterer.py:114-201 _cluster (the SMLM clusterer),
 *                      :34-111 _frame_analysis / frame_analysis, :410-445 _dbscan
 *   pmi_centers_*      picasso/clusterer.py:694-897 find_cluster_centers and its helpers
 *   pmi_areas_*        picasso/clusterer.py:1068-1169 _cluster_area, cluster_areas (picasso/masking.py:408-446
 *                      threshold_otsu)
 *   pmi_average_*      picasso/average.py:49-118 align_group_core, :354-530 average (the average image of
 *                      picasso/render.py:739-773 render_hist_numba, the rotation and shift search, the transform)
 *   pmi_cumexp_fit*    picasso/lib.py:1263-1327 cumulative_exponential, fit_cum_exp, estimate_kinetic_rate, under
 *                      picasso/postprocess.py:1634-1917 evaluate_picks, pick_kinetics, pick_properties
 *   pmi_g5m_*          picasso/g5m.py:212-318 _euclidean_distances, _kmeans_plusplus, :630-692 _check_G5M_resolution_2D,
 *                      :695-817 _initialize_G5M_2D .. _m_step_2D, :820-902 _find_optimal_G5M_2D, :455-462, :1037-1043
 *                      bic, n_parameters, :1699-1740 _estimate_gaussian_parameters_diag_cov, :1829-2064
 *                      _convert_G5M_results, :2126-2298 _fit_G5M (picasso/lib.py:1243-1260 find_local_minima)
 *   pmi_kinetics_*     picasso/postprocess.py:1985-2004 _dark_times (:1920-1982 compute_dark_times,
 *                      dark_times), :3580-3649 groupprops
 *   pmi_pairs_*        picasso/postprocess.py:37-94 get_index_blocks, :169-204
 *                      _fill_index_blocks, :1543-1579 _local_density (:1582-1631
 *                      compute_local_density), :960-999 _distance_histogram
 *                      (:1002-1055 distance_histogram, :1505-1540 pair_correlation)
 *   pmi_knn_*          picasso/postprocess.py:3704-3739 nn_analysis, picasso/spinna.py:696-747
 *                      get_NN_dist (scipy.spatial.KDTree(X2).query(X1, k))
 *   pmi_frc_*, pmi_radial_sum  picasso/postprocess.py:1398-1502 _frc (from the two rendered histograms to the curve),
 *                      picasso/masking.py:649-671 threshold_tukey, picasso/imageprocess.py:283-321 radial_sum
 *   pmi_picks_*        picasso/postprocess.py:207-372 _picked_circular_locs, _picked_rectangular_locs,
 *                      _picked_polygonal_locs, _picked_square_locs (:375-473 picked_locs), :849-928
 *                      _get_block_locs_at_numba, _locs_at_numba, picasso/lib.py:1884-2004 check_if_in_polygon,
 *                      check_if_in_rectangle
 *   pmi_fiducials_*    picasso/postprocess.py:3062-3156 undrift_from_picked, _undrift_from_picked_coordinate
 *   pmi_similar_*      picasso/postprocess.py:476-736 pick_similar, _pick_similar, :820-845 _n_block_locs_at, :848-957
 *                      get_block_locs_at_numba, locs_at_numba, rmsd_at_com
 */
#ifndef PICASSO_HIP_H
#define PICASSO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMI_OK            0
#define PMI_ERR_CAPACITY  1  /* output capacity too small; *out_n = rows needed */
#define PMI_ERR_ARG      -1
#define PMI_ERR_HIP      -2
#define PMI_ERR_NODEVICE -3

/* movie pixel types (the reference casts every frame to float32,
 * picasso/localize.py:332; integers up to 24 bits are exact) */
enum pmi_dtype { PMI_U16 = 0, PMI_U8 = 1, PMI_I16 = 2, PMI_U32 = 3, PMI_I32 = 4, PMI_F32 = 5 };
/* picasso/gaussmle.py:413 method: "sigma" | "sigmaxy" */
enum pmi_mle_method { PMI_MLE_SIGMA = 0, PMI_MLE_SIGMAXY = 1 };

#define PMI_MAX_BOX 21   /* odd box sizes 3..21 */

/* ---- library / device ------------------------------------------------ */
int         pmi_version(void);
const char *pmi_last_error(void);            /* gpufit_get_last_error analogue  */
int         pmi_device_count(void);          /* gpufit_cuda_available analogue: 0 = no GPU */
/* The device of the CALLING THREAD (HIP keeps it per thread).  Everything the library keeps on a device — scratch banks,
 * unit-vector tables, FFT plans, side streams, the statistics of the last fit — is keyed by the device current in the thread
 * that calls in, so one process may drive several GPUs from one host thread each (at most 16 devices).  A device that does
 * not exist is refused (PMI_ERR_ARG) and the thread stays where it was.                                       */
int         pmi_set_device(int device);
int         pmi_get_device(int *device);     /* the calling thread's current device */
int         pmi_device_info(char *name, size_t name_len, int *compute_units,
                            size_t *total_mem_bytes);

/* ---- device memory, for hosts without a HIP binding ------------------- */
int pmi_malloc(void **dptr, size_t bytes);
int pmi_free(void *dptr);
int pmi_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int pmi_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);
int pmi_stream_synchronize(void *stream);
/* A non-blocking HIP stream of the library's own (for callers without torch): the *_dev entry points queued on
 * it do not order against default-stream copies, so the upload of the next frame chunk (pmi_memcpy_h2d from
 * another host thread) overlaps them.  pmi_memcpy_d2h_async queues a copy on a stream; the host buffer is valid
 * after pmi_stream_synchronize.                                                                              */
int pmi_stream_create(void **stream);
int pmi_stream_destroy(void *stream);
int pmi_memcpy_d2h_async(void *dst_host, const void *src_dev, size_t bytes, void *stream);
int pmi_release_scratch(void);               /* frees the library's cached scratch buffers */
/* Scratch of the calls that follow ON THE CALLING THREAD comes from bank 0 (default) or 1: a caller that keeps two
 * pipelines in flight on two streams (the fit of one frame range beside the scan of the next) selects a bank before
 * queueing each; two host threads that drive one stream each select a bank each, once.  Calls that share a bank must
 * not overlap in time (one thread at a time per bank). */
int pmi_scratch_bank(int bank);

/* ---- identify --------------------------------------------------------- *
 * movie: (F, Y, X) pixels of `dtype`.  roi4 = {y0, x0, y1, x1} already
 * normalised to the frame (numpy slice semantics), or NULL.  Frames outside
 * [f_lo, f_hi] (inclusive) are skipped.  A pixel is reported when it is the
 * first maximum of its box x box window and its net gradient is > min_ng.
 * Output rows are ordered by (frame, y, x); coordinates are frame coordinates.
 * If more than `cap` rows exist, returns PMI_ERR_CAPACITY and *out_n = needed.
 * Every pixel type compares as float32, as in the reference (picasso/localize.py:332).  uint16 / int16 / uint8 movies take the
 * packed scan; float32, int32 and uint32 movies — whatever they hold: counts, fractions, negatives, values beyond 16 bits,
 * NaN, +-inf — are scanned in one pass on 16-bit keys (the upper half of the order-preserving integer image of the float32
 * the reference would see; 32-bit integers are converted as its cast does), with the first-argmax rule, the net gradient and
 * the threshold decided on those float32 values; 32-bit integer movies of 16-bit counts on frames of at most 256 columns are
 * narrowed to uint16 chunk by chunk instead; the generic kernel serves boxes 19 / 21 and crops narrower than a stencil.
 * Same table whichever kernel runs. */
int pmi_identify(const void *movie, int dtype, int64_t F, int64_t Y, int64_t X,
                 int box, double min_ng, const int64_t *roi4, int64_t f_lo, int64_t f_hi,
                 int32_t *out_frame, int32_t *out_y, int32_t *out_x, float *out_ng,
                 int64_t cap, int64_t *out_n);

/* 32-bit integer movies of 16-bit counts on narrow frames (above) pass through a uint16 copy, `frames` frames at a time
 * (0 = default: as many as fit 1 GiB).  A memory knob; the table does not depend on it. */
int pmi_identify_set_narrow_chunk(int64_t frames);

/* Device form.  d_out_n is a device int64 receiving the row count (rows beyond
 * cap are counted but not written).  Nothing is synchronised. */
int pmi_identify_dev(const void *d_movie, int dtype, int64_t F, int64_t Y, int64_t X,
                     int box, double min_ng, const int64_t *roi4, int64_t f_lo, int64_t f_hi,
                     int32_t *d_frame, int32_t *d_y, int32_t *d_x, float *d_ng,
                     int64_t cap, int64_t *d_out_n, void *stream);

/* ---- get_spots -------------------------------------------------------- *
 * spots[i] = float32(movie[frame, y-r:y+r+1, x-r:x+r+1]); then
 * (s - baseline) * sensitivity / gain in float32, in that order.            */
int pmi_get_spots(const void *movie, int dtype, int64_t F, int64_t Y, int64_t X,
                  const int32_t *frame, const int32_t *y, const int32_t *x, int64_t N,
                  int box, double baseline, double sensitivity, double gain,
                  float *out_spots);
/* d_n: optional device count (rows = min(*d_n, N)); NULL = N rows. */
int pmi_get_spots_dev(const void *d_movie, int dtype, int64_t F, int64_t Y, int64_t X,
                      const int32_t *d_frame, const int32_t *d_y, const int32_t *d_x,
                      int64_t N, const int64_t *d_n, int box, double baseline,
                      double sensitivity, double gain, float *d_spots, void *stream);

/* ---- gaussmle --------------------------------------------------------- *
 * spots: (N, box, box) float32 photons.  Outputs as gaussmle.py:455-459
 * allocates them: thetas (N,6) = x, y, photons, bg, sx, sy in box-origin
 * coordinates; crlbs (N,6); loglik (N); iterations (N) int32.              */
int pmi_gaussmle(const float *spots, int64_t N, int box, double eps, int max_it, int method,
                 float *thetas, float *crlbs, float *loglik, int32_t *iterations);
int pmi_gaussmle_dev(const float *d_spots, int64_t N, const int64_t *d_n, int box,
                     double eps, int max_it, int method, float *d_thetas, float *d_crlbs,
                     float *d_loglik, int32_t *d_iterations, void *stream);
/* Fused ROI extraction + photon conversion + fit straight from the movie
 * (no (N,box,box) round trip through HBM). */
int pmi_gaussmle_movie_dev(const void *d_movie, int dtype, int64_t F, int64_t Y, int64_t X,
                           const int32_t *d_frame, const int32_t *d_y, const int32_t *d_x,
                           int64_t N, const int64_t *d_n, int box, double baseline,
                           double sensitivity, double gain, double eps, int max_it, int method,
                           float *d_thetas, float *d_crlbs, float *d_loglik,
                           int32_t *d_iterations, void *stream);

/* How the Newton loop of pmi_gaussmle* runs.  The reference (picasso/gaussmle.py:745-857 under numba) keeps theta
 * and its accumulators in float32 arrays and evaluates every per-pixel intermediate in float64; its convergence
 * test |delta| < eps (:844-852, :632-638) is a discrete decision.
 *   PMI_MLE_FAST    the float32 loop only: ~1e-5 px from the reference, but a step that lands within rounding
 *                   distance of eps can end the fit an iteration earlier or later than the reference does;
 *   PMI_MLE_REFIT   (default) float32 loop, and every spot on which the two arithmetics can part — its largest tested
 *                   step came within `margin` (relative) of eps in some iteration; a curvature term was not negative;
 *                   a width fell below 0.5 px; a parameter swung back and forth without its steps shrinking (the
 *                   iteration does not contract); a pixel lay far off the model (|data / model - 1| or
 *                   |data / model^2| above 16); the fit took more than 64 iterations; or, seen from the Fisher matrix at the
 *                   fitted theta, the per-parameter update does not contract there (lambda_max of the normalised
 *                   Fisher matrix above 1.9: a rounding difference would be multiplied by 1 - lambda_max per
 *                   iteration) — is fitted again from its initial
 *                   parameters in the reference's own arithmetic (float64 intermediates, float32 stores, the
 *                   reference's summation order) inside the same call;
 *   PMI_MLE_STRICT  every spot in the reference's arithmetic.
 * Process-wide; the environment variable PMI_MLE_MODE = fast | refit | strict overrides the mode.
 * pmi_mle_last_refit_count: spots the calling thread's last pmi_gaussmle*_dev / pmi_localize_mle_dev call on `stream`
 * fitted again (synchronises the stream); pmi_mle_last_flag_reasons: of those, how many each criterion flagged, in the
 * order margin, curvature, narrow width, swing, far-off pixel, slow, unstable (n <= 7 counters; a spot can carry
 * several, and one that carries `unstable` beside another was fitted again twice, to the same result).        */
enum pmi_mle_mode { PMI_MLE_FAST = 0, PMI_MLE_REFIT = 1, PMI_MLE_STRICT = 2 };
int pmi_mle_set_mode(int mode, double margin);
int pmi_mle_get_mode(int *mode, double *margin);
/* math.erf / math.exp of the reference (gaussmle.py:279, 295, 313, 357) are the C library's under numba, and faithful, not
 * correctly rounded: which last bit they return depends on the libm.  A fit that contracts mostly forgets such a bit when
 * it rounds to float32; a fit that does not — 3x3 boxes whose width collapses, fits that wander for a thousand iterations —
 * carries it into another trajectory.  The reference-arithmetic kernel (the re-fit of PMI_MLE_REFIT, every spot of
 * PMI_MLE_STRICT) evaluates the two functions
 *   PMI_LIBM_GLIBC   operation for operation as glibc >= 2.28 on x86-64 with FMA does (the libm of the machines the
 *                    reference runs on, and of the oracle's) — csrc/libm_glibc.h; the kernel takes 12 - 18 % longer;
 *   PMI_LIBM_DEVICE  with the device library's functions (the behaviour up to round 5; on 1e6 ordinary 7x7 fits no row
 *                    differs);
 *   PMI_LIBM_AUTO    (default) glibc's bits wherever a result was ever seen to hang on them: every spot of
 *                    PMI_MLE_STRICT at any box, and the re-fit of PMI_MLE_REFIT on boxes up to 5x5; the device
 *                    library's in the re-fit of larger boxes, where the default mode's contract (the reference's
 *                    iteration count on every row, 1e-3 px wherever it converged) has not depended on them in 1e8
 *                    fuzzed fits and the list's latency is part of the timed step (2 % of config 2's).
 * Process-wide; the environment variable PMI_MLE_LIBM = auto | glibc | device overrides it.                       */
enum pmi_libm { PMI_LIBM_DEVICE = 0, PMI_LIBM_GLIBC = 1, PMI_LIBM_AUTO = 2 };
int pmi_mle_set_libm(int which);
int pmi_mle_get_libm(int *which);
/* Diagnostic: d_out[i] = f(d_x[i]) for n float64 device values — fn 0 / 1: exp / erf as the kernel evaluates them under
 * PMI_LIBM_GLIBC (the test compares them with the host's C library, bit for bit); fn 2 / 3: the device library's.     */
int pmi_libm_eval_dev(int fn, const double *d_x, int64_t n, double *d_out, void *stream);
int pmi_mle_last_refit_count(int64_t *n_refit, void *stream);
int pmi_mle_last_flag_reasons(int64_t *counts, int n, void *stream);

/* ---- locs_from_fits (gaussmle.py:957-1037) ---------------------------- *
 * Builds the 17-column localization table as structure-of-arrays, row i from
 * identification i (rows stay in identification order = frame order).
 * d_cols: 17 device pointers in this order, each N elements of 4 bytes:
 *  0 frame(u32) 1 x 2 y 3 photons 4 sx 5 sy 6 bg 7 lpx 8 lpy 9 ellipticity
 * 10 net_gradient 11 log_likelihood 12 iterations(u32) 13 photons_unc
 * 14 bg_unc 15 sx_unc 16 sy_unc   (all float32 unless noted)               */
#define PMI_LOC_COLUMNS 17
int pmi_locs_from_fits_dev(const int32_t *d_frame, const int32_t *d_y, const int32_t *d_x,
                           const float *d_ng, const float *d_thetas, const float *d_crlbs,
                           const float *d_loglik, const int32_t *d_iterations, int64_t N,
                           const int64_t *d_n, int box, void *const *d_cols, void *stream);

/* ---- whole path on a resident movie ----------------------------------- *
 * identify -> fused cut+fit -> table, one asynchronous submission.  d_table is
 * one device block of PMI_LOC_COLUMNS * cap * 4 bytes (column c starts at
 * element c*cap).  d_out_n: device int64 row count.  When it comes back
 * larger than cap the table is untouched: resubmit with cap >= *d_out_n.
 * Schedule: a large frame range is cut in two and the scan of the second half runs beside the fit of the first, on
 * a stream of the library's that joins the caller's stream at the start of the call and is joined again before the
 * table is written (the scan is bound by memory requests, the fit by VALU issue); the table is the same, bit for bit.
 * pmi_localize_set_ranges(1) keeps a call on the caller's stream alone (2 = default).                  */
int pmi_localize_set_ranges(int ranges);
/* Deferred exact stage (default on): on uint16 / uint8 / int16 movies, boxes up to 7 and a positive threshold the packed
 * scan of pmi_localize_mle_dev only emits CANDIDATES (window maximum, floor, neighbour rule) and the start-value kernel
 * of the fit — which reads a candidate's rows anyway — evaluates the float32 net gradient in the reference's (k, l)
 * order, the first-argmax rule and the threshold (picasso/localize.py:97-134, 202-244, 288): the scan no longer re-reads
 * nine lines per candidate.  Same table, bit for bit.  The identification / fit scratch then holds cap + cap / 2 + 4096
 * candidates; if a call finds more, *d_out_n reports the number of CANDIDATES (an upper bound of the rows needed), nothing is
 * fitted and the table is untouched, exactly as for a table that is too small.  0: the exact stage stays in the scan. */
int pmi_localize_set_defer(int on);
/* Accept-rate prior of the deferring scan.  A wave of the scan may emit its candidates undecided only while its own exact
 * rounds keep three in four of them; what the waves of a scan measured — how many candidates they decided, how many of those
 * they kept — is summed and handed to the scan of the call's second frame range and to the next call on the same device and
 * scratch bank, whose waves start from it (and check it on their first 8 candidates) instead of each proving the rate to
 * itself.  It changes who decides a candidate, never the table: the fit decides exactly.  The prior lives with the scratch of
 * the (device, bank), next to a key of dtype, Y, X, roi, box and min_ng: a call with another key starts without one, and so
 * does the first call after pmi_release_scratch, pmi_localize_set_defer or pmi_localize_reset_defer_prior.
 * pmi_localize_last_scan_decisions: of the calling thread's last pmi_localize_mle_dev on its device and bank, out4 =
 * (candidates range A decided in the scan, candidates it emitted undecided, the same two of range B; zeros for a range the
 * call did not have and for a call that did not defer).  Synchronises the stream, like pmi_mle_last_flag_reasons.
 * (Candidates decided by the rescan of a chunk whose plateau flooded the candidate ring are in neither count.) */
int pmi_localize_reset_defer_prior(void);
int pmi_localize_last_scan_decisions(int64_t *out4, void *stream);
int pmi_localize_mle_dev(const void *d_movie, int dtype, int64_t F, int64_t Y, int64_t X,
                         int box, double min_ng, const int64_t *roi4, int64_t f_lo, int64_t f_hi,
                         double baseline, double sensitivity, double gain,
                         double eps, int max_it, int method,
                         void *d_table, int64_t cap, int64_t *d_out_n, void *stream);

/* ---- net gradient at given pixels (picasso/localize.py:202-244 _net_gradient) ---- *
 * image: one (Y, X) float32 frame; y, x: n pixel positions; uy, ux: (box, box)
 * float32 unit-vector tables (the centre entry is not read).  out_ng[i] = sum over
 * the box x box window around (y, x), centre excluded, of gy*uy + gx*ux with
 * central differences, accumulated in float32 in the reference's order.  Index -1
 * wraps to the last row / column as the reference's unchecked indexing does;
 * positions whose window reaches past the far edge are refused.                   */
int pmi_net_gradient(const float *image, int64_t Y, int64_t X, const int32_t *y, const int32_t *x,
                     int64_t n, int box, const float *uy, const float *ux, float *out_ng);

/* ---- gausslq (picasso/gausslq.py:206-300) ------------------------------- *
 * spots: (N, box, box) float32 photons, box odd in [3, 21].  thetas (N,6) =
 * x, y, photons, bg, sx, sy with x, y relative to the box CENTRE (the least-
 * squares model is point-sampled on the grid -r..r, gausslq.py:228).  info /
 * nfev (N, int32, may be NULL) are MINPACK's termination code and the number of
 * residual evaluations, what leastsq(full_output=1) would report.
 * The _dev forms never wait for their stream (round 4): per batch of 2 Mi spots they queue the start values, five rounds
 * of (Jacobian + QR, step) — more for boxes above 7x7 —, one kernel that finishes on the device whatever fit is still
 * running, and the second pass of the mode over a device-side list; every count stays on the device.
 * pmi_localize_lq_dev keeps two frame ranges in flight like pmi_localize_mle_dev (pmi_localize_set_ranges).
 * Arithmetic (modes below): MINPACK adds the box^2 residual rows of a column norm, a Householder product or Q^T f one
 * after the other; tree reductions over the lanes of a spot's group differ from that in the last bits of float64, which
 * matters where one of lmdif's tests (the gain ratio against 1e-4 / 0.25 / 0.75, the termination tests, lmpar's 10 %
 * band, qrfac's pivot choice) is decided within those bits.  REFIT fits every such spot AGAIN from its start values with
 * the sums in MINPACK's order, inside the same call (pmi_gausslq_last_refit_count: how many spots of the calling thread's
 * last call were); STRICT, the default, uses MINPACK's order for every spot from the start.                    */
int pmi_gausslq(const float *spots, int64_t N, int box, float *thetas, int32_t *info, int32_t *nfev);
/* How those sums run (the counterpart of pmi_mle_set_mode for scipy.optimize.leastsq, picasso/gausslq.py:240-242):
 *   PMI_LQ_FAST    tree sums only: theta within ~1e-3 px on all but ~2e-5 of adversarial spots, no second fit;
 *   PMI_LQ_REFIT   tree sums, and the spots with a decision inside rounding distance of its threshold, a pivot tie or a
 *                  nearly rank-deficient Jacobian fitted again in MINPACK's order.  theta, info and nfev are lmdif's on
 *                  99.998 % of adversarial spots; 5e-6 of them end beyond 1e-3 px (up to 2.4 px measured) with the same
 *                  `info` — a float32 rounding of the stored model flipped by the last bits of a tree sum, which no
 *                  test of the fit sees;
 *   PMI_LQ_STRICT  (default) every sum over the residual rows — enorm, qrfac's Householder products, Q^T fvec — in
 *                  MINPACK's sequential order from the first Jacobian on (one chain per column, side by side in the lanes
 *                  of a spot's group): theta, info and nfev are lmdif's on EVERY spot, bit for bit.  Since round 5
 *                  (the image columns on the lanes, csrc/gausslq_w.hip) also the faster mode up to 9x9 boxes (7x7: 0.8x
 *                  the time of REFIT); 1.1x REFIT's time at 11x11 and 13x13, 1.8x at 15x15, 2.4x at 21x21.
 * Process-wide; the environment variable PMI_LQ_MODE = fast | refit | strict overrides the mode.                 */
enum pmi_lq_mode { PMI_LQ_FAST = 0, PMI_LQ_REFIT = 1, PMI_LQ_STRICT = 2 };
int pmi_gausslq_set_mode(int mode);
int pmi_gausslq_get_mode(int *mode);
int pmi_gausslq_last_refit_count(int64_t *n_refit);
/* ... and which test sent them there (n <= 10 counters: pivot choice, lmpar's band, 0.1 fnorm1 < fnorm, the gain-ratio
 * thresholds, the ftol tests, a reduction at the noise level, the xtol test, [7] strict mode: a float32 rounding of the
 * model within a few float64 ulps of a tie / a Jacobian outside the range of the short divisions; a spot can carry
 * several; [8], [9]: rounds queued by the first pass, second passes run)                                     */
int pmi_gausslq_last_tie_reasons(int64_t *counts, int n);
int pmi_gausslq_dev(const float *d_spots, int64_t N, const int64_t *d_n, int box, float *d_thetas,
                    int32_t *d_info, int32_t *d_nfev, void *stream);
int pmi_gausslq_movie_dev(const void *d_movie, int dtype, int64_t F, int64_t Y, int64_t X,
                          const int32_t *d_frame, const int32_t *d_y, const int32_t *d_x,
                          int64_t N, const int64_t *d_n, int box, double baseline,
                          double sensitivity, double gain, float *d_thetas, int32_t *d_info,
                          int32_t *d_nfev, void *stream);
/* 11-column table of gausslq.locs_from_fits: 0 frame(u32) 1 x 2 y 3 photons
 * 4 sx 5 sy 6 bg 7 lpx 8 lpy 9 ellipticity 10 net_gradient.  em != 0 doubles
 * the variance of lpx/lpy (EMCCD excess noise, gausslq.py:584-585).           */
#define PMI_LQ_COLUMNS 11
int pmi_locs_from_fits_lq_dev(const int32_t *d_frame, const int32_t *d_y, const int32_t *d_x,
                              const float *d_ng, const float *d_thetas, int64_t N, const int64_t *d_n,
                              int em, void *const *d_cols, void *stream);
/* identify -> fused cut + least-squares fit -> table; d_table holds
 * PMI_LQ_COLUMNS * cap * 4 bytes, column c at element c*cap.                  */
int pmi_localize_lq_dev(const void *d_movie, int dtype, int64_t F, int64_t Y, int64_t X,
                        int box, double min_ng, const int64_t *roi4, int64_t f_lo, int64_t f_hi,
                        double baseline, double sensitivity, double gain, int em,
                        void *d_table, int64_t cap, int64_t *d_out_n, void *stream);

/* ---- zfit (picasso/zfit.py:254-291, 327-382) ---------------------------- *
 * Per localization: argmin over z in [-1000, 1000] of
 * (sqrt(sx) - sqrt(wx(z)))^2 + (sqrt(sy) - sqrt(wy(z)))^2, wx/wy degree-6
 * polynomials (cx7/cy7, highest power first), by the bounded Brent minimiser of
 * scipy.optimize.minimize_scalar (xatol 1e-5, maxiter 500).  Outputs are float64:
 * z before the magnification factor and the squared residual (d_zcalib^2).   */
int pmi_zfit(const float *sx, const float *sy, int64_t N, const double *cx7, const double *cy7,
             double *z, double *sq_residual);
int pmi_zfit_dev(const float *d_sx, const float *d_sy, int64_t N, const int64_t *d_n, const double *cx7,
                 const double *cy7, double *d_z, double *d_sq_residual, void *stream);

/* ---- avg (picasso/avgroi.py:24-65) -------------------------------------- *
 * theta (N,6) = [0, 0, sum, sum, 1, 1] with a float64 ROI sum.               */
int pmi_avgroi(const float *spots, int64_t N, int box, float *theta);
int pmi_avgroi_dev(const float *d_spots, int64_t N, const int64_t *d_n, int box, float *d_theta, void *stream);

/* ---- render (picasso/render.py:37-175 render with blur_method None / "gaussian") --- *
 * x, y (and lpx, lpy) are the float32 columns of the localization table in
 * camera pixels.  The viewport (y_min, x_min)-(y_max, x_max) and oversampling
 * define an image of ny x nx = ceil(oversampling * extent) float32 pixels
 * (pmi_render_dims; render.py:177-232); localizations strictly inside the
 * viewport are drawn, *n_rendered receives their number.
 *   hist:     image[int(y'), int(x')] += 1                       (render.py:451-467)
 *   gaussian: separable Gaussian over +-3 sigma, sigma = oversampling *
 *             max(lp, min_blur_width), in TABLE ORDER per pixel   (render.py:494-575);
 *             iso != 0: both widths = their mean ("gaussian_iso", :1148-1216)
 * The image buffer is overwritten (zeroed first).  The Gaussian _dev form
 * synchronises the stream once: the number of (tile, localization) pairs sizes
 * its sort buffers.                                                          */
int pmi_render_dims(double oversampling, double y_min, double x_min, double y_max, double x_max,
                    int64_t *ny, int64_t *nx);
int pmi_render_hist(const float *x, const float *y, int64_t N, double oversampling,
                    double y_min, double x_min, double y_max, double x_max,
                    float *image, int64_t ny, int64_t nx, int64_t *n_rendered);
int pmi_render_hist_dev(const float *d_x, const float *d_y, int64_t N, double oversampling,
                        double y_min, double x_min, double y_max, double x_max,
                        float *d_image, int64_t ny, int64_t nx, int64_t *d_n_rendered, void *stream);
int pmi_render_gaussian(const float *x, const float *y, const float *lpx, const float *lpy, int64_t N,
                        double oversampling, double y_min, double x_min, double y_max, double x_max,
                        double min_blur_width, int iso, float *image, int64_t ny, int64_t nx, int64_t *n_rendered);
int pmi_render_gaussian_dev(const float *d_x, const float *d_y, const float *d_lpx, const float *d_lpy,
                            int64_t N, double oversampling, double y_min, double x_min, double y_max,
                            double x_max, double min_blur_width, int iso, float *d_image, int64_t ny,
                            int64_t nx, int64_t *d_n_rendered, void *stream);

/* ---- rotated views (picasso/render.py:1571-1637 locs_rotation; _render_hist / _render_gaussian / _render_gaussian_iso
 * with ang; :578-679 _draw_gaussian_rot_loc) --- *
 * x, y, z are the three coordinate columns of the table: all float32 (coords_f64 == 0, the usual table; the viewport's
 * centre is then subtracted in float32, as on the float32 array the reference takes) or all float64 (coords_f64 != 0,
 * what a table of mixed column types becomes).  matrix is the rotation as scipy gives it (float64[9], row major, a HOST
 * pointer in both forms); matrix_f32 the same rounded to float32 (the covariance of the Gaussian).  The rows are rotated
 * about the centre of the viewport, r_i = (M[i][0] v0 + M[i][1] v1) + M[i][2] v2 in float64 (N == 1:
 * (M[i][0] v0 + M[i][2] v2) + M[i][1] v1, as scipy on a one-row array), and are in view when strictly inside it after
 * the rotation.
 *   pmi_rotate_locs       per row x' = os (x - x_min), y' = os (y - y_min), z' = os z and in_view (0 / 1): what
 *                         locs_rotation returns before it drops the rows out of view
 *   pmi_render_hist_rot   image[int(y'), int(x')] += 1 for the rows in view
 *   pmi_render_gaussian_rot  the projection of the rotated 3-D Gaussian with widths os * max(lp, min_blur_width)
 *                         (lpz NULL: twice the mean of lpx and lpy; iso != 0: sx = sy = their mean), float32 2x2 projected
 *                         covariance, rows with det < 1e-10 counted and not drawn, +-3 sigma footprint, per pixel in
 *                         TABLE ORDER  pix = float32(pix + norm * exp(-0.5 * e))  with glibc's exp.
 * *n_rendered receives the number of rows in view.  The image is overwritten.  The Gaussian _dev form synchronises the
 * stream once, as pmi_render_gaussian_dev.                                                                        */
int pmi_rotate_locs(const void *x, const void *y, const void *z, int coords_f64, int64_t N, const double *matrix,
                    double oversampling, double y_min, double x_min, double y_max, double x_max,
                    double *xr, double *yr, double *zr, uint8_t *in_view);
int pmi_rotate_locs_dev(const void *d_x, const void *d_y, const void *d_z, int coords_f64, int64_t N, const double *matrix,
                        double oversampling, double y_min, double x_min, double y_max, double x_max,
                        double *d_xr, double *d_yr, double *d_zr, uint8_t *d_in_view, void *stream);
int pmi_render_hist_rot(const void *x, const void *y, const void *z, int coords_f64, int64_t N, const double *matrix,
                        double oversampling, double y_min, double x_min, double y_max, double x_max,
                        float *image, int64_t ny, int64_t nx, int64_t *n_rendered);
int pmi_render_hist_rot_dev(const void *d_x, const void *d_y, const void *d_z, int coords_f64, int64_t N,
                            const double *matrix, double oversampling, double y_min, double x_min, double y_max,
                            double x_max, float *d_image, int64_t ny, int64_t nx, int64_t *d_n_rendered, void *stream);
int pmi_render_gaussian_rot(const void *x, const void *y, const void *z, int coords_f64, const float *lpx,
                            const float *lpy, const float *lpz, int64_t N, const double *matrix, const float *matrix_f32,
                            double oversampling, double y_min, double x_min, double y_max, double x_max,
                            double min_blur_width, int iso, float *image, int64_t ny, int64_t nx, int64_t *n_rendered);
int pmi_render_gaussian_rot_dev(const void *d_x, const void *d_y, const void *d_z, int coords_f64, const float *d_lpx,
                                const float *d_lpy, const float *d_lpz, int64_t N, const double *matrix,
                                const float *matrix_f32, double oversampling, double y_min, double x_min, double y_max,
                                double x_max, double min_blur_width, int iso, float *d_image, int64_t ny, int64_t nx,
                                int64_t *d_n_rendered, void *stream);

/* ---- image blur (picasso/render.py:1413-1460 _fftconvolve; the "smooth" and "convolve" renders) --- *
 * A separable blur of a float32 image of ny x nx pixels, axis 0 (y, weights wy, radius ry) first, then axis 1
 * (x, wx, rx).  An axis whose weight pointer is NULL is skipped; a radius of 0 multiplies by its one weight.  Each
 * weight vector holds 2 r + 1 float64 values and is taken to be symmetric (only w[0 .. r] are read).  The image is
 * extended by zeros (scipy's mode="constant", cval=0); a radius beyond the image side is legal.  Per axis and output
 * sample l of a line, in float64 and in this order, contraction off:
 *     tmp = line[l] * w[r];   for j = r, r - 1, ..., 1:   tmp += (line[l - j] + line[l + j]) * w[r - j];
 * which is scipy.ndimage.correlate1d for symmetric weights.
 *   round_between != 0  tmp is rounded to float32 after each axis, the second axis reads the float32 values back:
 *                       scipy.ndimage.gaussian_filter(output=float32, mode="constant") in every bit when the weights
 *                       are its _gaussian_kernel1d; `scale` is not used.  With both axes skipped the output is a copy.
 *   round_between == 0  float64 between the axes, then tmp * scale and one rounding to float32: the direct sum that
 *                       stands in for the reference's single-precision FFT convolution (weights = its window
 *                       functions, scale = 1 / kernel.sum()).
 * Sides are limited as the render's are (below 2^31, at most 2^31 - 1 tiles of 32 x 32 pixels).  d_in and d_out
 * must not overlap.  The _dev form is asynchronous, all pointers device pointers, its intermediate image in the
 * library's scratch.  pmi_render_blurred is pmi_render_hist followed by pmi_blur without the histogram leaving the
 * device: only the blurred image and *n_rendered come back.                                                  */
int pmi_blur_dev(const float *d_in, float *d_out, int64_t ny, int64_t nx, const double *d_wy, int64_t ry,
                 const double *d_wx, int64_t rx, int round_between, double scale, void *stream);
int pmi_blur(const float *in, float *out, int64_t ny, int64_t nx, const double *wy, int64_t ry,
             const double *wx, int64_t rx, int round_between, double scale);
int pmi_render_blurred(const float *x, const float *y, int64_t N, double oversampling,
                       double y_min, double x_min, double y_max, double x_max,
                       const double *wy, int64_t ry, const double *wx, int64_t rx, int round_between, double scale,
                       float *image, int64_t ny, int64_t nx, int64_t *n_rendered);

/* ---- cross-correlation for RCC undrift (picasso/imageprocess.py:27-217) ---- *
 * pmi_xcorr: out = fftshift(real(ifft2(fft2(A) * conj(fft2(B))))) / sqrt(Y*X),
 * float64 images of Y x X (imageprocess.py:27-50).
 * pmi_rcc_pairs: for every pair i < j of n_seg float64 images (pair index in
 * the order of imageprocess.py:197-205), everything get_image_shift (:53-161)
 * does before its curve_fit: correlation, centre crop to `roi` (0 = none;
 * crop_yx = {Y_, X_} rows/columns removed on each side), first maximum in
 * row-major order (peak_yx[2p], peak_yx[2p+1], cropped coordinates) and the
 * box x box window around it (fit_rois[p*box*box ..]).  valid[p] = 1 when the
 * window lies inside the cropped correlation, 0 when numpy's slicing would
 * truncate it (the reference then reports a zero shift), -1 when one of the
 * two images is empty (zero shift by imageprocess.py:85-86).                  */
int pmi_xcorr(const double *image_a, const double *image_b, int64_t Y, int64_t X, double *out);
int pmi_rcc_pairs(const double *segments, int64_t n_seg, int64_t Y, int64_t X, int64_t roi, int box,
                  int32_t *peak_yx, int32_t *valid, double *fit_rois, int32_t *crop_yx);
/* The same for an explicit list of n_pairs (i, j) index pairs — the share of one rank when the
 * n(n-1)/2 correlations of RCC are split over several GPUs.      */
int pmi_rcc_pair_list(const double *segments, int64_t n_seg, int64_t Y, int64_t X, int64_t roi, int box,
                      const int32_t *pairs, int64_t n_pairs, int32_t *peak_yx, int32_t *valid,
                      double *fit_rois, int32_t *crop_yx);

/* ---- the sharded path: every rank's localization table on every GPU ---- *
 * The reference has no distributed code; its workers split the movie frame by frame inside one process
 * (picasso/localize.py:438-454).  Here each GPU (one process per GPU) localizes a contiguous frame range and the
 * tables are all-gathered with RCCL, called from this library (loaded at the first pmi_comm_* call).
 *   pmi_comm_available  PMI_OK when RCCL and the entry points used here resolve on this rank; creates nothing.  A
 *                       host AGREES on this over its own channel before any rank enters pmi_comm_init: the
 *                       communicator set-up is itself a collective, and a rank that cannot join it leaves the others
 *                       waiting inside ncclCommInitRank;
 *   pmi_comm_unique_id  rank 0 fills a 128-byte id, which the HOST hands to every rank (file, socket, MPI, ...);
 *   pmi_comm_init       every rank, on its own device (pmi_set_device first);
 *   pmi_allgather_locs  d_table: this rank's ncols x cap column-major table of 4-byte cells (PMI_LOC_COLUMNS or
 *                       PMI_LQ_COLUMNS columns, the same cap on every rank), d_n its device row count;
 *                       d_all_tables receives world x ncols x cap cells (rank-major), d_all_counts world counts.
 *                       One grouped submission on `stream`, asynchronous, no host synchronisation;
 *   pmi_compact_gathered_dev  the gathered tables as ONE ncols x table_cap column-major table, rows in rank order
 *                       (= frame order for contiguous frame shards, picasso/gaussmle.py:1036), total in *d_total.  */
int pmi_comm_available(void);
int pmi_comm_unique_id(void *id128);
int pmi_comm_init(const void *id128, int world, int rank, void **comm);
int pmi_comm_info(void *comm, int *world, int *rank);         /* as RCCL reports them (ncclCommCount / ncclCommUserRank) */
int pmi_comm_library_path(char *path, size_t path_len);         /* the librccl the collectives resolved to (dladdr) */
int pmi_comm_destroy(void *comm);
int pmi_allgather_locs(void *comm, const void *d_table, int ncols, int64_t cap, const int64_t *d_n,
                       void *d_all_tables, int64_t *d_all_counts, void *stream);
int pmi_compact_gathered_dev(const void *d_all_tables, const int64_t *d_all_counts, int world, int ncols, int64_t cap,
                             void *d_table, int64_t table_cap, int64_t *d_total, void *stream);

/* ---- sub-pixel correlation peak (picasso/imageprocess.py:121-141) ---------------------------- *
 * The reference fits a * exp(-0.5 ((x - xc)^2 + (y - yc)^2) / s^2) + b to the box x box window around
 * the correlation maximum with scipy.optimize.curve_fit(p0 = [max, 0, 0, 1, min], bounds = ([0, -inf,
 * -inf, 0, 0], inf)) = least_squares(method="trf", jac="2-point"): the Trust Region Reflective algorithm
 * of scipy 1.15.3, restated for one thread per window (csrc/peakfit.hip).
 * pmi_peak_fit: rois (n, box, box) float64 -> popt (n, 5) = a, xc, yc, s, b and scipy's termination
 * status (1 gtol, 2 ftol, 3 xtol, 4 both; 0 max_nfev, where curve_fit raises RuntimeError; -2: window minimum
 * < 0, where curve_fit raises "x0 is infeasible"; -3: a NaN or an infinity in the window, where curve_fit raises
 * ValueError).
 * pmi_rcc_shifts: all of get_image_shift (:53-161) for a list of (i, j) pairs of the n_seg float64
 * images — correlation, centre crop, first maximum, window, fit — -> shift_yx (n_pairs, 2) = (-yc, -xc);
 * fit_status as above, or -1 where the reference returns (0, 0) without fitting (empty image, window
 * truncated by the border).                                                                         */
/* Makes (and caches) the FFT plans of Y x X images ahead of the first correlation: rocFFT compiles a plan's kernels when
 * the plan is made (2.5 s at 2048 x 2048).  Thread-safe; meant for a side thread of the host while it localizes. */
int pmi_fft_prewarm(int64_t Y, int64_t X);
int pmi_peak_fit(const double *rois, int64_t n, int box, double *popt, int32_t *status);
int pmi_rcc_shifts(const double *segments, int64_t n_seg, int64_t Y, int64_t X, int64_t roi, int box,
                   const int32_t *pairs, int64_t n_pairs, double *shift_yx, int32_t *fit_status);

/* ---- AIM undrift: intersection counts (picasso/aim.py:517-773, csrc/aim.hip) ---------------------- *
 * Key arithmetic of a round (the reference's column dtypes, see aim.hip):
 *   PMI_AIM_XY_F32  x / y round 1: float32 x, y; rel added in float32
 *   PMI_AIM_XY_F64  x / y round 2: float64 x, y
 *   PMI_AIM_Z_F32   z round 1: float64 x, y; float32 z (already divided by the pixel size); rel added to z in float32
 *   PMI_AIM_Z_F64   z round 2: float64 x, y, z
 * shifts: n_shifts int32 (x / y modes: the reference's shifts_xy, row-major box x box) or float64 (z modes: shifts_z).
 * pmi_aim_partition_dev  d_frame: n int64 frames numbered from 1 (aim.py:852); rows of segment s (frames in
 *                        (s * seg_len, min((s + 1) * seg_len, n_frames)]) go to d_rows[seg_offsets[s] .. seg_offsets[s+1]),
 *                        in no particular order; rows outside [1, n_frames] to none.  seg_offsets: host, ceil(n_frames /
 *                        seg_len) + 1 entries.  Synchronises `stream`.
 * pmi_aim_table_create_dev  counts the reference keys of rows d_rows[0 .. n_ref) (NULL: rows 0 .. n_ref-1) of the device
 *                        columns once per round; returns an opaque table that owns its device memory.  Synchronises.
 * pmi_aim_count_dev      roi_cc of the target rows d_rows[0 .. n_rows) shifted by rel: d_out[0 .. n_shifts) = the counts,
 *                        d_out[n_shifts] = status (0 ok; 1 the target hash overflowed).  Asynchronous on `stream`; a table
 *                        serves one stream at a time.
 * pmi_aim_roi_cc         the same for host columns (one table, one count), -> int64 roi_cc[n_shifts].
 * pmi_aim_set_dense_limit  spans of more target-counter entries than this (default 2^28) take the sorted form.         */
enum pmi_aim_mode { PMI_AIM_XY_F32 = 0, PMI_AIM_XY_F64 = 1, PMI_AIM_Z_F32 = 2, PMI_AIM_Z_F64 = 3 };
int pmi_aim_set_dense_limit(int64_t entries);
int pmi_aim_partition_dev(const int64_t *d_frame, int64_t n, int64_t seg_len, int64_t n_frames, int32_t *d_rows,
                          int64_t *seg_offsets, void *stream);
int pmi_aim_table_create_dev(int mode, const void *d_x, const void *d_y, const void *d_z, const int32_t *d_rows,
                             int64_t n_ref, double intersect_d, double width_units, double height_units,
                             const void *shifts, int n_shifts, void **table, void *stream);
int pmi_aim_table_info(void *table, int *dense, int64_t *entries);   /* dense: 1 dense form, 0 sorted; entries of it */
int pmi_aim_count_dev(void *table, const void *d_x, const void *d_y, const void *d_z, const int32_t *d_rows,
                      int64_t n_rows, double rel_x, double rel_y, double rel_z, int32_t *d_out, void *stream);
int pmi_aim_table_destroy(void *table);
int pmi_aim_roi_cc(int mode, const void *ref_x, const void *ref_y, const void *ref_z, int64_t n_ref, const void *x,
                   const void *y, const void *z, int64_t n, double rel_x, double rel_y, double rel_z,
                   double intersect_d, double width_units, double height_units, const void *shifts, int n_shifts,
                   int64_t *roi_cc);

/* ---- link and NeNA (picasso/postprocess.py:2441-2661, :1212-1272, csrc/link.hip) ------------------------- *
 * Device columns of a table SORTED BY FRAME: d_frame and d_group int64 (the host widens any integer column), d_x / d_y
 * float32 or float64 (PMI_LINK_F32 / PMI_LINK_F64, each on its own).  At most 2^31 - 2 rows.  Scratch comes from the
 * library's arena; every call runs on `stream`.
 *
 * pmi_link_frame_index_dev  d_lo[i] = first row j > i with frame[j] >= frame[i] + 1, d_hi[i] = first row j > i with
 *                        frame[j] > frame[i] + k; n where there is none.
 * pmi_link_groups_dev    the reference's int32 link_group of every row, group numbers in the order of their first row;
 *                        r2 = d_max ** 2, k = max_dark_time + 1.  The last row of the table has no next row (the reference
 *                        is undefined there).  *n_groups = the number of groups; synchronises the stream.
 * pmi_link_combine_dev   per link group g < n_groups: d_count (uint32), d_first / d_last (min / max of d_frame, may be
 *                        NULL with d_frame), d_last_row (the group's last row, -1 for an empty group), and per column
 *                        descriptor a sum IN ROW ORDER in the column's own type:
 *                          PMI_LINK_SUM    out[g] = sum data[i]                       out has data's type
 *                          PMI_LINK_WSUM   out[g] = sum 1 / weight[i]^2                out has weight's type
 *                          PMI_LINK_XWSUM  out[g] = sum data[i] * (1 / weight[i]^2)    float64 unless both are float32
 *                        32-bit integers of either sign sum as PMI_LINK_U32 (the same bits), 64-bit ones as PMI_LINK_U64.
 *                        Values of d_link_group outside [0, n_groups) are not summed.  At most 24 columns.
 * pmi_nena_hist_dev      d_hist[n_bins] (uint64, device): next-frame neighbour distances d <= d_max of the same group,
 *                        bin int(d / bin_size); rows i < 100 * int(n / 100) look forward, the last row of the table is
 *                        never a neighbour and never looks forward, d / bin_size >= n_bins is dropped.  n_bins <= 8192. */
enum pmi_link_type { PMI_LINK_F32 = 0, PMI_LINK_F64 = 1, PMI_LINK_U32 = 2, PMI_LINK_U64 = 3 };
enum pmi_link_op { PMI_LINK_SUM = 0, PMI_LINK_WSUM = 1, PMI_LINK_XWSUM = 2 };
typedef struct pmi_link_column {
    const void *data;     /* device column (SUM, XWSUM) */
    const void *weight;   /* device precision column lp (WSUM, XWSUM) */
    void *out;            /* device, n_groups entries */
    int32_t op, type, w_type;
} pmi_link_column;
int pmi_link_frame_index_dev(const int64_t *d_frame, int64_t n, int64_t k, int32_t *d_lo, int32_t *d_hi, void *stream);
int pmi_link_groups_dev(const int64_t *d_frame, const void *d_x, int x_type, const void *d_y, int y_type,
                        const int64_t *d_group, int64_t n, double r2, int64_t k, int32_t *d_link_group,
                        int64_t *n_groups, void *stream);
int pmi_link_combine_dev(const int32_t *d_link_group, int64_t n, int64_t n_groups, const int64_t *d_frame,
                         const pmi_link_column *columns, int n_columns, uint32_t *d_count, int64_t *d_first,
                         int64_t *d_last, int32_t *d_last_row, void *stream);
int pmi_nena_hist_dev(const int64_t *d_frame, const void *d_x, int x_type, const void *d_y, int y_type,
                      const int64_t *d_group, int64_t n, double d_max, double bin_size, int n_bins, uint64_t *d_hist,
                      void *stream);

/* ---- DBSCAN and the SMLM clusterer (picasso/clusterer.py:34-201, :410-445, csrc/cluster.hip) ------------------ *
 * d_X: the points as float64, one column per dimension (dims * n values, dimension k at d_X + k * n), dims = 2 or 3, the
 * third already scaled by radius_xy / radius_z.  lo / hi: host arrays of dims values that bound every column (rows outside
 * are binned into the border cells: correct, slower).  r is the radius (it sizes the cells), r2 = r * r as the caller's
 * float64 product: row j is a neighbour of row i, itself included, iff dx*dx + dy*dy (+ dz*dz) <= r2 in float64.  At most
 * 2^31 - 2 rows; memory is O(n) whatever (hi - lo) / r is.  Scratch comes from the library's arena; every call runs on
 * `stream` and the label calls synchronise it.
 *
 * pmi_cluster_counts_dev   d_counts[i] (int32) = the number of neighbours of row i.
 * pmi_cluster_smlm_dev     d_labels[i] (int32) of _cluster: local maxima of the neighbour count (> min_locs), numbered in
 *                          row order, merged and spread as the reference's loops do; labels of fewer than min_locs rows
 *                          become -1; with d_frame (int64 per row, else NULL) the frame analysis below then runs on every
 *                          label (fa_lo = 0.2 * n_frames, fa_hi = 0.8 * n_frames, fa_edges = the 21 bin edges, host).
 * pmi_cluster_dbscan_dev   d_labels[i] (int32) of _dbscan: core rows have >= min_samples neighbours, clusters are numbered
 *                          by their lowest core row, a border row takes the lowest number among its core neighbours,
 *                          clusters of fewer than min_locs rows become -1 (the numbering keeps its gaps).
 * pmi_cluster_frame_analysis_dev  d_pass[g] (int32) for the ids g < n_ids of d_ids (int32 per row, others ignored): 0 iff
 *                          the mean of d_frame over the id's rows is < fa_lo or > fa_hi, or one of the 20 bins
 *                          [fa_edges[k], fa_edges[k + 1]) (the last closed) holds more than 0.8 of its rows. */
int pmi_cluster_counts_dev(const double *d_X, int dims, int64_t n, const double *lo, const double *hi, double r,
                           double r2, int32_t *d_counts, void *stream);
int pmi_cluster_smlm_dev(const double *d_X, int dims, int64_t n, const double *lo, const double *hi, double r,
                         double r2, int64_t min_locs, const int64_t *d_frame, double fa_lo, double fa_hi,
                         const double *fa_edges, int32_t *d_labels, void *stream);
int pmi_cluster_dbscan_dev(const double *d_X, int dims, int64_t n, const double *lo, const double *hi, double r,
                           double r2, int64_t min_samples, int64_t min_locs, int32_t *d_labels, void *stream);
int pmi_cluster_frame_analysis_dev(const int32_t *d_ids, const int64_t *d_frame, int64_t n, int64_t n_ids, double fa_lo,
                                   double fa_hi, const double *fa_edges, int32_t *d_pass, void *stream);

/* ---- local density and the distance histogram (picasso/postprocess.py:37-204, :960-999, :1543-1579, csrc/pairs.hip) - *
 * A table binned into square blocks of the search radius: d_x_index / d_y_index (uint32, computed on the host as the
 * reference does), K x L blocks.  d_x / d_y are the table's columns IN THE CALLER'S ROW ORDER, float32 or float64
 * (PMI_LINK_F32 / PMI_LINK_F64, each on its own).  At most 2^31 - 2 rows; memory is O(n) whatever K x L is (no block
 * table: a block's rows are two bisections of the sorted keys).  Scratch comes from the library's arena; every call runs
 * on `stream` and synchronises it before it returns.
 *
 * pmi_pairs_order_dev    d_rows[q] (int32) = the row at sorted position q, equal to np.lexsort([x_index, y_index]);
 *                        d_keys[q] (uint64) = y_index << 32 | x_index of that row; *p = the first sorted position whose
 *                        block lies outside the grid (n when there is none): the reference's block table stops filling
 *                        there, so only the positions < p are ever found as neighbours.
 * pmi_pairs_density_dev  d_density[q] (uint32) of sorted position q < n: the positions j < p in the nine blocks
 *                        (ki - 1 .. ki + 1, li - 1 .. li + 1) with dx2 < r2, dy2 < r2 and dx2 + dy2 < r2, q itself
 *                        included when q < p.  A block index of -1 is K - 1 / L - 1 (a negative index in the reference:
 *                        with K or L <= 2 a block is counted twice); an index >= K / L is an empty block (the reference
 *                        reads outside its table there).  r2 = radius ** 2.
 * pmi_pairs_distance_hist_dev  d_hist[n_bins] (uint64, device): the pairs of positions a < b < p with block(b) - block(a)
 *                        one of (0, 0), (0, 1), (1, 0), (1, 1) -- (1, -1) is not visited, as in the reference -- and
 *                        dx2 < r2, dy2 < r2, d = sqrt(dx2 + dy2) < r_max, bin floor(d / bin_size) < n_bins.  Up to 8192
 *                        bins are counted in LDS, more with one integer atomic per pair.  r2 = r_max ** 2. */
int pmi_pairs_order_dev(const uint32_t *d_x_index, const uint32_t *d_y_index, int64_t n, int64_t K, int64_t L,
                        int32_t *d_rows, uint64_t *d_keys, int64_t *p, void *stream);
int pmi_pairs_density_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int32_t *d_rows,
                          const uint64_t *d_keys, int64_t n, int64_t p, int64_t K, int64_t L, double r2,
                          uint32_t *d_density, void *stream);
int pmi_pairs_distance_hist_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int32_t *d_rows,
                                const uint64_t *d_keys, int64_t n, int64_t p, int64_t K, int64_t L, double r_max,
                                double r2, double bin_size, int64_t n_bins, uint64_t *d_hist, void *stream);

/* ---- cluster centers (picasso/clusterer.py:694-897 find_cluster_centers, csrc/centers.hip) --------------------- *
 * The per-cluster statistics of a table with a `group` column.  d_group is int64 (the host widens any integer column),
 * g_min / g_max its smallest and largest value (they size the sort: keys are group - g_min, so negative labels come
 * first).  Columns are device arrays IN THE CALLER'S ROW ORDER, of the type named beside them.  At most 2^31 - 2 rows.
 * Scratch comes from the library's arena; every call runs on `stream` and synchronises it before it returns.
 *
 * pmi_centers_order_dev    d_rows[q] (int32, n entries) = the row at sorted position q, equal to
 *                          np.argsort(group, kind="stable"); d_unique[g] (int64, room for n) = the distinct labels,
 *                          ascending; d_start[g] (int32, room for n + 1) = the first sorted position of label g, with
 *                          d_start[*n_groups] = n.
 * pmi_centers_weights_dev  d_w[i] = 1 / (lpx[i] + lpy[i])^2 in the columns' type (PMI_CENTERS_F32 / _F64), per row.
 * pmi_centers_stats_dev    per column descriptor, one sequential chain per label over its rows in sorted order (which is
 *                          table order within a label), as pandas' group_mean / group_sum / group_var run them:
 *                            PMI_CENTERS_MEAN    sum / mean: Kahan-compensated sum of the values that are not NaN, in
 *                                                float32 for a float32 column and in float64 (of the converted value)
 *                                                for every other; the compensation is reset to 0 when it becomes NaN;
 *                                                mean = sum / count of those values in the same type, NaN for none.
 *                                                std: Welford's update in float64 for every type, ddof 1, square root in
 *                                                float64, NaN for fewer than two values.  sum / mean / std are written
 *                                                where the pointer is not NULL (sum and mean in the summing type, std
 *                                                float64).
 *                            PMI_CENTERS_XSUM    the same sum of data[i] * weight[i], float64 unless both are float32
 *                                                (float columns only).
 *                            PMI_CENTERS_FIRST   sum[g] = the label's first value that is not NaN (NaN where there is
 *                                                none), in the column's own type.
 *                            PMI_CENTERS_EVENTS  sum[g] (int32) = the sorted positions of the label that are its first
 *                                                or whose frame - previous frame > 3, the difference taken in the
 *                                                integer column's own type (an unsigned column that decreases wraps
 *                                                and counts).
 *                          At most 32 descriptors.
 * pmi_centers_hull_dev     d_area[g] (float64) = the area of the convex hull of the label's (x, y) as float64: rows are
 *                          ordered by (label, x, y) with three stable radix sorts, one lane per label runs the monotone
 *                          chain and sums the shoelace terms relative to the first hull vertex.  0.0 for fewer than three
 *                          hull vertices or collinear rows.  x / y float32 or float64, each on its own. */
enum pmi_centers_type { PMI_CENTERS_F32 = 0, PMI_CENTERS_F64 = 1, PMI_CENTERS_U32 = 2, PMI_CENTERS_I32 = 3,
                        PMI_CENTERS_U64 = 4, PMI_CENTERS_I64 = 5 };
enum pmi_centers_op { PMI_CENTERS_MEAN = 0, PMI_CENTERS_XSUM = 1, PMI_CENTERS_FIRST = 2, PMI_CENTERS_EVENTS = 3 };
typedef struct pmi_centers_column {
    const void *data;     /* device column */
    const void *weight;   /* device column (XSUM) */
    void *sum;            /* device, n_groups entries; may be NULL for MEAN */
    void *mean;           /* device, n_groups entries (MEAN), may be NULL */
    void *std;            /* device, n_groups float64 entries (MEAN), may be NULL */
    int32_t op, type, w_type;
} pmi_centers_column;
int pmi_centers_order_dev(const int64_t *d_group, int64_t n, int64_t g_min, int64_t g_max, int32_t *d_rows,
                          int32_t *d_start, int64_t *d_unique, int64_t *n_groups, void *stream);
int pmi_centers_weights_dev(const void *d_lpx, const void *d_lpy, int type, int64_t n, void *d_w, void *stream);
int pmi_centers_stats_dev(const int32_t *d_rows, const int32_t *d_start, int64_t n, int64_t n_groups,
                          const pmi_centers_column *columns, int n_columns, void *stream);
int pmi_centers_hull_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int64_t *d_group,
                         int64_t g_min, int64_t g_max, const int32_t *d_start, int64_t n, int64_t n_groups,
                         double *d_area, void *stream);

/* ---- dark times and group properties (picasso/postprocess.py:1985-2004 _dark_times, :3580-3649 groupprops,
 * csrc/kinetics.hip) --------------------------------------------------------------------------------------------- *
 * Columns are int64 device arrays IN THE CALLER'S ROW ORDER unless said otherwise (the host widens any integer column).
 * At most 2^31 - 2 rows.  Scratch comes from the library's arena; every call runs on `stream` and synchronises it.
 *
 * pmi_kinetics_dark_order_dev   orders the rows by (group - g_min, last_frame - l_min) with two stable radix sorts;
 *                               l_min / l_max and g_min / g_max are the smallest and largest value of the two columns.
 *                               d_rows[q] (int32, n) = the row at sorted position q, d_last_sorted[q] (int64, n) its
 *                               last frame, d_run[q] (int32, n) the number of its group's run, d_start[r] (int32, room
 *                               for n + 1) the first sorted position of run r, closed by n.
 * pmi_kinetics_dark_search_dev  d_dark[i] (int64, n) = the smallest frame[i] - last_frame[j] > 0 over the other rows j
 *                               of row i's group, as a signed 64-bit difference, when it is < max_frame; -1 otherwise.
 *                               One lane per sorted position bisects its own run.
 * pmi_kinetics_stats_dev        per column descriptor and group (d_rows / d_start are pmi_centers_order_dev's: rows in
 *                               table order within a group) what pandas' Series.mean() / Series.std() return, as
 *                               float64: NaN counted as 0 and counted out; every sum is NumPy's add.reduce (an
 *                               accumulator from 0 over the pairwise sums of 8192-element chunks).  mean: the sum in
 *                               float32 for a float32 column and in float64 (of the converted value) for every other,
 *                               over the count in that type; NaN for no value.  std (ddof 1): avg = the float64 sum over
 *                               the count, the float64 sum of (avg - v)^2 over count - 1, the root in float32 for a
 *                               float32 column and in float64 otherwise; NaN for fewer than two values.  `type` is a
 *                               pmi_centers_type.  mean / std are written where the pointer is not NULL.  At most 64
 *                               descriptors. */
typedef struct pmi_kinetics_column {
    const void *data;     /* device column */
    double *mean;         /* device, n_groups entries, may be NULL */
    double *std;          /* device, n_groups entries, may be NULL */
    int32_t type;
} pmi_kinetics_column;
int pmi_kinetics_dark_order_dev(const int64_t *d_last, const int64_t *d_group, int64_t n, int64_t l_min, int64_t l_max,
                                int64_t g_min, int64_t g_max, int32_t *d_rows, int64_t *d_last_sorted, int32_t *d_run,
                                int32_t *d_start, void *stream);
int pmi_kinetics_dark_search_dev(const int64_t *d_frame, const int32_t *d_rows, const int64_t *d_last_sorted,
                                 const int32_t *d_run, const int32_t *d_start, int64_t n, int64_t max_frame,
                                 int64_t *d_dark, void *stream);
int pmi_kinetics_stats_dev(const int32_t *d_rows, const int32_t *d_start, int64_t n, int64_t n_groups,
                           const pmi_kinetics_column *columns, int n_columns, void *stream);

/* ---- kinetic rates of picks (picasso/lib.py:1263-1327 estimate_kinetic_rate, fit_cum_exp; csrc/cumexp.hip,
 * csrc/cumexp_core.h) ------------------------------------------------------------------------------------------- *
 * The samples of n_seg segments as a CSR: float64 `values` (n_values of them, below 2^31 - 1) and int64
 * `offsets[n_seg + 1]` ascending from 0 to at most n_values (checked; PMI_ERR_ARG otherwise).  `kind` names the column
 * the values were converted from: 0 an integer column (exact in float64 below 2^53), 1 float32, 2 float64.  Per
 * segment of n samples, as lib.estimate_kinetic_rate decides:
 *   n <= 2, or max - min == 0    t = np.nanmean of the samples in the column's arithmetic (kind 0: the exact float64 sum
 *                                over n; kinds 1, 2: NumPy's add.reduce with NaN as 0 in float32 / float64 over the count
 *                                of the values that are not NaN); NaN for no sample; a, c, cost NaN; 0 iterations
 *   otherwise                    the samples in ascending order x, y = 1 .. n, and the bounded least-squares fit of
 *                                a (1 - exp(-x / t)) + c in float64 from p0 = (n, mean, min) with a in [0, inf),
 *                                t in [min, max], c in [0, inf): a damped Newton method (cumexp_core.h) that only ever
 *                                accepts a point whose cost is not above the last one, and ends on its own tolerances
 * d_fit holds 4 x n_seg float64: a, t, c and the final cost 0.5 sum r^2, one array behind the other; d_info 2 x n_seg
 * int32: the passes over the samples, then the status: 0 converged (or not fitted), 1 the iteration cap (300 passes),
 * 2 an input scipy refuses with ValueError (a NaN or an infinity in a segment that would be fitted, or a negative
 * minimum); with status 2 the four values are NaN.  Bit parity with scipy's trust-region solver is not claimed: the
 * contract is a cost that is not above scipy's (tests/test_gpu_pickkin.py).  One wavefront per segment, no atomics;
 * scratch from the library's arena; runs on `stream` and synchronises it.  pmi_cumexp_fit is the same from host arrays. */
int pmi_cumexp_fit_dev(const double *d_values, int64_t n_values, const int64_t *d_offsets, int64_t n_seg, int kind,
                       double *d_fit, int32_t *d_info, void *stream);
int pmi_cumexp_fit(const double *values, int64_t n_values, const int64_t *offsets, int64_t n_seg, int kind, double *fit,
                   int32_t *info);

/* ---- nearest-neighbour distances (picasso/postprocess.py:3704-3739 nn_analysis, picasso/spinna.py:696-747 get_NN_dist,
 * csrc/knn.hip, csrc/knn_search.h) ------------------------------------------------------------------------------- *
 * Point sets are float64 device arrays of shape (rows, dims), row-major, dims 2 or 3, finite, at most 2^31 - 2 rows.
 * Scratch comes from the library's arena; every call runs on `stream` and synchronises it.
 *
 * pmi_knn_limit       the largest k of a query (32).
 * pmi_knn_order_dev   orders the set X2 for queries: lo / hi (host, 2 entries each) are the smallest and largest x and y
 *                     of the set (anything when m = 0); *grid receives the uniform grid over that box, planned for
 *                     queries of k neighbours (it serves any k).  d_sorted (m * dims) receives the rows sorted by cell,
 *                     d_start (int32, room for max(m, 1) + 1) the first sorted row of every cell, closed by m.
 * pmi_knn_query_dev   d_out[i * k + j] (n x k) = the j-th smallest float64 distance sqrt(dx * dx + dy * dy (+ dz * dz))
 *                     from row i of X1 to the rows of the ordered set, +inf where the set has fewer than k rows: what
 *                     scipy.spatial.KDTree(X2).query(X1, k) returns as distances, in every bit.  One ordered set
 *                     serves any number of query sets. */
typedef struct pmi_knn_grid {
    double lo[2], w[2];   /* corner and cell size */
    int32_t n[2];         /* cells in x and y */
} pmi_knn_grid;
int pmi_knn_limit(void);
int pmi_knn_order_dev(const double *d_x2, int dims, int64_t m, const double *lo, const double *hi, int64_t k,
                      double *d_sorted, int32_t *d_start, pmi_knn_grid *grid, void *stream);
int pmi_knn_query_dev(const double *d_x1, int dims, int64_t n, const double *d_sorted, const int32_t *d_start, int64_t m,
                      const pmi_knn_grid *grid, int64_t k, double *d_out, void *stream);

/* ---- cluster combine and its nearest-cluster distances (picasso/postprocess.py:2174-2288 cluster_combine, :2291-2419
 * cluster_combine_dist, csrc/combine.hip, csrc/segment_stats.h) ------------------------------------------------------ *
 * Label columns are int64 device arrays IN THE CALLER'S ROW ORDER (the host widens any integer column).  At most
 * 2^31 - 2 rows.  Scratch comes from the library's arena; every call runs on `stream` and synchronises it.
 *
 * pmi_combine_order_dev    orders the rows by (group - g_min, cluster - c_min) with two stable radix sorts; g_min / g_max
 *                          and c_min / c_max are the smallest and largest label of the two columns.  A segment is a run of
 *                          one (group, cluster) pair: groups ascend, clusters ascend within a group, rows keep their table
 *                          order within a segment.  d_rows[p] (int32, n) = the row at sorted position p, d_start[s] (int32,
 *                          room for n + 1) the first sorted position of segment s, closed by n, d_seg_group[s] /
 *                          d_seg_cluster[s] (int64, n) its labels, d_group_start[g] (int32, room for n + 1) the first
 *                          SEGMENT of group g, closed by *n_segments.  d_rows / d_start are a table of the kind
 *                          pmi_centers_order_dev returns: pmi_kinetics_stats_dev takes them too.
 * pmi_combine_stats_dev    per column descriptor and segment, as float64, where the pointer is not NULL:
 *                            mean / std        pandas' Series.mean() / Series.std() (ddof 1), exactly as
 *                                              pmi_kinetics_stats_dev computes them (one shared header).
 *                            average           np.average(data, weights=weight) of two columns of ONE floating type T
 *                                              (`type`; the host promotes as np.average does): the products rounded to T,
 *                                              NumPy's add.reduce of the products and of the weights in T (pairwise, 8192-
 *                                              element chunks), one division in T.  Nothing is skipped: NaN gives NaN.
 *                            weight_sum        that sum of the weights; where it is exactly 0 np.average raises, and so
 *                                              does the host.
 *                          `type` is a pmi_centers_type.  At most 32 descriptors.
 * pmi_combine_mindist_dev  d_points (n x dims float64, row-major, dims 2 or 3, caller's row order) with the order of
 *                          pmi_combine_order_dev in which EVERY SEGMENT IS ONE ROW (n_segments = n is the host's to
 *                          check).  d_min_dist[p] (float64, n, SORTED position p) = the smallest
 *                          sqrt(((dx * dx) + (dy * dy)) (+ (dz * dz))) from that row to the other rows of its group, as
 *                          scipy's cdist and np.amin give it: the row itself is left out by position, not by distance; a
 *                          NaN stays; +inf for a group of one row.  With dims = 3, d_min_dist_xy[p] is the same over x
 *                          and y alone (it may be NULL with dims = 2).  One workgroup per tile of 256 rows of one group,
 *                          the group's rows streamed through LDS: quadratic in the rows of a group. */
typedef struct pmi_combine_column {
    const void *data;     /* device column */
    const void *weight;   /* device column of the same type (average / weight_sum), else NULL */
    double *mean;         /* device, n_segments entries, may be NULL */
    double *std;          /* device, n_segments entries, may be NULL */
    double *average;      /* device, n_segments entries, may be NULL */
    double *weight_sum;   /* device, n_segments entries, may be NULL */
    int32_t type;
} pmi_combine_column;
int pmi_combine_order_dev(const int64_t *d_group, const int64_t *d_cluster, int64_t n, int64_t g_min, int64_t g_max,
                          int64_t c_min, int64_t c_max, int32_t *d_rows, int32_t *d_start, int64_t *d_seg_group,
                          int64_t *d_seg_cluster, int32_t *d_group_start, int64_t *n_segments, int64_t *n_groups,
                          void *stream);
int pmi_combine_stats_dev(const int32_t *d_rows, const int32_t *d_start, int64_t n, int64_t n_segments,
                          const pmi_combine_column *columns, int n_columns, void *stream);
int pmi_combine_mindist_dev(const double *d_points, int dims, const int32_t *d_rows, const int32_t *d_start,
                            const int32_t *d_group_start, int64_t n, int64_t n_segments, int64_t n_groups,
                            double *d_min_dist, double *d_min_dist_xy, void *stream);

/* ---- cluster areas and volumes (picasso/clusterer.py:1068-1169 _cluster_area / cluster_areas, picasso/masking.py:408-446
 * threshold_otsu, csrc/areas.hip) ------------------------------------------------------------------------------------ *
 * d_rows / d_start are the group order of pmi_centers_order_dev.  The coordinates are device columns in the caller's row
 * order, each float32 or float64 (a pmi_centers_type); the points of a group are those columns in their common type T
 * (`f32` says it is float32), z divided by z_div and rounded to T.  One workgroup per group.  Every call runs on
 * `stream` and synchronises it.
 *
 * pmi_areas_lds_bins    PMI_AREAS_LDS_BINS: an image of at most that many bins is built, blurred and thresholded in LDS
 *                       (two float64 copies of it, 64 KiB: two workgroups fit a CU); larger ones in global scratch.
 * pmi_areas_max_bins    PMI_AREAS_MAX_BINS: the most bins one image may have; the host refuses a larger one (MemoryError)
 *                       before any image is built, and likewise an axis of more than that many bins.
 * pmi_areas_shape_dev   d_geom[g]: per dimension the smallest and largest coordinate give np.arange(min, max + bin, bin)
 *                       as NumPy computes it from scalars: with PT = float32 when T and the bin are both float32, else
 *                       float64, len = ceil(((max + bin) - min) / bin) in PT (-1: not a number, -2: beyond int64),
 *                       start = min, next = min + bin in PT; edge 0 is start, edge 1 next, edge i is
 *                       start + i * (next - start) in float64.  bin_xy serves x and y, bin_z z.
 * pmi_areas_image_dev   for each of the n_list groups d_list[k]: the float64 counts of np.histogramdd over those edges
 *                       (searchsorted from the right, a value on the last edge in the last bin, rows outside dropped), the
 *                       blur of scipy.ndimage.gaussian_filter(sigma=2) with the 17 host weights d_weights (axes in order,
 *                       reflect, tmp = line[l] * w[8]; for j = 8 .. 1: tmp += (line[l - j] + line[l + j]) * w[8 - j]),
 *                       threshold_otsu on np.histogram(image, 256), and d_area[g] (float32) = count(image >= threshold)
 *                       / 4, or / (16 / 5) with three dimensions, evaluated in float64.  No contraction anywhere.
 *                       d_offset == NULL: every listed image has at most PMI_AREAS_LDS_BINS bins and lives in LDS.
 *                       Otherwise image k lives in d_scratch[d_offset[k] .. + 2 * bins) (float64 entries, scratch_len in
 *                       all).  Both paths run the same arithmetic in the same order.  Groups without bins are the
 *                       host's (area 0).  With want_group >= 0 the blurred image of that group is also copied to
 *                       d_want_image (row-major, room for its bins). */
#define PMI_AREAS_LDS_BINS 4096
#define PMI_AREAS_MAX_BINS (1 << 24)
typedef struct pmi_areas_columns {
    const void *data[3];  /* x, y, z device columns (z NULL with two dimensions) */
    int32_t type[3];      /* PMI_CENTERS_F32 / PMI_CENTERS_F64 */
    int32_t dims;         /* 2 or 3 */
    int32_t f32;          /* the common type of the columns is float32 */
    double z_div;         /* the pixel size z is divided by */
} pmi_areas_columns;
typedef struct pmi_areas_geom {
    double start[3], next[3];
    int64_t len[3];       /* edges per dimension; bins are max(len - 1, 0) */
} pmi_areas_geom;
int pmi_areas_lds_bins(void);
int pmi_areas_max_bins(void);
int pmi_areas_shape_dev(const pmi_areas_columns *cols, const int32_t *d_rows, const int32_t *d_start, int64_t n,
                        int64_t n_groups, double bin_xy, double bin_z, int bin_f32, pmi_areas_geom *d_geom, void *stream);
int pmi_areas_image_dev(const pmi_areas_columns *cols, const int32_t *d_rows, const int32_t *d_start, int64_t n,
                        int64_t n_groups, const pmi_areas_geom *d_geom, const int32_t *d_list, const int64_t *d_offset,
                        int64_t n_list, double *d_scratch, int64_t scratch_len, const double *d_weights, float *d_area,
                        int64_t want_group, double *d_want_image, void *stream);

/* ---- particle averaging (picasso/average.py:49-118 align_group_core, :354-530 average, csrc/average.hip) ------------- *
 * d_rows / d_start are the group order of pmi_centers_order_dev; d_x / d_y are the float32 coordinates the reference
 * keeps in its shared arrays, in the caller's row order.  The view is t_min < v < t_max (strict), the image n_pixel x
 * n_pixel, all given as the host computed them in the reference's expressions.  Every call runs on `stream` and
 * synchronises it.  csrc/average_core.h holds the arithmetic and compiles for the host.
 *
 * pmi_average_limits     PMI_AVERAGE_LDS_BINS: an average image of at most that many pixels is held in LDS by the align
 *                        kernel (64 KiB of int32, with the 8 KiB pixel list two workgroups fit a CU), a larger one is
 *                        read from global memory; PMI_AVERAGE_LIST: the rows of a group rotated at a time (larger groups
 *                        go in tiles); PMI_AVERAGE_MAX_PIXELS: the most pixels per axis.
 * pmi_average_image_dev  render_hist_numba of the table: d_image[row * n_pixel + column] (int32, zeroed here) counts the
 *                        rows in view at int32(oversampling * (v - t_min)), the difference taken in float32 when sub_f32
 *                        and the product in float32 when mul_f32 (NumPy's types for a float32 column), else in float64.
 *                        *d_dropped counts rows in view whose pixel rounding carried outside the image (the reference
 *                        fails on them).
 * pmi_average_align_dev  per group and per chunk c of the angle list (angles c * ceil(n_angles / chunks) ...): over every
 *                        angle a and every entry (iy, ix) of np.fft.fftshift of the circular cross-correlation of the
 *                        group's image with d_image, the integer
 *                            sum over the group's rows in view of d_image[(py - sy) mod n][(px - sx) mod n],
 *                            (sy, sx) = ((iy - n / 2) mod n, (ix - n / 2) mod n),
 *                        rows rotated as cos(a) * x - sin(a) * y, sin(a) * x + cos(a) * y in float64 with d_cos / d_sin,
 *                        each operation rounded on its own.  d_parts[3 * (g * chunks + c)] = the largest value, then the
 *                        lowest angle, then the lowest iy * n + ix; (0, -1, -1) when every value is 0.  use_lds: the
 *                        image has at most PMI_AVERAGE_LDS_BINS pixels and is held in LDS; both paths give the same
 *                        integers.  A sum must stay below 2^31: the caller checks rows-of-largest-group * max(image).
 * pmi_average_apply_dev  d_choice[3 * g] = the chunks of group g reduced in the same order (value, angle index, flat index;
 *                        (0, -1, -1): nothing chosen, the rows stay as they are), and for its rows
 *                            x' = cos * x - sin * y - ceil(ix - n / 2) / oversampling, y' likewise with iy,
 *                        in float64, stored as float32 in d_x_out / d_y_out (same row order as d_x / d_y). */
#define PMI_AVERAGE_LDS_BINS 16384
#define PMI_AVERAGE_LIST 2048
#define PMI_AVERAGE_MAX_PIXELS 4096
int pmi_average_limits(int *lds_bins, int *list, int *max_pixels);
int pmi_average_image_dev(const float *d_x, const float *d_y, int64_t n, int64_t n_pixel, double t_min, double t_max,
                          double oversampling, int sub_f32, int mul_f32, int32_t *d_image, int32_t *d_dropped, void *stream);
int pmi_average_align_dev(const float *d_x, const float *d_y, const int32_t *d_rows, const int32_t *d_start, int64_t n,
                          int64_t n_groups, int64_t n_pixel, double t_min, double t_max, double oversampling,
                          const double *d_cos, const double *d_sin, int64_t n_angles, int64_t chunks,
                          const int32_t *d_image, int use_lds, int32_t *d_parts, int32_t *d_dropped, void *stream);
int pmi_average_apply_dev(const float *d_x, const float *d_y, const int32_t *d_rows, const int32_t *d_start, int64_t n,
                          int64_t n_groups, int64_t n_pixel, double oversampling, const double *d_cos, const double *d_sin,
                          int64_t n_angles, const int32_t *d_parts, int64_t chunks, int32_t *d_choice, float *d_x_out,
                          float *d_y_out, void *stream);

/* ---- Fourier ring correlation (picasso/postprocess.py:1398-1502 _frc, picasso/imageprocess.py:283-321 radial_sum, ------- *
 *      csrc/frc.hip, csrc/frc_core.h)
 * pmi_frc_curve[_dev]    im1, im2: two float32 images of side m, row-major.  An even m loses its last row and column
 *                        (n = m - 1), an odd one keeps all (n = m).  w: the n float64 values of the Tukey profile
 *                        (threshold_tukey's one row, computed by the caller with NumPy's cos).  Outputs, with
 *                        rings = n / 2 + 1: masked1 / masked2 (n x n float32) = float32(float64(im) * (w[j] * w[n - 1 - i])),
 *                        NumPy's bits for `im *= mask`; sums (3 x rings float64) = the ring sums of real(F1 conj F2),
 *                        |F1|^2, |F2|^2 over the whole fftshifted plane, F the float64 transforms of the masked images;
 *                        curve (rings float64) = sums[0] / sqrt(|sums[1] * sums[2]|), NaN -> 0.  Ring r holds the bins
 *                        with r^2 <= kx^2 + ky^2 < (r + 1)^2 in integer arithmetic; the corners beyond ring n / 2 are
 *                        dropped.  Deterministic: no atomics, a fixed order of additions.  The _dev variant takes device
 *                        pointers, runs on `stream`, synchronises it, and fills ms4 (host, may be NULL) with the
 *                        milliseconds of window, transforms, ring sums and curve by device events.
 * pmi_radial_sum         host arrays: out[r] = the sum of the bins of ring r of a centred n x n image (n odd), summed in
 *                        float64 per component and cast to the image's type (PMI_RADIAL_*).
 * PMI_FRC_MAX_SIDE       the largest odd side: kx^2 + ky^2 stays below 2^28, and the two float64 images and two half
 *                        spectra take 32 n^2 bytes of scratch (8.6 GB) beside hipFFT's own work area.              */
#define PMI_FRC_MAX_SIDE 16385
#define PMI_RADIAL_F32 0
#define PMI_RADIAL_F64 1
#define PMI_RADIAL_C64 2
#define PMI_RADIAL_C128 3
int pmi_frc_max_side(void);
int pmi_frc_curve(const float *im1, const float *im2, int64_t m, const double *w, double *sums, double *curve,
                  float *masked1, float *masked2);
int pmi_frc_curve_dev(const float *d_im1, const float *d_im2, int64_t m, const double *d_w, double *d_sums, double *d_curve,
                      float *d_masked1, float *d_masked2, float *ms4, void *stream);
int pmi_radial_sum(const void *image, int dtype, int64_t n, void *out);

/* ---- picked localizations (picasso/postprocess.py:207-473, :849-928, picasso/lib.py:1884-2004, csrc/picks.hip) ------- *
 * The member rows of every pick of one call, as a CSR pair: d_offsets[n_picks + 1] (int64) and d_members (int32 rows in
 * the caller's row order).  Each of the two pick calls is made twice: with d_members == NULL it counts, fills d_offsets
 * and *total (the one device-to-host copy, which sizes d_members); with d_members it reads d_offsets and writes at most
 * `capacity` rows.  One workgroup per pick, all picks in one launch.  d_x / d_y are the table's columns, float32 or
 * float64 (PMI_LINK_F32 / PMI_LINK_F64, each on its own); d_rows / d_keys / p are what pmi_pairs_order_dev returned.
 * Every call runs on `stream` and synchronises it before it returns.  Divisions follow IEEE.
 *
 * pmi_picks_circle_dev   over the sanity-filtered table in the block order of get_index_blocks (K x L blocks of the pick
 *                        radius).  Pick i lies at (d_pick_x[i], d_pick_y[i]) in block (d_block_y[i], d_block_x[i]) =
 *                        int(y / r), int(x / r), computed by the host; it walks the blocks k = by - 1 .. by + 1,
 *                        l = bx - 1 .. bx + 1 with 0 <= k < K, 0 <= l < L, k outside l, over the positions < p, and keeps
 *                        the rows with dx ** 2 + dy ** 2 < r2 in that order (the reference's order before its sort by
 *                        frame).  d_flags[i] bit 0 / bit 1 keep the x / y difference and its square in float32 when
 *                        that column is float32 (an integer or float32 pick coordinate, as numba types it), bit 2
 *                        compares a sum of two float32 squares with float32(r2); all else is float64.
 * pmi_picks_cells_dev    the uint32 cell indices of every row on a grid of CX x CY cells of `cell` from (x0, y0); a row
 *                        outside [x0, x1] x [y0, y1] (a NaN too) gets (x_index, y_index) = (0, CY), outside the grid.
 *                        pmi_pairs_order_dev(.., K = CY, L = CX, ..) then gives the order pmi_picks_shape_dev walks.
 * pmi_picks_shape_dev    shape 0 Square, 1 Rectangle, 2 Polygon over the whole table binned as above (the same grid
 *                        arguments).  d_bounds[4 i ..] = x_min, x_max, y_min, y_max of pick i, strict; bit b of
 *                        d_flags[i] says bound b is a weak (Python) scalar, compared in the column's own type, else the
 *                        compare is float64.  Rectangle and Polygon then test the corners
 *                        d_corner_x / d_corner_y [d_corner_offsets[i] .. d_corner_offsets[i + 1]) in float64, in the
 *                        operation order of check_if_in_rectangle (4 corners) / check_if_in_polygon.  Members of a pick
 *                        ascend by row (a segmented radix sort), as a boolean mask leaves them.                     */
int pmi_picks_circle_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int32_t *d_rows,
                         const uint64_t *d_keys, int64_t n, int64_t p, int64_t K, int64_t L, const double *d_pick_x,
                         const double *d_pick_y, const int64_t *d_block_x, const int64_t *d_block_y,
                         const uint8_t *d_flags, int64_t n_picks, double r2, int64_t *d_offsets, int32_t *d_members,
                         int64_t capacity, int64_t *total, void *stream);
int pmi_picks_cells_dev(const void *d_x, int x_type, const void *d_y, int y_type, int64_t n, double x0, double y0,
                        double x1, double y1, double cell, int64_t CX, int64_t CY, uint32_t *d_x_index,
                        uint32_t *d_y_index, void *stream);
int pmi_picks_shape_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int32_t *d_rows,
                        const uint64_t *d_keys, int64_t n, int64_t p, double x0, double y0, double x1, double y1,
                        double cell, int64_t CX, int64_t CY, int shape, const double *d_bounds, const uint8_t *d_flags,
                        const int32_t *d_corner_offsets, const double *d_corner_x, const double *d_corner_y,
                        int64_t n_corners, int64_t n_picks, int64_t *d_offsets, int32_t *d_members, int64_t capacity,
                        int64_t *total, void *stream);

/* ---- fiducial undrift (picasso/postprocess.py:3062-3156 undrift_from_picked, _undrift_from_picked_coordinate,
 *      csrc/fiducials.hip, csrc/group_reduce.h) ------- *
 * pmi_fiducials_drift_dev  the drift of n_columns (1 .. 3) coordinates from the member rows of n_picks >= 1 picks, in
 *   the bits NumPy 2 gives the reference.  The rows come as a CSR in pick order: d_offsets[n_picks + 1] (int64, ascending,
 *   d_offsets[0] == 0, d_offsets[n_picks] == n_rows), d_frame[n_rows] (int64) and the columns d_columns[c][n_rows] of
 *   types[c] (PMI_LINK_F32 / PMI_LINK_F64); d_columns and types are host arrays, the pointers in d_columns device
 *   pointers.  d_out[n_frames * n_columns] (float64, frame-major) receives the drift.  Per column, of type T:
 *     1. mean_p = add.reduce(c[rows of pick p, in the given order]) / T(n_p) in T: NumPy's sum, an accumulator that takes
 *        the pairwise sum of each 8192-element chunk in order, by one workgroup per pick; an empty pick has a NaN mean;
 *     2. D[p, frame] = float64(c - mean_p), subtracted in T, into a P x Frames float64 matrix of NaN; on a repeated frame
 *        of a pick the row latest in the given order wins, whatever the launch order; a frame f < 0 means f + n_frames;
 *     3. m0[f] = (sum over p = 0 .. P - 1 in order, from row 0, of D or 0 for a NaN) / (number that are not NaN), 0 / 0 NaN;
 *     4. msd_p = add.reduce over f of ((D - m0) ** 2 or 0 for a NaN) / (number that are not NaN); w_p = 1 / msd_p;
 *     5. num[f] = sum over p in order of (D * w_p, or 0 for a NaN of D), den[f] = sum of (w_p * 1.0, or 0 for a NaN of D);
 *        the frame has no value where no pick has it or where |num| * DBL_MIN >= |den|, else num / den;
 *     6. a frame without a value (or with a NaN one) takes np.interp over the frames with one: the first / last value
 *        outside them, slope * (f - f_lo) + y_lo with slope = (y_hi - y_lo) / (f_hi - f_lo) between.
 *   Steps 2 - 6 are float64; nothing is contracted.  *status (host) is 0, or has bit 0 set when a frame lies outside
 *   [-n_frames, n_frames) (NumPy: IndexError) and bit 1 when a column leaves no frame with a value (np.interp:
 *   ValueError); d_out is then not to be read.  n_picks * n_frames <= pmi_fiducials_max_cells() (2^28: the matrix and
 *   the winner table of step 2 take 12 bytes per cell of SCR_STAGE_A, shared by the columns), n_rows <= 2^31 - 2, else
 *   PMI_ERR_ARG.  Runs on `stream` and synchronises it.
 * pmi_fiducials_reduce_dev  step 1's sum alone: d_out[r] (of `type`) = add.reduce(d_values[d_offsets[r] .. d_offsets[r + 1]))
 *   in `type`, one workgroup per run; what the tests hold against np.add.reduce.                                    */
int64_t pmi_fiducials_max_cells(void);
int pmi_fiducials_drift_dev(const int64_t *d_offsets, int64_t n_picks, const int64_t *d_frame, int64_t n_rows,
                            const void *const *d_columns, const int *types, int n_columns, int64_t n_frames,
                            double *d_out, int *status, void *stream);
int pmi_fiducials_reduce_dev(const void *d_values, int type, int64_t n_values, const int64_t *d_offsets, int64_t n_runs,
                             void *d_out, void *stream);

/* ---- pick similar (picasso/postprocess.py:597-736 _pick_similar, :820-845 _n_block_locs_at, :848-957
 *      get_block_locs_at_numba, locs_at_numba, rmsd_at_com; csrc/similar.hip) ------- *
 * pmi_similar_shift_dev  the mean shift of every point of pick_similar's hexagonal grid, one lane per point, in the bits
 *   numba gives the reference.  d_x / d_y are the sanity-filtered table's columns, float32 or float64 (PMI_LINK_F32 /
 *   PMI_LINK_F64, each on its own); d_rows / d_keys / p / K / L are what pmi_pairs_order_dev returned for blocks of the
 *   pick radius.  The grid comes as the host built it: column i lies at d_grid_x[i] in block column d_block_x[i]
 *   (i < n_x); its n_y points lie at d_grid_y_base[j] in block row d_block_y_base[j] when i is even and at
 *   d_grid_y_shift[j], d_block_y_shift[j] when i is odd.  Point i * n_y + j (the reference's loop order) writes
 *   d_out_x, d_out_y (float64), d_out_n (int32) and d_out_rmsd (float64):
 *     1. the gate: the rows of the blocks k = by - 1 .. by + 1, l = bx - 1 .. bx + 1 with 0 < k < K and 0 < l < L (block
 *        row 0 and block column 0 never count; no such block: 0) must number >= gate, else n = 0;
 *     2. the point's rows are those of the same blocks with 0 <= k < K, 0 <= l < L, k outside l, positions < p, gathered
 *        once in the columns' common type S (float32 only when both are) and not taken again as the centre moves;
 *     3. members of a centre c (float64): (S - c.x) ** 2 + (S - c.y) ** 2 < r2 in float64, strict; their mean is
 *        float64(sum in S, in block order, from S(0)) / n.  At most one member around the grid point: n = 0;
 *     4. the centre moves to the mean; while |dx| > 1e-3 or |dy| > 1e-3, at most max_shifts times (the reference: 500;
 *        at most 65536), the members are taken around the new centre; at most one member ends the loop;
 *     5. n is the size of the last set, (out_x, out_y) its mean (the mean before it when n <= 1) and out_rmsd =
 *        sqrt(sum in order of ((S - out_x) ** 2 + (S - out_y) ** 2) / n), 0 when n <= 1.  A skipped point (n = 0 from
 *        step 1 or 3) writes the grid point and 0.
 *   Nothing is contracted; the divisions and the square root are correctly rounded.  The gathered columns take 2 p
 *   values of SCR_STAGE_A.  n_x * n_y <= 2^31 - 2.  Runs on `stream` and synchronises it.
 * pmi_similar_filter     the reference's greedy pass, on the host, over host arrays: candidate i (in grid order) gets
 *   keep[i] = 1 when every given pick and every earlier kept candidate q has (q.x - x) ** 2 + (q.y - y) ** 2 > d2 in
 *   float64, uncontracted, else 0.  `cell` is the pick diameter d: the picks are held on a uniform grid of cells a
 *   little wider than it and a candidate looks at the 3 x 3 cells around its own (any cell is correct when cell is not
 *   positive; the given picks may lie closer together than d and are all checked).  Non-finite input: PMI_ERR_ARG.  */
int pmi_similar_shift_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int32_t *d_rows,
                          const uint64_t *d_keys, int64_t n, int64_t p, int64_t K, int64_t L, const double *d_grid_x,
                          const int64_t *d_block_x, int64_t n_x, const double *d_grid_y_base,
                          const double *d_grid_y_shift, const int64_t *d_block_y_base, const int64_t *d_block_y_shift,
                          int64_t n_y, double r2, double gate, int64_t max_shifts, double *d_out_x, double *d_out_y,
                          int32_t *d_out_n, double *d_out_rmsd, void *stream);
int pmi_similar_filter(const double *cand_x, const double *cand_y, int64_t n_candidates, const double *pick_x,
                       const double *pick_y, int64_t n_picks, double d2, double cell, uint8_t *keep);

/* ---- G5M molecular mapping in 2-D (picasso/g5m.py:820-902 _find_optimal_G5M_2D, :482-567 G5M.fit, :2126-2298
 * _fit_G5M, :1829-2064 _convert_G5M_results; csrc/g5m.hip, csrc/g5m_core.h) ------------------------------------------ *
 * Clusters are a CSR over float64 x, y, lp (lp: the mean of lpx and lpy per row; read only with "local" bounds but
 * always present): int64 offsets[n_clusters + 1] ascending from 0 (checked).  The kernels draw no random numbers.  The
 * caller draws, with NumPy's legacy generator, for every seed 42 + ii and every cluster size n: RandomState(seed), one
 * choice(n) -> `first`, then uniform()s in order -> `uniform`; every K reads a prefix of them with its own
 * n_local_trials = 2 + int(log K), (K - 1) n_local_trials values.  `table` holds 4 int64 per cluster: where its model
 * starts in the model arrays (K_max = min(100, n / min_locs) components from there, or K for a fixed fit), where its
 * first draws start in `first` (one per seed), where its uniforms start in `uniform`, and how many uniforms each seed has.
 *
 * flags: PMI_G5M_LP_ABS the sigma bounds are absolute (loc_prec_handle "abs"), else factors of the resp-weighted lp;
 *        PMI_G5M_FORCE_SCRATCH the responsibilities live in the scratch arena even where n K <= PMI_G5M_LDS_RESP would keep
 *        them in LDS (the same bits either way).
 * The model arrays hold `total` components: model = 5 x total float64 (weights_ after set_parameters, means_ x, means_ y,
 * covariances_, precisions_cholesky_, one plane behind the other), imodel = 2 x total int32 (n_locs of the valid
 * components in valid order, then valid_idx padded with -1).  info = 4 int32 per cluster: the chosen K (0: no model), the
 * number of valid components, converged, the last K tried.  bic: the model's BIC (inf without one, or for a fixed fit that
 * the Sparrow criterion rejects).
 *
 * pmi_g5m_fit*        the search of _find_optimal_G5M_2D for every cluster: round r fits K = r with max(K, 3)
 *                     initialisations for every cluster still searching, until K_max or max_rounds rounds without a better
 *                     BIC.  `progress` (may be NULL) is called after every round with the round, the clusters it fitted
 *                     and its device time in milliseconds.
 * pmi_g5m_fit_fixed*  G5M_2D(n_components).fit for every cluster (a cluster of fewer rows than components gets no model),
 *                     with optional means_init (n_clusters x n_components x 2 float64).
 * pmi_g5m_assign*     _convert_G5M_results per cluster from its model (table: 2 int64 per cluster, the model's start and
 *                     the start of its n x n_valid block in lp_out / wlp_out): per row the label and the log likelihood,
 *                     per valid component stats = 7 float64 (frame, std_frame, mol_log_likelihood, p_val, the resp-weighted
 *                     lp, the sum of its responsibilities, the resp-weighted log likelihood), n_events and the resp-weighted mean of every column of `cols`
 *                     (n_cols x n_rows float64 -> col_means n_cols x total), per cluster group_log_likelihood.  frame is
 *                     float64.  PMI_G5M_QUAD_F32: x and y hold float32 values and the quadratic form is accumulated in
 *                     float32, as the reference does with a float32 table; PMI_G5M_FRAME_U32: frame differences wrap as
 *                     uint32.  lp_out / wlp_out (may be NULL): estimate_log_prob and estimate_weighted_log_prob of the rows.
 * The _dev forms take device arrays, run on `stream` and synchronise it; the others stage host arrays. */
#define PMI_G5M_LDS_RESP 4096
#define PMI_G5M_MAX_K 100
#define PMI_G5M_LP_ABS 1
#define PMI_G5M_FORCE_SCRATCH 2
#define PMI_G5M_QUAD_F32 4
#define PMI_G5M_FRAME_U32 8
typedef void (*pmi_g5m_progress)(int round, int64_t clusters, double device_ms, void *user);
int pmi_g5m_limits(int *lds_resp, int *max_k, int *threads);
int pmi_g5m_fit_dev(const double *d_x, const double *d_y, const double *d_lp, const int64_t *d_offsets, int64_t n_clusters,
                    int64_t n_rows, const int64_t *d_table, const int32_t *d_first, const double *d_uniform, int min_locs,
                    double sigma_lo, double sigma_hi, int max_rounds, int flags, double *d_model, int32_t *d_imodel, int64_t total,
                    int32_t *d_info, double *d_bic, pmi_g5m_progress progress, void *user, void *stream);
int pmi_g5m_fit(const double *x, const double *y, const double *lp, const int64_t *offsets, int64_t n_clusters, const int64_t *table,
                const int32_t *first, int64_t n_first, const double *uniform, int64_t n_uniform, int min_locs, double sigma_lo,
                double sigma_hi, int max_rounds, int flags, double *model, int32_t *imodel, int64_t total, int32_t *info, double *bic,
                pmi_g5m_progress progress, void *user);
int pmi_g5m_fit_fixed_dev(const double *d_x, const double *d_y, const double *d_lp, const int64_t *d_offsets, int64_t n_clusters,
                          int64_t n_rows, const int64_t *d_table, const int32_t *d_first, const double *d_uniform,
                          const double *d_means_init, int n_components, int min_locs, double sigma_lo, double sigma_hi, int flags,
                          double *d_model, int32_t *d_imodel, int64_t total, int32_t *d_info, double *d_bic, void *stream);
int pmi_g5m_fit_fixed(const double *x, const double *y, const double *lp, const int64_t *offsets, int64_t n_clusters,
                      const int64_t *table, const int32_t *first, int64_t n_first, const double *uniform, int64_t n_uniform,
                      const double *means_init, int n_components, int min_locs, double sigma_lo, double sigma_hi, int flags,
                      double *model, int32_t *imodel, int64_t total, int32_t *info, double *bic);
int pmi_g5m_assign_dev(const double *d_x, const double *d_y, const double *d_lp, const double *d_frame, const int64_t *d_offsets,
                       int64_t n_clusters, int64_t n_rows, const int64_t *d_table, const double *d_model, const int32_t *d_imodel,
                       int64_t total, const int32_t *d_info, const double *d_cols, int n_cols, int flags, int32_t *d_label,
                       double *d_loglik, double *d_stats, int32_t *d_events, double *d_group_ll, double *d_col_means, double *d_lp_out,
                       double *d_wlp_out, int64_t n_prob, void *stream);
int pmi_g5m_assign(const double *x, const double *y, const double *lp, const double *frame, const int64_t *offsets, int64_t n_clusters,
                   const int64_t *table, const double *model, const int32_t *imodel, int64_t total, const int32_t *info,
                   const double *cols, int n_cols, int flags, int32_t *label, double *loglik, double *stats, int32_t *events,
                   double *group_ll, double *col_means, double *lp_out, double *wlp_out, int64_t n_prob);

/* ---- timing hooks for bench.py (HIP events on the given stream) ------- */
int pmi_event_create(void **event);
int pmi_event_record(void *event, void *stream);
int pmi_event_elapsed_ms(void *start, void *stop, float *ms);   /* synchronises on stop */
int pmi_event_destroy(void *event);
/* Milliseconds the last pmi_identify_dev / pmi_gaussmle*_dev spent in its
 * dominant kernel, measured with HIP events around that kernel when enabled. */
/* name of the scan kernel the calling thread's last identify / localize call launched, as rocprofv3 prints it (e.g.
 * "identify_scan_u16_fast_kernel<3, 3, 1, 0, false>", + " defer" when the exact stage may be left to the fit) */
int pmi_last_scan_kernel(char *name, size_t name_len);
int pmi_set_kernel_timing(int enabled);
int pmi_last_kernel_ms(float *scan_ms, float *fit_ms);

#ifdef __cplusplus
}
#endif
#endif /* PICASSO_HIP_H */
