/*
 * libdvh — MI355X (gfx950) C-ABI for the vehicle-pass imaging hot path of NohPei/das_diff_veh.
 *
 * The reference is pure Python; its "FFI" for this path is the Python call surface of
 * apis/virtual_shot_gather.py, apis/dispersion_classes.py and modules/utils.py.  Each entry point
 * below replaces the reference function cited next to it; the Python mirror of the reference API in
 * das_diff_veh_amd/ binds them with ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every pointer is DEVICE memory owned by the caller (e.g. a torch tensor); nothing is
 *     allocated inside;  `stream` is a hipStream_t (NULL = default stream); calls are
 *     stream-ordered, asynchronous and graph-capturable (no host synchronisation inside)
 *   - windows are float32, channel-major: sample (pass p, channel c, time t) is
 *     win[p * pass_stride + c * ch_stride + t]  (strides in elements)
 *   - return 0 on success; negative on error: -2 invalid argument, -3 HIP launch error,
 *     -4 unsupported size; dvh_last_error() describes the calling thread's last error
 */
#ifndef DVH_H
#define DVH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int dvh_abi_version(void);
const char* dvh_last_error(void);

/* Host function: `times` successive random.sample(range(lo, lo + n), k) draws of CPython's `random`
 * (bootstrap_disp's draws, apis/imaging_classes.py:8-48), bit for bit, from the Mersenne Twister state
 * random.getstate()[1] (624 words + index, uint32[625], updated in place for random.setstate()).
 * out: int64 [times][k] (host memory). */
int dvh_random_sample(uint32_t* state, int64_t lo, int64_t n, int32_t k, int32_t times, int64_t* out);

/* Host function: n blocks of nbytes, src[i] -> dst + i * nbytes (host memory, non-temporal stores): the packing
 * of the drop-in classes' NumPy windows (VirtualShotGathersFromWindows, apis/imaging_classes.py:91-126) into a
 * pinned staging buffer before their H2D copy.  Thread-safe; callers split the windows over threads. */
int dvh_host_gather(void* dst, const void* const* src, int64_t nbytes, int32_t n);

/* ---------------------------------------------------------------- virtual shot gathers
 * pass_tab [n_pass][2] = {row0 (= start_idx), pivot_idx};  gather row i is channel row0 + i.
 * seg_tab  [n_pass][R][2 sides][2] = {slice start, slice length} of the row's time slice on the
 *          forward (0) and other (1) side, exactly as the reference slices them
 *          (apis/virtual_shot_gather.py:111-126, 14-43, 152, 172).
 * w = int(wlen / dt), hop = int(w * 0.5) (modules/utils.py:255-256, 292-294).
 * flags: 1 include_other_side, 2 norm (row L2), 4 norm_amp (divide by the pivot row's max).
 */

/* FFT length used for correlation windows of w samples (0 if unsupported). */
int dvh_vsg_fft_length(int32_t w);

/* Per-pass time slices seg_tab[n_pass][R][2][2] derived on the device, float64, with the reference's
 * expressions (preprocessing_window apis/virtual_shot_gather.py:111-126: interp1d extrapolation of
 * the trajectory, pt = argmax(t >= f(pivot) +- delta_t); xcorr_two_traces_based_on_traj :24-35: the
 * per-row t_idx and Python-slice clamping) -- what das_diff_veh_amd.plan.pass_geometry computes on the
 * host, bit for bit.  Inputs per pass p (strides in elements, 0 = shared by every pass):
 *   x_axis[p * x_stride + c] channel positions, t_axis[p * t_stride + t] ascending sample times (n_t),
 *   trajectory trk_x / trk_t[p * trk_stride + k], k < trk_len[p], trk_x strictly ascending,
 *   pivot_x[p] the `pivot` argument, pass_tab[p] = {row0 = start_idx, pivot_idx} (from the spatial
 *   searches, which the host does once per channel axis).
 * flags bit 0: include_other_side.  status[p] = 1 when the trajectory has < 2 points or is not strictly
 * ascending (interp1d would raise / sort); that pass's rows get empty slices. */
int dvh_pass_geometry(const double* x_axis, int64_t x_stride, const double* t_axis, int64_t t_stride, int32_t n_t,
                      const double* trk_x, const double* trk_t, int64_t trk_stride, const int32_t* trk_len,
                      const double* pivot_x, const int32_t* pass_tab, int32_t n_pass, int32_t R, double delta_t,
                      int32_t nsamp, int32_t flags, int32_t* seg_tab, int32_t* status, void* stream);

/* ||window||_F^2 per pass (np.linalg.norm(window.data)**2, apis/virtual_shot_gather.py:125). */
int dvh_window_sumsq(const float* win, int64_t pass_stride, int64_t ch_stride, int32_t n_pass, int32_t n_ch,
                     int32_t n_t, double* out, void* stream);

/* Per-pass, per-side amplitude normalisation: scales[p][side] = 1 / amax(pivot row)
 * (post_processing_XCF, apis/virtual_shot_gather.py:137-138), or 1 / ||window||_F^2 when
 * neither norm nor norm_amp is set (win_sumsq from dvh_window_sumsq; required then, optional
 * otherwise).  When win_sumsq is given, a pass whose window is not finite or all zero gets NaN
 * scales: the reference's data / ||data||_F (:125) makes that whole gather NaN. */
int dvh_vsg_scales(const float* win, int64_t pass_stride, int64_t ch_stride, int32_t n_pass, const int32_t* pass_tab,
                   const int32_t* seg_tab, int32_t R, int32_t w, int32_t hop, int32_t flags, const double* win_sumsq,
                   float* scales, void* stream);

/* Per-pass gathers out[n_pass][R][w]: VirtualShotGather(window, include_other_side, ...).XCF_out
 * (apis/virtual_shot_gather.py:184-192 with construct_shot_gather[_other_side] :145-180,
 * XCORR_vshot / XCORR_two_traces modules/utils.py:253-314). */
int dvh_vsg_gathers(const float* win, int64_t pass_stride, int64_t ch_stride, int32_t n_pass, const int32_t* pass_tab,
                    const int32_t* seg_tab, int32_t R, int32_t w, int32_t hop, int32_t flags, const float* scales,
                    float* out, void* stream);

/* Class stacks, accumulated: stack[slot][R][w] += sum_{p in slot} weight[p] * gather_p.
 * With weight[p] = 1 / count[slot] this is sum(images) / len(images) per class
 * (ImagesFromWindows.get_images, apis/imaging_classes.py:106-107; VirtualShotGather.__add__ /
 * __truediv__ apis/virtual_shot_gather.py:195-210).  order[] lists passes grouped by slot;
 * chunk_tab [n_chunk][3] = {begin, end (into order), slot}.  spec_ws: see dvh_vsg_stack_workspace. */
int dvh_vsg_stack(const float* win, int64_t pass_stride, int64_t ch_stride, int32_t n_pass, const int32_t* pass_tab,
                  const int32_t* seg_tab, int32_t R, int32_t w, int32_t hop, int32_t flags, const float* scales,
                  const int32_t* order, const int32_t* chunk_tab, int32_t n_chunk, const float* weight, float* stack,
                  void* spec_ws, void* stream);

/* dvh_vsg_stack with the windows' validity decided in the same launch.  The reference divides every
 * window by ||data||_F (preprocessing_window, apis/virtual_shot_gather.py:125), so a NaN / inf
 * anywhere in a window [n_ch][n_t], or an all-zero window, makes that pass's gather -- and the mean of
 * its class -- NaN.  This entry reads every sample of every pass's window once, alongside the
 * correlations (at w = 500 the validity scan leaves out the samples the correlations load, which check them
 * themselves), and sets stack[slot] to NaN for each slot (< n_slot) holding such a pass; the
 * scales must then come from dvh_vsg_scales WITHOUT win_sumsq.  Requires flags & (norm | norm_amp):
 * with neither, the scale itself is 1 / ||data||_F^2 (use dvh_window_sumsq).
 * Scan windows: with scan_tab == NULL window p is pass p (win + p * pass_stride, n_ch rows); a unit
 * launch (pass stride 0 over one flattened record, each (pass, pivot) unit a "pass") gives instead
 * n_scan windows of n_ch rows starting at record rows scan_tab[s], and unit_scan[p] = the window
 * whose validity unit p takes (a pass imaged at several pivots is read once).  work: device
 * workspace of (scan_tab ? n_scan : n_pass) + 2 uint32 (per-window max |x| bit pattern, two work
 * counters), zeroed inside. */
int dvh_vsg_stack_validated(const float* win, int64_t pass_stride, int64_t ch_stride, int32_t n_pass, int32_t n_ch,
                            int32_t n_t, const int32_t* pass_tab, const int32_t* seg_tab, int32_t R, int32_t w,
                            int32_t hop, int32_t flags, const float* scales, const int32_t* order,
                            const int32_t* chunk_tab, int32_t n_chunk, int32_t n_slot, const float* weight, float* stack,
                            const int32_t* scan_tab, int32_t n_scan, const int32_t* unit_scan, uint32_t* work,
                            void* spec_ws, void* stream);

/* Bytes of the spec_ws workspace dvh_vsg_stack / dvh_vsg_stack_validated take for n_pass passes at
 * window length w: the spectra of every pass's pivot slices that many rows share (w = 500: the shared
 * windows of both sides and the far rows' clamped windows, 24 KiB + 32 B per pass), which lets the
 * stack launch transform only receivers for those rows (EngF500::spectra_tab).  0 when w does not use
 * it; with spec_ws == NULL the stack entries run the per-sub-window engine instead. */
int64_t dvh_vsg_stack_workspace(int32_t n_pass, int32_t w);

/* The block shape dvh_vsg_stack_validated launches for window length w when it scans n_win windows of
 * n_ch x n_t samples and correlates n_pass passes of R gather rows: 16 x correlation waves + scan waves
 * per block (w = 500: 7 + 1, or 5 + 3 for a launch held by its scan), 0 when the scan is a launch of
 * its own.  Launches nothing. */
int dvh_vsg_stack_validated_waves(int32_t w, int32_t n_win, int32_t n_ch, int32_t n_t, int32_t n_pass, int32_t R);

/* ---------------------------------------------------------------- dispersion (map_fv)
 * Gathers data[B][nch][nt] (strides in elements).  Only the FK bins the (f, k = f / v) queries
 * touch are formed: n_fb frequency bins (twiddles wt[nt][2 * n_fb] = cos | -sin) and n_kb
 * wavenumber bins (atab [2 * MT][K2] float64 = [[Er, -Ei], [Ei, Er]], MT = 16 * ceil(n_kb / 16),
 * K2 = 2 * nch rounded up to a multiple of 4).  Replaces fk (modules/utils.py:236-248) and map_fv (:457-475). */

/* 1 / ||row||_1 per gather row (map_fv norm=True, modules/utils.py:461-464). */
int dvh_disp_row_l1(const float* data, int64_t b_stride, int64_t ch_stride, int32_t B, int32_t nch, int32_t nt,
                    float* inv_l1, void* stream);

/* Time DFT on the float64 MFMA pipe: D[B * nch][2 * n_fb] float64 (re, im interleaved), rows
 * scaled by row_scale (nullable).  wt[nt][2 * n_fb] float64. */
int dvh_disp_tdft(const float* data, int64_t b_stride, int64_t ch_stride, int32_t B, int32_t nch, int32_t nt,
                  const double* wt, int32_t n_fb, const float* row_scale, double* D, void* stream);

/* Channel contraction (complex GEMM on MFMA) + |.|: FK[B][n_kb][n_fb]; with slot/weight
 * (both non-NULL) FK[slot[b]] += weight[b] * |Z_b| instead (class mean of |FK|), FK holding n_slot
 * slots (a slot outside [0, n_slot) is never written; callers validate slots on the host).
 * Any nch and n_kb: tables of up to 160 KB of LDS (8 * 33 * (K2 + 2 * MT) bytes, e.g. 128 channels x 127
 * wavenumbers) run one block per (gather, 32 f-bins); larger ones are tiled over 64 wavenumbers per block with
 * the channels chunked through LDS, with the same sums in the same order.  What
 * remains is the caller's dense atab (2 * MT * K2 doubles) and B <= 65535 gathers per launch.  -2 for a table
 * shape that breaks the rules above (MT % 16, n_kb > MT, K2 < 2 * nch, K2 % 4); FK is then not written. */
int dvh_disp_fk(const double* D, int32_t B, int32_t nch, int32_t n_fb, const double* atab, int32_t MT, int32_t K2,
                int32_t n_kb, double* FK, const int32_t* slot, const float* weight, int32_t n_slot, void* stream);

/* dvh_disp_fk with the kernel named: AUTO is dvh_disp_fk's rule, TILED the tiled kernel at any table size (bitwise
 * the one-block kernel's result), ONE_BLOCK the one-block kernel or -4 when the table needs more than 160 KB. */
enum { DVH_FK_FORM_AUTO = 0, DVH_FK_FORM_ONE_BLOCK = 1, DVH_FK_FORM_TILED = 2 };
int dvh_disp_fk_as(const double* D, int32_t B, int32_t nch, int32_t n_fb, const double* atab, int32_t MT, int32_t K2,
                   int32_t n_kb, double* FK, const int32_t* slot, const float* weight, int32_t n_slot, int32_t form,
                   void* stream);

/* f-v sampling: fv[B][nV][nF] = savgol(float32(bilinear(FK; k = kq[f][v], f)))  with the
 * interp2d query order (kq sorted per frequency), FITPACK clamping to [kmin, kmax], the compact
 * k grid kgrid[n_kb], per-frequency lower bin fj[nF] and weights fw[nF][2], and the
 * Savitzky-Golay operator sg = {h[sgl], left[sgl/2][sgl], right[sgl/2][sgl]}. */
int dvh_disp_fv(const double* FK, int32_t B, int32_t n_kb, int32_t n_fb, const double* kgrid, double kmin,
                double kmax, const double* kq, int32_t nF, int32_t nV, const int32_t* fj, const double* fw,
                const double* sg, int32_t sgl, float* fv, void* stream);

/* The three kernels behind dvh_disp_fv, all with the same outputs: per-image (one block per image and 4 velocities),
 * batched (G images per block share the per-(f, v) weights; nF <= 1024 and an FK grid of <= 4 096 bins) and
 * frequency-tiled (tiles of ~200 outputs, G images per block; the FK grid and the filter within 64 KB of LDS, and
 * sgl <= 25: a block samples 12 frequencies to either side of its tile, which is as far as the filter may reach).
 * dvh_disp_fv is dvh_disp_fv_as(..., DVH_FV_AUTO, 0): each kernel where it measured fastest.  A named form drops
 * the size thresholds of that choice, never a kernel's own limits: where the named kernel cannot run the chain
 * goes on, tiled -> batched -> per-image (a refused DVH_FV_TILED still drops the batched kernel's size threshold;
 * sgl = 27 named TILED runs batched).  DVH_FV_NOT_TILED leaves the tiled kernel out and chooses
 * between the other two by size.  images_per_block > 0 sets G of the named kernel (TILED, BATCHED); 0 is the
 * launcher's count. */
enum { DVH_FV_AUTO = 0, DVH_FV_PER_IMAGE = 1, DVH_FV_NOT_TILED = 2, DVH_FV_BATCHED = 3, DVH_FV_TILED = 4 };
int dvh_disp_fv_as(const double* FK, int32_t B, int32_t n_kb, int32_t n_fb, const double* kgrid, double kmin,
                   double kmax, const double* kq, int32_t nF, int32_t nV, const int32_t* fj, const double* fw,
                   const double* sg, int32_t sgl, float* fv, int32_t form, int32_t images_per_block, void* stream);

/* What dvh_disp_fv_as would launch for this shape, form and images_per_block: *form_out = DVH_FV_PER_IMAGE,
 * DVH_FV_BATCHED or DVH_FV_TILED (where the chain ended) and *G_out its images per block (0 for the per-image
 * kernel); both 0 when B <= 0 or nV <= 0 (nothing runs).  Host arithmetic only: no launch, no device.  The same
 * status as dvh_disp_fv_as for the same arguments. */
int dvh_disp_fv_pick(int32_t B, int32_t n_kb, int32_t n_fb, int32_t nF, int32_t nV, int32_t sgl, int32_t form,
                     int32_t images_per_block, int32_t* form_out, int32_t* G_out);

/* dvh_disp_fv for large batches with the FK cells staged per block: 256-thread blocks of 4 velocities x a
 * frequency tile (TO outputs, n_tile tiles, 12-sample halos; one tile when nF <= 256), block ct =
 * chunk * n_tile + tile stages only the cells its bilinear stencils read: cell_off[ct][max_cell] (FK
 * offsets m * n_fb + j, column-major per column), n_cell[ct], and per (f, v) of the block
 * qidx[ct][256][4][4] int32 = {compact index of (m, j), of (m, j + 1), m, 0}, f = tile start - halo + thread.
 * Tables: das_diff_veh_amd.disp.DispPlan.cell_tables.  VT must be 4.  Same outputs as dvh_disp_fv.  -4 for
 * sgl > 25 (the window reaches past the halo; cell_tables returns None for such a plan), for a tile wider than the
 * block, or a last tile of fewer than 13 outputs. */
int dvh_disp_fv_cells(const double* FK, int32_t B, int32_t n_kb, int32_t n_fb, const double* kgrid, double kmin,
                      double kmax, const double* kq, int32_t nF, int32_t nV, const double* fw, const double* sg,
                      int32_t sgl, int32_t TO, int32_t n_tile, int32_t VT, int32_t max_cell, const int32_t* cell_off,
                      const int32_t* n_cell, const int32_t* qidx, float* fv, void* stream);

/* dvh_disp_fv_cells with images_per_block > 0 images per block (0: the launcher's count, ~8 k blocks of at most
 * 64 images, which is what dvh_disp_fv_cells passes). */
int dvh_disp_fv_cells_as(const double* FK, int32_t B, int32_t n_kb, int32_t n_fb, const double* kgrid, double kmin,
                         double kmax, const double* kq, int32_t nF, int32_t nV, const double* fw, const double* sg,
                         int32_t sgl, int32_t TO, int32_t n_tile, int32_t VT, int32_t max_cell,
                         const int32_t* cell_off, const int32_t* n_cell, const int32_t* qidx, float* fv,
                         int32_t images_per_block, void* stream);

/* dvh_disp_fv with the Savitzky-Golay filter on the float64 matrix pipe (map_fv's savgol,
 * modules/utils.py:473): each (16 velocities x 16 frequencies) output tile is one banded GEMM of
 * 10 v_mfma_f64_16x16x4_f64 steps over the float32-rounded bilinear samples.  Plan tables
 * (DispPlan.mfma_tables): hx[nF][nV][2] float64 = the FITPACK weights {fx (khi - q), fx (q - klo)} of
 * every clamped query on its interval m, cb[nF][nV] int32 = m * n_fb + fj[f] (the (m, j) cell of the
 * compact grid), fw[nF][2] as dvh_disp_fv.  G images per block (0: chosen by the launcher).  Needs
 * sgl == 25, nF >= 32, n_kb * n_fb <= 8192.  Same outputs as dvh_disp_fv. */
int dvh_disp_fv_mfma(const double* FK, int32_t B, int32_t n_kb, int32_t n_fb, const double* hx, const int32_t* cb,
                     int32_t nF, int32_t nV, const double* fw, const double* sg, int32_t sgl, int32_t G, float* fv,
                     void* stream);

/* Phase-shift (frequency-domain slant-stack) transform, map_fv_FD_slant_stack (modules/utils.py:429-454):
 * fv[b][v][f] = float32(| sum_{r < n_row} D[b*nch + row0 + r][fb[f]] * exp(+i 2 pi freqs[f] (dx r) / vels[v]) |),
 * D as dvh_disp_tdft writes it ([B*nch][2*n_fb] float64, re/im interleaved), fb[nF] the column of D for each frequency,
 * images b_stride floats apart.  n_row == 0 writes zeros.  freqs, vels, fb are device arrays.
 * Float64 throughout (sincos, the steering powers by recurrence, the sum in ascending row order), rounded once at the
 * store; an image does not depend on the batch it is part of.  -2 for negative counts, row0 + n_row > nch, n_fb <= 0
 * or overlapping images (B > 1 and b_stride < nF * nV); fv is then not written.  The caller validates fb against
 * n_fb on the host. */
int dvh_disp_slant(const double* D, int32_t B, int32_t nch, int32_t n_fb, int32_t row0, int32_t n_row,
                   const int32_t* fb, const double* freqs, int32_t nF, const double* vels, int32_t nV, double dx,
                   float* fv, int64_t b_stride, void* stream);

/* ---------------------------------------------------------------- bootstrap / convergence
 * bootstrap_disp (apis/imaging_classes.py:8-48): per-pass gathers once, then per resample the mean
 * stack, its f-v image (dvh_disp_*) and the ridge picks (extract_ridge_ref_idx, modules/utils.py:621-678). */

/* out[b][k] = (sum_{j < m} G[sel[b * m + j] * pass_stride + k]) / m for k < K, summed in selection
 * order (sum(images) / len(images), apis/imaging_classes.py:106-107).  The sum starts at the first selected pass, as
 * sum() does: a selection of one pass returns it bit for bit, -0.0 included. */
int dvh_select_mean(const float* G, int64_t pass_stride, int64_t K, const int32_t* sel, int32_t B, int32_t m,
                    float* out, int64_t out_stride, void* stream);

/* dvh_select_mean for resamples of different sizes in one launch: resample b averages the cnt[b] >= 1 passes
 * sel[off[b] .. off[b] + cnt[b]) (device arrays; convergence_test's bt_size = 1 .. max_size draws). */
int dvh_select_mean_var(const float* G, int64_t pass_stride, int64_t K, const int32_t* sel, const int32_t* off,
                        const int32_t* cnt, int32_t B, float* out, int64_t out_stride, void* stream);

/* extract_ridge_ref_idx on the frequency band [c0, c0 + nb) of fv[b] ([nV][nF], b_stride elements
 * apart), rows = velocities vel[nV] strictly descending.  ref == INT32_MIN: vel_max mode (raw picks
 * below argmin |vel_max - vel|); vref (nullable, [nb]): per-frequency reference velocities; otherwise
 * the walk from column ref with the window (v - sigma, v + sigma); -nb <= ref < 0 indexes like Python
 * (column nb + ref, then the reference's loop order: forward to the end, then 0 .. nb - 1 again).  Picks of the last two modes are
 * smoothed by savgol(sgl, 2) given as sg = {h[sgl], left[sgl/2][sgl], right[sgl/2][sgl]}.
 * out[B][nb] float64; status[b] = 1 when a window held no velocity (the reference raises); picks
 * (nullable, [B][nb] float64) receives the raw picks before the smoothing; in vel_max mode, where nothing is
 * smoothed, the kernel writes picks[b][i] = out[b][i]. */
int dvh_ridge(const float* fv, int64_t b_stride, int32_t B, int32_t nV, int32_t nF, int32_t c0, int32_t nb,
              const double* vel, int32_t ref, double sigma, double vel_max, const double* vref, const double* sg,
              int32_t sgl, double* out, int32_t* status, double* picks, void* stream);

/* dvh_ridge on the phase-shift image of dvh_disp_slant without forming it: the walk computes the values it compares,
 * float32(| sum_{r < n_row} D[b*n_row + r][fb[c0 + i]] * exp(+i 2 pi freqs[c0 + i] (dx r) / vel[row]) |), by the
 * arithmetic of dvh_disp_slant, so that every compared value equals, bit for bit, what dvh_disp_slant stores for the
 * same D (all n_row rows of a gather: nch = n_row, row0 = 0) and velocities vel[nV], strictly descending.  D, n_fb,
 * fb[nF], freqs[nF] and dx as dvh_disp_slant takes them; the band [c0, c0 + nb), ref, sigma, vel_max, vref, sg, sgl,
 * out, status and picks as dvh_ridge takes them, with the same results and the same refusals (-2 for a null pointer,
 * a negative count, n_fb <= 0, a band outside nF or a ref outside the band; -4 for an even sgl, sgl > nb or nb > 1024),
 * and -4 for n_row > 1024.  B == 0 launches nothing.  The caller validates fb against n_fb on the host. */
int dvh_slant_ridge(const double* D, int32_t B, int32_t n_row, int32_t n_fb, const int32_t* fb, const double* freqs,
                    int32_t nF, double dx, int32_t c0, int32_t nb, const double* vel, int32_t nV, int32_t ref,
                    double sigma, double vel_max, const double* vref, const double* sg, int32_t sgl, double* out,
                    int32_t* status, double* picks, void* stream);

/* ---------------------------------------------------------------- phase-weighted stack (Schimmel & Paulssen 1997)
 * out = lin * c^power per sample, lin the linear stack of a draw and c = |sum_j (g_j + i h_j) / |g_j + i h_j|| / m the
 * coherence of the drawn passes' instantaneous phases ("Phase-weighted stack"). */
#define DVH_PWS_MAX_LEN 1024

/* H[r][t] = imag(scipy.signal.hilbert(X[r][:N]))[t] for t < N = row_len[r] (row_len null: N = W), 0 for N <= t < W:
 * n_row rows of float32, row_stride >= W floats apart in X and in H alike; row_len[n_row] a device array with
 * 0 <= row_len[r] <= W (a length outside is clamped).  The circular convolution with the transform's taps, summed in
 * float64 in ascending tap order and rounded once.  A row with a non-finite sample is NaN at every t < N.
 * -2 for a null X or H, a negative count or row_stride < W; -4 for W > DVH_PWS_MAX_LEN; n_row == 0 or W == 0 return 0
 * and write nothing. */
int dvh_hilbert_rows(const float* X, int64_t row_stride, int32_t n_row, int32_t W, const int32_t* row_len, float* H,
                     void* stream);

/* Host function: dvh_hilbert_rows by the same arithmetic over host memory; a row_len[r] outside [0, W] is -2. */
int dvh_hilbert_rows_host(const float* X, int64_t row_stride, int32_t n_row, int32_t W, const int32_t* row_len,
                          float* H);

/* The phase-weighted stack of dvh_select_mean_var's draws: G, pass_stride, K, sel, off, cnt, B, out and out_stride as
 * there, H (dvh_hilbert_rows of G's rows) laid out as G.  Float32, three sums in selection order: the linear sum by
 * dvh_select_mean's adds, and the real and imaginary parts of the phasors g / |a|, h / |a| with 1 / |a| =
 * 1 / sqrtf(g*g + h*h), 0 where that is not positive.  power 0 gives the linear stack bit for bit; 1 and 2 multiply by
 * c and c * c, any other by powf(c, power).  -2 for a null pointer, a negative count or a power that is negative,
 * non-finite or inside (0, 1); -4 for B > 65535; B == 0 or K == 0 return 0 and write nothing.  cnt is read on the
 * device only, so this entry cannot refuse cnt[b] < 1: such a resample reads no pass; cnt[b] == 0 comes out NaN
 * (-0 / 0) and a negative cnt[b] comes out 0.
 * Amplitudes: g*g + h*h is formed in float32, so the phasor is exact to its roundings for 1.1e-19 <= |g + i h| <=
 * 1.8e19.  Above, the sum of squares overflows, 1 / |a| is 0 and the sample drops out of c (not out of lin or m); below,
 * it is subnormal and the phase loses precision, and under 2.6e-23 it is 0 and the sample counts as dead.  Gathers
 * outside that range want scaling by a power of two first: lin scales with it, c does not change. */
int dvh_select_pws(const float* G, const float* H, int64_t pass_stride, int64_t K, const int32_t* sel,
                   const int32_t* off, const int32_t* cnt, int32_t B, float power, float* out, int64_t out_stride,
                   void* stream);

/* Host function: dvh_select_pws by the same arithmetic over host memory; a cnt[b] < 1 is -2 and nothing is written. */
int dvh_select_pws_host(const float* G, const float* H, int64_t pass_stride, int64_t K, const int32_t* sel,
                        const int32_t* off, const int32_t* cnt, int32_t B, float power, float* out,
                        int64_t out_stride);

/* ---------------------------------------------------------------- preprocessing
 * dtype: 0 float32, 1 float64; data modified in place. */

/* scipy.signal.sosfiltfilt(sos, x, axis=-1) per row (bandpass_data, modules/utils.py:179-189);
 * zi = sosfilt_zi(sos) [n_sec][2] (device).  Any cascade of 1 <= n_sec <= 16 sections (else -4), in both forms; a
 * section may be first-order (b2 = a2 = 0: odd-order low-pass and high-pass designs), with SciPy's padlen for it.
 * n_t > padlen (else -4, x untouched).  Time-parallel: each row is filtered in blocks
 * (zero-state block filters, a scan of the 2 n_sec block states, re-filter), forward then backward, the blocks by
 * the filter's own recursion (any stable design).  work: 16-byte aligned device buffer of
 * dvh_sosfiltfilt_workspace(n_rows, n_t, n_sec, padlen) bytes. */
int64_t dvh_sosfiltfilt_workspace(int64_t n_rows, int32_t n_t, int32_t n_sec, int32_t padlen);
int dvh_sosfiltfilt(void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t, const double* sos,
                    int32_t n_sec, int32_t padlen, const double* zi, double* work, void* stream);
/* The matrix-pipe form: the blocks as float64 MFMA GEMMs with the block operators (impulse response, zero-input
 * responses, state responses, the block and group transitions), formed once per filter design and record length n_t
 * (they depend on n_t + 2 padlen through the scan's group size): plan = device buffer of dvh_sosfiltfilt_plan_bytes(
 * n_sec) bytes.  dvh_sosfiltfilt_planned filters with them (work: 16-byte aligned, dvh_sosfiltfilt_workspace bytes;
 * plan NULL: the recursion, as dvh_sosfiltfilt).  Its rounding grows with the largest pole radius r (host sos: dvh_sos_pole_radius):
 * 1e-13 relative at r = 0.9956, 5e-10 at r = 0.99973, so plan it only for r <= DVH_SOS_MFMA_MAX_POLE.
 * bandpass_data (modules/utils.py:179-189) called once per record of the same shape designs the same filter every
 * time; the drop-in caches the plan per (design, n_t).  A plan is valid only for the (n_t, padlen) it was formed for:
 * it records its group sizes, and a call whose scans need another group transition gets NaN in the output there
 * (records short enough to need no carried groups never read the transition and filter correctly). */
#define DVH_SOS_MFMA_MAX_POLE 0.999
double dvh_sos_pole_radius(const double* sos_host, int32_t n_sec);
int64_t dvh_sosfiltfilt_plan_bytes(int32_t n_sec);
int dvh_sosfiltfilt_plan(const double* sos, int32_t n_sec, const double* zi, int32_t n_t, int32_t padlen, double* plan,
                         void* stream);
int dvh_sosfiltfilt_planned(void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t, const double* sos,
                            int32_t n_sec, int32_t padlen, const double* zi, const double* plan, double* work,
                            void* stream);

/* SurfaceWaveWindow.mute_along_traj (apis/data_classes.py:49-72): tab[n_pass][n_t][3] =
 * {start, end, taper_start} per time sample; contiguous [n_ch][n_t] per pass, passes pass_stride elements
 * apart.  One launch with a block row per (channel, pass): n_ch or n_pass above 65 535 returns -4 before
 * anything is launched and the data is left as it was. */
int dvh_mute_traj(void* data, int32_t dtype, int32_t n_pass, int64_t pass_stride, int32_t n_ch, int32_t n_t,
                  const int32_t* tab, const double* taper, void* stream);

/* TimeLapseImaging._preprocessing_for_surface_waves after the bandpass (apis/timeLapseImaging.py:
 * 51-71) on traces x[n_rows][n_t] (row_stride elements): flags 1 = impute the first empty trace
 * (||x_r|| < noise_threshold), 2 = then the first noisy trace (max x_r > noise_threshold), 4 = then
 * divide every trace by its L2 norm.  find_noise_idx / impute_noisy_trace (modules/utils.py:316-329)
 * semantics: np.argmax picks trace 0 when none qualifies; an interior trace becomes the SUM of its
 * neighbours.  stats: n_rows * 2 doubles of work ({sum x^2, max x} per trace); idx_out (nullable,
 * 2 ints) receives the imputed trace indices. */
int dvh_trace_cleanup(void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t, int32_t flags,
                      double noise_threshold, double* stats, int32_t* idx_out, void* stream);

/* SurfaceWaveSelector.locate_windows' cut (apis/data_classes.py:208-216): for every accepted pass w,
 * out[w][c][t] = rec[x_start + c][t_start[w] + t] (c < n_ch, t < n_t) into a contiguous batch,
 * converted from in_dtype to out_dtype (0 = float32, 1 = float64).  rec is [n_rows][rec_n_t] with
 * row_stride elements; t_start (device, n_win int64) is checked on the device: a window outside the
 * record sets *status (nullable) to 1 and is left unwritten. */
int dvh_cut_windows(const void* rec, int32_t in_dtype, int64_t n_rows, int64_t row_stride, int64_t rec_n_t,
                    const int64_t* t_start, int32_t n_win, int64_t x_start, int32_t n_ch, int32_t n_t, void* out,
                    int32_t out_dtype, int32_t* status, void* stream);

/* SurfaceWaveWindow.mute_along_time (apis/data_classes.py:100-104). */
int dvh_mute_time(void* data, int32_t dtype, int64_t n_rows, int32_t n_t, const double* taper, void* stream);

/* ---------------------------------------------------------------- tracking-grid preprocessing
 * TimeLapseImaging._preprocess_for_tracking (apis/timeLapseImaging.py:74-102): the median gate, then
 * dvh_trace_cleanup (flags 1, threshold 30), dvh_sosfiltfilt_planned along time, the resampler below
 * (fused with the [:, ::subsamp_factor] decimation, written transposed), dvh_sosfiltfilt_planned on the
 * transposed rows (= along space, bandpass_data_space modules/utils.py:584-594) and the transpose back. */

/* means = np.median(np.abs(x), axis=-1); x[means > noise_level] *= 0 (:76-77) on traces x[n_rows][n_t]
 * (row_stride elements), in place.  The median is the exact order statistic (even n_t: (a + b) / 2 of the two
 * middle values, in float64), any n_t >= 1; a trace holding a NaN has median NaN and is not gated; a gated
 * trace is multiplied by 0 (-0.0 for negative samples, NaN for infinite ones, as numpy).  med_out (nullable):
 * n_rows doubles; gated_out (nullable): n_rows int32, 1 where the trace was gated. */
int dvh_median_abs_gate(void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t, double noise_level,
                        double* med_out, int32_t* gated_out, void* stream);

/* scipy.signal.resample_poly(x[:, ::t_step], up, down, axis=0).T of x[n_in][..] (row_stride elements, at least
 * (n_t_out - 1) * t_step + 1 samples per row), float64 out[n_t_out][n_out] (out_stride doubles per row):
 *   out[t][m] = sum_k h[half_len + down * m - up * k] * x[k][t * t_step],  0 <= k < n_in,
 * over the k whose h index lies in [0, 2 * half_len]; h = the host-designed filter of 2 * half_len + 1 device
 * doubles (resample_poly's default: firwin(2 * half_len + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up with
 * half_len = 10 * max(up, down), up / down reduced by their gcd).  n_out must be ceil(n_in * up / down) (-2
 * otherwise, nothing launched).  Accumulates in float64. */
int dvh_resample_rows_t(const void* x, int32_t dtype, int32_t n_in, int64_t row_stride, int32_t t_step,
                        int32_t n_t_out, const double* h, int32_t half_len, int32_t up, int32_t down, double* out,
                        int64_t out_stride, int32_t n_out, void* stream);

/* dst[c][r] = src[r][c] for r < n_rows, c < n_cols (strides in doubles; src and dst must not overlap). */
int dvh_transpose_f64(const double* src, int64_t n_rows, int64_t n_cols, int64_t src_stride, double* dst,
                      int64_t dst_stride, void* stream);

/* ---------------------------------------------------------------- record ingest
 * ImagingIO.__getitem__ (modules/imaging_IO.py:37-48) after the file is read: savgol_filter(data, 21, 15) along time
 * and data /= scale, one pass. */

/* scipy.signal.savgol_filter(x, wlen, order, mode='interp', axis=-1) of rows x[n_rows][n_t] (row_stride elements)
 * into y (y_stride elements per row, x's dtype: 0 float32, 1 float64; must not overlap x), as three linear maps formed
 * on the host (das_diff_veh_amd.preprocess.savgol_interp_operator; float64 device tables), half = wlen / 2:
 *   interior    y[t] = sum_j h[j] x[t - half + j]                        half <= t < n_t - half
 *   left edge   y[t] = sum_j el[t][j] x[j]                               t < half           (el: half x wlen)
 *   right edge  y[n_t - half + t] = sum_j er[t][j] x[n_t - wlen + j]     t < half           (er: half x wlen)
 * Every sum is float64 in tap order j = 0 .. wlen - 1 and rounded once to the output dtype; a sample's value does not
 * depend on its row, stride or position in a tile.  divisor != 1: the rounded value is then divided in the output dtype
 * (float32: / (float)divisor, correctly rounded), as ImagingIO's data /= scale.  wlen odd, 3 <= wlen <= 63,
 * wlen <= n_t <= INT32_MAX - 4096 (-4 otherwise, nothing launched). */
int dvh_savgol_rows(const void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t, const double* h,
                    int32_t wlen, const double* el, const double* er, double divisor, void* y, int64_t y_stride,
                    void* stream);

/* x[r][t] /= divisor in x's dtype (float32: / (float)divisor), in place, for rows x[n_rows][n_t] (row_stride
 * elements): ImagingIO's data /= scale on a record that is not smoothed. */
int dvh_divide_rows(void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t, double divisor,
                    void* stream);

/* ---------------------------------------------------------------- vehicle tracking
 * KF_tracking (apis/tracking.py:21-168) on the float64 tracking grid: peak picking per grid row, the detection
 * curve of detect_in_one_section and the association / Kalman loop of tracking_with_veh_base.  The rejection of
 * unrealistic tracks and the NaN interpolation work on the small result on the host. */

/* Longest row dvh_find_peaks_rows takes (-4 above it, nothing launched).  Rows of up to 6 000 samples are staged
 * in LDS, longer ones are read from global memory. */
#define DVH_FIND_PEAKS_MAX_NT 16384

/* scipy.signal.find_peaks(sign * x[r], distance=distance, prominence=min_prominence, wlen=wlen)[0] for the n_sel
 * rows r = row0 + k * row_step of the row-major float64 matrix x (row_stride doubles per row, n_t >= 1 samples).
 * sign is +1 or -1 and is applied on load (negation is exact).  SciPy's order and rules:
 *   local maxima  a sample strictly above its left neighbour whose run of equal samples is followed by a strictly
 *                 lower one is one peak at (left + right) / 2 (integer division); the first and last sample are
 *                 never peaks and a run touching either end gives none; a comparison with NaN is false.
 *   distance      (<= 0: off; else ceil(distance)) peaks are visited from the highest to the lowest, a peak that is
 *                 still kept removes every peak closer than `distance` samples on both sides, a removed peak
 *                 removes nothing; equal heights are visited larger index first.
 *   prominence    (use_prominence == 0: off) of the peaks the distance rule kept: scans run outward from the peak
 *                 while x[i] <= x[peak], inside [peak - wlen / 2, peak + wlen / 2] clipped to the row with
 *                 wlen = ceil(wlen) (wlen <= 1, 0 or negative included: the whole row), tracking the minimum;
 *                 prominence = x[peak] - max(left_min, right_min); kept when prominence >= min_prominence.
 * peaks[n_sel][cap] receives the ascending sample indices and count[n_sel] their number; a row with more than cap
 * peaks gets count = cap, its first cap peaks and status = 1 (status: nullable, n_sel int32, 0 otherwise); nothing
 * is written past cap.  prominences (nullable): [n_sel][cap], the prominence of every stored peak (computed even
 * when use_prominence is 0). */
int dvh_find_peaks_rows(const double* x, int64_t row_stride, int32_t n_t, int64_t row0, int64_t row_step,
                        int32_t n_sel, int32_t sign, double distance, int32_t use_prominence, double min_prominence,
                        double wlen, int32_t* peaks, int32_t cap, int32_t* count, double* prominences,
                        int32_t* status, void* stream);

/* detect_in_one_section's curve (apis/tracking.py:30-42, likelihood_1d modules/car_tracking_utils.py:21-26):
 *   out[t] = sum_r sum_p norm.pdf(t_axis[t], loc=t_axis[peaks[r][p]], scale=sigma),  r < n_rows, p < count[r],
 * accumulated in the reference's order (a row's peaks first, then the rows); peaks / count as written by
 * dvh_find_peaks_rows with the same cap; t_axis, out: n_t device doubles.  n_rows = 0 gives zeros.  The vehicle
 * bases are then dvh_find_peaks_rows on out with the distance on and the prominence off (the reference's
 * height = max * 0. holds for every sample of a non-negative sum). */
int dvh_peak_likelihood(const int32_t* peaks, int32_t cap, const int32_t* count, int32_t n_rows,
                        const double* t_axis, int32_t n_t, double sigma, double* out, void* stream);

/* The association and Kalman loop of tracking_with_veh_base (apis/tracking.py:101-155), one thread per vehicle,
 * over the peak lists of the n_steps tracked rows (peaks[n_steps][cap], count[n_steps], every row ascending as
 * dvh_find_peaks_rows writes it: the match is found by bisection) at positions x_sel[n_steps] (device doubles).  veh_states[n_veh][n_steps] receives NaN or the matched peak index.  Per step and vehicle, as the
 * reference has it:
 *   search base  veh_base[v] while the vehicle has 0 or 1 matches; with exactly 1 the state is re-seeded every step
 *                as [that match, 0] with P = 0 and Xv = that row's position; otherwise the predicted arrival
 *                truncated toward zero, with delta_x = x_sel[k] - Xv, A = [[1, delta_x], [0, 1]] and
 *                Q = sigma_a [[delta_x^4 / 4, delta_x^3 / 2], [delta_x^3 / 2, delta_x^2]].
 *   match        the nearest peak with 0 < peak - base <= 30, else the nearest with -15 < peak - base <= 0, else NaN.
 *   update       with R = 1, C = [1, 0], only once the vehicle has more than two matches and this step matched; Xv
 *                moves only then. */
int dvh_kf_track(const int32_t* peaks, int32_t cap, const int32_t* count, int32_t n_steps, const double* x_sel,
                 const int32_t* veh_base, int32_t n_veh, double sigma_a, double* veh_states, void* stream);

/* ---------------------------------------------------------------- spectra (win_avg_psd, plot_psd_vs_offset)
 * scipy.signal.welch(x, fs, nperseg, nfft=nfft) with SciPy's defaults, for float32 rows
 * x[n_groups][rows_per_group][n_t] (group_stride, row_stride in elements; the time axis is contiguous):
 *   noverlap = nperseg / 2, step = nperseg - noverlap, nseg = (n_t - noverlap) / step (the tail is ignored);
 *   per segment: minus its own mean (float64), times win[nperseg] (float64, the caller's periodic Hann), rFFT of
 *   length nfft (zero padded), re^2 + im^2; the mean over segments times scale = 1 / (fs sum win^2), every bin but
 *   DC (and Nyquist when nfft is even) doubled.
 * out[n_groups][nfft / 2 + 1] float64 is the mean of that over the group's rows: rows_per_group = 1 gives the rows'
 * own spectra (a gather), rows_per_group = C the per-window spectrum of win_avg_psd (modules/utils.py:715-728)
 * without the rows' spectra ever being stored.  A segment holding NaN or +-inf makes its group NaN in every bin.
 *   nfft 256, 512, 1024, 2048, 4096   one wave per segment, a packed nfft / 2-point float32 transform (the window is
 *                                     rounded to float32 with the products it forms); means and every sum over
 *                                     segments, rows and waves in float64 in a fixed order (a value does not depend
 *                                     on strides, alignment or n_groups); tab may be NULL
 *   any other nfft                    direct float64 sums against tab[nfft][2] = (cos, -sin)(2 pi m / nfft); needs
 *                                     16 nfft + 8 nperseg bytes of one block's LDS (160 KiB), else -4
 * ws: dvh_welch_rows_workspace bytes (0 for at most 64 rows per group and for the direct form; NULL is then fine).
 * The caller clips nperseg to n_t as SciPy does: nperseg > n_t, nfft < nperseg and an nfft neither form takes are -4,
 * bad pointers, strides shorter than the rows and overlapping buffers -2; nothing is launched then. */
int64_t dvh_welch_rows_workspace(int64_t n_groups, int32_t rows_per_group, int32_t nfft);
int dvh_welch_rows(const float* x, int64_t n_groups, int64_t group_stride, int32_t rows_per_group, int64_t row_stride,
                   int32_t n_t, const double* win, int32_t nperseg, int32_t nfft, double scale, const double* tab,
                   double* out, void* ws, void* stream);

/* ---------------------------------------------------------------- vehicle classes
 * The notebooks' class split (imaging_diff_speed.ipynb cells 5-11, imaging_diff_weight.ipynb cells 5-11): the
 * quasi-static curve and peak of every pass, and the per-class mean and std curves.  The thresholds on the peaks and
 * speeds are host work (das_diff_veh_amd.classes). */

/* Interior outputs per block of the Savitzky-Golay stage of dvh_qs_curves, and the longest window it takes. */
#define DVH_QS_TILE 512
#define DVH_QS_MAX_WLEN 255

/* Per pass p < n_pass, all in float64:
 *   m[t]   = (sum_c x[row_off[p][c] + t]) / n_ch      c = 0 .. n_ch - 1 in order, one division (np.mean(axis=0))
 *   y      = savgol_filter(m, wlen, order) as the three maps h [wlen], el, er [wlen / 2][wlen] of dvh_savgol_rows
 *   z      = scipy.signal.detrend(y): y minus its least-squares line on [(t + 1) / n_t, 1], in closed form
 *   curve  = z - z[0],   peaks[p] = max_t |curve[t]|
 * x: float32 (dtype 0) or float64 (1) samples; row_off [n_pass][n_ch] (device) holds the element offset from x of the
 * first of the n_t samples of every row: (p n_ch + c) n_t for a contiguous batch, (ch0 + c) row_stride + t_start[p][c]
 * for rows cut from a record.  Rows may overlap and start at any element alignment.  The table is the caller's to
 * check: the kernel trusts it.  curves (nullable: peaks only): [n_pass] rows of curve_stride >= n_t doubles, nothing
 * is written between them.  A pass whose curve holds a non-finite value gets peaks[p] = NaN and status[p] |= 1
 * (status: nullable, n_pass int32 the caller has zeroed); other passes are not affected.  Every sum has a fixed order
 * that depends on (n_ch, n_t, wlen) alone, and no atomics are used: a pass's curve and peak do not depend on n_pass, on
 * its position, or on where its rows lie.  ws: dvh_qs_curves_workspace bytes.
 * -4, nothing launched: wlen even, < 3 or > DVH_QS_MAX_WLEN, n_t < wlen, n_ch < 1, n_pass < 0.  n_pass = 0 returns 0
 * without a launch. */
int64_t dvh_qs_curves_workspace(int32_t n_pass, int32_t n_t);
int dvh_qs_curves(const void* x, int32_t dtype, const int64_t* row_off, int32_t n_pass, int32_t n_ch, int32_t n_t,
                  const double* h, int32_t wlen, const double* el, const double* er, double* curves,
                  int64_t curve_stride, double* peaks, int32_t* status, void* ws, void* stream);

/* np.mean(states, axis=0) and np.std(states, axis=0) (population, two passes) over the passes of every class slot:
 * curves [n_pass] rows of curve_stride doubles, slots [n_pass] device int32 (a pass with a slot outside
 * 0 .. n_slot - 1, -1 by convention, is in no class) -> mean, std [n_slot][n_t] and count [n_slot].  The sums run in
 * pass order in float64, squares formed before they are added, as NumPy does; an empty slot gives NaN rows and
 * count 0. */
int dvh_class_curve_stats(const double* curves, int64_t curve_stride, const int32_t* slots, int32_t n_pass,
                          int32_t n_t, int32_t n_slot, double* mean, double* std, int32_t* count, void* stream);

/* ---------------------------------------------------------------- Rayleigh forward model (inversion notebooks)
 * The stage the notebooks give to disba's surf96 and evodcinv.  Neither is restated: the secular function, the scan
 * that defines a mode and the misfit are this library's own definitions, pinned to an 80-digit
 * Thomson-Haskell oracle by the tests.
 *
 * A model is n_layer rows (h, alpha, beta, rho) of float64 in km, km/s, km/s, g/cm^3, top to bottom; the last row is
 * the half-space and its h is ignored.  The secular function D(c, omega) is the determinant of the two traction
 * components at the free surface of the two solutions that decay in the half-space (real arithmetic, a sign that is
 * continuous in c, |D| <= 1: csrc/rayleigh.h). */

#define DVH_RAYLEIGH_MAX_LAYERS 32
#define DVH_RAYLEIGH_MAX_MODES 16

/* Modal phase velocities of layers[n_model][n_layer][4] at periods[n_period] (s; omega = 2 pi / period), one wave per
 * (model, period).  The scan is the definition: the points are c_k = fma(k, dc, c_min), k = 0, 1, .. while c_k is
 * below the model's half-space beta, and mode m is the (m + 1)-th change of sign of D between consecutive points.  Two
 * roots closer than dc therefore vanish as a pair, as in surf96's search; a dc below the closest pair of roots finds
 * them all.  need[n_period] (0 .. n_mode, clipped) is the number of modes wanted at a period; the scan stops once
 * they are bracketed and 0 skips the period.  Each wanted bracket is narrowed 65-fold a step until its width is at
 * most tol times its lower end, and the midpoint is stored.  A step takes the 64 points that cut the bracket into 65
 * equal parts, and the first change of sign among them closes the new bracket: of a bracket that holds three roots or
 * more, the lowest one those points separate is returned.
 *   out_c     [n_model][n_period][n_mode] float64, NaN where a mode is not wanted or has no bracket below beta; every
 *             slot is written
 *   out_count [n_model][n_period] int32, the brackets found (at most need)
 * A period <= 0 or NaN gives NaN and 0.  The layer values are the caller's to check (alpha > beta > 0, rho > 0): the
 * kernel's loops are bounded on any input (256 sublayers a layer, 65 536 scan points), but its values are then
 * meaningless.
 * -2: NULL pointers, negative counts, n_layer or n_mode < 1, c_min, dc or tol not positive and finite.
 * -4: n_layer > 32, n_mode > 16.  n_model = 0 or n_period = 0 returns 0 without a launch. */
int dvh_rayleigh_modes(const double* layers, int32_t n_model, int32_t n_layer, const double* periods,
                       int32_t n_period, const int32_t* need, double c_min, double dc, double tol, int32_t n_mode,
                       double* out_c, int32_t* out_count, void* stream);

/* The misfit of c[n_model][n_period][n_mode] (the layout above) against n_curve observed curves given as one table of
 * n_sample samples: sample_period and sample_mode index c, sample_obs and sample_sigma are the observed velocity and
 * its uncertainty, sample_curve (0 .. n_curve - 1) names the curve a sample belongs to.  Per model
 *   out = sum_i w_i sqrt(mean_j(((obs_j - c_j) / sigma_j)^2)) / sum_i w_i       j over the samples of curve i
 * in float64, every sum over the samples in table order and over the curves in order.  +inf where any sampled
 * (period, mode) is NaN or outside c, or a curve has no sample.
 * -2: NULL pointers, negative counts, n_period, n_mode, n_sample or n_curve < 1.  n_model = 0 returns 0. */
int dvh_curve_misfit(const double* c, int32_t n_model, int32_t n_period, int32_t n_mode, const int32_t* sample_period,
                     const int32_t* sample_mode, const double* sample_obs, const double* sample_sigma,
                     const int32_t* sample_curve, int32_t n_sample, const double* curve_weight, int32_t n_curve,
                     double* out, void* stream);

/* D(c_host[i], omega) of one model for i < n_c, the same code on the CPU over host memory (no device is touched);
 * each point takes its own sublayer counts.  c <= 0 gives NaN.  It pins the arithmetic where there is no GPU and is
 * no fallback: nothing computes curves with it.
 * -2: NULL pointers, n_layer < 1, n_c < 0, omega not positive and finite, a layer without h >= 0, alpha > beta > 0
 * and rho > 0.  -4: n_layer > 32.  n_c = 0 returns 0. */
int dvh_rayleigh_secular_host(const double* layers_host, int32_t n_layer, const double* c_host, int32_t n_c,
                              double omega, double* out_host);

/* Sensitivity kernels and group velocity at the roots c[n_model][n_period][n_mode] of a dvh_rayleigh_modes call on the
 * same layers and periods, one wave per (model, period, mode).  At a root of D(c, omega, layers)
 *   dc/dp = -D_p / D_c  for a layer value p,    dc/domega = -D_omega / D_c,    U = c / (1 - (omega / c) dc/domega),
 * the derivatives taken through the recurrences of the secular function itself (csrc/rayleigh_tangent.h).  The wave
 * first takes one Newton step c <- c - D / D_c from the given root and keeps it if it moves c by at most 4 tol c (tol:
 * the width the roots were refined to); everything else is evaluated at that polished root.
 *   par_mask  bits 0 .. 3 select the columns h, alpha, beta, rho of out_dcdp
 *   out_c     [n_model][n_period][n_mode] the polished root
 *   out_u     [n_model][n_period][n_mode] the group velocity (km/s)
 *   out_dcdp  [n_model][n_period][n_mode][n_layer][4] dc/dp in km/s per unit of the column; an unselected column is
 *             NaN; a row with h = 0 (skipped by the secular function) and the half-space's h give 0
 * Each output may be NULL, not all three; every slot of the others is written.  A NaN (or non-positive) root or
 * period gives NaN in all of them.  The layer values are the caller's to check, as for dvh_rayleigh_modes.
 * -2: NULL inputs, no output, negative counts, n_layer or n_mode < 1, tol not positive and finite, par_mask outside
 * 0 .. 15.  -4: n_layer > 32, n_mode > 16.  n_model = 0 or n_period = 0 returns 0 without a launch. */
int dvh_rayleigh_sens(const double* layers, int32_t n_model, int32_t n_layer, const double* periods, int32_t n_period,
                      const double* c, int32_t n_mode, int32_t par_mask, double tol, double* out_c, double* out_u,
                      double* out_dcdp, void* stream);

/* D(c_host[i], omega) and its derivative along each direction of dirs_host[n_dir], on the CPU over host memory (no
 * device is touched): out_D [n_c], out_dD [n_c][n_dir].  A direction is 0 (c), 1 (omega) or 2 + 4 l + q (column q of
 * layer l).  out_D equals dvh_rayleigh_secular_host's value; c <= 0 gives NaN.  It measures the tangent arithmetic
 * where there is no GPU and is no fallback.
 * -2: NULL pointers, n_layer or n_dir < 1, n_c < 0, omega not positive and finite, a layer without h >= 0,
 * alpha > beta > 0 and rho > 0, a direction outside 0 .. 1 + 4 n_layer.  -4: n_layer > 32.  n_c = 0 returns 0. */
int dvh_rayleigh_tangent_host(const double* layers_host, int32_t n_layer, const double* c_host, int32_t n_c,
                              double omega, const int32_t* dirs_host, int32_t n_dir, double* out_D, double* out_dD);

/* ---------------------------------------------------------------- Gauss-Newton refinement of inverted models
 * A damped Gauss-Newton (Levenberg-Marquardt) step on dvh_curve_misfit's quantity in the unit cube u of the bounds
 * (x = lo + u (hi - lo)); the definitions are this library's own ("Gauss-Newton refinement"). */

#define DVH_LM_MAX_PARAMS 96
#define DVH_LM_MAX_CURVES 64

/* The misfit, its gradient and the Gauss-Newton matrix of n_model models, one workgroup per model.
 *   c      [n_model][n_period][n_mode]              roots (dvh_rayleigh_sens's out_c)
 *   dcdp   [n_model][n_period][n_mode][n_layer][4]  its out_dcdp with all four columns
 *   chain  [n_model][4 n_layer][n_param]            float64, the derivative of the layer values (row 4 l + q: column q
 *                                                   of layer l) with respect to u
 * and the sample table, curve weights and counts as dvh_curve_misfit takes them.  With r_s = (c_s - obs_s) / sigma_s,
 * per curve i of n_i samples rho_i = sqrt(mean_s r_s^2), W = sum_i w_i and a_i = w_i / (W n_i max(rho_i, rho_floor)),
 * and j_s[k] = (sum_r dcdp[slot of s][r] chain[r][k]) / sigma_s,
 *   out_f      [n_model]                   sum_i w_i rho_i / W, dvh_curve_misfit's quantity
 *   out_g      [n_model][n_param]          sum_s a_i(s) r_s j_s, the gradient of f in u
 *   out_H      [n_model][n_param][n_param] sum_s a_i(s) j_s j_s^T, full and symmetric
 *   out_status [n_model] int32             0, or 1 for a flagged model
 * Only the sampled (period, mode) slots of c and dcdp are read; the others may hold anything.  A model is flagged when
 * a sampled root or any value of a sampled dcdp row is not finite, a sample indexes outside c or names a curve outside
 * 0 .. n_curve - 1, or a curve has no sample: its f is +inf and its g and H are zeros.  Every entry is one sum over the
 * samples in table order (r over the layer values in order inside it) and no atomics are used, so a model's outputs
 * depend neither on n_model nor on its place in the batch.
 * -2: NULL pointers, negative counts, n_period, n_mode, n_layer, n_param, n_sample or n_curve < 1, rho_floor not
 * positive and finite.  -4: n_param > 96, n_layer > 32, n_mode > 16, n_curve > 64.  n_model = 0 returns 0 without a
 * launch. */
int dvh_lm_normal(const double* c, const double* dcdp, const double* chain, int32_t n_model, int32_t n_period,
                  int32_t n_mode, int32_t n_layer, int32_t n_param, const int32_t* sample_period,
                  const int32_t* sample_mode, const double* sample_obs, const double* sample_sigma,
                  const int32_t* sample_curve, int32_t n_sample, const double* curve_weight, int32_t n_curve,
                  double rho_floor, double* out_f, double* out_g, double* out_H, int32_t* out_status, void* stream);

/* dvh_lm_normal with an observation set per model: the models of one batch are each scored against their own
 * observations.  sample_period, sample_mode, sample_curve and curve_weight are shared by the sets;
 *   set_obs    [n_set][n_sample]  the observations of every set, NaN for a sample the set lacks
 *   set_sigma  [n_set][n_sample]  their uncertainties
 *   model_set  [n_model] int32    model m is scored against set model_set[m]; several models may name one set
 * A sample is present in set k iff set_obs[k][s] is finite.  Per set, n_i counts the present samples of curve i, and a
 * curve without one is left out of both the weighted sum and W; rho_i, a_i, j_s and rho_floor are dvh_lm_normal's over
 * the present samples, and nothing else of an absent sample (its sigma, its slot of c and dcdp, its indices) is read.
 * A model is flagged (f = +inf, g and H zeros, status 1) when dvh_lm_normal would flag it on its present samples, when
 * its set has no present sample at all, when a present sample's sigma is not positive and finite, or when model_set[m]
 * is outside 0 .. n_set - 1.  Every entry is again one sum over the present samples in table order without atomics:
 * with every sample present the operations are dvh_lm_normal's, with some absent they are dvh_lm_normal's on the table
 * without them (an emptied curve and its weight removed), and a model's outputs depend on nothing but its own rows.
 * Return codes as dvh_lm_normal, and -2 also for n_set < 1 or a NULL model_set.  n_model = 0 returns 0 without a
 * launch. */
int dvh_lm_normal_sets(const double* c, const double* dcdp, const double* chain, int32_t n_model, int32_t n_period,
                       int32_t n_mode, int32_t n_layer, int32_t n_param, const int32_t* sample_period,
                       const int32_t* sample_mode, const double* set_obs, const double* set_sigma,
                       const int32_t* model_set, int32_t n_set, const int32_t* sample_curve, int32_t n_sample,
                       const double* curve_weight, int32_t n_curve, double rho_floor, double* out_f, double* out_g,
                       double* out_H, int32_t* out_status, void* stream);

/* The damped step of every model, one wave per model: over the parameters k with free_mask[k] != 0,
 *   A = H + lambda diag(d),  d_k = max(H_kk, 1e-12 max_j H_jj),   A delta = -g
 * by a float64 Cholesky factorisation of the packed lower triangle in LDS and two triangular solves; only the lower
 * triangle of H [n_model][n_param][n_param] is read.  g is [n_model][n_param], lambda [n_model], free_mask int32
 * [n_param] (shared by the models).
 *   out_delta  [n_model][n_param]  the step; exactly 0 for a parameter that is not free
 *   out_status [n_model] int32     0, or 2: a pivot that is not positive and finite (so also a model whose H_kk are all
 *                                  0, or one without a free parameter) or a step that is not finite; delta is then 0
 *                                  in every parameter, for that model only
 * -2: NULL pointers, n_model < 0, n_param < 1.  -4: n_param > 96.  n_model = 0 returns 0 without a launch. */
int dvh_lm_solve(const double* H, const double* g, const double* lambda, const int32_t* free_mask, int32_t n_model,
                 int32_t n_param, double* out_delta, int32_t* out_status, void* stream);

/* The damped step of chains of models tied by first differences, one workgroup per chain.  Rows c chain_len + k,
 * k = 0 .. chain_len - 1, of H, g and u [n_model = n_chain chain_len] are the positions of chain c; u is each row's
 * point in the unit cube.  Over the free parameters of all positions of a chain the system is block tridiagonal:
 *   A_k = H_k + lambda_c diag(d_k) + (w_{k-1} + w_k) diag(mu)   on the diagonal, d_k as in dvh_lm_solve per row,
 *   B_k = -w_k diag(mu)                                         between positions k and k + 1,
 *   r_k = -(g_k + q_k),  q_k = mu [ w_{k-1} (u_k - u_{k-1}) - w_k (u_{k+1} - u_k) ]
 * with w = link [n_chain][chain_len - 1] and mu [n_param], both >= 0 (not checked: device data); a term whose
 * neighbour does not exist is left out.  Block Cholesky in float64 along the chain, every inner product one sequential
 * sum; the factors of every position go through workspace (dvh_lm_solve_chain_workspace(n_model, n_param) bytes,
 * 8-byte aligned) for the back sweep.  lambda is [n_chain], free_mask int32 [n_param].
 *   out_delta  [n_model][n_param]  the step; exactly 0 for a parameter that is not free
 *   out_status [n_chain] int32     0, or 2: a pivot that is not positive and finite at any position, a step that is
 *                                  not finite, or a stretch of positions between cut links (w = 0) or chain ends
 *                                  without a positive H_kk (coupling alone is singular); delta is then 0 in every
 *                                  row of that chain, and of that chain only
 * With chain_len = 1, or with mu or link all 0, out_delta is dvh_lm_solve's with lambda_c at each row, bit for bit.
 * -2: NULL pointers, n_chain < 0, chain_len < 1, n_param < 1.  -4: n_param > 96.  n_chain = 0 returns 0 without a
 * launch.  dvh_lm_solve_chain_workspace returns 0 for arguments that dvh_lm_solve_chain refuses. */
int64_t dvh_lm_solve_chain_workspace(int32_t n_model, int32_t n_param);
int dvh_lm_solve_chain(const double* H, const double* g, const double* u, const double* lambda,
                       const int32_t* free_mask, const double* mu, const double* link, int32_t n_chain,
                       int32_t chain_len, int32_t n_param, void* workspace, double* out_delta, int32_t* out_status,
                       void* stream);

/* dvh_lm_solve_chain on the CPU over host memory (workspace included), as the host entries below. */
int dvh_lm_solve_chain_host(const double* H, const double* g, const double* u, const double* lambda,
                            const int32_t* free_mask, const double* mu, const double* link, int32_t n_chain,
                            int32_t chain_len, int32_t n_param, void* workspace, double* out_delta,
                            int32_t* out_status);

/* dvh_lm_normal, dvh_lm_normal_sets and dvh_lm_solve on the CPU over host memory, from the same header
 * (csrc/refine.h) and in the same order of operations; no device is touched.  They pin the arithmetic where there is no
 * GPU and are no fallback: nothing refines models with them.  Arguments, outputs and return codes as above. */
int dvh_lm_normal_sets_host(const double* c, const double* dcdp, const double* chain, int32_t n_model,
                            int32_t n_period, int32_t n_mode, int32_t n_layer, int32_t n_param,
                            const int32_t* sample_period, const int32_t* sample_mode, const double* set_obs,
                            const double* set_sigma, const int32_t* model_set, int32_t n_set,
                            const int32_t* sample_curve, int32_t n_sample, const double* curve_weight, int32_t n_curve,
                            double rho_floor, double* out_f, double* out_g, double* out_H, int32_t* out_status);
int dvh_lm_normal_host(const double* c, const double* dcdp, const double* chain, int32_t n_model, int32_t n_period,
                       int32_t n_mode, int32_t n_layer, int32_t n_param, const int32_t* sample_period,
                       const int32_t* sample_mode, const double* sample_obs, const double* sample_sigma,
                       const int32_t* sample_curve, int32_t n_sample, const double* curve_weight, int32_t n_curve,
                       double rho_floor, double* out_f, double* out_g, double* out_H, int32_t* out_status);
int dvh_lm_solve_host(const double* H, const double* g, const double* lambda, const int32_t* free_mask,
                      int32_t n_model, int32_t n_param, double* out_delta, int32_t* out_status);

#ifdef __cplusplus
}
#endif

#endif /* DVH_H */
