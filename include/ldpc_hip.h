/*
 * ldpc_hip.h -- C ABI of libldpc_hip.so, the MI355X (gfx950) SPA decoder.
 *
 * This is the drop-in boundary for the reference's hot path
 * (python_ldpc_app/spa_decoder.py).  Plain C types only: pointers, sizes,
 * int32/int64/double, and an opaque hipStream_t passed as void*.  The Python
 * host (ldpc-simulator_amd/ldpc_amd/) binds it with ctypes; INTEGRATION.md
 * shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - Every function returns 0 on success or a negative LDPC_E* code; the
 *     message of the last failure on the calling thread is ldpc_last_error().
 *   - Decoding failure is NOT an error: it is status 1 (Result.DATA_TRANSFER_NOT_OK),
 *     exactly as spa_decoder.py:253 returns it.
 *   - The caller owns every I/O buffer.  Without LDPC_F_DEVICE_PTRS the I/O
 *     pointers are host memory and the call returns after the results are
 *     copied back; with it they are device pointers on the decoder's GPU and
 *     the call is asynchronous on `stream`.
 *   - A graph is immutable after creation and may be shared read-only by
 *     several decoders/threads.  A decoder (device workspace) is used by one
 *     thread at a time, like the reference's SPA_Decoder instance (main.py:221).
 *   - Frames are independent; a batch is split into chunks of at most the
 *     decoder's capacity and each chunk runs all its iterations on the GPU.
 */
#ifndef LDPC_HIP_H
#define LDPC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_ABI_VERSION 5  /* 5: LDPC_F_TEST_ZERO + ldpc_rare_rows_read (4: profile kinds LDPC_K_NKINDS 11);
                             * ldpc_fixed_point_read was added under 5: an addition only, nothing else changed;
                             * likewise ldpc_mc_stats_enable / ldpc_mc_stats_read and ldpc_channel_set /
                             * ldpc_channel_get, and ldpc_rate_match_set / ldpc_rate_match_get: new symbols,
                             * the version stays 5 */

/* error codes */
#define LDPC_OK 0
#define LDPC_EINVAL (-22)  /* bad argument / malformed matrix                   */
#define LDPC_ENOMEM (-12)  /* host or device allocation failed                  */
#define LDPC_EDEVICE (-5)  /* HIP runtime error (message in ldpc_last_error)    */
#define LDPC_ERANGE (-34)  /* size does not fit the decoder / 32-bit indexing   */

/* decode flags */
#define LDPC_F_NLLR 0x1u        /* normalized-LLR metric, spa_decoder.py:210-228  */
#define LDPC_F_DEVICE_PTRS 0x2u /* I/O pointers are device pointers, async        */
#define LDPC_F_STATIC 0x4u      /* ldpc_mc_run: chunked schedule, no slot refill  */
#define LDPC_F_PHYS_HBM 0x8u    /* physical mode: HBM-resident state even if LDS fits */
#define LDPC_F_SPLIT 0x10u      /* parity decoder: separate CN/VN launches per iteration even
                                   where the tile-resident decoder applies (A/B, tests) */
#define LDPC_F_TEST_ZERO 0x20u  /* TEST ONLY (ldpc_generate_frames, ldpc_mc_run): frames whose global
                                   index F has F % 4 == 1 get a channel LLR of exactly 0.0 on identity
                                   column k + (131 F + 7) mod m and information column (37 F + 3) mod k,
                                   so their rows take spa_decoder.py:159-164's |t| <= 1e-10 branch (an
                                   identity column's M = (0 + E) - E is 0 on every iteration) */
#define LDPC_F_LAYERED_TILE 0x40u /* physical mode, LDPC_SCHED_LAYERED: the HBM tile kernels even if
                                     the state fits LDS (tests, A/B); LDPC_EINVAL with LDPC_SCHED_FLOODING */
#define LDPC_F_QUANT_TILE 0x80u /* fixed-point entries (ldpc_phys_decode_q, ldpc_phys_mc_run_q): the HBM tile
                                   kernels even if the state fits LDS (tests, A/B); LDPC_EINVAL on the
                                   fp32 physical-mode entries */

typedef struct ldpc_hstd ldpc_hstd;       /* standard-form parity-check matrix  */
typedef struct ldpc_graph ldpc_graph;     /* H_std uploaded to one GPU          */
typedef struct ldpc_decoder ldpc_decoder; /* device workspace for one stream    */

/* ---------------------------------------------------------------- misc */
const char *ldpc_last_error(void);
int ldpc_abi_version(void);
/* number of visible GPUs (0 when none; never fails) */
int ldpc_device_count(void);

/* --------------------------------------------------- graph provider (host)
 * Replaces EncoderDecoderData.create_standart_parity_check_matrix
 * (encoder_decoder_data.py:269-317) and gaussian_elimination (:13-183):
 * GF(2) Gauss-Jordan with the same pivot rule (first row >= cur_row with a 1,
 * columns scanned 0..n-1), back-elimination, rank-deficient row drop (:280-305)
 * and the column permutation [non-pivot cols ascending] + [pivot cols in pivot
 * order] (:307-315).  Input: H (as read from the ALIST file, utils.py:21-113)
 * in CSR, 0-based, any column order within a row; duplicate (row,col) entries
 * are rejected with LDPC_EINVAL.
 */
int ldpc_hstd_build(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                    ldpc_hstd **out);
/* Borrowed views valid until ldpc_hstd_free.  m_std = rank (rows kept). */
int ldpc_hstd_get(const ldpc_hstd *h, int32_t *m_std, int32_t *n, int64_t *nnz,
                  const int32_t **row_ptr, const int32_t **col_idx, const int32_t **perm);
void ldpc_hstd_free(ldpc_hstd *h);

/* ------------------------------------------------------------ graph (GPU)
 * Replaces SPA_Decoder.__init__ (spa_decoder.py:16-42): binds H_std (CSR,
 * ascending columns in every row -- the reference's check_to_var order) and
 * builds the column view (var_to_check, rows ascending) on the device of the
 * calling thread's current HIP device (`device` >= 0 selects one explicitly).
 * k = n - m information bits sit in columns 0..k-1 (H_std = [A | I_m]).
 */
int ldpc_graph_create(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                      int32_t device, ldpc_graph **out);
int ldpc_graph_destroy(ldpc_graph *g);
/* Name of the check-node kernel the split parity path launches for this graph
 * on large batches ("cn_row_kernel": rows of degree <= 192 kept in registers,
 * 16 B/edge; "cn_kernel": one wavefront per row, 24 B/edge) -- measurement
 * labels.  Batches of <= 128 tiles of the 2304 codes (the streaming tail,
 * small split batches) run "cn_sub_kernel" instead (16-frame sub-tiles, t in
 * registers, 16 B/edge); the LDPC_K_CN profile kind counts whichever ran. */
const char *ldpc_cn_kernel_name(const ldpc_graph *g);
/* LDS bytes per workgroup of the tile-resident decoder for this graph, or 0 if
 * it does not apply.  It needs H_std = [A | I_m] and the A column sums of the
 * workgroup's frames in LDS: 64 frames (tile_kernels.hip: k*512 B + ~13 KB <=
 * 160 KB, row degree <= 192, e.g. wimax_576_0.5), else 16 or 8 frames
 * (tile_sub.hip: the WiMAX 2304 codes).  Where it applies, ldpc_decode_f64 and
 * the static schedule of ldpc_mc_run decode a whole chunk in ONE launch; the
 * separate per-iteration launches remain available via LDPC_F_SPLIT. */
int64_t ldpc_tile_lds_bytes(const ldpc_graph *g);
/* The tile-resident decoder this graph runs -- "tile_kernel" (64 frames per
 * workgroup), "tile_sub_kernel" (16 frames: wimax_2304_0.5) or "tile8_kernel"
 * (8 frames: the r3/4 codes, or any 2304 code whose graph was created with
 * LDPC_TILE8=1) -- or "" when it does not apply; measurement label. */
const char *ldpc_tile_kernel_name(const ldpc_graph *g);
/* Physical-mode kernel for this (sparse) graph: "phys_reg_kernel" / "phys_kernel"
 * (state in LDS) or "phys_cn_tile_kernel" (state in HBM). */
const char *ldpc_phys_kernel_name(const ldpc_graph *g, uint32_t flags);
/* The same for a check-node rule and schedule (LDPC_CN_*, LDPC_SCHED_*, below):
 * the flooding names above whatever the rule (the rule is a template parameter
 * of those kernels); for the layered schedule "phys_layered_kernel" (state in
 * LDS) or "phys_layer_tile_kernel" (state in HBM: LDPC_F_LAYERED_TILE, or a
 * graph too large for LDS); "" for a combination ldpc_phys_decode_ex rejects. */
const char *ldpc_phys_kernel_name_ex(const ldpc_graph *g, uint32_t flags, int32_t cn_rule, int32_t schedule);
int ldpc_graph_info(const ldpc_graph *g, int32_t *m, int32_t *n, int64_t *nnz,
                    int32_t *max_row_deg, int32_t *max_col_deg);

/* ---------------------------------------------------------- decoder
 * Device workspace for chunks of up to `max_frames` frames (rounded up to a
 * multiple of 64): fp64 messages E[tile][edge][64 frames], posteriors and
 * channel LLRs [tile][col][64], per-frame state.  Bytes needed:
 * ldpc_decoder_bytes().
 */
int64_t ldpc_decoder_bytes(const ldpc_graph *g, int32_t max_frames);
int ldpc_decoder_create(const ldpc_graph *g, int32_t max_frames, ldpc_decoder **out);
int ldpc_decoder_destroy(ldpc_decoder *d);
int32_t ldpc_decoder_capacity(const ldpc_decoder *d);

/*
 * Batched SPA decode, fp64, results equal to spa_decoder.py:63-280 per frame.
 * Replaces SPA_Decoder.decode(data_buffer) for `batch` frames at once.
 *   llr          [batch][n]  channel LLRs in H_std column order (data_buffer._channel_data)
 *   max_iter     >= 1        settings.get_max_iterations()
 *   z_out        [batch][n]  hard output z (= data_buffer._decoded_data), uint8, or NULL
 *   conv_out     [batch]     convergence_iteration (-1 if not converged) or NULL
 *   status_out   [batch]     0 = Result.OK, 1 = Result.DATA_TRANSFER_NOT_OK, or NULL
 *   post_out     [batch][n]  final a-posteriori LLRs, or NULL
 *   nllr_out     [batch]     _d_summarize_normalized_llr (needs LDPC_F_NLLR), or NULL
 *   nllr_hist    [batch][max_iter] per-iteration normalized LLR
 *                            (_normalized_llr_by_iterations; unused tail = -1), or NULL
 *   iters_out    [batch]     iterations executed (conv+1, or max_iter), or NULL
 *   msg_out      [batch][nnz] final check->variable messages E in H_std CSR
 *                            edge order (debug/parity; host memory only), or NULL
 *   stream       hipStream_t or NULL (null stream)
 */
int ldpc_decode_f64(ldpc_decoder *d, int32_t batch, const double *llr, int32_t max_iter,
                    uint32_t flags, uint8_t *z_out, int32_t *conv_out, int32_t *status_out,
                    double *post_out, double *nllr_out, double *nllr_hist, int32_t *iters_out,
                    double *msg_out, void *stream);

/* ------------------------------------------- on-device Monte-Carlo frames
 * Synthetic frame source that replaces DataBuffer(k) + encode + Channel
 * mode 1 (data_buffer.py:16-82, channel.py:38-81, generator.py:7-9) on the GPU:
 *   u  ~ iid bits from Philox4x32-10, key (seed), counter (frame, snr_point, block, 0)
 *   c  = [u, A.u mod 2]  (H_std = [A | I_m]), or for an IRA graph
 *        H = [H_info | staircase]: c = [u, p], p_r = p_{r-1} ^ (H_info u)_r
 *   x  = BPSK, bit 0 -> -1, bit 1 -> +1          (channel.py:49)
 *   y  = x + sigma^2 * g,  g ~ N(0,1) Box-Muller  (channel.py:68-76: noise std is sigma^2)
 *   llr = 2 y / sigma^2                           (channel.py:80)
 * sigma = 1/sqrt(2*speed*10^(snr/10)) is computed by the caller (channel.py:113).
 * ldpc_generate_frames writes them to host/device arrays (testing);
 * ldpc_mc_run generates, decodes and reduces counters without leaving the GPU.
 */
int ldpc_generate_frames(ldpc_decoder *d, uint64_t seed, int32_t snr_point, double sigma,
                         int64_t frame0, int32_t count, uint32_t flags, uint8_t *u_out,
                         double *llr_out, void *stream);

/* Counter vector per SNR point, int64[LDPC_MC_NCOUNT] (main.py:130-175 semantics):
 *   [0] frames  [1] failed (Result != OK)  [2] error bits in failed frames' info part
 *   [3] sum of convergence_iteration over converged frames  [4] converged frames
 *   [5] sum over frames of the final normalized-LLR count (nllr = count/k)
 *   [6] iterations executed (for roofline byte accounting)
 * Schedule: by default the decoder's max_frames are slots that are refilled
 * with the next frame index as soon as their frame stops (syndrome zero or
 * max_iter), so throughput follows the average iteration count rather than
 * the slowest frame of a tile; LDPC_F_STATIC decodes chunks of max_frames to
 * completion instead.  Both decode the same frames: counters are identical.
 */
#define LDPC_MC_NCOUNT 7
/* The streaming schedule's supply order of one point (ABI 4): the point's
 * local frame indices 0..count-1 (global frame0 + i) sorted by descending
 * syndrome weight of the channel hard decisions (llr > 0) on H_std, ties in
 * index order -- longest job first; order_out [count] int32, host memory.
 * ldpc_mc_run streams frames in this order unless LDPC_LPT=0 (the counters
 * are order-independent sums). */
int ldpc_frame_order(ldpc_decoder *d, uint64_t seed, int32_t snr_point, double sigma, int64_t frame0,
                     int32_t count, int32_t *order_out, void *stream);
int ldpc_mc_run(ldpc_decoder *d, uint64_t seed, int32_t n_points, const double *sigmas,
                int64_t frames_per_point, int64_t frame0, int32_t max_iter, uint32_t flags,
                int64_t *counters_out, void *stream);

/* ------------------------------------------------- physical mode (§8 f4)
 * NOT the reference's arithmetic.  Standard sum-product on a SPARSE graph --
 * pass H[:, perm] (the ALIST matrix in H_std column order, same code) to
 * ldpc_graph_create -- with the sign convention made consistent with the tanh
 * rule (Lambda = -llr), fp32.  A frame's state lives in LDS (one workgroup per
 * frame) when it fits (ldpc_phys_lds_bytes <= ~159 KB), otherwise -- or with
 * LDPC_F_PHYS_HBM -- in HBM, 64 frames per tile (csrc/phys_tile.hip); both
 * paths compute bit-identical results, on any graph ldpc_graph_create accepts
 * (a column without edges keeps L = Lambda on both).  Inputs/outputs keep the
 * reference's conventions: llr as produced by channel.py, z = (bit estimate) ^ 1,
 * status 0 = OK.  The HBM path of ldpc_phys_decode synchronises before it
 * returns (it uses a temporary workspace), also with LDPC_F_DEVICE_PTRS.
 * The LDS path runs phys_reg_kernel (a thread's rows and columns in registers)
 * on the graphs whose shape it has, else the generic phys_kernel, with the same
 * operations in the same order: bit-identical.  LDPC_PHYS_REG=0 in the
 * environment (read per launch, as LDPC_PHYS_Q_REG) forces the generic kernel
 * (tests, A/B); ldpc_phys_kernel_name* follow it.
 */
int64_t ldpc_phys_lds_bytes(const ldpc_graph *g);
int ldpc_phys_decode(const ldpc_graph *g, int32_t batch, const double *llr, int32_t max_iter, uint32_t flags,
                     uint8_t *z_out, int32_t *conv_out, int32_t *status_out, int32_t *iters_out, float *post_out,
                     void *stream);
/* On-device frames decoded in physical mode on g_phys; counters as
 * ldpc_mc_run (slot [5] unused).  The frame source is d_std's graph: either
 * the code's H_std = [A|I] (same generator as ldpc_mc_run), or -- for an IRA
 * code H = [H_info | staircase] such as the DVB-S2-profile code -- g_phys
 * itself (d_std created on g_phys; parities by accumulation).  On the HBM
 * path the running frames of a chunk are compacted into its first tiles once
 * at most a quarter of the slots still run (the finished frames counted
 * first): the counters are those of the uncompacted decode. */
int ldpc_phys_mc_run(ldpc_decoder *d_std, const ldpc_graph *g_phys, uint64_t seed, int32_t n_points,
                     const double *sigmas, int64_t frames_per_point, int64_t frame0, int32_t max_iter,
                     uint32_t flags, int64_t *counters_out, void *stream);

/* Check-node rules and schedules of physical mode (ldpc_phys_decode_ex,
 * ldpc_phys_mc_run_ex).  All arithmetic is fp32, every operation rounds once:
 *   Q_e = L[c_e] - E_e over a row's edges in CSR order, s_e = (Q_e < 0);
 *   LDPC_CN_SPA  the phi-domain sum-product rule above;
 *   LDPC_CN_NMS  R_e = +-alpha * min over the other edges of |Q|   (normalized min-sum)
 *   LDPC_CN_OMS  R_e = +-max(min over the other edges of |Q| - beta, 0)   (offset min-sum)
 *                sign: negative iff the parity of the other edges' s is odd;
 *                a graph with a row of fewer than 2 edges is LDPC_EINVAL;
 *   LDPC_SCHED_FLOODING  every row from the same L and E, then L = Lambda + sum E
 *                        over a column's edges, rows ascending;
 *   LDPC_SCHED_LAYERED   layers in order (ldpc_layers_build), per row
 *                        L[c_e] = Q_e + R_e, E_e = R_e: later layers of an
 *                        iteration see the earlier ones' posteriors.
 * Both stop after the first full iteration whose b = (L < 0) has H b = 0.
 * Supported: SPA flooding (= ldpc_phys_decode, the default); NMS / OMS flooding
 * on the LDS and the HBM path (bit-identical); NMS / OMS layered with E and L
 * in LDS when they fit (ldpc_phys_lds_bytes minus 4 n bytes <= ~159 KB:
 * phys_layered_kernel), else -- or with LDPC_F_LAYERED_TILE -- on the HBM
 * tiles (phys_layer_tile_kernel, csrc/phys_tile.hip: one launch per layer and
 * iteration, then a syndrome sweep and the exit on the device; the DVB-S2
 * profile takes this path with no flag).  Both layered paths do the same
 * operations in the same order: bit-identical.  Monte-Carlo runs on the tile
 * path compact as ldpc_phys_mc_run does; ldpc_phys_decode_ex there works in
 * chunks of 1024 frames and synchronises before it returns, as the flooding
 * HBM path.
 * SPA layered is LDPC_EINVAL, and so is LDPC_F_LAYERED_TILE with
 * LDPC_SCHED_FLOODING; layered with LDPC_F_PHYS_HBM (the flooding tile
 * kernels' flag), with or without LDPC_F_LAYERED_TILE, is LDPC_ERANGE.  The
 * min-sum results equal a CPU restatement of these rules bit for bit
 * (tests/minsum_ref.py). */
#define LDPC_CN_SPA 0
#define LDPC_CN_NMS 1
#define LDPC_CN_OMS 2
#define LDPC_SCHED_FLOODING 0
#define LDPC_SCHED_LAYERED 1
/* ldpc_phys_decode with a rule and a schedule.  param: alpha in (0, 1] for
 * LDPC_CN_NMS, beta >= 0 for LDPC_CN_OMS, ignored for LDPC_CN_SPA.  With
 * LDPC_CN_SPA and LDPC_SCHED_FLOODING it is ldpc_phys_decode. */
int ldpc_phys_decode_ex(const ldpc_graph *g, int32_t batch, const double *llr, int32_t max_iter, uint32_t flags,
                        int32_t cn_rule, int32_t schedule, float param, uint8_t *z_out, int32_t *conv_out,
                        int32_t *status_out, int32_t *iters_out, float *post_out, void *stream);
/* ldpc_phys_mc_run with a rule and a schedule (same counters). */
int ldpc_phys_mc_run_ex(ldpc_decoder *d_std, const ldpc_graph *g_phys, uint64_t seed, int32_t n_points,
                        const double *sigmas, int64_t frames_per_point, int64_t frame0, int32_t max_iter,
                        uint32_t flags, int32_t cn_rule, int32_t schedule, float param, int64_t *counters_out,
                        void *stream);
/* The layers of the layered schedule, on the host (no device is touched):
 * first-fit over the rows in ascending order -- a row joins the lowest-numbered
 * layer none of whose rows shares a column with it, else it opens a new layer.
 * layer_of_row_out [m]; *n_layers_out = layers made.  Input as
 * ldpc_graph_create (same checks).  A graph builds its own table with this rule
 * on its first layered decode, not at creation. */
int ldpc_layers_build(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                      int32_t *layer_of_row_out, int32_t *n_layers_out);

/* ------------------------------- physical mode, fixed-point min-sum (q bits)
 * What a hardware decoder computes: min-sum on saturating q-bit integer
 * messages (csrc/phys_quant.hip).  All integer arithmetic is exact; two fp32
 * operations happen, at the load only, and each rounds once.
 *   qbits = q in 4..8;  llr_scale fp32, finite and > 0;
 *   Qmax = 2^(q-1) - 1 (messages),  Pmax = 2^(q+1) - 1 (posteriors; 511 at q = 8);
 *   load:  x = (-(float)llr[j]) * llr_scale  (lam[j] * llr_scale for on-device frames),
 *          Lam[j] = (int)clamp(rintf(x), -Qmax, Qmax), rintf = round half to even,
 *          the clamp in float before the conversion (non-finite input: unspecified);
 *          L = Lam, E = 0;
 *   check row, edges in CSR order:  Q_e = clamp(L[c_e] - E_e, -Qmax, Qmax),
 *          a_e = |Q_e|, s_e = (Q_e < 0); min1 = smallest a, min2 = smallest over
 *          the other edges (= min1 on a tie); mag_e = min2 at the argmin, else min1;
 *          LDPC_CN_NMS: mag_e = (alpha_q * mag_e + 8) >> 4, alpha_q in 1..16 (sixteenths);
 *          LDPC_CN_OMS: mag_e = max(mag_e - beta_q, 0), beta_q in 0..Qmax (quantizer steps);
 *          R_e = (parity(all s) ^ s_e) ? -mag_e : mag_e;
 *   LDPC_SCHED_FLOODING: every row from the same L and E, E = R, then
 *          L[j] = clamp(Lam[j] + sum E, -Pmax, Pmax) -- an int32 sum clamped once;
 *   LDPC_SCHED_LAYERED:  ldpc_layers_build's layers in order, per row
 *          L[c_e] = Q_e + R_e, E_e = R_e.  |L| <= 2 Qmax < Pmax by construction:
 *          this schedule has no posterior clamp;
 *   exit:  after each full iteration b = (L < 0) (L == 0 is bit 0); conv = the
 *          first iteration with H b = 0; iters, status, z = b ^ 1 and the
 *          Monte-Carlo counters as ldpc_phys_decode / ldpc_phys_mc_run.
 * Example (q = 6, Qmax 31, NMS alpha_q = 12): a row with L - E = [5, -3, 40, 0]
 * has Q = [5, -3, 31, 0], min1 = 0 at edge 3, min2 = 3, magnitudes
 * [0, 0, 0, (36 + 8) >> 4 = 2], parity 1: R = [0, 0, 0, -2].  With llr_scale 4,
 * llr 0.625 gives Lam -2 and llr 0.875 gives Lam -4 (both ties round to even).
 * A frame's state (int8 E, int16 L, int8 Lam) lives in LDS when it fits
 * (ldpc_phys_q_lds_bytes; n < 65535), else -- or with LDPC_F_QUANT_TILE -- in
 * HBM, 64 frames per tile (csrc/phys_qtile.hip: any n, e.g. the DVB-S2 profile
 * n = 64800; a temporary or the decoder's fp32 tile workspace holds it); both
 * give the same integers.  LDPC_F_PHYS_HBM and LDPC_F_LAYERED_TILE select the
 * fp32 tile kernels: on these entries they are LDPC_ERANGE, with or without
 * LDPC_F_QUANT_TILE.  LDPC_CN_SPA, a row of fewer than 2 edges, or a parameter
 * out of range is LDPC_EINVAL.  Every check runs before any device work.  The results equal a
 * numpy int32 restatement of these rules (tests/qminsum_ref.py).
 * LDPC_PHYS_Q_GRID=<workgroups> in the environment (read per launch) caps the
 * grid, so that one workgroup decodes many frames in sequence (tests, A/B). */
/* param_q: alpha_q for LDPC_CN_NMS, beta_q for LDPC_CN_OMS.  post_out
 * [batch][n]: the integer posterior, in units of 1 / llr_scale.  Honours
 * LDPC_F_DEVICE_PTRS. */
int ldpc_phys_decode_q(const ldpc_graph *g, int32_t batch, const double *llr, int32_t max_iter, uint32_t flags,
                       int32_t cn_rule, int32_t schedule, int32_t qbits, float llr_scale, int32_t param_q,
                       uint8_t *z_out, int32_t *conv_out, int32_t *status_out, int32_t *iters_out, int16_t *post_out,
                       void *stream);
/* ldpc_phys_mc_run_ex on the same on-device frames (read as fp32 Lambda: rows
 * for the LDS kernels, tiles for the HBM tile kernels), decoded in fixed point
 * (same counters).  The tile path polls and compacts as ldpc_phys_mc_run's
 * (LDPC_PHYS_COMPACT=0 switches the compaction off; the counters are the same). */
int ldpc_phys_mc_run_q(ldpc_decoder *d_std, const ldpc_graph *g_phys, uint64_t seed, int32_t n_points,
                       const double *sigmas, int64_t frames_per_point, int64_t frame0, int32_t max_iter,
                       uint32_t flags, int32_t cn_rule, int32_t schedule, int32_t qbits, float llr_scale,
                       int32_t param_q, int64_t *counters_out, void *stream);
/* The kernel ldpc_phys_decode_q runs: "phys_quant_reg_kernel" (flooding, on a
 * graph the register-index kernel has a shape for) or "phys_quant_kernel" (any
 * graph; the layered schedule; flooding with LDPC_PHYS_Q_REG=0 in the
 * environment); on the HBM tiles "phys_qlayer_tile_kernel" (layered) or
 * "phys_qcn_tile_kernel" (flooding); "" for a combination the decode rejects. */
const char *ldpc_phys_kernel_name_q(const ldpc_graph *g, uint32_t flags, int32_t cn_rule, int32_t schedule,
                                    int32_t qbits);
/* LDS bytes of a frame's quantized state under a schedule (-1: bad arguments). */
int64_t ldpc_phys_q_lds_bytes(const ldpc_graph *g, int32_t schedule);

/* ------------------------------------ physical mode, bit-flipping decoders
 * The hard-decision baseline (csrc/phys_bitflip.hip): parallel gradient-descent
 * bit flipping (Wadayama et al.), one family with two parameters, weight w >= 0
 * and theta.  w = 0 is plain hard-decision bit flipping; with theta = 0 that is
 * the majority rule (flip a bit when more than half of its checks fail).  The
 * reference advertises such a decoder (LDPCDecoderType.BIT_FLIPPING,
 * --decoder bitflipping) and never dispatches one.
 * All arithmetic is fp32 and every operation rounds once.  Any graph
 * ldpc_graph_create accepts: empty rows, empty columns and degree-1 rows are
 * fine.  d_j is the degree of column j.
 *   init:  Lam_j = -(float)llr_j (lam_j for on-device frames), b_j = (Lam_j < 0);
 *          -0.0 gives 0, so a punctured column (llr = +0.0) starts as bit 0;
 *   iteration it = 0 .. max_iter - 1:
 *     1. s_r = XOR of b over row r's columns;
 *     2. if any s_r is 1:  u_j = sum of s_r over column j's rows,
 *          c_j = b_j ? -Lam_j : Lam_j,
 *          Delta_j = fl(fl(w * c_j) + (float)(d_j - 2 u_j));
 *          when w == 0 the product term is ABSENT, Delta_j = (float)(d_j - 2 u_j):
 *          Lam is then used for nothing but the initial b, so a non-finite
 *          LLR cannot make the two kernels differ;
 *          every j with Delta_j < theta flips, all from the same s; s is recomputed;
 *     3. if no s_r is 1: conv = it, stop.
 *   So a frame whose channel hard decisions already form a codeword has conv 0
 *   and no flips.
 *   outputs:  z = b ^ 1; status = 0 if converged, else 1; conv = -1 if not
 *          converged; iters = conv + 1, or max_iter if not converged; synw = sum of
 *          s_r at exit (0 when converged).
 * Two kernels, identical outputs and counters.  "bitflip_kernel": one frame per
 * workgroup, Lam[n] fp32 and b[n], s[m] as bytes in LDS, any w.
 * "bitflip_sliced_kernel": w == 0 only; 64 frames per workgroup, one 64-bit
 * word per column and per row in LDS (bit f = frame f of the tile); the flip
 * rule becomes u_j >= t(d_j) with t(d) the smallest u in 0..d with
 * (float)(d - 2u) < theta by that same fp32 comparison (d + 1, "never", if there
 * is none), u_j of 64 frames counted in bit planes.  It runs when w == 0, every
 * column degree is <= 63, its 8 (n + m) bytes (plus scratch) fit LDS, the run
 * collects no Monte-Carlo statistics and LDPC_F_BF_GENERIC is not set; else the
 * per-frame kernel does.  Neither has an HBM path: a graph whose state does
 * not fit LDS (4n + n + m bytes for the per-frame kernel; the DVB-S2 profile,
 * n = 64800) is LDPC_ERANGE.
 * LDPC_EINVAL, before any device work: NULL graph, decoder or counters;
 * batch < 1; NULL llr; max_iter < 1; weight not finite or < 0; theta not
 * finite; any flag other than LDPC_F_DEVICE_PTRS and LDPC_F_BF_GENERIC
 * (ldpc_bf_mc_run takes no LDPC_F_DEVICE_PTRS).
 * The results equal a numpy fp32 restatement of these rules (tests/bitflip_ref.py). */
#define LDPC_F_BF_GENERIC 0x100u /* the per-frame kernel even where the sliced one applies (tests, A/B) */
/* llr [batch][n] fp64.  z_out [batch][n]; conv_out, status_out, iters_out,
 * synw_out [batch]; every output pointer may be NULL.  Host pointers are staged,
 * copied and synchronised; LDPC_F_DEVICE_PTRS: device pointers, launched
 * asynchronously on `stream`. */
int ldpc_bf_decode(const ldpc_graph *g, int32_t batch, const double *llr, int32_t max_iter, uint32_t flags,
                   float weight, float theta, uint8_t *z_out, int32_t *conv_out, int32_t *status_out,
                   int32_t *iters_out, int32_t *synw_out, void *stream);
/* ldpc_phys_mc_run with a bit-flipping decoder: exactly its frame source
 * (d_std on H_std or on the IRA graph itself, the same shape checks, the
 * decoder's channel and rate-matching pattern; frames as fp32 Lambda rows).
 * The seven counters keep their meaning; slot [5] is 0.  While
 * ldpc_mc_stats_enable is on, the run fills the statistics as the other
 * physical runs do (ldpc_mc_stats_read unchanged) and uses the per-frame
 * kernel for it, also where the sliced one would apply.  The decode launches
 * are timed under LDPC_K_PHYS. */
int ldpc_bf_mc_run(ldpc_decoder *d_std, const ldpc_graph *g_phys, uint64_t seed, int32_t n_points,
                   const double *sigmas, int64_t frames_per_point, int64_t frame0, int32_t max_iter,
                   uint32_t flags, float weight, float theta, int64_t *counters_out, void *stream);
/* The kernel ldpc_bf_decode runs: "bitflip_sliced_kernel", "bitflip_kernel", or
 * "" when the state does not fit LDS or an argument is invalid (the launch's
 * own decision; a Monte-Carlo run with statistics on runs "bitflip_kernel"). */
const char *ldpc_bf_kernel_name(const ldpc_graph *g, uint32_t flags, float weight);
/* Dynamic LDS bytes of that kernel's workgroup (-1: bad arguments). */
int64_t ldpc_bf_lds_bytes(const ldpc_graph *g, uint32_t flags, float weight);

/* ------------------------------------------------------------ profiling
 * HIP-event timing of the decoder's own launches, on the stream they are
 * launched on (used by bench.py for the live roofline).  While enabled, every
 * kernel launch of this decoder is bracketed by events; ldpc_profile_read
 * synchronises, returns the summed milliseconds and launch counts per kind
 * (LDPC_K_*), and resets the accumulators.
 */
#define LDPC_K_CN 0      /* cn_kernel / cn_row_kernel / cn_sub_kernel (+ cn_rare_kernel): the split path's CN */
#define LDPC_K_VN 1      /* vn_kernel: the split path's per-tile VN */
#define LDPC_K_GEN 2
#define LDPC_K_COUNT 3
#define LDPC_K_PHYS 4
#define LDPC_K_PHYS_CN 5
#define LDPC_K_PHYS_VN 6
#define LDPC_K_TILE 7 /* tile-resident decoder: all iterations of a chunk (or a streamed SNR point) */
#define LDPC_K_CN_EDGE 8  /* few-frame path: cn_edge_kernel (lanes over a row's edges) */
#define LDPC_K_VN_EDGE 9  /* few-frame path: vn_edge_kernel + syn_kernel + tail_exit_kernel */
#define LDPC_K_VN_COLS 10 /* column-parallel VN: vn_cols_kernel + tail_exit_kernel (small batches,
                             streaming tail) */
#define LDPC_K_NKINDS 11
int ldpc_profile_enable(ldpc_decoder *d, int enable);
int ldpc_profile_read(ldpc_decoder *d, double *ms_out, int64_t *launches_out);
/* Rare rows (some |t| <= 1e-10, spa_decoder.py:159-164) this decoder has taken
 * since the last call, then reset (synchronises the device): out[0] = rows
 * queued to the split path's cn_rare_kernel (one per tile/row and iteration),
 * out[1] = rare rows the tile-resident decoders took in-kernel (one per
 * workgroup, row and pass).  A test hook: which code path saw the branch. */
int ldpc_rare_rows_read(ldpc_decoder *d, int64_t *out);
/* Fixed-point exit of the static 16-frame sub-tile decoder (tile_sub_kernel:
 * wimax_2304_0.5): a frame whose pass reproduced its messages and posteriors
 * bit for bit stops there with the outputs it would have after max_iter passes
 * (status 1, conv -1, iters = max_iter); so does a frame whose posteriors
 * repeated and whose pass proved that the next one forms the same
 * variable-to-check values bit for bit, although messages moved (tile_sub.hip
 * "Fixed-point exit").  Since the last call, then reset (synchronises the
 * device): out[0] = frames stopped this way, out[1] = frame-passes they did
 * not execute.  LDPC_FIXED_POINT=0 (environment, read per launch) switches the
 * exit off, LDPC_FP_NEXT=0 the second rule alone; results are identical
 * either way. */
int ldpc_fixed_point_read(ldpc_decoder *d, int64_t *out);

/* ------------------------------------------- Monte-Carlo statistics
 * Per-frame facts of the physical-mode Monte-Carlo runs (ldpc_phys_mc_run,
 * _ex, _q), collected on the device next to the seven counters, which do not
 * change.  While enabled, every such run on d clears the statistics at its
 * start and fills them; they stay readable until the next run, a disable or
 * the decoder's destruction.  Per SNR point p (the index into sigmas) of a run
 * with max_iter = T over the frames frame0 .. frame0 + frames_per_point - 1:
 *   hist[t], t < T   frames with conv == t;  hist[T]  frames with status != 0
 *                    (sum = c[0], hist[T] = c[1], sum_{t<T} hist[t] = c[4],
 *                    sum_{t<T} t hist[t] = c[3] of the run's counters row c);
 *   undetected       {frames, info-bit errors} of the frames that converged
 *                    (status 0) to info bits other than the ones sent -- the
 *                    counters take such a frame for a success, as main.py does;
 *   failed           records {global frame index, info-bit errors} of the frames
 *                    with status != 0, at most max_failed per point, sorted by
 *                    index.  With F failures: F <= max_failed -> all of them
 *                    (their errors sum to c[2]); else max_failed distinct true
 *                    failures, unspecified which, and dropped = F - max_failed.
 *                    The index regenerates the frame: ldpc_generate_frames(seed,
 *                    p, sigma_p, index, 1).
 * ldpc_mc_stats_read: hist_len must be T + 1 of the last run; undetected_out
 * [2]; failed_out [failed_cap][2] (may be NULL with failed_cap 0; failed_cap
 * must hold the stored records); n_failed_out [2] = {stored, dropped}.  It
 * synchronises the device.  LDPC_EINVAL when statistics are not enabled, no
 * physical run has filled them, the last run was the parity-mode ldpc_mc_run
 * (it collects none), point is out of range, hist_len is wrong or failed_cap is
 * too small.  max_failed >= 0; 0 keeps no failed-frame list. */
int ldpc_mc_stats_enable(ldpc_decoder *d, int32_t enable, int32_t max_failed);
int ldpc_mc_stats_read(ldpc_decoder *d, int32_t point, int64_t *hist_out, int32_t hist_len,
                       int64_t *undetected_out, int64_t *failed_out, int32_t failed_cap, int64_t *n_failed_out);

/* --------------------------------- channel models (physical mode only)
 * The frame source above restates the reference's mode-1 channel: its noise
 * standard deviation is sigma^2 and its SNR axis has no code-rate term.  That is
 * what parity mode must reproduce.  For physical mode a decoder can carry a
 * textbook channel instead, {model, modulation, demap} (new symbols under ABI 5:
 * an addition only, the version stays 5):
 *   model       LDPC_CH_REFERENCE  the source above, bit for bit (the default);
 *                                  needs BPSK, demap is ignored;
 *               LDPC_CH_AWGN       additive white Gaussian noise, h = 1;
 *               LDPC_CH_RAYLEIGH   flat fading, an independent fade h per symbol
 *                                  (BPSK: per bit), E[h^2] = 1, known to the receiver;
 *   modulation  bits per symbol bps: 1 BPSK, 2 QPSK, 4 16-QAM, 6 64-QAM.  A code
 *               with n % bps != 0 is LDPC_EINVAL when frames are generated;
 *   demap       LDPC_DEMAP_EXACT or LDPC_DEMAP_MAXLOG.
 * sigma under LDPC_CH_AWGN / LDPC_CH_RAYLEIGH is the noise standard deviation
 * per real dimension at unit average symbol energy -- the true sigma, not
 * sigma^2: N0 = 2 sigma^2 and Es/N0 = 1 / (2 sigma^2) for every modulation;
 * Eb/N0 = Es/N0 / (rate * bps).
 * Signs as everywhere: llr_j = ln P(y | b_j = 1) - ln P(y | b_j = 0), positive
 * means bit 1; the decoders get Lambda = -(float)llr.
 * Mapping: symbol s carries the codeword bits j = s*bps .. s*bps + bps - 1 in
 * the frame's column order (H_std / IRA; a symbol may straddle the info/parity
 * boundary k).  BPSK is real: x = +1 for bit 1, -1 for bit 0, noise on that one
 * dimension.  QPSK / 16-QAM / 64-QAM are square and Gray mapped, the first
 * bps/2 bits on the I axis, the rest on Q.  Per axis with bits a0 .. a(m-1),
 * m = bps/2: binary b0 = a0, b_i = b_(i-1) xor a_i, B = sum b_i 2^(m-1-i), level
 * (2B - (2^m - 1)) d with d = 1/sqrt(2), 1/sqrt(10), 1/sqrt(42):
 *   a0a1:    00 -> -3d, 01 -> -d, 11 -> +d, 10 -> +3d;
 *   a0a1a2:  000 -> -7d, 001 -> -5d, 011 -> -3d, 010 -> -d, 110 -> +d,
 *            111 -> +3d, 101 -> +5d, 100 -> +7d.
 * Draws (the Philox streams above, so a frame index still names one frame):
 * the info bits are unchanged; the noise of symbol s is the N(0,1) pair of
 * counter {F lo, F hi, s, (p<<1)|1}, g[0] on I and g[1] on Q; for BPSK bit j
 * takes element j&1 of the pair j>>1, as the reference channel does; the fade
 * of symbol (BPSK: bit) i comes from counter {F lo, F hi, 0x80000000 | (i>>1),
 * (p<<1)|1}: u = the 52-bit uniform of words (0,1) for even i, of (2,3) for odd
 * i, h = sqrt(-log u).
 * Received value and LLR, all fp64: per axis r = h x + sigma g; the metric of
 * level i is mu_i = (r - h x_i)^2 / (2 sigma^2);
 *   exact    llr_t = LSE_{i: a_t(i)=1}(-mu_i) - LSE_{i: a_t(i)=0}(-mu_i), each
 *            log-sum-exp with its maximum taken out first (finite for every
 *            finite input);
 *   max-log  llr_t = min_{a_t=0} mu_i - min_{a_t=1} mu_i;
 *   one bit per axis (BPSK d = 1, QPSK): both are 2 h d r / sigma^2, computed
 *   as that one expression, so the two demappers give identical bits.
 * Example (16-QAM, AWGN, sigma = 0.5, I axis, bits a0a1 = 11 -> x = +d = 0.3162,
 * g = 0.2 -> r = 0.4162): mu = (r - x_i)^2 / 0.5 = {3.726, 1.073, 0.020, 0.567}
 * for the levels {-3d, -d, +d, +3d}; max-log llr_0 = 1.073 - 0.020 = 1.053 and
 * llr_1 = 0.567 - 0.020 = 0.547.
 * ldpc_channel_set validates the enums, reserved == 0 and REFERENCE => BPSK,
 * then the decoder (NULL: LDPC_EINVAL); it does no device work.  ch == NULL puts
 * the reference channel back.  The setting applies to ldpc_generate_frames,
 * ldpc_phys_mc_run, _ex and _q on that decoder, so a failed-frame record of
 * ldpc_mc_stats_read still regenerates with ldpc_generate_frames on the same
 * decoder.  With a non-reference channel set, the parity-mode ldpc_mc_run and
 * ldpc_frame_order are LDPC_EINVAL (the channel models are physical mode's), and
 * so is LDPC_F_TEST_ZERO; all of these are checked before any device work.  The
 * generated frames equal a numpy restatement over all 2^bps constellation
 * points (tests/channel_ref.py). */
#define LDPC_CH_REFERENCE 0
#define LDPC_CH_AWGN 1
#define LDPC_CH_RAYLEIGH 2
#define LDPC_DEMAP_EXACT 0
#define LDPC_DEMAP_MAXLOG 1
typedef struct {
    int32_t model, modulation, demap, reserved;
} ldpc_channel;
int ldpc_channel_set(ldpc_decoder *d, const ldpc_channel *ch);
int ldpc_channel_get(const ldpc_decoder *d, ldpc_channel *out);

/* ------------------------------------ rate matching (physical mode only)
 * A decoder can carry a rate-matching pattern {punctured columns, shortened
 * columns} for the frames of ldpc_generate_frames, ldpc_phys_mc_run, _ex and
 * _q (new symbols under ABI 5: an addition only, the version stays 5).  It is
 * set as the channel is and is independent of it, but it belongs to the channel
 * models: under the reference channel a pattern is LDPC_EINVAL when frames are
 * generated.  No decoder kernel knows of it; it only changes the frames.
 * Columns are indices in the frame's column order -- H_std order, or the IRA
 * graph's: info 0 .. k-1, parity k .. n-1, the order ldpc_generate_frames
 * writes.  A column is transmitted, punctured or shortened:
 *   punctured   not sent, the receiver knows nothing; any column may be;
 *   shortened   an information bit both ends know to be 0, not sent; only
 *               columns j < k may be.
 * Bits: the info words are drawn as without a pattern, then the shortened
 * positions are cleared, before any parity is formed (for an IRA graph before
 * the accumulator).  So the codeword is a codeword with zeros there, u_out
 * shows the zeros, and the Monte-Carlo counters compare against them.
 * Mapping: the transmitted columns in ascending order form the sequence
 * t = 0 .. E-1, E = n - n_punct - n_short.  Everything the channel-model
 * contract says of "codeword bit j" holds for transmitted position t: symbol s
 * carries the transmitted bits s*bps .. s*bps + bps - 1 (as columns they may be
 * far apart), takes the noise pair of counter word s and the fade of index s;
 * BPSK bit t takes element t&1 of noise pair t>>1 and the fade of index t.  An
 * empty pattern therefore gives the frames of no pattern, bit for bit.
 * E % bps != 0 is LDPC_EINVAL when frames are generated; while a pattern is set
 * this replaces the n % bps check.
 * LLRs: a transmitted column's as under the channel model; a punctured column
 * llr = +0.0 exactly; a shortened column llr = -LDPC_RM_KNOWN_LLR (bit 0 is
 * known; positive means bit 1).  The decoders get Lambda = -(float)llr by the
 * same expression as for every other column; the fixed-point decoders'
 * quantizer saturates it to +Qmax.  Every output form (fp64 ch tiles, fp32
 * Lam / L tiles, fp32 rows) writes every column on every launch: the buffers
 * are reused from chunk to chunk and from pattern to pattern.
 * Axis: sigma keeps its meaning (Es/N0 = 1 / (2 sigma^2)); Eb/N0 uses the
 * effective rate (k - n_short) / E, which the caller applies (ldpc_amd.ratematch).
 * Counters and statistics keep their meaning: info-bit errors are counted over
 * all k columns, the shortened ones against 0; a failed-frame record
 * regenerates with ldpc_generate_frames on the same decoder (same channel,
 * same pattern).
 * ldpc_rate_match_set validates, copies the indices into the decoder's host
 * memory and does no device work: the device tables are uploaded by the first
 * run that needs them, on that run's stream, and freed with the decoder.
 * n_punct == n_short == 0 (the pointers may be NULL) clears the pattern.  It is
 * LDPC_EINVAL, and the earlier pattern stays in force, for: a NULL decoder; a
 * negative count; a NULL pointer with a positive count; an index outside
 * [0, n); a duplicate within or across the two lists; a shortened index >= k;
 * E < 1; k - n_short < 1.  LDPC_EINVAL when frames are to be generated, before
 * any device work: a pattern under the reference channel, with
 * LDPC_F_TEST_ZERO, in the parity-mode ldpc_mc_run and in ldpc_frame_order.
 * ldpc_rate_match_get writes the counts and, where a list pointer is not NULL,
 * that list in ascending order (its capacity must hold it). */
#define LDPC_RM_KNOWN_LLR 1.0e4
int ldpc_rate_match_set(ldpc_decoder *d, int32_t n_punct, const int32_t *punct_cols,
                        int32_t n_short, const int32_t *short_cols);
int ldpc_rate_match_get(const ldpc_decoder *d, int32_t *n_punct, int32_t *n_short,
                        int32_t *punct_out, int32_t punct_cap, int32_t *short_out, int32_t short_cap);

/* -------------------- bit interleaver and block fading (physical mode only)
 * Two more properties of the frame source, set as the channel and the pattern
 * are and independent of them (new symbols under ABI 5: an addition only, the
 * version stays 5).  No decoder kernel knows of either; they only change the
 * frames of ldpc_generate_frames, ldpc_phys_mc_run, _ex, _q and ldpc_bf_mc_run.
 * Interleaver: let tx[0 .. E-1] be the transmitted columns in ascending order;
 * with no rate-matching pattern this is every column and E = n.  perm is a
 * permutation pi of 0 .. E-1, read-from: transmitted position t carries column
 * col(t) = tx[pi[t]].  Everything the channel-model and rate-matching contracts
 * say of "transmitted position t" holds with col(t) in place of tx[t]: symbol s
 * carries the positions s*bps .. s*bps + bps - 1, takes the noise pair of
 * counter word s and the fade of index s; BPSK position t takes element t&1 of
 * noise pair t>>1; the LLR of position t is written to column col(t) -- writing
 * it there is the de-interleaving, so the decoders see the frame in column
 * order as always.  The columns not sent, the info bits, the parities, the
 * shortening, the counters, the statistics and the regeneration of a
 * failed-frame record are unchanged.  The identity gives the frames of no
 * interleaver.  The permutation is fixed until it is set again (one pattern for
 * a run, as in a real link).
 * Example: n = 6, no pattern, pi = {0, 3, 1, 4, 2, 5} (a block interleaver of 2
 * rows, written by rows and read by columns), QPSK: symbol 0 carries the
 * columns 0 and 3, symbol 1 carries 1 and 4, symbol 2 carries 2 and 5.
 * Block fading (LDPC_CH_RAYLEIGH): with block_len = L the fade of symbol s
 * (BPSK: of transmitted position t) is the fade of index B = floor(s / L)
 * (floor(t / L)) under the channel model's draw: counter {F lo, F hi,
 * 0x80000000 | (B>>1), (p<<1)|1}, u = the 52-bit uniform of words (0,1) for
 * even B, of (2,3) for odd B, h = sqrt(-log u).  L = 1 (the default) is the
 * channel-model section's channel, bit for bit; L >= the number of symbols is
 * one fade per frame (quasi-static); the last block may be ragged.  The noise
 * draws do not change.
 * Both setters do no device work; the composite table col[] is uploaded by the
 * first run that needs it, into the block the rate-matching tables use.
 * ldpc_interleaver_set copies perm; len == 0 (perm may be NULL) clears it.
 * LDPC_EINVAL, and the earlier setting stays in force, for: a NULL decoder;
 * len < 0; NULL perm with len > 0; an entry outside [0, len); a duplicate
 * entry; block_len < 1; for ldpc_interleaver_get a capacity too small for the
 * stored permutation (perm_out == NULL only asks for the length).
 * LDPC_EINVAL when frames are to be generated, before any device work, with a
 * message that names the setting and how to clear it: an interleaver under the
 * reference channel; len != E of the pattern set at that time; block_len > 1
 * with a model other than LDPC_CH_RAYLEIGH.  The parity-mode ldpc_mc_run and
 * ldpc_frame_order are LDPC_EINVAL while either setting is active. */
int ldpc_interleaver_set(ldpc_decoder *d, int32_t len, const int32_t *perm);
int ldpc_interleaver_get(const ldpc_decoder *d, int32_t *len, int32_t *perm_out, int32_t cap);
int ldpc_fading_set(ldpc_decoder *d, int32_t block_len);
int ldpc_fading_get(const ldpc_decoder *d, int32_t *block_len);

/* ------------------------------------------------ HARQ (physical mode only)
 * Retransmissions with Chase or incremental-redundancy combining in the frame
 * source (new symbols under ABI 5: an addition only, the version stays 5).  A
 * plan is R = n_tx transmissions, 1 <= R <= LDPC_HARQ_MAX_TX.  Transmission r
 * sends E_r = tx_len[r] positions; position t of transmission r carries column
 * cols_r[t]; cols is the lists one after another (sum of tx_len entries).  A
 * column may appear in any number of transmissions, at most once within one.
 * The order within a list is the order on the air, so a plan carries its own
 * puncturing and interleaving.  The plan applies to ldpc_generate_frames,
 * ldpc_phys_mc_run, _ex, _q and ldpc_bf_mc_run on that decoder; no decoder
 * kernel knows of it.
 * Bits: unchanged.  The info words come from seed; shortened positions (the
 * rate-matching pattern's, which may still be set) are cleared before the
 * parities; u_out, the counters and the statistics keep their meaning.
 * One transmission: transmission r is exactly the interleaver contract's frame
 * with col(t) = cols_r[t] and E = E_r, and with the Philox key
 *   seed_r = (seed + r * 0x9E3779B97F4A7C15) mod 2^64
 * for the noise and fade draws (transmission 0 uses the draws of a frame sent
 * once).  Symbol s carries the positions s*bps .. s*bps + bps - 1 and takes the
 * noise pair of counter word s; under LDPC_CH_RAYLEIGH the fade of symbol s
 * (BPSK: of position t) is that of index s (t), or of index floor(s / block_len)
 * under ldpc_fading_set: every transmission fades independently.  sigma is the
 * same for every transmission.  This gives llr_r[j] in fp64 for the columns of
 * transmission r.
 * Combining: for every column j, llr[j] starts at +0.0; for r ascending, if
 * transmission r carries j, llr[j] = llr[j] + llr_r[j], one fp64 addition each.
 * A column in no transmission and not shortened is punctured: +0.0 exactly.  A
 * shortened column is -LDPC_RM_KNOWN_LLR.  ldpc_generate_frames returns this
 * llr; every decoder gets Lambda = -(float)llr, so the frames the decoders see
 * are the frames ldpc_generate_frames returns.  Every output form writes every
 * column on every launch.  A one-transmission plan whose list is tx[pi[t]]
 * gives the frames of that pattern and interleaver: the LLRs are equal as
 * numbers (an LLR of -0.0 becomes +0.0).
 * ldpc_harq_set copies the lists and does no device work; n_tx == 0 (the
 * pointers may be NULL) clears the plan.  The device tables are uploaded, and
 * the fp64 accumulator of a chunk ([frames][n], freed with the decoder;
 * LDPC_ENOMEM if it cannot be had) is allocated, by the first run that needs
 * them.  LDPC_EINVAL, and the earlier plan stays in force, for: a NULL decoder;
 * n_tx < 0 or n_tx > LDPC_HARQ_MAX_TX; a NULL pointer with n_tx > 0;
 * tx_len[r] < 1; a column outside [0, n); a duplicate within one transmission.
 * LDPC_EINVAL when frames are to be generated, before any device work, with a
 * message that names the setting: a plan under the reference channel; a plan
 * with LDPC_F_TEST_ZERO; a plan together with an interleaver; a plan together
 * with a pattern that has punctured columns (the plan says what is sent); a
 * plan column that the pattern shortens; E_r % bps != 0 for any r (this
 * replaces the n % bps and E % bps checks).  The parity-mode ldpc_mc_run and
 * ldpc_frame_order are LDPC_EINVAL while a plan is set.
 * ldpc_harq_get: *n_tx and tx_len_out[0 .. LDPC_HARQ_MAX_TX) (zeros past n_tx;
 * tx_len_out may be NULL); cols_out == NULL only asks for those, else cols_cap
 * must hold the sum of the lengths (LDPC_EINVAL if too small).  A failed-frame
 * record of ldpc_mc_stats_read still regenerates with ldpc_generate_frames on
 * the same decoder. */
#define LDPC_HARQ_MAX_TX 8
int ldpc_harq_set(ldpc_decoder *d, int32_t n_tx, const int32_t *tx_len, const int32_t *cols);
int ldpc_harq_get(const ldpc_decoder *d, int32_t *n_tx, int32_t *tx_len_out, int32_t *cols_out, int32_t cols_cap);

/* --------------------------------------- constellations (physical mode only)
 * The channel models' modulations are square Gray QAM, demapped one axis at a
 * time.  A decoder can instead carry a table of 2^bps complex points, 1 <= bps
 * <= LDPC_CONST_MAX_BPS: PSK, APSK, cross or rotated QAM, any labelling (new
 * symbols under ABI 5: an addition only, the version stays 5).  It is set as
 * the channel, the pattern, the interleaver and the plan are and is independent
 * of them.  points holds 2^bps pairs (re, im), indexed by label.  No decoder
 * kernel knows of it; it only changes the frames of ldpc_generate_frames,
 * ldpc_phys_mc_run, _ex, _q and ldpc_bf_mc_run.
 * While a table is set and the channel model is LDPC_CH_AWGN or
 * LDPC_CH_RAYLEIGH, the table replaces the channel's modulation: the bits per
 * symbol and the mapping.  ldpc_channel_set / ldpc_channel_get are untouched
 * and keep reporting what was set.  Everything the channel-model, rate-matching,
 * interleaver, block-fading and HARQ contracts say of "symbol s" and
 * "transmitted position t" holds with the table's bps: symbol s carries the
 * positions s*bps .. s*bps + bps - 1.  This also holds for bps = 1: a one-bit
 * table is a complex symbol with a noise pair of its own, it does not follow
 * the built-in BPSK's two-bits-per-pair rule.
 * Label: a = sum_t bit(s*bps + t) << (bps - 1 - t), the first bit the most
 * significant; the point sent is x = points[a].
 * Draws: the noise of symbol s is the N(0,1) pair of counter word s, g[0] on I
 * and g[1] on Q; under LDPC_CH_RAYLEIGH there is one real fade h per symbol, of
 * index s, or floor(s / block_len) under ldpc_fading_set, drawn exactly as for a
 * QAM symbol.  The info bits and the parities are unchanged.
 * Received value and LLRs, all fp64: r = h x + sigma (g0 + i g1); over all 2^bps
 * points mu_i = ((r_I - h x_i,I)^2 + (r_Q - h x_i,Q)^2) / (2 sigma^2);
 *   exact    llr_t = LSE_{a_t(i)=1}(-mu_i) - LSE_{a_t(i)=0}(-mu_i), each
 *            log-sum-exp with its own maximum taken out first (finite for every
 *            finite input);
 *   max-log  llr_t = min_{a_t=0} mu_i - min_{a_t=1} mu_i.
 * There is no one-bit-per-axis special case: a table that spells out QPSK goes
 * through the same expressions, and gives the built-in QPSK's frames to within
 * rounding, not bit for bit.  sigma keeps its meaning, Es/N0 = 1 / (2 sigma^2);
 * for that to hold the table must have unit mean energy.
 * The library ships no standard's table.  The built-in names of the Python
 * layer (ldpc_amd.Constellation.psk8, .apsk16) are this project's own
 * labellings, written out in its documentation; they claim no conformity with
 * any standard, whose table a user loads from a file.
 * ldpc_constellation_set validates, copies the table into the decoder's host
 * memory and does no device work; bps == 0 (points may be NULL) clears the
 * table.  The kernels of the first run that needs it get it as an argument; no
 * device memory is held for it.  It is LDPC_EINVAL, and the earlier table stays
 * in force, for: a NULL decoder; bps < 0 or bps > LDPC_CONST_MAX_BPS; NULL
 * points with bps > 0; a coordinate that is not finite; |mean |x|^2 - 1| > 1e-9;
 * two points equal in both coordinates.
 * LDPC_EINVAL when frames are to be generated, before any device work, with a
 * message that names the setting and how to clear it: a table under the
 * reference channel; a table with LDPC_F_TEST_ZERO; n, E or any E_r not
 * divisible by the table's bps (this replaces the check against the channel's
 * modulation).  The parity-mode ldpc_mc_run and ldpc_frame_order are
 * LDPC_EINVAL while a table is set.
 * ldpc_constellation_get writes *bps (0: no table); points_out == NULL only
 * asks for that, else cap, counted in doubles, must hold 2 * 2^bps values
 * (LDPC_EINVAL if too small).  A failed-frame record of ldpc_mc_stats_read
 * still regenerates with ldpc_generate_frames on the same decoder.  The
 * generated frames equal a numpy restatement (tests/constellation_ref.py). */
#define LDPC_CONST_MAX_BPS 6
int ldpc_constellation_set(ldpc_decoder *d, int32_t bps, const double *points);
int ldpc_constellation_get(const ldpc_decoder *d, int32_t *bps, double *points_out, int32_t cap);

/* ------------------------------------------------ multi-GPU (RCCL, xGMI)
 * One process per GPU; frames are sharded by global index, so the only
 * exchange is ONE all-reduce of the int64 counter matrix per Monte-Carlo step
 * -- the reference's additive parent reduction of its workers' per-block
 * results (main.py:149-175).  librccl.so.1 (ROCm) is loaded on first use with
 * dlopen, so single-GPU users never load it.  No PyTorch.
 *   1. rank 0: ldpc_comm_unique_id(id); hand the 128 bytes to every rank
 *      (bench.py / ldpc_amd.comm: a file rendezvous on one node);
 *   2. every rank: ldpc_comm_init(id, rank, world, device, &c);
 *   3. ldpc_comm_allreduce(c, buf, count, dtype, op, flags, stream): in place;
 *      host buffers unless LDPC_F_DEVICE_PTRS (then async on `stream`);
 *      host buffers: synchronous.  dtype LDPC_DT_*, op LDPC_OP_*;
 *   4. ldpc_comm_barrier(c): all ranks arrive, then the device is synchronised;
 *   5. ldpc_comm_destroy(c).
 */
#define LDPC_COMM_ID_BYTES 128
#define LDPC_DT_I64 0
#define LDPC_DT_F64 1
#define LDPC_OP_SUM 0
#define LDPC_OP_MAX 1
typedef struct ldpc_comm ldpc_comm;
int ldpc_comm_unique_id(uint8_t *id_out);
int ldpc_comm_init(const uint8_t *id, int32_t rank, int32_t world, int32_t device, ldpc_comm **out);
int ldpc_comm_allreduce(ldpc_comm *c, void *buf, int64_t count, int32_t dtype, int32_t op, uint32_t flags,
                        void *stream);
int ldpc_comm_barrier(ldpc_comm *c);
int ldpc_comm_destroy(ldpc_comm *c);
/* hipDeviceSynchronize on `device` (bench.py's barrier brackets; no PyTorch) */
int ldpc_device_synchronize(int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_HIP_H */
