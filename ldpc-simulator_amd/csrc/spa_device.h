// spa_device.h -- device-side layout and kernel entry points of libldpc_hip.so.
//
// Data layout in HBM ("frame tiles"): 64 frames form one tile, one frame per
// lane of a wavefront.  Every per-edge / per-column array is stored
// [tile][item][64 lanes], so a wavefront touching item i of its tile reads
// 64 consecutive doubles (512 contiguous bytes): fully coalesced, with no
// index math per lane.
//   E   [tile][nnz][64]  fp64 check->variable messages (CSR edge order of H_std);
//                        for tile8.hip's graphs [tile][8][nnz][8] (e_base below)
//   T   [slot][max_row_deg][64] fp64 scratch of cn_rare_kernel (slot = its
//                        global wavefront id; nslots = 4 x its grid)
//   L   [tile][n][64]    fp64 a-posteriori LLRs
//   ch  [tile][n][64]    fp64 channel LLRs
//   ub  [tile][kw][64]   info bits (Monte-Carlo path), kw = ceil(k/32)
// Per frame: done / conv / status / iters / nllr count (+ fresh / refill of the
// streaming Monte-Carlo schedule); per tile: active flag.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ldpc {

constexpr int kTile = 64;  // frames per tile == wavefront width on CDNA

// wavefronts per sub-tile workgroup (tile_sub.hip); the host builds the
// P3 order table (DevGraph::p3dep) for this chunking
constexpr int kSubWaves = 16;
// message-array slack (edges x 64 lanes) past the last tile: the sub-tile
// decoder's unclamped slot loads overshoot a row by < Q*K = 64 edges
constexpr int kEPadEdges = 128;

struct DevGraph {
    int m, n, k, nnz;
    int max_row_deg, max_col_deg;
    int std_form;            // 1 if H_std = [A | I_m] exactly (encoder usable)
    int ira;                 // 1 if H = [H_info | staircase] (IRA encoder usable)
    const int *row_ptr;      // [m+1]
    const int *col_idx;      // [nnz]
    const int *csc_ptr;      // [n+1]
    const int *csc_edge;     // [nnz] CSR edge id, rows ascending within a column
    const int *csc_row;      // [nnz] row of that edge
    const uint32_t *a_packed;  // [m][kw] bit j of row r = A[r][j] (encoder; std_form only)
    const int *p3dep;          // [m][16] sub-tile S order: lo | hi << 8 (tile_sub.hip sub_p3)
    const int *p3dep8;         // [m][16] the same over each row's A edges (tile8.hip: identity excluded)
    int ef;                    // frames per E block (64, or 8 for tile8.hip's graphs): e_base
    int t8pair;                // tile8.hip runs its pair form (two rows per wavefront) on this graph
    int lpt_weak_id;           // frame_order.hip: rank equal syndromes by the weakest identity bit of an
                               // odd-degree row (set when at most half the rows have odd degree)
    int zinj;                  // test-only erasure injection of the frame source (LDPC_F_TEST_ZERO): 0 = off,
                               // else frame_source.h test_zero_llr (set per call, never on the graph itself)
};

// E layout inside a tile: the 64 frames in blocks of g.ef, each block
// [nnz][ef], so a workgroup that decodes ef frames reads whole cache lines
// (ef = 64: [tile][nnz][64]; ef = 8: [tile][8][nnz][8], the 8-frame sub-tile
// decoder of tile8.hip).  Element (tile, e, lane) = E[e_base(tile, lane) + e * ef].
__host__ __device__ inline size_t e_base(const DevGraph &g, int tile, int lane) {
    return (size_t)tile * g.nnz * kTile + (size_t)(lane / g.ef) * g.nnz * g.ef + (size_t)(lane % g.ef);
}

struct DevState {
    double *E, *T, *L, *ch;
    int *done, *conv, *status, *iters, *nllr_cnt;
    int *tile_active;
    int *fresh, *refill;     // streaming Monte-Carlo: lane holds a new frame / lane wants one
    const int *order;        // streaming Monte-Carlo: local frame index of supply position i (frame_order.hip:
                             // heaviest syndrome first), or null: frame index order
    int *rare_list;          // [ntiles*m] tile*m+row of rows left to cn_rare_kernel
    int *rare_count;         // [2] per iteration parity, then two running totals (ldpc_rare_rows_read):
                             // [2] rows cn_rare_kernel took, [3] rare rows the tile decoders took in-kernel
    unsigned long long *fp_count;  // [2] running totals of tile_sub_kernel's fixed-point exit (ldpc_fixed_point_read):
                             // frames stopped at a bitwise fixed point, frame-passes they did not execute
    int *active_count;       // [max_iter] or null: vn_kernel adds the tiles still running after it
    int nslots;
    uint32_t *ubits;         // MC only (may be null)
    double *nllr_hist;       // [frame][hist_stride] or null
    int hist_stride;
    int ntiles;              // tiles in this chunk
    int count;               // valid frames in this chunk
};

// Physical mode with HBM-resident state (phys_tile.hip), same tile layout.
struct PhysTile {
    float *E;          // [tile][nnz][64] check->variable messages
    float *L;          // [tile][n][64] posteriors (Lambda convention: L < 0 -> bit 1)
    float *Lam;        // [tile][n][64] Lambda = -channel LLR
    int *bad;          // [2][cap] row-syndrome flags, by iteration parity
    uint32_t *pbits;   // [tile][m/32][64] IRA: in-word prefix XOR of s = H_info u (generator scratch)
    uint32_t *wpar;    // [tile][m/1024][64] IRA: bit w = parity of s words before w
    int cap;           // frames of capacity (stride of bad)
    uint8_t *zb;       // [tile][ceil(n/8)][64] hard-decision bits of the last VN sweep (bit j&7 of byte j>>3: L < 0)
};

// --- launchers (spa_kernels.hip); all asynchronous on `s` ---
hipError_t launch_reset(const DevGraph &g, const DevState &st, hipStream_t s);
hipError_t launch_load_llr(const DevGraph &g, const DevState &st, const double *llr, hipStream_t s);
// stream = the streaming Monte-Carlo schedule (lanes at different iterations,
// see refill_kernel); stream_ctr != null selects the streaming VN.
hipError_t launch_cn(const DevGraph &g, const DevState &st, int it, hipStream_t s, bool stream = false);
bool use_cn_row(const DevGraph &g);  // launch_cn runs cn_row_kernel (else cn_kernel)
hipError_t launch_cn_rare(const DevGraph &g, const DevState &st, int it, hipStream_t s, bool stream = false);
hipError_t launch_vn(const DevGraph &g, const DevState &st, int it, int max_iter, bool nllr, hipStream_t s,
                     unsigned long long *stream_ctr = nullptr);
// tile-resident decoder (tile_kernels.hip): all iterations of a tile in one
// workgroup, check- and variable-node updates fused; [A | I_m] graphs whose A
// column sums fit in LDS (tile_lds_bytes > 0).  Needs st.ntiles <= st.nslots.
// Codes whose column sums of 64 frames do not fit (the WiMAX 2304 codes) run
// the sub-tile decoder (tile_sub.hip: 16 or 8 frames per workgroup).
size_t tile_lds_bytes(const DevGraph &g);
const char *tile_kernel_name(const DevGraph &g);  // "tile_kernel", "tile_sub_kernel" or ""
bool use_tile(const DevGraph &g);
hipError_t launch_tile(const DevGraph &g, const DevState &st, int max_iter, bool nllr, hipStream_t s);
// Streaming Monte-Carlo through the tile-resident decoder (one launch per SNR
// point; LDPC_TILE_STREAM=0 keeps the split CN/VN/refill loop).
bool use_tile_stream(const DevGraph &g);
// handoff > 0 (the 16- and 8-frame sub-tile decoders): the kernel stops once
// the supply is out and at most `handoff` frames still run, leaving them as
// split-path slot state (done / iters / fresh; E, L, ch, ubits in place)
hipError_t launch_tile_stream(const DevGraph &g, const DevState &st, int max_iter, bool nllr, uint64_t seed,
                              int snr_point, double sigma, int64_t frame0, int64_t total, unsigned long long *next,
                              unsigned long long *ctr, int64_t handoff, hipStream_t s);
// 8-frame sub-tile decoder (tile8.hip): the WiMAX 2304 codes; its graphs keep
// E in 8-frame blocks (DevGraph::ef = 8, chosen at graph creation)
bool tile8_applies(const DevGraph &g);
// whether tile8.hip's pair form can run this graph (set DevGraph::t8pair from it at graph creation)
bool tile8_pair_fits(const DevGraph &g);
size_t tile8_lds_bytes(const DevGraph &g);
// rare-row scratch rows per tile it needs: 2, or 4 for its pair form (two alternating
// rare-row buffers per row slot)
int tile8_scratch_per_tile(const DevGraph &g);
hipError_t launch_tile8(const DevGraph &g, const DevState &st, int max_iter, bool nllr, hipStream_t s);
// its streaming Monte-Carlo form (one persistent launch per SNR point, handoff as launch_tile_stream)
size_t tile8_stream_lds_bytes(const DevGraph &g);
hipError_t launch_tile8_stream(const DevGraph &g, const DevState &st, int max_iter, bool nllr, uint64_t seed,
                               int snr_point, double sigma, int64_t frame0, int64_t total, unsigned long long *next,
                               unsigned long long *ctr, int64_t handoff, hipStream_t s);
size_t tile64_lds_bytes(const DevGraph &g);  // tile_kernel (64 frames per workgroup), 0 if it does not apply
int sub_frames(const DevGraph &g);
size_t sub_lds_bytes(const DevGraph &g);
hipError_t launch_tile_sub(const DevGraph &g, const DevState &st, int max_iter, bool nllr, hipStream_t s);
hipError_t launch_tile_sub_stream(const DevGraph &g, const DevState &st, int max_iter, bool nllr, uint64_t seed,
                                  int snr_point, double sigma, int64_t frame0, int64_t total,
                                  unsigned long long *next, unsigned long long *ctr, int64_t handoff, hipStream_t s);
hipError_t launch_stream_init(const DevGraph &g, const DevState &st, hipStream_t s);
// streaming tail (few tiles): column-parallel VN + per-tile syndrome/exits,
// the same frames' results and counters as launch_vn(stream).  zb
// [cap_tiles][ceil(n/32)][64] u32 and cnt [cap_tiles*64] int, all zero on entry
// (left zero on exit); std_form graphs with k <= 2048
hipError_t launch_vn_tail(const DevGraph &g, const DevState &st, int max_iter, bool nllr, uint32_t *zb, int *cnt,
                          unsigned long long *ctr, hipStream_t s);
hipError_t launch_vn_cols_decode(const DevGraph &g, const DevState &st, int it, bool last, bool nllr, uint32_t *zb,
                                 int *cnt, hipStream_t s);
// tail_exit_kernel's decode exits; gbad (null: the kernel forms the syndrome
// itself) holds the per-frame row-parity flags of syn_kernel, cleared after use
hipError_t launch_tail_exit_decode(const DevGraph &g, const DevState &st, int it, bool last, bool nllr, uint32_t *zb,
                                   int *cnt, int *gbad, hipStream_t s);
// few-frame decode path (edge_kernels.hip): lanes over a row's / column's
// edges, frame after frame; bit-identical to launch_cn + launch_cn_rare and
// launch_vn_cols_decode.  Rows and columns of up to edge_max_deg() edges;
// gbad [cap_tiles*64] int, zero on entry (left zero)
int edge_max_deg();
hipError_t launch_cn_edge(const DevGraph &g, const DevState &st, int it, hipStream_t s);
hipError_t launch_vn_edge_decode(const DevGraph &g, const DevState &st, int it, bool last, bool nllr, uint32_t *zb,
                                 int *cnt, int *gbad, hipStream_t s);
// split CN on 16-frame sub-tiles, t in registers (cn_sub.hip): rows of the
// 2304 codes; 0 when no shape fits the graph
int cn_sub_shape(const DevGraph &g);
hipError_t launch_cn_sub(const DevGraph &g, const DevState &st, int it, hipStream_t s, bool stream);
// rare-row list entries (cn_rare_kernel): tile * m + row in bits 0..27, and
// in bits 28..31 the 16-frame sub-tiles of the tile it covers (0 = all 64
// frames: cn_kernel / cn_row_kernel; bit s = frames 16 s .. 16 s + 15: cn_sub_kernel)
__host__ __device__ inline uint32_t rare_code(int tile_row, uint32_t subs) {
    return (uint32_t)tile_row | (subs << 28);
}
// supply order of a streamed point (frame_order.hip): keys 2 x total uint32,
// vals total int scratch, order total int out, temp frame_order_temp_bytes
size_t frame_order_temp_bytes(int total);
hipError_t launch_frame_order(const DevGraph &g, uint64_t seed, int snr_point, double sigma, int64_t frame0,
                              int total, uint32_t *keys, int *vals, int *order, void *temp, size_t temp_bytes,
                              hipStream_t s);
// the global frame index of supply position idx of a point starting at frame0
__device__ __forceinline__ long long supply_frame(const DevState &st, int64_t frame0, int64_t idx) {
    return (long long)(frame0 + (st.order ? (int64_t)st.order[idx] : idx));
}
hipError_t launch_refill(const DevGraph &g, const DevState &st, uint64_t seed, int snr_point, double sigma,
                         int64_t frame0, int64_t total, unsigned long long *next, hipStream_t s);
// streaming tail: move the frames running in tiles >= nt into finished slots
// of tiles < nt (pairs: 1 + 2 cap ints of scratch)
hipError_t launch_compact(const DevGraph &g, const DevState &st, int nt, int cap, int *pairs, hipStream_t s);
// the plan alone (phys_tile_state.hip's compaction moves its own arrays)
hipError_t launch_compact_plan(const DevState &st, int nt, int cap, int *pairs, hipStream_t s);
hipError_t launch_finalize(const DevGraph &g, const DevState &st, uint8_t *z, double *post,
                           hipStream_t s);
hipError_t launch_export_msgs(const DevGraph &g, const DevState &st, double *out, hipStream_t s);
hipError_t launch_export_frames(const DevGraph &g, const DevState &st, uint8_t *u_out, double *llr_out,
                                hipStream_t s);
hipError_t launch_count(const DevGraph &g, const DevState &st, unsigned long long *counters,
                        hipStream_t s);

// physical mode: check-node rule (LDPC_CN_*) and, for the layered schedule,
// the graph's layer table on the device (ldpc_api.cpp builds it on first use)
constexpr int kCnSpa = 0, kCnNms = 1, kCnOms = 2;
struct PhysRule {
    int cn = kCnSpa;
    float param = 0.0f;             // alpha (kCnNms) or beta (kCnOms)
    const int *layer_ptr = nullptr;  // [n_layers + 1]; null: flooding
    const int *layer_rows = nullptr; // [m]
    int n_layers = 0;
    int max_layer = 0;              // rows of the largest layer
    const int *h_layer_ptr = nullptr;  // layer_ptr on the host (the tile path sizes a layer's launch by it)
    bool layered_tile = false;      // layered: the HBM tile kernels (phys_tile.hip), not the LDS kernel
};

// Monte-Carlo statistics of one SNR point (ldpc_mc_stats_*), filled by every
// physical-mode Monte-Carlo path as a frame finishes; hist == null: off.
struct McStats {
    unsigned long long *hist = nullptr;  // [max_iter + 1]: frames by conv; [max_iter]: failed frames
    unsigned long long *und = nullptr;   // [0] undetected frames, [1] their info-bit errors, [2] failed frames seen
                                         // (a failed frame reserves record und[2]++ and writes it if < max_failed)
    long long *failed = nullptr;         // [max_failed][2]: global frame index, info-bit errors
    long long *slot_frame = nullptr;     // tile paths: [cap] global frame index of the frame in each slot
    int *slot_err = nullptr;             // tile paths: [cap] info-bit errors of a slot's frame, summed over the count
                                         // kernel's blocks of the tile; zero between launches
    int *tile_arrive = nullptr;          // tile paths: [cap / 64] blocks of the tile that added theirs; zero likewise
    long long frame_base = 0;            // LDS paths: global frame index of the launch's frame 0
    int max_failed = 0;
    int max_iter = 0;
};

// physical mode (phys_kernels.hip)
size_t phys_lds_bytes(const DevGraph &g);
int phys_block_threads(const DevGraph &g);  // threads per workgroup launch_phys uses
// layout 0: llr [count][n] fp64; 1: llr = ch tile layout; 2: lam [count][n] fp32 Lambda
hipError_t launch_phys(const DevGraph &g, const double *llr, const float *lam, int layout, int count, int max_iter,
                       uint8_t *z, int *conv, int *status, int *iters, float *post, const uint32_t *ubits,
                       unsigned long long *ctr, int grid, hipStream_t s, const PhysRule &rule = PhysRule{},
                       const McStats &ms = McStats{});
// layered min-sum (phys_layered.hip): E and L of a frame in LDS, one workgroup
// barrier per layer; rule.cn is kCnNms or kCnOms and the layer table is set
size_t phys_layered_lds_bytes(const DevGraph &g);
int phys_layered_threads(const PhysRule &rule);
hipError_t launch_phys_layered(const DevGraph &g, const double *llr, const float *lam, int layout, int count,
                               int max_iter, uint8_t *z, int *conv, int *status, int *iters, float *post,
                               const uint32_t *ubits, unsigned long long *ctr, int grid, hipStream_t s,
                               const PhysRule &rule, const McStats &ms = McStats{});

// fixed-point min-sum with q-bit messages (phys_quant.hip): int8 E, int16 L and
// (flooding) int8 Lam of a frame in LDS.  QuantTab is the graph's padded message
// layout on the device (ldpc_api.cpp builds it on first use): row r's messages
// are the deg bytes at the 4-byte aligned offset row[r].x.
struct QuantTab {
    const int2 *row = nullptr;      // [m] {padded byte offset of the row's messages, its degree}
    const uint16_t *col = nullptr;  // [epad] column of each padded slot (n in the padding)
    const int *csc = nullptr;       // [nnz] padded offset of CSC position p (DevGraph::csc_ptr order)
    int epad = 0;                   // padded message bytes of a frame (a multiple of 4)
};
struct QuantRule {
    int cn = kCnNms;                // kCnNms or kCnOms
    int qbits = 6;                  // 4..8
    float scale = 4.0f;             // llr_scale
    int param_q = 12;               // alpha_q (kCnNms, 1..16) or beta_q (kCnOms, 0..Qmax)
    const int *layer_ptr = nullptr;  // as PhysRule; null: flooding
    const int *layer_rows = nullptr;
    int n_layers = 0;
    int max_layer = 0;
    QuantTab tab;                   // the LDS kernels' layout; unset on the tile path
    bool tile = false;              // the HBM tile kernels (phys_qtile.hip), not the LDS kernels
    const int *h_layer_ptr = nullptr;  // as PhysRule (the tile path sizes a layer's launch by it)
};
size_t phys_quant_lds_bytes(const DevGraph &g, int epad, bool layered);
// >= 0: the flooding decoder runs phys_quant_reg_kernel (indices in registers), else phys_quant_kernel
int phys_quant_reg_shape(const DevGraph &g, int epad, bool layered);
int phys_quant_threads(const DevGraph &g, const QuantRule &rule);
// llr [count][n] fp64, or lam [count][n] fp32 Lambda (then llr is ignored).  The grid is the workgroups
// the device holds at once (CUs x resident per CU), at most max_grid and count.
hipError_t launch_phys_quant(const DevGraph &g, const double *llr, const float *lam, int count, int max_iter,
                             uint8_t *z, int *conv, int *status, int *iters, int16_t *post, const uint32_t *ubits,
                             unsigned long long *ctr, int max_grid, hipStream_t s, const QuantRule &rule,
                             const McStats &ms = McStats{});

// bit-flipping decoders (phys_bitflip.hip): Delta_j = w c_j + (d_j - 2 u_j), flip where Delta_j < theta.
// sliced: bitflip_sliced_kernel, 64 frames per workgroup as one 64-bit word per
// column (w == 0, bitflip_sliced_applies, no statistics); else bitflip_kernel,
// one frame per workgroup.  Both keep a frame's / a tile's whole state in LDS.
struct BitflipRule {
    float weight = 0.0f;
    float theta = 0.0f;
    bool sliced = false;
};
size_t bitflip_lds_bytes(const DevGraph &g);         // bitflip_kernel: Lam[n] fp32, b[n] and s[m] bytes
size_t bitflip_sliced_lds_bytes(const DevGraph &g);  // bitflip_sliced_kernel: 8 (n + m)
bool bitflip_sliced_applies(const DevGraph &g);      // every column degree <= 63
int bitflip_threads();                               // threads per workgroup of both kernels
// input layouts as launch_phys; synw [count] or null: the syndrome weight at exit
hipError_t launch_bitflip(const DevGraph &g, const double *llr, const float *lam, int layout, int count, int max_iter,
                          uint8_t *z, int *conv, int *status, int *iters, int *synw, const uint32_t *ubits,
                          unsigned long long *ctr, int grid, hipStream_t s, const BitflipRule &rule,
                          const McStats &ms = McStats{});

// physical mode, HBM-resident tiles + IRA frame source (phys_tile.hip)
// on-device frames of a chunk (frame_kernels.hip): info bits -> st.ubits,
// parities via pt.pbits/pt.wpar (H_std [A|I] or IRA graph), channel LLRs as
enum FramesOut {
    kFramesCh = 0,          // st.ch, fp64 tile layout (parity decoder, export)
    kFramesTileLambda = 1,  // pt.Lam and pt.L, fp32 tile layout (physical tile decoder)
    kFramesRowLambda = 2,   // row_out [count][n] fp32 Lambda (physical LDS decoder)
};
// The channel of the frame source (include/ldpc_hip.h "channel models"; the
// values are LDPC_CH_*, bits per symbol, LDPC_DEMAP_*).  The default is the
// reference's mode-1 channel: frame_kernels.hip's own kernels, nothing else.
struct FrameChannel {
    int model = 0;
    int bps = 1;
    int demap = 0;
    int fade_block = 1;  // Rayleigh: symbols (BPSK: bits) that share a fade (ldpc_fading_set); 1: a fade each
    // a constellation table (ldpc_constellation_set; include/ldpc_hip.h "constellations"): 2 * 2^bps doubles in
    // host memory, and bps is the table's; null: the channel's own modulation
    const double *table = nullptr;
};
// A decoder's rate-matching pattern as the frame source's kernels read it
// (include/ldpc_hip.h "rate matching"; tables built by rate_match_host.h, in
// device memory the decoder owns).  Per decoder, so not in DevGraph: a graph is
// shared.  The default (E == 0) is no tables: every column is sent, in column
// order.  With a bit interleaver (ldpc_interleaver_set) tx_col is the composite
// tx[perm[t]], and n_fill may be 0 (an interleaver without a pattern, E == n).
struct RateMatchDev {
    const int32_t *tx_col = nullptr;    // [E] the column of transmitted position t (ascending without an interleaver)
    const int32_t *fill_col = nullptr;  // [n_fill] the columns not sent
    const float *fill_llr = nullptr;    // [n_fill] their LLR: +0.0 punctured, -LDPC_RM_KNOWN_LLR shortened
    const uint32_t *umask = nullptr;    // [kw] AND mask of st.ubits (shortened bits clear)
    int E = 0, n_fill = 0, n_short = 0;
};
// A decoder's HARQ plan as the frame source's kernels read it (include/ldpc_hip.h
// "HARQ"; frame_harq.hip).  The default (n_tx == 0) is no plan: launch_frames
// runs as it does without one.  With a plan, rm carries at most shortened
// columns (rm.umask, rm.n_short): the plan says what is sent.
constexpr int kHarqMaxTx = 8;  // LDPC_HARQ_MAX_TX
struct HarqDev {
    const int32_t *cols = nullptr;  // the transmissions' column lists, one after another
    double *acc = nullptr;          // fp64 accumulator of the chunk, tile layout [tile][n][64] as DevState::ch
    int n_tx = 0;
    int tx_len[kHarqMaxTx] = {};    // E_r
    int tx_off[kHarqMaxTx] = {};    // where transmission r's list starts in cols
};
hipError_t launch_frames(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed, int snr_point,
                         double sigma, int64_t frame0, FramesOut out, float *row_out, const FrameChannel &ch,
                         hipStream_t s, const RateMatchDev &rm = RateMatchDev{}, const HarqDev &hq = HarqDev{});
// The last stage of launch_frames under a HARQ plan (frame_harq.hip; hq.n_tx > 0,
// ch.model != 0, every hq.tx_len[r] % ch.bps == 0): zero the accumulator, add
// transmission 0 .. n_tx - 1 into it, write the requested form from it.
hipError_t launch_frame_harq(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed, int snr_point,
                             double sigma, int64_t frame0, FramesOut out, float *row_out, const FrameChannel &ch,
                             const RateMatchDev &rm, const HarqDev &hq, hipStream_t s);
// The last stage of launch_frames under a channel model (frame_channel_models.hip;
// ch.model != 0, g.n % ch.bps == 0): the codeword bits are in st.ubits / pt.pbits /
// pt.wpar already.
hipError_t launch_frame_channel_model(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed,
                                      int snr_point, double sigma, int64_t frame0, FramesOut out, float *row_out,
                                      const FrameChannel &ch, hipStream_t s);
// The same under a rate-matching pattern and / or a bit interleaver (rm.E > 0,
// rm.E % ch.bps == 0): the transmitted columns' LLRs, then the fill of the
// others if there are any (rm.n_fill > 0).
hipError_t launch_frame_channel_model_rm(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed,
                                         int snr_point, double sigma, int64_t frame0, FramesOut out, float *row_out,
                                         const FrameChannel &ch, const RateMatchDev &rm, hipStream_t s);
// What the three above launch in place of their per-axis kernels under a constellation table
// (frame_constellation.hip; ch.table set): the E positions of the column list tx (null: the n columns in
// order) as the form `out`, or with acc (a HARQ transmission) added into it.
hipError_t launch_frame_table(const DevGraph &g, const DevState &st, const PhysTile &pt, uint64_t seed, int snr_point,
                              double sigma, int64_t frame0, FramesOut out, float *row_out, const FrameChannel &ch,
                              const int32_t *tx, int E, double *acc, hipStream_t s);
// st.ubits &= rm.umask, between the info words and the parity stage (rm.n_short > 0)
hipError_t launch_frame_shorten(const DevGraph &g, const DevState &st, const RateMatchDev &rm, hipStream_t s);
// convert: L = Lambda = -(float)ch (else the generator already wrote them)
hipError_t launch_phys_tile_init(const DevGraph &g, const DevState &st, const PhysTile &pt, bool convert,
                                 hipStream_t s);
hipError_t launch_phys_tile_cn(const DevGraph &g, const DevState &st, const PhysTile &pt, int it, bool syn_only,
                               hipStream_t s, const PhysRule &rule = PhysRule{});
// active_count[it] += tiles that still have a running frame after VN(it)
hipError_t launch_phys_tile_vn(const DevGraph &g, const DevState &st, const PhysTile &pt, int it, int *active_count,
                               int max_iter, hipStream_t s);  // active_count [2 max_iter]: tiles, then frames
// Syndrome of the posterior of iteration it right after VN(it), from the VN's
// hard-decision bytes, into bad[(it+1)&1]: launch_phys_tile_exit then stops the
// frames that converged there, which skip CN(it+1)
hipError_t launch_phys_tile_syn(const DevGraph &g, const DevState &st, const PhysTile &pt, int it, hipStream_t s);
// Layered min-sum on the tiles: the rows layer_rows[lbeg .. lbeg + lrows) of one
// layer (rule.cn kCnNms / kCnOms, rule.layer_rows set); launches on one stream
// are the order of the layers.
hipError_t launch_phys_layer_tile(const DevGraph &g, const DevState &st, const PhysTile &pt, int it, int lbeg,
                                  int lrows, hipStream_t s, const PhysRule &rule);

// fixed-point min-sum with the state in HBM (phys_qtile.hip): the tile layout
// and the per-frame state (DevState, bad flags) of phys_tile.hip, the integers
// of phys_quant.hip.  One byte per message and two per posterior.  The members
// E, L, Lam, bad and cap are what the shared bookkeeping (below) takes.
struct QTile {
    int8_t *E;     // [tile][nnz][64] check->variable messages, CSR edge order
    int16_t *L;    // [tile][n][64] posteriors (L < 0 -> bit 1)
    int8_t *Lam;   // [tile][n][64] quantized Lambda, flooding only (layered: null)
    int *bad;      // [2][cap] row-syndrome flags, by iteration parity (layered: slot 0)
    int cap;       // frames of capacity (stride of bad)
    int qmax, pmax, param_q;
    float scale;   // llr_scale
};
// The contract's load: Lam = quantized lam32 * scale (fp32 Lambda tiles of the
// frame generator) or, lam32 null, of -(float)st.ch * scale; L = Lam (Lam kept
// only with `flooding`); per-frame state as launch_phys_tile_init.
hipError_t launch_phys_qtile_init(const DevGraph &g, const DevState &st, const QTile &qt, const float *lam32,
                                  bool flooding, hipStream_t s);
// one layer of the layered schedule (as launch_phys_layer_tile); cn kCnNms / kCnOms
hipError_t launch_phys_qlayer_tile(const DevGraph &g, const DevState &st, const QTile &qt, int cn, int it, int lbeg,
                                   int lrows, const int *layer_rows, hipStream_t s);
// flooding: check sweep and variable sweep
hipError_t launch_phys_qtile_cn(const DevGraph &g, const DevState &st, const QTile &qt, int cn, int it, hipStream_t s);
hipError_t launch_phys_qtile_vn(const DevGraph &g, const DevState &st, const QTile &qt, int it, int *active_count,
                                int max_iter, hipStream_t s);

// The bookkeeping both tile families share (phys_tile_state.hip): bad [2][cap]
// and cap are PhysTile's / QTile's, E / L / Lam their arrays -- float / float /
// float or int8_t / int16_t / int8_t, the two instances of the templates.
// Row parities of b = (L < 0) of the running frames, read from L -> bad[slot]
template <class TL>
hipError_t launch_phys_tile_lsyn(const DevGraph &g, const DevState &st, const TL *L, int *bad, int cap, int slot,
                                 hipStream_t s);
// Flooding, after a syndrome into bad[(it+1)&1]: the frames whose flag stayed 0
// stop (conv = it); active_count[it] / [max_iter + it] recounted
hipError_t launch_phys_tile_exit(const DevState &st, int *bad, int cap, int it, int *active_count, int max_iter,
                                 hipStream_t s);
// Flooding, after the syndrome of the last posterior into bad[max_iter&1]: every running frame stops
hipError_t launch_phys_tile_final(const DevState &st, int *bad, int cap, int max_iter, hipStream_t s);
// Layered, after an iteration's last layer: syndrome of b = (L < 0) into bad[0], then the exits
// (converged at it; unconverged after it = max_iter - 1) and the running counts
// active_count[it], active_count[max_iter + it] (zeroed by the caller).
template <class TL>
hipError_t launch_phys_layer_exit(const DevGraph &g, const DevState &st, const TL *L, int *bad, int cap, int it,
                                  int *active_count, int max_iter, hipStream_t s);
// the tiles to row-major z = (L < 0 ? 0 : 1) and post (either may be null)
template <class TL>
hipError_t launch_phys_tile_out(const DevGraph &g, const DevState &st, const TL *L, uint8_t *z, TL *post,
                                hipStream_t s);
// main.py's counters and McStats of the frames with done == 1
template <class TL>
hipError_t launch_phys_tile_count(const DevGraph &g, const DevState &st, const TL *L, unsigned long long *ctr,
                                  hipStream_t s, const McStats &ms = McStats{});
// Monte-Carlo compaction of the running frames into tiles < nt (the finished ones counted first);
// Lam null: no Lambda plane to move; slot_frame (McStats, or null) moves with the frames.
// cap: the decoder's frame capacity, the stride of bad and of the plan in pairs.
template <class TE, class TL, class TLam>
hipError_t launch_phys_compact(const DevGraph &g, const DevState &st, TE *E, TL *L, TLam *Lam, int *bad, int nt,
                               int cap, int *pairs, hipStream_t s, long long *slot_frame = nullptr);
// McStats::slot_frame of a freshly generated chunk: slot f holds frame base + f
hipError_t launch_mc_stats_slots(long long *slot_frame, long long base, int count, hipStream_t s);

// --- Philox4x32-10 (Salmon et al., SC'11), shared by host tests and device ---
__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1;
        c[3] = (uint32_t)p0;
        c[0] = n0;
        c[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

}  // namespace ldpc
