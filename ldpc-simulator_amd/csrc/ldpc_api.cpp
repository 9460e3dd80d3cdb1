// ldpc_api.cpp -- the C ABI of libldpc_hip.so (include/ldpc_hip.h).
//
// Host orchestration only: argument checks, device allocation, chunking of a
// batch into frame tiles that fit the workspace, and the per-iteration launch
// sequence (spa_kernels.hip).  Nothing here computes a decode result on the
// CPU: without a GPU every entry point fails with LDPC_EDEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "ldpc_internal.h"
#include "mc_stats_host.h"
#include "constellation_host.h"
#include "rate_match_host.h"
#include "spa_device.h"

using ldpc::DevGraph;
using ldpc::DevState;
using ldpc::PhysRule;
using ldpc::PhysTile;
using ldpc::kTile;

static thread_local std::string g_last_error;

int ldpc_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return ldpc_fail(LDPC_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                             __FILE__, __LINE__);                                              \
    } while (0)

struct ldpc_graph {
    int device = 0;
    DevGraph dg{};
    std::vector<int> h_row_ptr, h_col_idx;
    int *d_ints = nullptr;       // one allocation for all index arrays
    uint32_t *d_apack = nullptr;  // bit-packed A (std_form graphs only)
    int min_row_deg = 0;
    // layer table of the layered schedule: built and uploaded on the graph's
    // first layered decode (graph_layers), by whichever thread gets there first
    mutable std::once_flag layers_once;
    mutable int layers_rc = LDPC_OK;
    mutable std::string layers_err;
    mutable int *d_layers = nullptr;  // layer_ptr [n_layers + 1], then layer_rows [m]
    mutable int n_layers = 0, max_layer = 0;
    mutable std::vector<int> h_layer_ptr;  // layer_ptr on the host (launch sizes of the tile path)
    // padded message layout of the fixed-point decoder (phys_quant.hip): built and
    // uploaded on the graph's first quantized decode (graph_quant_tab), likewise
    mutable std::once_flag qtab_once;
    mutable int qtab_rc = LDPC_OK;
    mutable std::string qtab_err;
    mutable void *d_qtab = nullptr;  // row int2 [m], col uint16 [epad], csc int [nnz]
    mutable ldpc::QuantTab qtab;
};

// ints ahead of the rare-row list in ldpc_decoder::rare: 4 rare-row counts, 2 x 64-bit fixed-point totals
constexpr int kRareHead = 8;

struct ldpc_decoder {
    const ldpc_graph *g = nullptr;
    int cap_tiles = 0;
    double *E = nullptr, *T = nullptr, *L = nullptr, *ch = nullptr;
    int *rare = nullptr;  // rare_count[2] + running totals[2] (ldpc_rare_rows_read) + fixed-point totals (2 x 64 bit,
                          // ldpc_fixed_point_read) + rare_list[cap_tiles*m*4]
    int nslots = 0;
    int *ints = nullptr;  // done, conv, status, iters, nllr_cnt, fresh, refill (cap frames each) + tile_active
    uint32_t *ubits = nullptr;
    // staging for host I/O
    double *llr_stage = nullptr, *post_stage = nullptr;
    uint8_t *z_stage = nullptr;
    // physical mode, HBM-resident state (phys_tile.hip); allocated on first use
    float *pE = nullptr, *pL = nullptr, *pLam = nullptr;
    int64_t pE_cap = 0;  // floats in pE
    int *pbad = nullptr;
    uint8_t *pzb = nullptr;  // [tile][ceil(n/8)][64] hard-decision bytes of the last VN sweep
    uint32_t *pbits = nullptr;
    int *pactive = nullptr;  // [pactive_cap] tiles still running after VN(it)
    int pactive_cap = 0;
    double *hist = nullptr;  // decode's normalized-LLR history [cap][hist_cap], kept between calls
    int hist_cap = 0;        // (main.py's one-frame calls ask for it every time: no hipMalloc per call)
    unsigned long long *counters = nullptr;  // [counters_cap] + 1 frame-index counter (streaming)
    int counters_cap = 0;
    int *cpairs = nullptr;  // streaming tail compaction plan (1 + 2 cap ints), on first use
    uint32_t *tzb = nullptr;  // streaming tail VN: z^1 bits [cap_tiles][ceil(n/32)][64], zero between uses
    int *tcnt = nullptr;      // streaming tail VN: normalized-LLR counts [cap_tiles*64], zero between uses
    int *tbad = nullptr;      // few-frame decode path: row-parity flags [cap_tiles*64], zero between uses
    // streaming supply order (frame_order.hip), grow-only: keys 2 x ord_cap, vals / order ord_cap each
    uint32_t *ord_keys = nullptr;
    int *ord_vals = nullptr, *ord = nullptr;
    int64_t ord_cap = 0;
    void *ord_tmp = nullptr;
    size_t ord_tmp_bytes = 0;
    DevState st{};
    // Monte-Carlo statistics (ldpc_mc_stats_*): per point a header and hist[ms_T + 1], then the points'
    // failed-frame records (mc_stats_host.h); ms_slots [cap] the tile paths' frame index of each slot
    bool ms_on = false;
    int ms_max_failed = 0;
    unsigned long long *ms_buf = nullptr;
    size_t ms_words = 0;
    long long *ms_slots = nullptr;
    int *ms_tile = nullptr;             // tile paths: slot_err [cap], then tile_arrive [cap_tiles] (McStats)
    int ms_state = 0;  // 0: nothing to read, 1: the last physical run's statistics, 2: the last run was ldpc_mc_run
    int ms_points = 0, ms_T = 0, ms_run_failed = 0;  // of the run in ms_buf
    // the frame source's channel (ldpc_channel_set); the default is the reference's
    ldpc::FrameChannel chan{};
    // the frame source's rate-matching pattern (ldpc_rate_match_set): the lists on the host; the kernels'
    // tables (rate_match_host.h) go to rm_dev on the first run that needs them, on that run's stream
    std::vector<int32_t> rm_punct, rm_short;
    ldpc::RateMatchTables rm_tab;  // what rm_dev holds (or is about to)
    uint32_t *rm_dev = nullptr;    // rate_match_max_words(n, k) words, allocated once
    bool rm_stale = false;         // the pattern or the interleaver changed since rm_dev was written
    // the frame source's bit interleaver (ldpc_interleaver_set): transmitted position t carries column
    // tx[il_perm[t]]; empty: none.  The coherence length (ldpc_fading_set) is chan.fade_block.
    std::vector<int32_t> il_perm;
    // the frame source's HARQ plan (ldpc_harq_set): the lengths and the column lists one after another on the
    // host; empty: none.  The lists go to hq_dev and the fp64 accumulator of a chunk (cap x n, tile layout) is
    // allocated on the first run that needs them, on that run's stream
    std::vector<int32_t> hq_len, hq_cols;
    int32_t *hq_dev = nullptr;  // LDPC_HARQ_MAX_TX x n column entries, allocated once
    bool hq_stale = false;      // the plan changed since hq_dev was written
    double *hq_acc = nullptr;
    // the frame source's constellation table (ldpc_constellation_set), on the host only: the kernels get it
    // as an argument; bps == 0: none
    ldpc::ConstellationTable ctab;
    // profiling (ldpc_profile_*)
    bool prof = false;
    struct Span {
        int kind;
        hipEvent_t a, b;
    };
    std::vector<Span> spans;
    std::vector<hipEvent_t> pool;
};

namespace {

// LDS a physical-mode workgroup may take (a frame's state must fit)
constexpr size_t kLdsLimit = 160 * 1024 - 1024;

// scratch slots (max_row_deg x 64 doubles) per tile the tile decoders need:
// two buffers of a row per workgroup (rare rows alternate), four for tile8's
// pair form (two rows per wavefront)
int tile_scratch_rows(const DevGraph &g) { return g.ef == 8 ? ldpc::tile8_scratch_per_tile(g) : 2; }

// Sub-tile decoder's S order (tile_sub.hip sub_p3): wavefront w's P3 of row r
// waits for row r-1's P3 by wavefronts [lo, hi], those whose chunk's extended
// column span (from just past the previous non-empty chunk's last column to
// its own last column; the last non-empty chunk runs to infinity) overlaps
// w's.  Chunking as sub_chunk: C = ceil(deg / 16) edges per wavefront.  An
// empty chunk waits for nothing (lo > hi); after an empty row, every
// wavefront waits for all 16 (whose in-order P3s then cover every row before).
// drop_last: chunk all but each row's last edge (tile8.hip: the identity
// column k + r of an [A | I_m] row is wavefront 0's, outside the chunks).
template <int W = ldpc::kSubWaves>
std::vector<int> sub_p3_deps(int m, const int *row_ptr, const int *col_idx, bool drop_last = false) {
    std::vector<int> dep((size_t)m * W, 1);  // lo 1 > hi 0: no wait
    auto spans = [&](int r, long long lo[W], long long hi[W], bool ne[W]) {
        const int beg = row_ptr[r];
        const int deg = std::max(0, row_ptr[r + 1] - beg - (drop_last ? 1 : 0)), C = (deg + W - 1) / W;
        long long prev = -1;
        int last = -1;
        for (int w = 0; w < W; ++w) {
            const int cnt = std::max(0, std::min(deg - w * C, C));
            ne[w] = cnt > 0;
            if (!ne[w]) continue;
            lo[w] = prev + 1;
            hi[w] = prev = col_idx[beg + w * C + cnt - 1];
            last = w;
        }
        if (last >= 0) hi[last] = LLONG_MAX;
        return last >= 0;
    };
    long long plo[W], phi[W], lo[W], hi[W];
    bool pne[W], ne[W];
    bool prev_any = m > 0 && spans(0, plo, phi, pne);
    for (int r = 1; r < m; ++r) {
        spans(r, lo, hi, ne);
        for (int w = 0; w < W; ++w) {
            if (!ne[w]) continue;
            int vlo = W, vhi = -1;
            for (int v = 0; v < W; ++v)
                if (!prev_any || (pne[v] && plo[v] <= hi[w] && lo[w] <= phi[v])) {
                    vlo = std::min(vlo, v);
                    vhi = std::max(vhi, v);
                }
            dep[(size_t)r * W + w] = vlo > vhi ? 1 : (vlo | vhi << 8);
        }
        std::copy(lo, lo + W, plo);
        std::copy(hi, hi + W, phi);
        std::copy(ne, ne + W, pne);
        prev_any = std::any_of(ne, ne + W, [](bool b) { return b; });
    }
    return dep;
}

int require_gpu() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return ldpc_fail(LDPC_EDEVICE, "no HIP device visible: the SPA decoder runs only on the GPU");
    return LDPC_OK;
}

template <class T>
int dev_alloc(T **p, size_t count) {
    *p = nullptr;
    if (count == 0) return LDPC_OK;
    hipError_t e = hipMalloc((void **)p, count * sizeof(T));
    if (e != hipSuccess) {
        *p = nullptr;
        return ldpc_fail(LDPC_ENOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    }
    return LDPC_OK;
}

// Message arrays (E: cap x nnz fp64; T: rare-branch scratch) are only needed by
// the parity-mode decoder; physical-mode Monte-Carlo never touches them.
int ensure_messages(ldpc_decoder *d) {
    if (d->E) return LDPC_OK;
    const DevGraph &G = d->g->dg;
    const size_t cap = (size_t)d->cap_tiles * kTile;
    // + kEPadEdges edges of slack: the sub-tile decoder's P1 loads every
    // register slot of a lane group unclamped (tile_sub.hip, sub_p1), up to 63
    // edges past a row's end -- past the last tile's region on its last row
    int rc = dev_alloc(&d->E, cap * (size_t)G.nnz + (size_t)ldpc::kEPadEdges * kTile);
    if (!rc) rc = dev_alloc(&d->T, (size_t)d->nslots * G.max_row_deg * kTile);
    if (rc) {
        (void)hipFree(d->E);
        d->E = nullptr;
    }
    return rc;
}

// IRA generator scratch (parity words) and physical-mode tile state for graph P
// (E32 sized by P's edges: P may differ from the decoder's own graph).
int ensure_pbits(ldpc_decoder *d, const DevGraph &P) {
    if (d->pbits) return LDPC_OK;
    const size_t mw = (size_t)(P.m + 31) / 32, mw32 = (mw + 31) / 32;
    return dev_alloc(&d->pbits, (size_t)d->cap_tiles * (mw + mw32) * kTile);  // pbits + wpar
}

// A Monte-Carlo run's counters, LDPC_MC_NCOUNT per point: on the device, zeroed on stream s.
int counters_begin(ldpc_decoder *d, int n_points, hipStream_t s) {
    const int need = n_points * LDPC_MC_NCOUNT;
    if (d->counters_cap < need) {
        (void)hipFree(d->counters);
        d->counters = nullptr;
        d->counters_cap = 0;
        if (int rc = dev_alloc(&d->counters, (size_t)need + 1)) return rc;
        d->counters_cap = need;
    }
    HIP_TRY(hipMemsetAsync(d->counters, 0, sizeof(unsigned long long) * need, s));
    return LDPC_OK;
}

// The run's end: the counters to the host, once everything on stream s is done.
int counters_read(ldpc_decoder *d, int n_points, int64_t *counters_out, hipStream_t s) {
    const int need = n_points * LDPC_MC_NCOUNT;
    std::vector<unsigned long long> h(need);
    HIP_TRY(hipMemcpyAsync(h.data(), d->counters, sizeof(unsigned long long) * need, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < need; ++i) counters_out[i] = (int64_t)h[i];
    return LDPC_OK;
}

int ensure_phys_tile(ldpc_decoder *d, const DevGraph &P) {
    const size_t cap = (size_t)d->cap_tiles * kTile;
    const int64_t need = (int64_t)(cap * (size_t)P.nnz);
    if (d->pE_cap < need) {
        (void)hipFree(d->pE);
        d->pE = nullptr;
        d->pE_cap = 0;
        if (int rc = dev_alloc(&d->pE, (size_t)need)) return rc;
        d->pE_cap = need;
    }
    if (!d->pL && dev_alloc(&d->pL, cap * (size_t)d->g->dg.n)) return LDPC_ENOMEM;
    if (!d->pLam && dev_alloc(&d->pLam, cap * (size_t)d->g->dg.n)) return LDPC_ENOMEM;
    if (!d->pbad && dev_alloc(&d->pbad, 2 * cap)) return LDPC_ENOMEM;
    if (!d->pzb && dev_alloc(&d->pzb, cap * (size_t)((d->g->dg.n + 7) / 8))) return LDPC_ENOMEM;
    return LDPC_OK;
}

PhysTile phys_tile(ldpc_decoder *d) {
    const DevGraph &G = d->g->dg;
    uint32_t *wpar = d->pbits ? d->pbits + (size_t)d->cap_tiles * ((G.m + 31) / 32) * kTile : nullptr;
    return PhysTile{d->pE, d->pL, d->pLam, d->pbad, d->pbits, wpar, d->cap_tiles * kTile, d->pzb};
}

void state_bind(ldpc_decoder *d, int ntiles, int count) {
    const size_t cap = (size_t)d->cap_tiles * kTile;
    DevState &s = d->st;
    s.E = d->E;
    s.T = d->T;
    s.rare_count = d->rare;
    s.active_count = nullptr;
    s.fp_count = reinterpret_cast<unsigned long long *>(d->rare + 4);  // 16 bytes into a hipMalloc block
    s.rare_list = d->rare + kRareHead;
    s.nslots = d->nslots;
    s.L = d->L;
    s.ch = d->ch;
    s.done = d->ints;
    s.conv = d->ints + cap;
    s.status = d->ints + 2 * cap;
    s.iters = d->ints + 3 * cap;
    s.nllr_cnt = d->ints + 4 * cap;
    s.fresh = d->ints + 5 * cap;
    s.refill = d->ints + 6 * cap;
    s.order = nullptr;
    s.tile_active = d->ints + 7 * cap;
    s.ubits = d->ubits;
    s.nllr_hist = nullptr;
    s.hist_stride = 0;
    s.ntiles = ntiles;
    s.count = count;
}

// The graph as one call sees it: LDPC_F_TEST_ZERO switches on the frame
// source's test-only erasures (frame_source.h test_zero_llr) for this call only.
DevGraph call_graph(const ldpc_decoder *d, uint32_t flags) {
    DevGraph G = d->g->dg;
    G.zinj = (flags & LDPC_F_TEST_ZERO) ? 1 : 0;
    return G;
}

// The channel as the frame source's launchers take it: under a constellation
// table (ldpc_constellation_set) bps is the table's and table points at it.
ldpc::FrameChannel frame_channel(const ldpc_decoder *d) {
    ldpc::FrameChannel c = d->chan;
    if (d->ctab.bps > 0) {
        c.bps = d->ctab.bps;
        c.table = d->ctab.xy.data();
    }
    return c;
}

// The bits per symbol that n, E and every E_r must divide into, and whose they are.
int frames_bps(const ldpc_decoder *d) { return d->ctab.bps > 0 ? d->ctab.bps : d->chan.bps; }
const char *frames_bps_of(const ldpc_decoder *d) {
    return d->ctab.bps > 0 ? "the constellation table's bits per symbol; ldpc_constellation_set(d, 0, NULL) clears the table"
                           : "the channel's bits per symbol";
}

// A constellation table replaces the modulation of a channel model: it has
// nothing to replace under the reference channel or its test erasures.
int constellation_frames_check(const char *fn, const ldpc_decoder *d, uint32_t flags) {
    if (d->ctab.bps == 0) return LDPC_OK;
    const char *clear = "ldpc_constellation_set(d, 0, NULL) clears the table";
    if (d->chan.model == LDPC_CH_REFERENCE)
        return ldpc_fail(LDPC_EINVAL, "%s: a constellation table (ldpc_constellation_set, bps = %d) needs LDPC_CH_AWGN or "
                                      "LDPC_CH_RAYLEIGH, this decoder has the reference channel (ldpc_channel_set; %s)",
                         fn, d->ctab.bps, clear);
    if (flags & LDPC_F_TEST_ZERO)
        return ldpc_fail(LDPC_EINVAL, "%s: LDPC_F_TEST_ZERO (test erasures) needs the reference channel, this decoder "
                                      "has a constellation table (ldpc_constellation_set; %s)", fn, clear);
    return LDPC_OK;
}

// The same under a HARQ plan (ldpc_harq_set): the plan says what is sent, so
// its own lengths divide into symbols and nothing else may say what is sent.
int harq_frames_check(const char *fn, const ldpc_decoder *d, uint32_t flags) {
    const char *clear = "ldpc_harq_set(d, 0, NULL, NULL) clears the plan";
    if (d->chan.model == LDPC_CH_REFERENCE)
        return ldpc_fail(LDPC_EINVAL, "%s: a HARQ plan (ldpc_harq_set) needs a channel model, this decoder has the "
                                      "reference channel (ldpc_channel_set; %s)", fn, clear);
    if (flags & LDPC_F_TEST_ZERO)
        return ldpc_fail(LDPC_EINVAL, "%s: LDPC_F_TEST_ZERO (test erasures) needs the reference channel, this decoder "
                                      "has a HARQ plan (ldpc_harq_set; %s)", fn, clear);
    if (!d->il_perm.empty())
        return ldpc_fail(LDPC_EINVAL, "%s: a HARQ plan (ldpc_harq_set) carries its own order on the air, this decoder "
                                      "also has a bit interleaver (ldpc_interleaver_set(d, 0, NULL) clears it; %s)", fn,
                         clear);
    if (!d->rm_punct.empty())
        return ldpc_fail(LDPC_EINVAL, "%s: a HARQ plan (ldpc_harq_set) says what is sent, this decoder's rate-matching "
                                      "pattern (ldpc_rate_match_set) also punctures %d columns (%s)", fn,
                         (int)d->rm_punct.size(), clear);
    if (!d->rm_short.empty())
        for (int32_t c : d->hq_cols)
            if (std::binary_search(d->rm_short.begin(), d->rm_short.end(), c))
                return ldpc_fail(LDPC_EINVAL, "%s: the HARQ plan (ldpc_harq_set) sends column %d, which the rate-matching "
                                              "pattern (ldpc_rate_match_set) shortens (%s)", fn, c, clear);
    if (d->chan.fade_block > 1 && d->chan.model != LDPC_CH_RAYLEIGH)
        return ldpc_fail(LDPC_EINVAL, "%s: block fading (ldpc_fading_set, block_len = %d) needs LDPC_CH_RAYLEIGH, this "
                                      "decoder's channel model is %d (ldpc_fading_set(d, 1) clears it)", fn,
                         d->chan.fade_block, d->chan.model);
    for (size_t r = 0; r < d->hq_len.size(); ++r)
        if (d->hq_len[r] % frames_bps(d) != 0)
            return ldpc_fail(LDPC_EINVAL, "%s: transmission %d of the HARQ plan (ldpc_harq_set) sends E_r = %d positions, "
                                          "not a multiple of bps = %d (%s)", fn, (int)r, d->hq_len[r], frames_bps(d),
                             frames_bps_of(d));
    return LDPC_OK;
}

// What a call that generates frames under the decoder's channel model must
// hold (no device work): the code length divides into symbols, and the
// test-only erasures belong to the reference channel.
int channel_frames_check(const char *fn, const ldpc_decoder *d, uint32_t flags) {
    if (int rc = constellation_frames_check(fn, d, flags)) return rc;
    if (!d->hq_len.empty()) return harq_frames_check(fn, d, flags);
    const int n_fill = (int)(d->rm_punct.size() + d->rm_short.size());
    if (n_fill > 0 && d->chan.model == LDPC_CH_REFERENCE)
        return ldpc_fail(LDPC_EINVAL, "%s: a rate-matching pattern (ldpc_rate_match_set) needs a channel model, this "
                                      "decoder has the reference channel (ldpc_channel_set)", fn);
    const int n = d->g->dg.n;
    if (!d->il_perm.empty() && d->chan.model == LDPC_CH_REFERENCE)
        return ldpc_fail(LDPC_EINVAL, "%s: a bit interleaver (ldpc_interleaver_set) needs a channel model, this decoder "
                                      "has the reference channel (ldpc_channel_set; ldpc_interleaver_set(d, 0, NULL) "
                                      "clears the interleaver)", fn);
    if (!d->il_perm.empty() && (int)d->il_perm.size() != n - n_fill)
        return ldpc_fail(LDPC_EINVAL, "%s: the bit interleaver (ldpc_interleaver_set) has length %d, the pattern now set "
                                      "transmits E = %d bits (ldpc_interleaver_set(d, 0, NULL) clears the interleaver)",
                         fn, (int)d->il_perm.size(), n - n_fill);
    if (d->chan.fade_block > 1 && d->chan.model != LDPC_CH_RAYLEIGH)
        return ldpc_fail(LDPC_EINVAL, "%s: block fading (ldpc_fading_set, block_len = %d) needs LDPC_CH_RAYLEIGH, this "
                                      "decoder's channel model is %d (ldpc_fading_set(d, 1) clears it)", fn,
                         d->chan.fade_block, d->chan.model);
    if (d->chan.model == LDPC_CH_REFERENCE) return LDPC_OK;
    if (n_fill > 0 && (n - n_fill) % frames_bps(d) != 0)
        return ldpc_fail(LDPC_EINVAL, "%s: E = %d transmitted bits (n = %d less %d punctured and %d shortened) is not a "
                                      "multiple of bps = %d (%s)", fn, n - n_fill, n, (int)d->rm_punct.size(),
                         (int)d->rm_short.size(), frames_bps(d), frames_bps_of(d));
    if (n_fill == 0 && n % frames_bps(d) != 0)
        return ldpc_fail(LDPC_EINVAL, "%s: n = %d is not a multiple of bps = %d (%s)", fn, n, frames_bps(d),
                         frames_bps_of(d));
    if (flags & LDPC_F_TEST_ZERO)
        return ldpc_fail(LDPC_EINVAL, "%s: LDPC_F_TEST_ZERO (test erasures) needs the reference channel, this decoder "
                                      "has a channel model set (ldpc_channel_set)", fn);
    return LDPC_OK;
}

// The parity-mode entries reproduce the reference: its channel only.
int channel_parity_check(const char *fn, const ldpc_decoder *d) {
    if (d->ctab.bps > 0)
        return ldpc_fail(LDPC_EINVAL, "%s: parity mode has the reference channel only; a constellation table is physical "
                                      "mode's (ldpc_constellation_set(d, 0, NULL) clears the table)", fn);
    if (!d->hq_len.empty())
        return ldpc_fail(LDPC_EINVAL, "%s: parity mode sends every code once; a HARQ plan is physical mode's "
                                      "(ldpc_harq_set(d, 0, NULL, NULL) clears the plan)", fn);
    if (!d->rm_punct.empty() || !d->rm_short.empty())
        return ldpc_fail(LDPC_EINVAL, "%s: parity mode sends every code whole; rate matching is physical mode's "
                                      "(ldpc_rate_match_set(d, 0, NULL, 0, NULL) clears the pattern)", fn);
    if (!d->il_perm.empty())
        return ldpc_fail(LDPC_EINVAL, "%s: parity mode sends every code in column order; the bit interleaver is physical "
                                      "mode's (ldpc_interleaver_set(d, 0, NULL) clears it)", fn);
    if (d->chan.fade_block > 1)
        return ldpc_fail(LDPC_EINVAL, "%s: parity mode has the reference channel only; block fading is physical mode's "
                                      "(ldpc_fading_set(d, 1) clears it)", fn);
    if (d->chan.model == LDPC_CH_REFERENCE) return LDPC_OK;
    return ldpc_fail(LDPC_EINVAL, "%s: parity mode has the reference channel only; the channel models are physical "
                                  "mode's (ldpc_channel_set(d, NULL) puts the reference channel back)", fn);
}

// The decoder's rate-matching pattern and bit interleaver for the frame source's
// kernels: nothing (E = 0) without either, else their tables in device memory
// (tx_col the composite tx[perm[t]]), built, checked and uploaded on stream s
// if either changed since they were (a copy from pageable host
// memory: rm_tab has been read when hipMemcpyAsync returns).
int rate_match_dev(ldpc_decoder *d, hipStream_t s, ldpc::RateMatchDev *out) {
    *out = ldpc::RateMatchDev{};
    if (d->rm_punct.empty() && d->rm_short.empty() && d->il_perm.empty()) return LDPC_OK;
    const DevGraph &G = d->g->dg;
    if (!d->rm_dev) {
        if (int rc = dev_alloc(&d->rm_dev, ldpc::rate_match_max_words(G.n, G.k))) return rc;
        d->rm_stale = true;
    }
    if (d->rm_stale) {
        // an interleaver alone: E = n, no fill lists, an all-ones mask; tx_col becomes tx[perm[t]]
        ldpc::RateMatchTables tab = ldpc::rate_match_build(G.n, G.k, d->rm_punct, d->rm_short);
        if ((!d->il_perm.empty() && !ldpc::interleaver_apply(tab, d->il_perm)) ||
            !ldpc::rate_match_tables_ok(tab, G.n, G.k))
            return ldpc_fail(LDPC_EINVAL, "the frame source's tables do not fit the code: interleaver length %d, E = %d",
                             (int)d->il_perm.size(), tab.E);
        d->rm_tab = std::move(tab);
        HIP_TRY(hipMemcpyAsync(d->rm_dev, d->rm_tab.words.data(), sizeof(uint32_t) * d->rm_tab.words.size(),
                               hipMemcpyHostToDevice, s));
        d->rm_stale = false;
    }
    const ldpc::RateMatchTables &t = d->rm_tab;
    out->tx_col = reinterpret_cast<const int32_t *>(d->rm_dev + t.tx_off());
    out->fill_col = reinterpret_cast<const int32_t *>(d->rm_dev + t.fill_off());
    out->fill_llr = reinterpret_cast<const float *>(d->rm_dev + t.llr_off());
    out->umask = d->rm_dev + t.mask_off();
    out->E = t.E;
    out->n_fill = t.n_fill;
    out->n_short = (int)d->rm_short.size();
    return LDPC_OK;
}

// The decoder's HARQ plan for the frame source's kernels: nothing (n_tx = 0)
// without one, else its column lists in device memory, uploaded on stream s if
// the plan changed since they were (a copy from pageable host memory, as
// rate_match_dev's), and the chunk's fp64 accumulator.
int harq_dev(ldpc_decoder *d, hipStream_t s, ldpc::HarqDev *out) {
    *out = ldpc::HarqDev{};
    if (d->hq_len.empty()) return LDPC_OK;
    const DevGraph &G = d->g->dg;
    if (d->hq_len.size() > (size_t)ldpc::kHarqMaxTx || d->hq_cols.size() > (size_t)ldpc::kHarqMaxTx * (size_t)G.n)
        return ldpc_fail(LDPC_EINVAL, "the HARQ plan does not fit the code: %d transmissions, %zu positions",
                         (int)d->hq_len.size(), d->hq_cols.size());
    if (!d->hq_dev) {
        if (int rc = dev_alloc(&d->hq_dev, (size_t)ldpc::kHarqMaxTx * (size_t)G.n)) return rc;
        d->hq_stale = true;
    }
    if (!d->hq_acc)
        if (int rc = dev_alloc(&d->hq_acc, (size_t)d->cap_tiles * kTile * (size_t)G.n)) return rc;
    if (d->hq_stale) {
        HIP_TRY(hipMemcpyAsync(d->hq_dev, d->hq_cols.data(), sizeof(int32_t) * d->hq_cols.size(),
                               hipMemcpyHostToDevice, s));
        d->hq_stale = false;
    }
    out->cols = d->hq_dev;
    out->acc = d->hq_acc;
    out->n_tx = (int)d->hq_len.size();
    int off = 0;
    for (int r = 0; r < out->n_tx; ++r) {
        out->tx_len[r] = d->hq_len[(size_t)r];
        out->tx_off[r] = off;
        off += d->hq_len[(size_t)r];
    }
    return LDPC_OK;
}

hipEvent_t take_event(ldpc_decoder *d) {
    if (!d->pool.empty()) {
        hipEvent_t e = d->pool.back();
        d->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// Launch `fn` bracketed by events when profiling is on.
template <class F>
hipError_t timed(ldpc_decoder *d, int kind, hipStream_t s, F &&fn) {
    if (!d->prof) return fn();
    hipEvent_t a = take_event(d), b = take_event(d);
    if (a) (void)hipEventRecord(a, s);
    hipError_t e = fn();
    if (b) (void)hipEventRecord(b, s);
    if (a && b) d->spans.push_back({kind, a, b});
    return e;
}

bool tail_vn_enabled();

// Few tiles of a long-row code: the per-tile vn_kernel (one workgroup per
// tile: ~11 ms a pass) and the sub-tile decoders (one workgroup per 16 or 8
// frames: ~11 / ~6 ms a pass whatever the frame count) are latency-bound there,
// while the split CN + the column-parallel VN (vn_cols_kernel +
// tail_exit_kernel<true>) spread a pass over the chip (~0.3 ms per tile) --
// the drop-in per-frame decode() path (64 slots): one wimax_2304_0.5 frame at
// T=50 in 100 ms instead of 746 ms (tools/probe_decode_latency.py, profiles/
// r3_ab/scols2).  LDPC_SMALL_COLS (read per call): the tile count up to which
// it applies (default: 32 for the 16-frame sub-tile codes, 16 for tile8's
// -- the measured cross-overs; 0 = never).
bool small_batch_cols(const DevGraph &G, int ntiles) {
    if (!G.a_packed || ((G.k + 31) >> 5) > 64 || !tail_vn_enabled()) return false;
    // the 64-frame tile_kernel codes (wimax_576_0.5, BCH): short rows, one launch;
    // beyond the edge path's few frames they stay on tile_kernel
    if (ldpc::tile64_lds_bytes(G) > 0) return false;
    const char *e = getenv("LDPC_SMALL_COLS");
    const int lim = e ? atoi(e) : (G.ef == 8 ? 16 : 32);
    if (ntiles > lim) return false;
    return !ldpc::use_tile(G) || ldpc::sub_frames(G) == 16 || G.ef == 8;
}

// Few frames: the lanes of a wavefront take a row's / column's edges instead
// of frames (edge_kernels.hip), so a pass's loads are all in flight at once --
// main.py's one-frame decode() calls: one wimax_2304_0.5 frame at T=50 in
// 5.1 ms instead of 102 ms (4.3 ms since), 8 frames in 20 ms (a frame costs ~2 ms more;
// profiles/r3g_edge).  LDPC_EDGE_FRAMES (read per call): the batch size up to
// which it applies (default 32 for the 2304 codes, below the frame-per-lane
// path's ~100 ms; 4 for the codes of the 64-frame tile_kernel, whose one
// launch takes 7.9 ms for wimax_576_0.5 against 2.9 ms + ~1.1 ms per frame;
// 0 = never; LDPC_SMALL_COLS=0, which keeps every small-batch path away, too).
bool small_batch_edge(const DevGraph &G, int count) {
    const char *c = getenv("LDPC_SMALL_COLS");
    if (c && atoi(c) == 0) return false;
    const char *e = getenv("LDPC_EDGE_FRAMES");
    const int lim = e ? atoi(e) : (ldpc::tile64_lds_bytes(G) > 0 ? 4 : 32);
    return count <= lim && G.max_row_deg <= ldpc::edge_max_deg() && G.max_col_deg <= ldpc::edge_max_deg();
}

// the column-parallel VN's per-tile buffers (zero between passes).  Each
// buffer is allocated under its own null check, so a failed allocation leaves
// the others consistent and a later call retries only what is missing.
int ensure_tail_bufs(ldpc_decoder *d, hipStream_t s) {
    const DevGraph &G = d->g->dg;
    const int cap = d->cap_tiles * kTile;
    const size_t nzb = (size_t)d->cap_tiles * ((G.n + 31) / 32) * kTile;
    if (!d->tzb)
        if (int rc = dev_alloc(&d->tzb, nzb)) return rc;
    if (!d->tcnt)
        if (int rc = dev_alloc(&d->tcnt, (size_t)cap)) return rc;
    if (!d->tbad)
        if (int rc = dev_alloc(&d->tbad, (size_t)cap)) return rc;
    // tail_exit_kernel leaves them zero, but a call that stopped early (an
    // error return) may not have: cleared per call, never trusted
    if (hipMemsetAsync(d->tzb, 0, nzb * sizeof(uint32_t), s) != hipSuccess ||
        hipMemsetAsync(d->tcnt, 0, (size_t)cap * sizeof(int), s) != hipSuccess ||
        hipMemsetAsync(d->tbad, 0, (size_t)cap * sizeof(int), s) != hipSuccess)
        return ldpc_fail(LDPC_EDEVICE, "tail buffers: memset failed");
    return LDPC_OK;
}

// Up to max_iter CN/VN sweeps.  With poll (callers that synchronise anyway),
// the host reads how many tiles are still running after VN(it) for it < 4 and
// every 4th iteration after, and stops once none is: launches over finished
// tiles cost ~0.3 ms each (a grid of early-exiting workgroups).  Which path
// runs is decided first (few-frame edge path, small-batch column-parallel VN,
// the tile-resident decoder, or the split CN/VN launches); an allocation or
// HIP failure is returned as an LDPC_E* code, never turned into another path.
int run_iterations(ldpc_decoder *d, const DevGraph &G, const DevState &st_in, int max_iter, bool nllr,
                   hipStream_t s, bool poll, bool split) {
    DevState st = st_in;
    // the edge path applies to every [A | I] code with k <= 2048 (the 64-frame
    // tile codes too: one wimax_576_0.5 frame, profiles/r3g_edge)
    const bool cols_ok = G.a_packed && ((G.k + 31) >> 5) <= 64 && tail_vn_enabled();
    const bool edge = cols_ok && small_batch_edge(G, st.count);
    const bool cols = edge || (cols_ok && small_batch_cols(G, st.ntiles));
    if (cols)
        if (int rc = ensure_tail_bufs(d, s)) return rc;
    auto hip = [](hipError_t e) {
        return e == hipSuccess ? LDPC_OK
                               : ldpc_fail(LDPC_EDEVICE, "decode iterations: %s", hipGetErrorString(e));
    };
    if (!split && !cols && ldpc::use_tile(G) && st.ntiles * tile_scratch_rows(G) <= st.nslots)  // one launch: every tile to its own exit
        return hip(timed(d, LDPC_K_TILE, s, [&] { return ldpc::launch_tile(G, st, max_iter, nllr, s); }));
    // cn_rare_kernel clears the OTHER parity's count for the next CN; the one
    // the last iteration used (or an early stop left) is cleared here
    hipError_t e = hipMemsetAsync(st.rare_count, 0, sizeof(int) * 2, s);
    if (e) return hip(e);
    if (poll) {
        if (d->pactive_cap < max_iter) {
            (void)hipFree(d->pactive);
            d->pactive = nullptr;
            d->pactive_cap = 0;
            if (int rc = dev_alloc(&d->pactive, (size_t)max_iter)) return rc;
            d->pactive_cap = max_iter;
        }
        if ((e = hipMemsetAsync(d->pactive, 0, sizeof(int) * max_iter, s))) return hip(e);
        st.active_count = d->pactive;
    }
    for (int it = 0; it < max_iter && e == hipSuccess; ++it) {
        if (edge) {  // the rare rows are handled inside cn_edge_kernel
            e = timed(d, LDPC_K_CN_EDGE, s, [&] { return ldpc::launch_cn_edge(G, st, it, s); });
        } else {
            e = timed(d, LDPC_K_CN, s, [&] { return ldpc::launch_cn(G, st, it, s); });
            if (e == hipSuccess) e = ldpc::launch_cn_rare(G, st, it, s);
        }
        if (e == hipSuccess) {
            const bool last = it + 1 == max_iter;
            if (edge)
                e = timed(d, LDPC_K_VN_EDGE, s, [&] {
                    return ldpc::launch_vn_edge_decode(G, st, it, last, nllr, d->tzb, d->tcnt, d->tbad, s);
                });
            else if (cols)
                e = timed(d, LDPC_K_VN_COLS, s, [&] {
                    return ldpc::launch_vn_cols_decode(G, st, it, last, nllr, d->tzb, d->tcnt, s);
                });
            else
                e = timed(d, LDPC_K_VN, s, [&] { return ldpc::launch_vn(G, st, it, max_iter, nllr, s); });
        }
        if (e == hipSuccess && poll && it + 1 < max_iter && (it < 4 || (it + 1) % 4 == 0)) {
            int running = 0;
            e = hipMemcpyAsync(&running, d->pactive + it, sizeof(int), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e == hipSuccess && running == 0) break;
        }
    }
    return hip(e);
}

// cn_rare_kernel runs 1024 blocks x 4 wavefronts; one scratch slot each.
int scratch_slots() { return 4096; }


size_t workspace_bytes(const DevGraph &g, int cap_tiles) {
    const size_t cap = (size_t)cap_tiles * kTile;
    const size_t kw = (size_t)((g.k + 31) / 32);
    size_t b = 0;
    b += cap * (size_t)g.nnz * 8;                                   // E
    const size_t slots = ldpc::use_tile(g) ? std::max(scratch_slots(), cap_tiles * tile_scratch_rows(g)) : scratch_slots();
    b += slots * g.max_row_deg * kTile * 8;  // T pool
    b += 4 * (kRareHead + (size_t)cap_tiles * g.m * 4);                   // rare + fixed-point counts, rare list
    b += 2 * cap * (size_t)g.n * 8;    // L, ch
    b += (7 * cap + cap_tiles) * 4;    // per-frame ints + tile flags
    b += cap * kw * 4;                 // ubits
    b += 2 * cap * (size_t)g.n * 8;    // llr/post staging
    b += cap * (size_t)g.n;            // z staging
    b += cap * ((size_t)(g.n + 31) / 32) * 4 + 2 * cap * 4;  // column-parallel VN / few-frame buffers (tzb, tcnt, tbad)
    // not included: the normalized-LLR history of decode() calls that ask for
    // it (cap x max_iter doubles, allocated on first use, grow-only) and the
    // Monte-Carlo counters (7 int64 per SNR point)
    return b;
}

}  // namespace

extern "C" {

const char *ldpc_last_error(void) { return g_last_error.c_str(); }
int ldpc_abi_version(void) { return LDPC_ABI_VERSION; }

int ldpc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------ graph
namespace {

// The CSR checks ldpc_graph_create and ldpc_layers_build share (`fn` names the
// caller in the message); max_row / min_row: the largest / smallest row degree.
int check_csr(const char *fn, int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx, int *max_row,
              int *min_row) {
    if (m <= 0 || n <= 0 || m > n || !row_ptr || !col_idx)
        return ldpc_fail(LDPC_EINVAL, "%s: bad shape m=%d n=%d", fn, m, n);
    if (row_ptr[0] != 0) return ldpc_fail(LDPC_EINVAL, "%s: row_ptr[0] != 0", fn);
    const int64_t nnz = row_ptr[m];
    // within-tile offsets are 32-bit: e*64 must fit
    if (nnz <= 0 || nnz > (int64_t)(INT32_MAX / kTile) || (int64_t)n > (int64_t)(INT32_MAX / kTile))
        return ldpc_fail(LDPC_ERANGE, "%s: nnz=%lld outside 32-bit tile indexing", fn, (long long)nnz);
    *max_row = 0;
    *min_row = INT_MAX;
    for (int r = 0; r < m; ++r) {
        const int b = row_ptr[r], e = row_ptr[r + 1];
        if (e < b) return ldpc_fail(LDPC_EINVAL, "%s: row_ptr not monotone at %d", fn, r);
        *max_row = std::max(*max_row, e - b);
        *min_row = std::min(*min_row, e - b);
        for (int i = b; i < e; ++i) {
            if (col_idx[i] < 0 || col_idx[i] >= n)
                return ldpc_fail(LDPC_EINVAL, "%s: column %d out of range", fn, col_idx[i]);
            if (i > b && col_idx[i] <= col_idx[i - 1])
                return ldpc_fail(LDPC_EINVAL,
                                 "%s: row %d columns not strictly ascending "
                                 "(the reference's check_to_var order is required)",
                                 fn, r);
        }
    }
    return LDPC_OK;
}

// First-fit layers: rows in ascending order, each into the lowest-numbered
// layer none of whose rows shares a column with it, else a new layer.
// O(nnz x layers): used[l][c] = layer l already holds column c.
int first_fit_layers(int m, int n, const int *row_ptr, const int *col_idx, int *layer_of_row) {
    std::vector<std::vector<uint8_t>> used;
    for (int r = 0; r < m; ++r) {
        size_t l = 0;
        for (; l < used.size(); ++l) {
            bool clash = false;
            for (int e = row_ptr[r]; e < row_ptr[r + 1] && !clash; ++e) clash = used[l][col_idx[e]] != 0;
            if (!clash) break;
        }
        if (l == used.size()) used.emplace_back((size_t)n, (uint8_t)0);
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) used[l][col_idx[e]] = 1;
        layer_of_row[r] = (int)l;
    }
    return (int)used.size();
}

}  // namespace

int ldpc_layers_build(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                      int32_t *layer_of_row_out, int32_t *n_layers_out) {
    int max_row = 0, min_row = 0;
    if (int rc = check_csr("ldpc_layers_build", m, n, row_ptr, col_idx, &max_row, &min_row)) return rc;
    if (!layer_of_row_out || !n_layers_out) return ldpc_fail(LDPC_EINVAL, "ldpc_layers_build: NULL output");
    *n_layers_out = first_fit_layers(m, n, row_ptr, col_idx, layer_of_row_out);
    return LDPC_OK;
}

int ldpc_graph_create(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx, int32_t device,
                      ldpc_graph **out) {
    if (!out) return ldpc_fail(LDPC_EINVAL, "ldpc_graph_create: out is NULL");
    *out = nullptr;
    int max_row = 0, min_row = 0;
    if (int rc = check_csr("ldpc_graph_create", m, n, row_ptr, col_idx, &max_row, &min_row)) return rc;
    const int64_t nnz = row_ptr[m];
    if (int rc = require_gpu()) return rc;
    auto *g = new ldpc_graph;
    g->min_row_deg = min_row;
    g->h_row_ptr.assign(row_ptr, row_ptr + m + 1);
    g->h_col_idx.assign(col_idx, col_idx + nnz);
    // CSC view with rows ascending (var_to_check order; also the order scipy's
    // E.tocsc() sums a column in, spa_decoder.py:177-182)
    std::vector<int> csc_ptr(n + 1, 0), csc_edge(nnz), csc_row(nnz);
    for (int64_t e = 0; e < nnz; ++e) csc_ptr[col_idx[e] + 1]++;
    for (int j = 0; j < n; ++j) csc_ptr[j + 1] += csc_ptr[j];
    std::vector<int> fill(csc_ptr.begin(), csc_ptr.end() - 1);
    int max_col = 0;
    for (int j = 0; j < n; ++j) max_col = std::max(max_col, csc_ptr[j + 1] - csc_ptr[j]);
    for (int r = 0; r < m; ++r)
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
            const int p = fill[col_idx[e]]++;
            csc_edge[p] = e;
            csc_row[p] = r;
        }
    const int k = n - m;
    // standard form check: row r's only column >= k is k+r (encoder needs it)
    int std_form = 1;
    for (int r = 0; r < m && std_form; ++r) {
        int hits = 0;
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e)
            if (col_idx[e] >= k) hits += (col_idx[e] == k + r) ? 1 : 100;
        std_form = hits == 1;
    }
    // IRA form: the parity columns are exactly the staircase p_r in rows r, r+1
    int ira = k > 0 && !std_form;
    for (int r = 0; r < m && ira; ++r) {
        int hits = 0;
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e)
            if (col_idx[e] >= k) hits += (col_idx[e] == k + r || (r > 0 && col_idx[e] == k + r - 1)) ? 1 : 100;
        ira = hits == (r > 0 ? 2 : 1);
    }
    g->device = device;
    DeviceGuard dg(device);
    if (device < 0) (void)hipGetDevice(&g->device);
    const std::vector<int> p3dep = sub_p3_deps(m, row_ptr, col_idx);
    const std::vector<int> p3dep8 = sub_p3_deps(m, row_ptr, col_idx, true);
    const size_t nints = (size_t)(m + 1) + nnz + (size_t)(n + 1) + 2 * (size_t)nnz + p3dep.size() + p3dep8.size();
    if (int rc = dev_alloc(&g->d_ints, nints)) {
        delete g;
        return rc;
    }
    int *p = g->d_ints;
    DevGraph &G = g->dg;
    G.m = m;
    G.n = n;
    G.k = k;
    G.nnz = (int)nnz;
    G.max_row_deg = max_row;
    G.max_col_deg = max_col;
    G.std_form = std_form;
    G.ira = ira;
    G.ef = kTile;
    {
        int odd = 0;
        for (int r = 0; r < m; ++r) odd += (row_ptr[r + 1] - row_ptr[r]) & 1;
        G.lpt_weak_id = std_form && m > 0 && 2 * odd <= m;
    }
    G.row_ptr = p;
    p += m + 1;
    G.col_idx = p;
    p += nnz;
    G.csc_ptr = p;
    p += n + 1;
    G.csc_edge = p;
    p += nnz;
    G.csc_row = p;
    p += nnz;
    G.p3dep = p;
    p += p3dep.size();
    G.p3dep8 = p;
    p += p3dep8.size();
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMemcpy((void *)G.row_ptr, row_ptr, sizeof(int) * (m + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((void *)G.col_idx, col_idx, sizeof(int) * nnz, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((void *)G.csc_ptr, csc_ptr.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((void *)G.csc_edge, csc_edge.data(), sizeof(int) * nnz, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((void *)G.csc_row, csc_row.data(), sizeof(int) * nnz, hipMemcpyHostToDevice);
    if (e == hipSuccess && m > 0)
        e = hipMemcpy((void *)G.p3dep, p3dep.data(), sizeof(int) * p3dep.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && m > 0)
        e = hipMemcpy((void *)G.p3dep8, p3dep8.data(), sizeof(int) * p3dep8.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && std_form && k > 0) {  // encoder table: A bit-packed per row
        const size_t kw = (size_t)(k + 31) / 32;
        std::vector<uint32_t> ap((size_t)m * kw, 0u);
        for (int r = 0; r < m; ++r)
            for (int i = row_ptr[r]; i < row_ptr[r + 1]; ++i)
                if (col_idx[i] < k) ap[(size_t)r * kw + (col_idx[i] >> 5)] |= 1u << (col_idx[i] & 31);
        if (dev_alloc(&g->d_apack, ap.size())) e = hipErrorOutOfMemory;
        if (e == hipSuccess)
            e = hipMemcpy(g->d_apack, ap.data(), sizeof(uint32_t) * ap.size(), hipMemcpyHostToDevice);
        G.a_packed = g->d_apack;
    }
    // the WiMAX 2304 codes run the 8-frame sub-tile decoder: E in 8-frame blocks
    if (e == hipSuccess && !ldpc::tile64_lds_bytes(G) && ldpc::tile8_applies(G)) G.ef = 8;
    // its pair form (two rows per wavefront): LDPC_T8_PAIR=1 (A/B)
    if (G.ef == 8 && ldpc::tile8_pair_fits(G)) {
        const char *ep = getenv("LDPC_T8_PAIR");
        G.t8pair = ep && atoi(ep) != 0 ? 1 : 0;
    }
    if (e != hipSuccess) {
        (void)hipFree(g->d_ints);
        (void)hipFree(g->d_apack);
        delete g;
        return ldpc_fail(LDPC_EDEVICE, "ldpc_graph_create: upload failed: %s", hipGetErrorString(e));
    }
    *out = g;
    return LDPC_OK;
}

int ldpc_graph_destroy(ldpc_graph *g) {
    if (!g) return LDPC_OK;
    DeviceGuard dg(g->device);
    (void)hipFree(g->d_ints);
    (void)hipFree(g->d_apack);
    (void)hipFree(g->d_layers);
    (void)hipFree(g->d_qtab);
    delete g;
    return LDPC_OK;
}

const char *ldpc_cn_kernel_name(const ldpc_graph *g) {
    if (!g) return "";
    return ldpc::use_cn_row(g->dg) ? "cn_row_kernel" : "cn_kernel";
}

const char *ldpc_tile_kernel_name(const ldpc_graph *g) {
    if (!g || !ldpc::use_tile(g->dg)) return "";
    return ldpc::tile_kernel_name(g->dg);
}

int64_t ldpc_tile_lds_bytes(const ldpc_graph *g) {
    if (!g) return 0;
    return ldpc::use_tile(g->dg) ? (int64_t)ldpc::tile_lds_bytes(g->dg) : 0;
}

namespace {
bool phys_use_lds(const DevGraph &P, uint32_t flags) {
    return !(flags & LDPC_F_PHYS_HBM) && ldpc::phys_lds_bytes(P) <= kLdsLimit;
}
}  // namespace

const char *ldpc_phys_kernel_name(const ldpc_graph *g, uint32_t flags) {
    if (!g) return "";
    if (flags & LDPC_F_QUANT_TILE) return "";  // the fixed-point entries' flag
    if (!phys_use_lds(g->dg, flags)) return "phys_cn_tile_kernel";
    return ldpc::phys_block_threads(g->dg) > 256 ? "phys_reg_kernel" : "phys_kernel";
}

const char *ldpc_phys_kernel_name_ex(const ldpc_graph *g, uint32_t flags, int32_t cn_rule, int32_t schedule) {
    if (!g || cn_rule < LDPC_CN_SPA || cn_rule > LDPC_CN_OMS) return "";
    if (flags & LDPC_F_QUANT_TILE) return "";
    if (schedule == LDPC_SCHED_FLOODING) return (flags & LDPC_F_LAYERED_TILE) ? "" : ldpc_phys_kernel_name(g, flags);
    if (schedule != LDPC_SCHED_LAYERED || cn_rule == LDPC_CN_SPA || (flags & LDPC_F_PHYS_HBM)) return "";
    if ((flags & LDPC_F_LAYERED_TILE) || ldpc::phys_layered_lds_bytes(g->dg) > kLdsLimit)
        return "phys_layer_tile_kernel";
    return "phys_layered_kernel";
}

int ldpc_graph_info(const ldpc_graph *g, int32_t *m, int32_t *n, int64_t *nnz, int32_t *max_row_deg,
                    int32_t *max_col_deg) {
    if (!g) return ldpc_fail(LDPC_EINVAL, "ldpc_graph_info: NULL graph");
    if (m) *m = g->dg.m;
    if (n) *n = g->dg.n;
    if (nnz) *nnz = g->dg.nnz;
    if (max_row_deg) *max_row_deg = g->dg.max_row_deg;
    if (max_col_deg) *max_col_deg = g->dg.max_col_deg;
    return LDPC_OK;
}

// ---------------------------------------------------------------- decoder
int64_t ldpc_decoder_bytes(const ldpc_graph *g, int32_t max_frames) {
    if (!g || max_frames <= 0) return -1;
    const int tiles = (max_frames + kTile - 1) / kTile;
    return (int64_t)workspace_bytes(g->dg, tiles);
}

int ldpc_decoder_create(const ldpc_graph *g, int32_t max_frames, ldpc_decoder **out) {
    if (!out) return ldpc_fail(LDPC_EINVAL, "ldpc_decoder_create: out is NULL");
    *out = nullptr;
    if (!g || max_frames <= 0) return ldpc_fail(LDPC_EINVAL, "ldpc_decoder_create: bad arguments");
    DeviceGuard dg(g->device);
    auto *d = new ldpc_decoder;
    d->g = g;
    d->cap_tiles = (max_frames + kTile - 1) / kTile;
    const size_t cap = (size_t)d->cap_tiles * kTile;
    const DevGraph &G = g->dg;
    const size_t kw = (size_t)((G.k + 31) / 32);
    int rc = LDPC_OK;
    d->nslots = scratch_slots();  // E and T are allocated on first parity-mode use
    if (ldpc::use_tile(G))  // one scratch row per tile workgroup (two for tile8's pair form)
        d->nslots = std::max(d->nslots, d->cap_tiles * tile_scratch_rows(G));
    // rare list: one entry per (tile, row), or per 16-frame sub-tile of it (cn_sub_kernel);
    // entries pack tile * m + row into 28 bits (spa_device.h rare_code)
    if ((int64_t)d->cap_tiles * G.m >= (int64_t)1 << 28) {
        delete d;
        return ldpc_fail(LDPC_ERANGE, "ldpc_decoder_create: %d frames x %d rows exceed the rare-row list", max_frames,
                         G.m);
    }
    if (!rc) rc = dev_alloc(&d->rare, kRareHead + (size_t)d->cap_tiles * G.m * 4);
    if (!rc && hipMemset(d->rare, 0, sizeof(int) * kRareHead) != hipSuccess)
        rc = ldpc_fail(LDPC_EDEVICE, "ldpc_decoder_create: memset failed");
    if (!rc) rc = dev_alloc(&d->L, cap * (size_t)G.n);
    if (!rc) rc = dev_alloc(&d->ch, cap * (size_t)G.n);
    if (!rc) rc = dev_alloc(&d->ints, 7 * cap + (size_t)d->cap_tiles);
    if (!rc) rc = dev_alloc(&d->ubits, std::max<size_t>(cap * kw, 1));
    if (!rc) rc = dev_alloc(&d->llr_stage, cap * (size_t)G.n);
    if (!rc) rc = dev_alloc(&d->post_stage, cap * (size_t)G.n);
    if (!rc) rc = dev_alloc(&d->z_stage, cap * (size_t)G.n);
    if (rc) {
        ldpc_decoder_destroy(d);
        return rc;
    }
    *out = d;
    return LDPC_OK;
}

int ldpc_decoder_destroy(ldpc_decoder *d) {
    if (!d) return LDPC_OK;
    DeviceGuard dg(d->g ? d->g->device : -1);
    (void)hipFree(d->E);
    (void)hipFree(d->T);
    (void)hipFree(d->rare);
    (void)hipFree(d->cpairs);
    (void)hipFree(d->tzb);
    (void)hipFree(d->tcnt);
    (void)hipFree(d->tbad);
    (void)hipFree(d->ord_keys);
    (void)hipFree(d->ord_vals);
    (void)hipFree(d->ord);
    (void)hipFree(d->ord_tmp);
    (void)hipFree(d->hist);
    (void)hipFree(d->L);
    (void)hipFree(d->ch);
    (void)hipFree(d->ints);
    (void)hipFree(d->ubits);
    (void)hipFree(d->llr_stage);
    (void)hipFree(d->post_stage);
    (void)hipFree(d->z_stage);
    (void)hipFree(d->counters);
    (void)hipFree(d->pE);
    (void)hipFree(d->pL);
    (void)hipFree(d->pLam);
    (void)hipFree(d->pbad);
    (void)hipFree(d->pzb);
    (void)hipFree(d->pbits);
    (void)hipFree(d->pactive);
    (void)hipFree(d->ms_buf);
    (void)hipFree(d->ms_slots);
    (void)hipFree(d->ms_tile);
    (void)hipFree(d->rm_dev);
    (void)hipFree(d->hq_dev);
    (void)hipFree(d->hq_acc);
    for (auto &sp : d->spans) {
        (void)hipEventDestroy(sp.a);
        (void)hipEventDestroy(sp.b);
    }
    for (auto e : d->pool) (void)hipEventDestroy(e);
    delete d;
    return LDPC_OK;
}

int32_t ldpc_decoder_capacity(const ldpc_decoder *d) { return d ? d->cap_tiles * kTile : 0; }

// ----------------------------------------------------------------- decode
int ldpc_decode_f64(ldpc_decoder *d, int32_t batch, const double *llr, int32_t max_iter, uint32_t flags,
                    uint8_t *z_out, int32_t *conv_out, int32_t *status_out, double *post_out, double *nllr_out,
                    double *nllr_hist, int32_t *iters_out, double *msg_out, void *stream) {
    if (!d) return ldpc_fail(LDPC_EINVAL, "ldpc_decode_f64: NULL decoder");
    if (batch < 0) return ldpc_fail(LDPC_EINVAL, "ldpc_decode_f64: batch < 0");
    if (max_iter < 1)
        return ldpc_fail(LDPC_EINVAL,
                         "ldpc_decode_f64: max_iter=%d; must be >= 1 (the reference loops until the "
                         "syndrome clears for T<1, spa_decoder.py:104)",
                         max_iter);
    if (batch == 0) return LDPC_OK;
    if (!llr) return ldpc_fail(LDPC_EINVAL, "ldpc_decode_f64: llr is NULL");
    const bool dev_ptrs = flags & LDPC_F_DEVICE_PTRS;
    const bool nllr = flags & LDPC_F_NLLR;
    if (dev_ptrs && msg_out) return ldpc_fail(LDPC_EINVAL, "ldpc_decode_f64: msg_out is host-only");
    DeviceGuard dg(d->g->device);
    if (int rc0 = ensure_messages(d)) return rc0;
    hipStream_t s = (hipStream_t)stream;
    const DevGraph &G = d->g->dg;
    const int n = G.n;
    const int cap = d->cap_tiles * kTile;

    double *d_hist = nullptr;
    double *d_msgs = nullptr;
    std::vector<int> h_ints;
    std::vector<double> h_dbl;
    int rc = LDPC_OK;
    if (nllr_hist) {
        if (d->hist_cap < max_iter) {  // grow-only, reused by later calls
            (void)hipFree(d->hist);
            d->hist = nullptr;
            d->hist_cap = 0;
            if ((rc = dev_alloc(&d->hist, (size_t)cap * max_iter))) return rc;
            d->hist_cap = max_iter;
        }
        d_hist = d->hist;
    }
    if (msg_out) {
        if ((rc = dev_alloc(&d_msgs, (size_t)cap * G.nnz))) return rc;
    }
    auto fail_dev = [&](hipError_t e, const char *what) {
        (void)hipFree(d_msgs);
        return ldpc_fail(LDPC_EDEVICE, "ldpc_decode_f64: %s: %s", what, hipGetErrorString(e));
    };
    hipError_t e = hipSuccess;
    for (int start = 0; start < batch; start += cap) {
        const int cnt = std::min(cap, batch - start);
        const int ntiles = (cnt + kTile - 1) / kTile;
        state_bind(d, ntiles, cnt);
        DevState st = d->st;
        if (d_hist) {
            st.nllr_hist = d_hist;
            st.hist_stride = max_iter;
            if ((e = hipMemsetD8Async((hipDeviceptr_t)d_hist, 0xFF, sizeof(double) * (size_t)cnt * max_iter, s)))
                return fail_dev(e, "memset");
        }
        const double *src = llr + (size_t)start * n;
        if (!dev_ptrs) {
            if ((e = hipMemcpyAsync(d->llr_stage, src, sizeof(double) * (size_t)cnt * n, hipMemcpyHostToDevice, s)))
                return fail_dev(e, "llr upload");
            src = d->llr_stage;
        }
        if ((e = ldpc::launch_reset(G, st, s))) return fail_dev(e, "reset");
        if ((e = ldpc::launch_load_llr(G, st, src, s))) return fail_dev(e, "load");
        if (int rc1 = run_iterations(d, G, st, max_iter, nllr, s, !dev_ptrs, flags & LDPC_F_SPLIT)) {
            (void)hipFree(d_msgs);
            return rc1;
        }
        uint8_t *zdst = dev_ptrs ? (z_out ? z_out + (size_t)start * n : nullptr) : d->z_stage;
        double *pdst = dev_ptrs ? (post_out ? post_out + (size_t)start * n : nullptr) : (post_out ? d->post_stage : nullptr);
        if (zdst || pdst) {
            uint8_t *zz = zdst ? zdst : d->z_stage;
            if ((e = ldpc::launch_finalize(G, st, zz, pdst, s))) return fail_dev(e, "finalize");
        }
        if (d_msgs && (e = ldpc::launch_export_msgs(G, st, d_msgs, s))) return fail_dev(e, "export");
        // per-frame scalars
        const size_t capz = (size_t)d->cap_tiles * kTile;
        auto copy_ints = [&](int32_t *dst, const int *srcp) -> hipError_t {
            if (!dst) return hipSuccess;
            return hipMemcpyAsync(dst + start, srcp, sizeof(int) * cnt,
                                  dev_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s);
        };
        if ((e = copy_ints(conv_out, st.conv))) return fail_dev(e, "conv copy");
        if ((e = copy_ints(status_out, st.status))) return fail_dev(e, "status copy");
        if ((e = copy_ints(iters_out, st.iters))) return fail_dev(e, "iters copy");
        (void)capz;
        if (!dev_ptrs) {
            if (z_out && (e = hipMemcpyAsync(z_out + (size_t)start * n, d->z_stage, (size_t)cnt * n,
                                             hipMemcpyDeviceToHost, s)))
                return fail_dev(e, "z copy");
            if (post_out && (e = hipMemcpyAsync(post_out + (size_t)start * n, d->post_stage,
                                                sizeof(double) * (size_t)cnt * n, hipMemcpyDeviceToHost, s)))
                return fail_dev(e, "post copy");
            if (msg_out && (e = hipMemcpyAsync(msg_out + (size_t)start * G.nnz, d_msgs,
                                               sizeof(double) * (size_t)cnt * G.nnz, hipMemcpyDeviceToHost, s)))
                return fail_dev(e, "msg copy");
            if (nllr_hist && (e = hipMemcpyAsync(nllr_hist + (size_t)start * max_iter, d_hist,
                                                 sizeof(double) * (size_t)cnt * max_iter, hipMemcpyDeviceToHost, s)))
                return fail_dev(e, "hist copy");
            if (nllr_out) {
                h_ints.resize(cnt);
                if ((e = hipMemcpyAsync(h_ints.data(), st.nllr_cnt, sizeof(int) * cnt, hipMemcpyDeviceToHost, s)))
                    return fail_dev(e, "nllr copy");
                if ((e = hipStreamSynchronize(s))) return fail_dev(e, "sync");
                for (int i = 0; i < cnt; ++i)
                    nllr_out[start + i] = nllr ? (G.k > 0 ? (double)h_ints[i] / G.k : 0.0) : 0.0;
            }
            // the staging buffers are reused by the next chunk
            if ((e = hipStreamSynchronize(s))) return fail_dev(e, "sync");
        } else if (nllr_out || nllr_hist) {
            if (nllr_hist && (e = hipMemcpyAsync(nllr_hist + (size_t)start * max_iter, d_hist,
                                                 sizeof(double) * (size_t)cnt * max_iter, hipMemcpyDeviceToDevice, s)))
                return fail_dev(e, "hist copy");
            if (nllr_out) {  // device path: convert counts on the host side of the stream
                h_ints.resize(cnt);
                h_dbl.resize(cnt);
                if ((e = hipMemcpyAsync(h_ints.data(), st.nllr_cnt, sizeof(int) * cnt, hipMemcpyDeviceToHost, s)))
                    return fail_dev(e, "nllr copy");
                if ((e = hipStreamSynchronize(s))) return fail_dev(e, "sync");
                for (int i = 0; i < cnt; ++i) h_dbl[i] = nllr ? (G.k > 0 ? (double)h_ints[i] / G.k : 0.0) : 0.0;
                if ((e = hipMemcpy(nllr_out + start, h_dbl.data(), sizeof(double) * cnt, hipMemcpyHostToDevice)))
                    return fail_dev(e, "nllr upload");
            }
        }
    }
    if (d_hist || d_msgs) {
        if ((e = hipStreamSynchronize(s))) return fail_dev(e, "sync");
    }
    (void)hipFree(d_msgs);
    if ((e = hipGetLastError())) return ldpc_fail(LDPC_EDEVICE, "ldpc_decode_f64: %s", hipGetErrorString(e));
    return LDPC_OK;
}

// ------------------------------------------------------- Monte-Carlo path
int ldpc_generate_frames(ldpc_decoder *d, uint64_t seed, int32_t snr_point, double sigma, int64_t frame0,
                         int32_t count, uint32_t flags, uint8_t *u_out, double *llr_out, void *stream) {
    if (!d) return ldpc_fail(LDPC_EINVAL, "ldpc_generate_frames: NULL decoder");
    const DevGraph G = call_graph(d, flags);
    if (!G.std_form && !G.ira)
        return ldpc_fail(LDPC_EINVAL, "ldpc_generate_frames: graph is neither [A | I_m] nor IRA [H_info | staircase]");
    if (count < 0 || count > d->cap_tiles * kTile || snr_point < 0 || frame0 < 0 || !(sigma > 0.0))
        return ldpc_fail(LDPC_EINVAL, "ldpc_generate_frames: bad arguments (count=%d cap=%d)", count,
                         d->cap_tiles * kTile);
    if (int rc = channel_frames_check("ldpc_generate_frames", d, flags)) return rc;
    if (count == 0) return LDPC_OK;
    DeviceGuard dg(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    const bool dev_ptrs = flags & LDPC_F_DEVICE_PTRS;
    state_bind(d, (count + kTile - 1) / kTile, count);
    uint8_t *u_dev = nullptr;
    double *l_dev = nullptr;
    int rc = LDPC_OK;
    if (!dev_ptrs) {
        if (u_out && (rc = dev_alloc(&u_dev, (size_t)count * G.k))) return rc;
        l_dev = llr_out ? d->llr_stage : nullptr;
    } else {
        u_dev = u_out;
        l_dev = llr_out;
    }
    ldpc::RateMatchDev rm;
    ldpc::HarqDev hq;
    if ((rc = ensure_pbits(d, G)) || (rc = rate_match_dev(d, s, &rm)) || (rc = harq_dev(d, s, &hq))) {
        (void)hipFree(dev_ptrs ? nullptr : u_dev);
        return rc;
    }
    HIP_TRY(ldpc::launch_frames(G, d->st, phys_tile(d), seed, snr_point, sigma, frame0, ldpc::kFramesCh, nullptr,
                                frame_channel(d), s, rm, hq));
    // export writes u only for j<k, at [f][k]: give it the [count][k] buffer
    HIP_TRY(ldpc::launch_export_frames(G, d->st, u_dev, l_dev, s));
    if (!dev_ptrs) {
        if (u_out) HIP_TRY(hipMemcpyAsync(u_out, u_dev, (size_t)count * G.k, hipMemcpyDeviceToHost, s));
        if (llr_out)
            HIP_TRY(hipMemcpyAsync(llr_out, l_dev, sizeof(double) * (size_t)count * G.n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        (void)hipFree(u_dev);
    }
    return LDPC_OK;
}

namespace {

// Streaming tail: the column-parallel VN (launch_vn_tail) replaces vn_kernel
// once at most kTailTiles tiles run; the sub-tile streaming kernel hands its
// frames over once the supply is out and at most LDPC_HANDOFF frames still
// run (default: handoff_frames).  LDPC_TAIL_VN=0 / LDPC_HANDOFF=0 switch them off.
constexpr int kTailTiles = 128;
bool tail_vn_enabled() {
    const char *e = getenv("LDPC_TAIL_VN");
    return !e || atoi(e) != 0;
}
// Default: once the supply is out and at most 3/5 of the slots the sub-tile
// kernel keeps resident (one 16-frame workgroup per CU) still run.  At 3 dB
// (wimax_2304_0.5) that is within a few passes -- about 2/3 of the slots then
// hold frames that will fail, at every stage of their 50 passes -- and the
// step takes 615 ms instead of 1.1 s; at 2 dB, where nearly every slot runs to
// 50 passes, the sub-tile kernel keeps the bulk (3/4: -2 % there;
// profiles/r2au_tail).
// fpw: frames per workgroup of the streaming sub-tile kernel (16, or 8 for
// tile8_stream_kernel), one workgroup per CU.  Round 4, with the
// longest-job-first supply order: the 16-frame kernel hands off as soon as the
// supply is out (every resident frame: 3 dB step 66.3k -> 69.1k cw/s; 3/5 of
// them, 4,000 and "always" measured 66.3k / 68.9k / 68.6k); the 8-frame kernel,
// whose pass is half as long, keeps 3/5 (r3/4A 3 dB: 52.3k vs 47.8k for all
// resident) -- profiles/r4c_ab.
int64_t handoff_frames(int64_t slots, int fpw) {
    const char *e = getenv("LDPC_HANDOFF");
    if (e) return atoll(e);
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const int64_t resident = std::min<int64_t>(slots, (int64_t)cus * fpw);
    return fpw == 16 ? resident : resident * 3 / 5;
}

// Longest job first (frame_order.hip): the point's frames enter the slots in
// descending syndrome weight of their channel hard decisions, so the frames
// that will run to max_iter start while the slots are still being refilled
// instead of forming a tail after the supply is out.  Counters are sums over
// the point's frames, identical in any order.  LDPC_LPT=0: frame index order.
bool lpt_enabled() {
    const char *e = getenv("LDPC_LPT");
    return !e || atoi(e) != 0;
}
int ensure_order(ldpc_decoder *d, int64_t total) {
    if (d->ord_cap < total) {
        (void)hipFree(d->ord_keys);
        (void)hipFree(d->ord_vals);
        (void)hipFree(d->ord);
        d->ord_keys = nullptr;
        d->ord_vals = d->ord = nullptr;
        d->ord_cap = 0;
        if (int rc = dev_alloc(&d->ord_keys, 2 * (size_t)total)) return rc;
        if (int rc = dev_alloc(&d->ord_vals, (size_t)total)) return rc;
        if (int rc = dev_alloc(&d->ord, (size_t)total)) return rc;
        d->ord_cap = total;
    }
    const size_t tb = ldpc::frame_order_temp_bytes((int)total);
    if (d->ord_tmp_bytes < tb) {
        (void)hipFree(d->ord_tmp);
        d->ord_tmp = nullptr;
        d->ord_tmp_bytes = 0;
        if (hipMalloc(&d->ord_tmp, tb) != hipSuccess)
            return ldpc_fail(LDPC_ENOMEM, "hipMalloc(%zu bytes) failed (frame order scratch)", tb);
        d->ord_tmp_bytes = tb;
    }
    return LDPC_OK;
}

// Streaming schedule of one SNR point: the decoder's cap frames are slots.  A
// slot whose frame finishes (vn_kernel) is refilled with the next frame index
// (refill_kernel), so no slot waits for the slowest frame of its tile or
// chunk; only the last frames of the point form a tail.  Frames, and the
// counters summed over them, are exactly the static schedule's.
int mc_stream_point(ldpc_decoder *d, const DevGraph &G, uint64_t seed, int p, double sigma, int64_t total,
                    int64_t frame0, int max_iter, bool nllr, bool split, hipStream_t s) {
    if (total == 0) return LDPC_OK;
    const int ntiles = (int)std::min<int64_t>(d->cap_tiles, (total + kTile - 1) / kTile);
    const int *order = nullptr;  // supply order (null: frame index order)
    // only when frames wait for a slot: with every frame running from the
    // start the order cannot change when any of them runs.  The split path
    // runs every slot each launch; a tile streaming kernel keeps one
    // workgroup per CU resident (its other workgroups start as those finish)
    int64_t running = (int64_t)ntiles * kTile;
    if (!split && ldpc::use_tile_stream(G)) {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess)
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        const int fpw = G.ef == 8 ? 8 : ldpc::sub_frames(G) == 16 ? 16 : kTile;
        running = std::min<int64_t>(running, (int64_t)cus * fpw);
    }
    if (lpt_enabled() && total > running && total <= INT32_MAX && G.std_form && G.a_packed && G.m <= 65535) {
        if (int rc = ensure_order(d, total)) return rc;
        HIP_TRY(timed(d, LDPC_K_GEN, s, [&] {
            return ldpc::launch_frame_order(G, seed, p, sigma, frame0, (int)total, d->ord_keys, d->ord_vals, d->ord,
                                            d->ord_tmp, d->ord_tmp_bytes, s);
        }));
        order = d->ord;
    }
    state_bind(d, ntiles, ntiles * kTile);
    d->st.order = order;
    DevState st = d->st;
    unsigned long long *ctr = d->counters + (size_t)p * LDPC_MC_NCOUNT;
    unsigned long long *next = d->counters + d->counters_cap;
    const int cap = d->cap_tiles * kTile;
    // streaming tail VN (column-parallel, launch_vn_tail) once few tiles run
    const bool tail_ok = G.a_packed && ((G.k + 31) >> 5) <= 64 && tail_vn_enabled();
    if (tail_ok)
        if (int rc = ensure_tail_bufs(d, s)) return rc;
    auto refill = [&] {
        return timed(d, LDPC_K_GEN, s,
                     [&] { return ldpc::launch_refill(G, st, seed, p, sigma, frame0, total, next, s); });
    };
    int cur = ntiles;  // tiles the steps launch (shrinks as the tail is compacted)
    if (!split && ldpc::use_tile_stream(G) && st.ntiles * tile_scratch_rows(G) <= st.nslots) {
        // one launch: every workgroup's lanes pull frames until the supply is
        // out; the sub-tile decoder hands its last running frames to the
        // column-parallel tail below (one pass of a sub-tile costs ~14 ms)
        const int fpw = G.ef == 8 ? 8 : ldpc::sub_frames(G) == 16 ? 16 : 0;  // 0: tile_stream_kernel, no hand-off
        const int64_t ho = tail_ok && fpw ? handoff_frames((int64_t)ntiles * kTile, fpw) : 0;
        HIP_TRY(hipMemsetAsync(next, 0, sizeof(unsigned long long), s));
        HIP_TRY(timed(d, LDPC_K_TILE, s, [&] {
            return ldpc::launch_tile_stream(G, st, max_iter, nllr, seed, p, sigma, frame0, total, next, ctr, ho, s);
        }));
        if (ho <= 0) return LDPC_OK;
        unsigned long long finished = 0;
        HIP_TRY(hipMemcpyAsync(&finished, ctr, sizeof(finished), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if ((int64_t)finished >= total) return LDPC_OK;
        // the running frames (split-path slot state, written by the kernel)
        // move into the first tiles; the loop below continues them
        const int nt = (int)((total - (int64_t)finished + kTile - 1) / kTile);
        if (!d->cpairs && dev_alloc(&d->cpairs, 1 + 2 * (size_t)cap)) return LDPC_ENOMEM;
        if (nt < cur) {
            HIP_TRY(ldpc::launch_compact(G, st, nt, cap, d->cpairs, s));
            state_bind(d, nt, nt * kTile);
            d->st.order = order;
            st = d->st;
            cur = nt;
        } else {
            HIP_TRY(ldpc::launch_compact(G, st, cur, cap, d->cpairs, s));  // tile_active of every tile
        }
    } else {
        HIP_TRY(ldpc::launch_stream_init(G, st, s));
        HIP_TRY(hipMemsetAsync(next, 0, sizeof(unsigned long long), s));
        HIP_TRY(refill());
    }
    HIP_TRY(hipMemsetAsync(st.rare_count, 0, sizeof(int) * 2, s));  // see run_iterations
    const int64_t slots = (int64_t)ntiles * kTile;
    const int64_t min_steps = (total + slots - 1) / slots;            // every slot needs >= 1 step per frame
    const int64_t max_steps = (min_steps + 1) * (int64_t)max_iter;   // every frame stops by max_iter
    constexpr int kPoll = 4;
    int64_t step = 0;
    const bool compact = [] {
        const char *e = getenv("LDPC_COMPACT");
        return !e || atoi(e) != 0;
    }();
    // compact once live <= cur * 64 * kc / 8 (LDPC_COMPACT_AT, eighths)
    const int kc = [] {
        const char *e = getenv("LDPC_COMPACT_AT");
        return e ? std::max(1, std::min(8, atoi(e))) : 4;
    }();
    const bool tlog = getenv("LDPC_TAIL_LOG") != nullptr;
    for (;;) {
        // every frame fits in the slots: all start now and stop by max_iter
        const int64_t until = total <= slots ? std::max<int64_t>(step + kPoll, max_iter)
                                             : std::max<int64_t>(step + kPoll, min_steps);
        for (; step < until; ++step) {
            const int par = (int)(step & 1);
            HIP_TRY(timed(d, LDPC_K_CN, s, [&] { return ldpc::launch_cn(G, st, par, s, true); }));
            HIP_TRY(ldpc::launch_cn_rare(G, st, par, s, true));
            if (tail_ok && cur <= kTailTiles)
                HIP_TRY(timed(d, LDPC_K_VN_COLS, s,
                              [&] { return ldpc::launch_vn_tail(G, st, max_iter, nllr, d->tzb, d->tcnt, ctr, s); }));
            else
                HIP_TRY(timed(d, LDPC_K_VN, s, [&] { return ldpc::launch_vn(G, st, 0, max_iter, nllr, s, ctr); }));
            HIP_TRY(refill());
        }
        unsigned long long finished = 0, handed = 0;
        HIP_TRY(hipMemcpyAsync(&finished, ctr, sizeof(finished), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&handed, next, sizeof(handed), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if ((int64_t)finished >= total) return LDPC_OK;
        // tail: the supply is out and at most half of the launched slots
        // still run -> move them into the first tiles and launch only those
        const int64_t live = std::min<int64_t>((int64_t)handed, total) - (int64_t)finished;
        if (tlog) fprintf(stderr, "[tail] step %lld cur %d live %lld\n", (long long)step, cur, (long long)live);
        const int nt = (int)((live + kTile - 1) / kTile);
        if (compact && (int64_t)handed >= total && cur > 1 && live > 0 && nt < cur &&
            live * 8 <= (int64_t)cur * kTile * kc) {
            if (!d->cpairs && dev_alloc(&d->cpairs, 1 + 2 * (size_t)cap)) return LDPC_ENOMEM;
            HIP_TRY(ldpc::launch_compact(G, st, nt, cap, d->cpairs, s));
            state_bind(d, nt, nt * kTile);
            d->st.order = order;
            st = d->st;
            cur = nt;
        }
        if (step > max_steps)
            return ldpc_fail(LDPC_EDEVICE, "ldpc_mc_run: streaming schedule did not drain (%llu of %lld frames)",
                             finished, (long long)total);
    }
}

}  // namespace

int ldpc_frame_order(ldpc_decoder *d, uint64_t seed, int32_t snr_point, double sigma, int64_t frame0,
                     int32_t count, int32_t *order_out, void *stream) {
    if (!d || count < 0 || snr_point < 0 || frame0 < 0 || !(sigma > 0.0) || (count > 0 && !order_out))
        return ldpc_fail(LDPC_EINVAL, "ldpc_frame_order: bad arguments");
    if (int rc = channel_parity_check("ldpc_frame_order", d)) return rc;
    const DevGraph &G = d->g->dg;
    if (!G.std_form || !G.a_packed || G.m > 65535)
        return ldpc_fail(LDPC_EINVAL, "ldpc_frame_order: graph is not [A | I_m] with m <= 65535");
    if (count == 0) return LDPC_OK;
    DeviceGuard dg(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure_order(d, count)) return rc;
    HIP_TRY(ldpc::launch_frame_order(G, seed, snr_point, sigma, frame0, count, d->ord_keys, d->ord_vals, d->ord,
                                     d->ord_tmp, d->ord_tmp_bytes, s));
    HIP_TRY(hipMemcpyAsync(order_out, d->ord, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return LDPC_OK;
}

int ldpc_mc_run(ldpc_decoder *d, uint64_t seed, int32_t n_points, const double *sigmas, int64_t frames_per_point,
                int64_t frame0, int32_t max_iter, uint32_t flags, int64_t *counters_out, void *stream) {
    if (!d || n_points <= 0 || !sigmas || frames_per_point < 0 || frame0 < 0 || max_iter < 1 || !counters_out)
        return ldpc_fail(LDPC_EINVAL, "ldpc_mc_run: bad arguments");
    if (int rc = channel_parity_check("ldpc_mc_run", d)) return rc;
    const DevGraph G = call_graph(d, flags);
    if (!G.std_form) return ldpc_fail(LDPC_EINVAL, "ldpc_mc_run: graph is not [A | I_m]");
    for (int p = 0; p < n_points; ++p)
        if (!(sigmas[p] > 0.0)) return ldpc_fail(LDPC_EINVAL, "ldpc_mc_run: sigma[%d] <= 0", p);
    DeviceGuard dg(d->g->device);
    if (d->ms_on) d->ms_state = 2;  // parity mode collects no statistics
    if (int rc0 = ensure_messages(d)) return rc0;
    hipStream_t s = (hipStream_t)stream;
    const bool nllr = flags & LDPC_F_NLLR;
    if (int rc = counters_begin(d, n_points, s)) return rc;
    const int64_t cap = (int64_t)d->cap_tiles * kTile;
    if (!(flags & LDPC_F_STATIC)) {
        for (int p = 0; p < n_points; ++p)
            if (int rc = mc_stream_point(d, G, seed, p, sigmas[p], frames_per_point, frame0, max_iter, nllr,
                                         flags & LDPC_F_SPLIT, s))
                return rc;
    } else {
        if (int rc = ensure_pbits(d, G)) return rc;
        for (int p = 0; p < n_points; ++p) {
            for (int64_t start = 0; start < frames_per_point; start += cap) {
                const int cnt = (int)std::min<int64_t>(cap, frames_per_point - start);
                state_bind(d, (cnt + kTile - 1) / kTile, cnt);
                HIP_TRY(ldpc::launch_reset(G, d->st, s));
                const DevState st = d->st;
                HIP_TRY(timed(d, LDPC_K_GEN, s,
                              [&] { return ldpc::launch_frames(G, st, phys_tile(d), seed, p, sigmas[p], frame0 + start,
                                                               ldpc::kFramesCh, nullptr, ldpc::FrameChannel{},
                                                               s); }));
                if (int rc = run_iterations(d, G, st, max_iter, nllr, s, true, flags & LDPC_F_SPLIT)) return rc;
                HIP_TRY(timed(d, LDPC_K_COUNT, s, [&] {
                    return ldpc::launch_count(G, st, d->counters + (size_t)p * LDPC_MC_NCOUNT, s);
                }));
            }
        }
    }
    return counters_read(d, n_points, counters_out, s);
}

int ldpc_rare_rows_read(ldpc_decoder *d, int64_t *out) {
    if (!d || !out) return ldpc_fail(LDPC_EINVAL, "ldpc_rare_rows_read: bad arguments");
    DeviceGuard dg(d->g->device);
    int h[2] = {0, 0};
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h, d->rare + 2, sizeof h, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(d->rare + 2, 0, sizeof h));
    out[0] = h[0];
    out[1] = h[1];
    return LDPC_OK;
}

int ldpc_fixed_point_read(ldpc_decoder *d, int64_t *out) {
    if (!d || !out) return ldpc_fail(LDPC_EINVAL, "ldpc_fixed_point_read: bad arguments");
    DeviceGuard dg(d->g->device);
    unsigned long long h[2] = {0, 0};
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h, d->rare + 4, sizeof h, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(d->rare + 4, 0, sizeof h));
    out[0] = (int64_t)h[0];
    out[1] = (int64_t)h[1];
    return LDPC_OK;
}

// ---------------------------------------------------------- physical mode
namespace {

int phys_grid(const DevGraph &G) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) cus = p.multiProcessorCount;
    }
    const size_t lds = ldpc::phys_lds_bytes(G) + 64;
    const int waves = ldpc::phys_block_threads(G) / 64;  // <= 32 waves / CU
    int per_cu = (int)std::min<size_t>(32 / waves, kLdsLimit / lds);
    if (per_cu < 1) per_cu = 1;
    return cus * per_cu;
}

// the layered kernel's grid, likewise: workgroups of phys_layered_threads
// resident per CU by LDS (E and L only) and by the 32-wave limit
int phys_layered_grid(const DevGraph &G, const PhysRule &rule) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) cus = p.multiProcessorCount;
    }
    const size_t lds = ldpc::phys_layered_lds_bytes(G) + 64;
    const int waves = ldpc::phys_layered_threads(rule) / 64;
    int per_cu = (int)std::min<size_t>(32 / waves, kLdsLimit / lds);
    // LDPC_LAYERED_PER_CU (read per launch): fewer workgroups per CU than fit (A/B)
    if (const char *e = getenv("LDPC_LAYERED_PER_CU")) per_cu = std::min(per_cu, atoi(e));
    if (per_cu < 1) per_cu = 1;
    return cus * per_cu;
}

// The graph's layer table on its device, built on the first call (any thread).
int graph_layers(const ldpc_graph *g, PhysRule *rule) {
    std::call_once(g->layers_once, [g] {
        const DevGraph &G = g->dg;
        std::vector<int> of_row(G.m);
        const int nl = first_fit_layers(G.m, G.n, g->h_row_ptr.data(), g->h_col_idx.data(), of_row.data());
        std::vector<int> tab((size_t)nl + 1 + G.m, 0);  // layer_ptr, then layer_rows (rows ascending in a layer)
        for (int r = 0; r < G.m; ++r) tab[of_row[r] + 1]++;
        int biggest = 0;
        for (int l = 0; l < nl; ++l) {
            biggest = std::max(biggest, tab[l + 1]);
            tab[l + 1] += tab[l];
        }
        std::vector<int> fill(tab.begin(), tab.begin() + nl);
        for (int r = 0; r < G.m; ++r) tab[(size_t)nl + 1 + fill[of_row[r]]++] = r;
        int *d = nullptr;
        hipError_t e = hipMalloc((void **)&d, sizeof(int) * tab.size());
        if (e == hipSuccess) e = hipMemcpy(d, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            g->layers_rc = LDPC_EDEVICE;
            g->layers_err = std::string("layer table upload failed: ") + hipGetErrorString(e);
            return;
        }
        g->d_layers = d;
        g->h_layer_ptr.assign(tab.begin(), tab.begin() + nl + 1);
        g->n_layers = nl;
        g->max_layer = biggest;
    });
    if (g->layers_rc) return ldpc_fail(g->layers_rc, "%s", g->layers_err.c_str());
    rule->layer_ptr = g->d_layers;
    rule->layer_rows = g->d_layers + g->n_layers + 1;
    rule->n_layers = g->n_layers;
    rule->max_layer = g->max_layer;
    rule->h_layer_ptr = g->h_layer_ptr.data();
    return LDPC_OK;
}

// Whether the layered schedule on graph P runs the HBM tile kernels.
bool layered_use_tile(const DevGraph &P, uint32_t flags) {
    return (flags & LDPC_F_LAYERED_TILE) || ldpc::phys_layered_lds_bytes(P) > kLdsLimit;
}

// Validate (cn_rule, schedule, param) for graph g and fill the kernels' rule;
// the layered schedule gets the graph's layer table (call with g's device current).
int phys_rule(const char *fn, const ldpc_graph *g, uint32_t flags, int32_t cn_rule, int32_t schedule, float param,
              PhysRule *rule) {
    if (cn_rule != LDPC_CN_SPA && cn_rule != LDPC_CN_NMS && cn_rule != LDPC_CN_OMS)
        return ldpc_fail(LDPC_EINVAL, "%s: unknown check-node rule %d", fn, cn_rule);
    if (schedule != LDPC_SCHED_FLOODING && schedule != LDPC_SCHED_LAYERED)
        return ldpc_fail(LDPC_EINVAL, "%s: unknown schedule %d", fn, schedule);
    if (cn_rule == LDPC_CN_NMS && !(param > 0.0f && param <= 1.0f))
        return ldpc_fail(LDPC_EINVAL, "%s: normalized min-sum needs alpha in (0, 1], got %g", fn, (double)param);
    if (cn_rule == LDPC_CN_OMS && !(param >= 0.0f))
        return ldpc_fail(LDPC_EINVAL, "%s: offset min-sum needs beta >= 0, got %g", fn, (double)param);
    if (cn_rule == LDPC_CN_SPA && schedule == LDPC_SCHED_LAYERED)
        return ldpc_fail(LDPC_EINVAL, "%s: the layered schedule is not implemented for the sum-product rule "
                                      "(use LDPC_CN_NMS or LDPC_CN_OMS)", fn);
    if (cn_rule != LDPC_CN_SPA && g->min_row_deg < 2)
        return ldpc_fail(LDPC_EINVAL, "%s: min-sum needs every check row to have at least 2 edges (a row has %d)",
                         fn, g->min_row_deg);
    if ((flags & LDPC_F_LAYERED_TILE) && schedule != LDPC_SCHED_LAYERED)
        return ldpc_fail(LDPC_EINVAL, "%s: LDPC_F_LAYERED_TILE needs LDPC_SCHED_LAYERED", fn);
    if (flags & LDPC_F_QUANT_TILE)
        return ldpc_fail(LDPC_EINVAL, "%s: LDPC_F_QUANT_TILE belongs to the fixed-point entries "
                                      "(ldpc_phys_decode_q, ldpc_phys_mc_run_q)", fn);
    *rule = PhysRule{};
    rule->cn = cn_rule;
    rule->param = cn_rule == LDPC_CN_SPA ? 0.0f : param;
    if (schedule == LDPC_SCHED_LAYERED) {
        if (flags & LDPC_F_PHYS_HBM)
            return ldpc_fail(LDPC_ERANGE, "%s: LDPC_F_PHYS_HBM selects the flooding tile kernels; the layered "
                                          "schedule's HBM path is LDPC_F_LAYERED_TILE", fn);
        // the HBM tile kernels on request, and for a graph too large for LDS
        rule->layered_tile = layered_use_tile(g->dg, flags);
        return graph_layers(g, rule);
    }
    return LDPC_OK;
}


}  // namespace

int64_t ldpc_phys_lds_bytes(const ldpc_graph *g) { return g ? (int64_t)ldpc::phys_lds_bytes(g->dg) : -1; }

extern "C++" {  // the function templates below cannot have C linkage
namespace {

// A one-shot decode by one launch: `launch(llr, z, ints, post)` gets device
// pointers, ints[k] the k-th of the per-frame integer outputs ints_out (3 or 4).
// With LDPC_F_DEVICE_PTRS those are the caller's own; otherwise the LLRs are
// staged up, and what the caller asked for (non-null) is copied back before a sync.
template <class Post, class Launch>
int phys_decode_staged(const char *fn, const DevGraph &G, int32_t batch, const double *llr, uint32_t flags,
                       uint8_t *z_out, std::initializer_list<int32_t *> ints_out, Post *post_out, hipStream_t s,
                       Launch &&launch) {
    if (flags & LDPC_F_DEVICE_PTRS) {
        HIP_TRY(launch(llr, z_out, ints_out.begin(), post_out));
        return LDPC_OK;
    }
    const size_t n = (size_t)G.n, B = (size_t)batch, n_ints = ints_out.size();
    double *d_llr = nullptr;
    uint8_t *d_z = nullptr;
    int *d_i = nullptr;
    Post *d_post = nullptr;
    int rc = dev_alloc(&d_llr, B * n);
    if (!rc) rc = dev_alloc(&d_z, B * n);
    if (!rc) rc = dev_alloc(&d_i, n_ints * B);
    if (!rc && post_out) rc = dev_alloc(&d_post, B * n);
    hipError_t e = hipSuccess;
    if (!rc) {
        int *const d_ints[4] = {d_i, d_i + B, d_i + 2 * B, d_i + 3 * B};  // n_ints of them exist
        e = hipMemcpyAsync(d_llr, llr, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
        if (!e) e = launch(d_llr, d_z, d_ints, d_post);
        if (!e && z_out) e = hipMemcpyAsync(z_out, d_z, B * n, hipMemcpyDeviceToHost, s);
        for (size_t k = 0; k < n_ints; ++k)
            if (int32_t *out = ints_out.begin()[k]; !e && out)
                e = hipMemcpyAsync(out, d_ints[k], sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (!e && post_out) e = hipMemcpyAsync(post_out, d_post, sizeof(Post) * B * n, hipMemcpyDeviceToHost, s);
        if (!e) e = hipStreamSynchronize(s);
        if (e) rc = ldpc_fail(LDPC_EDEVICE, "%s: %s", fn, hipGetErrorString(e));
    }
    (void)hipFree(d_llr);
    (void)hipFree(d_z);
    (void)hipFree(d_i);
    (void)hipFree(d_post);
    return rc;
}

// the running counts the tile kernels keep for the host: [2 max_iter] tiles, then frames
int ensure_pactive(ldpc_decoder *d, int max_iter) {
    if (d->pactive_cap >= 2 * max_iter) return LDPC_OK;
    (void)hipFree(d->pactive);
    d->pactive = nullptr;
    d->pactive_cap = 0;
    if (int rc = dev_alloc(&d->pactive, 2 * (size_t)max_iter)) return rc;
    d->pactive_cap = 2 * max_iter;
    return LDPC_OK;
}

// LDPC_PHYS_COMPACT=0: no compaction (A/B, diagnosis; the counters are the same)
bool phys_compact_enabled() {
    const char *e = getenv("LDPC_PHYS_COMPACT");
    return !e || atoi(e) != 0;
}

// Monte-Carlo statistics: start of a physical run.  Clears what the last run
// left and, when enabled, sizes and zeroes the device arrays for this one.
int mc_stats_begin(ldpc_decoder *d, int n_points, int max_iter, bool tiles, hipStream_t s) {
    d->ms_state = 0;
    if (!d->ms_on) return LDPC_OK;
    const size_t words = ldpc::mc_stats_words(n_points, max_iter, d->ms_max_failed);
    if (d->ms_words < words) {
        (void)hipFree(d->ms_buf);
        d->ms_buf = nullptr;
        d->ms_words = 0;
        if (int rc = dev_alloc(&d->ms_buf, words)) return rc;
        d->ms_words = words;
    }
    const size_t cap = (size_t)d->cap_tiles * kTile;
    if (tiles && !d->ms_slots)
        if (int rc = dev_alloc(&d->ms_slots, cap)) return rc;
    if (tiles && !d->ms_tile)
        if (int rc = dev_alloc(&d->ms_tile, cap + (size_t)d->cap_tiles)) return rc;
    if (tiles) HIP_TRY(hipMemsetAsync(d->ms_tile, 0, sizeof(int) * (cap + (size_t)d->cap_tiles), s));
    HIP_TRY(hipMemsetAsync(d->ms_buf, 0, sizeof(unsigned long long) * words, s));
    d->ms_points = n_points;
    d->ms_T = max_iter;
    d->ms_run_failed = d->ms_max_failed;
    return LDPC_OK;
}

// The kernels' view of point p of the run mc_stats_begin prepared (off: all null).
void mc_stats_point(const ldpc_decoder *d, int p, int64_t frame_base, ldpc::McStats *out) {
    ldpc::McStats &ms = *out;
    ms = ldpc::McStats{};
    if (!d->ms_on) return;
    const size_t pw = ldpc::mc_stats_point_words(d->ms_T);
    unsigned long long *head = d->ms_buf + (size_t)p * pw;
    ms.und = head;
    ms.hist = head + ldpc::kMcStatsHead;
    ms.failed = reinterpret_cast<long long *>(d->ms_buf + (size_t)d->ms_points * pw) +
                (size_t)p * 2 * (size_t)d->ms_run_failed;
    ms.slot_frame = d->ms_slots;
    ms.slot_err = d->ms_tile;
    ms.tile_arrive = d->ms_tile ? d->ms_tile + (size_t)d->cap_tiles * kTile : nullptr;
    ms.frame_base = frame_base;
    ms.max_failed = d->ms_run_failed;
    ms.max_iter = d->ms_T;
}

// Decode the frames bound in d->st with HBM-resident tile kernels, a family's
// own behind `ops` (TileOps: PhysTileOps, QTileOps): up to max_iter sweeps, then what
// the family needs to finish.  The host reads the running-tile and
// running-frame counts after sweep(it) for it < 4 and every 4th iteration
// after, and stops issuing sweeps once they are zero.  With ops.ctr (a
// Monte-Carlo run: only the counters leave the device) the running frames are
// compacted into the first tiles once at most a quarter of the launched slots
// hold them, the finished frames counted into ctr first (phys_tile_state.hip), and
// the rest at the end.  ops.st is the family's copy of d->st: its ntiles
// shrinks with each compaction.
template <class Ops>
int phys_tile_sweeps(ldpc_decoder *d, int max_iter, hipStream_t s, Ops &&ops) {
    if (int rc = ensure_pactive(d, max_iter)) return rc;
    const int cap = d->cap_tiles * kTile;
    const bool compact = phys_compact_enabled();
    HIP_TRY(hipMemsetAsync(d->pactive, 0, sizeof(int) * 2 * max_iter, s));
    HIP_TRY(ops.init());
    for (int it = 0; it < max_iter; ++it) {
        HIP_TRY(ops.sweep(it));
        if (it + 1 < max_iter && (it < 4 || (it + 1) % 4 == 0)) {
            // iterations 1 and 2 (flooding): the frames whose posterior already
            // satisfies every check stop now instead of after the next CN
            // sweep (DVB-S2 profile at 1 dB, 2 iterations per frame: +25 %).
            // Each early syndrome costs ~1 ms on 128 tiles, more than it saves
            // where frames stop after 20-40 iterations (the -2.5 dB
            // waterfall: -1.4 % with it at every poll of it < 4,
            // profiles/r5_ab/r5ao_ab)
            if (!ops.layered() && (it == 1 || it == 2))
                HIP_TRY(timed(d, LDPC_K_PHYS_VN, s, [&] { return ops.early_exit(it); }));
            int running[2] = {0, 0};  // tiles, frames
            HIP_TRY(hipMemcpyAsync(&running[0], d->pactive + it, sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(&running[1], d->pactive + max_iter + it, sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (running[0] == 0) break;  // every frame has stopped (converged; finish() leaves them alone)
            const int nt = (running[1] + kTile - 1) / kTile;
            // (a quarter: half measured the same, profiles/r5_ab/r5am_ab)
            if (ops.ctr && compact && nt < ops.st.ntiles &&
                4 * (int64_t)running[1] <= (int64_t)ops.st.ntiles * kTile) {
                if (!d->cpairs && dev_alloc(&d->cpairs, 1 + 2 * (size_t)cap)) return LDPC_ENOMEM;
                HIP_TRY(timed(d, LDPC_K_COUNT, s, [&] { return ops.count(); }));
                HIP_TRY(ops.compact(nt));
                ops.st.ntiles = nt;
            }
        }
    }
    HIP_TRY(ops.finish());
    if (ops.ctr) {  // the frames no compaction counted, over all of the chunk's tiles again
        ops.st.ntiles = d->st.ntiles;
        HIP_TRY(timed(d, LDPC_K_COUNT, s, [&] { return ops.count(); }));
    }
    return LDPC_OK;
}

// What phys_tile_sweeps runs, once for both families: the layers of an
// iteration, a sweep with its two timed brackets, and the bookkeeping of
// phys_tile_state.hip -- early exit, count, compaction, the end.  Self (CRTP)
// adds what differs: `t` (a PhysTile / QTile: E, L, Lam, bad, cap), `rule`
// (layer_ptr set: layered), init(), layer(it, lbeg, lrows), cn(it), vn(it) and
// the flooding syndromes early_syn(it) -> bad[(it+1)&1] and last_syn() ->
// bad[max_iter&1].  Layered: per iteration one launch per layer, in order on
// the stream, then the syndrome of b = (L < 0) and the exits -- on the device
// every iteration, so the results never depend on the polls; the exit of
// iteration max_iter - 1 stops the frames still running (no final sweep).
template <class Self>
struct TileOps {
    ldpc_decoder *d;
    const DevGraph &P;
    DevState st;
    int max_iter;
    hipStream_t s;
    unsigned long long *ctr;
    const ldpc::McStats &ms;

    Self &self() { return static_cast<Self &>(*this); }
    bool layered() { return self().rule.layer_ptr != nullptr; }
    hipError_t layers(int it) {
        const auto &rule = self().rule;
        for (int l = 0; l < rule.n_layers; ++l) {
            const int lbeg = rule.h_layer_ptr[l], lrows = rule.h_layer_ptr[l + 1] - lbeg;
            if (hipError_t e = self().layer(it, lbeg, lrows)) return e;
        }
        return hipSuccess;
    }
    hipError_t sweep(int it) {
        const auto &t = self().t;
        if (hipError_t e = timed(d, LDPC_K_PHYS_CN, s, [&] { return layered() ? layers(it) : self().cn(it); }))
            return e;
        return timed(d, LDPC_K_PHYS_VN, s, [&] {
            return layered() ? ldpc::launch_phys_layer_exit(P, st, t.L, t.bad, t.cap, it, d->pactive, max_iter, s)
                             : self().vn(it);
        });
    }
    hipError_t early_exit(int it) {  // flooding only
        if (hipError_t e = self().early_syn(it)) return e;
        return ldpc::launch_phys_tile_exit(st, self().t.bad, self().t.cap, it, d->pactive, max_iter, s);
    }
    hipError_t count() { return ldpc::launch_phys_tile_count(P, st, self().t.L, ctr, s, ms); }
    hipError_t compact(int nt) {
        const auto &t = self().t;
        return ldpc::launch_phys_compact(P, st, t.E, t.L, t.Lam, t.bad, nt, d->cap_tiles * kTile, d->cpairs, s,
                                         ms.hist ? ms.slot_frame : nullptr);
    }
    hipError_t finish() {  // flooding: the frames that converge on the last iteration
        if (layered()) return hipSuccess;
        if (hipError_t e = self().last_syn()) return e;
        return ldpc::launch_phys_tile_final(st, self().t.bad, self().t.cap, max_iter, s);
    }
};

// The fp32 tile kernels (phys_tile.hip), channel LLRs in d->ch (from_ch) or
// the generator's Lambda tiles.  Flooding: a CN and a VN sweep per iteration;
// the early syndrome comes from the VN sweep's hard-decision bytes, the last
// one from a syndrome-only CN sweep.
struct PhysTileOps : TileOps<PhysTileOps> {
    PhysTile t;
    bool from_ch;
    const PhysRule &rule;

    hipError_t init() { return ldpc::launch_phys_tile_init(P, st, t, from_ch, s); }
    hipError_t layer(int it, int lbeg, int lrows) {
        return ldpc::launch_phys_layer_tile(P, st, t, it, lbeg, lrows, s, rule);
    }
    hipError_t cn(int it) { return ldpc::launch_phys_tile_cn(P, st, t, it, false, s, rule); }
    hipError_t vn(int it) { return ldpc::launch_phys_tile_vn(P, st, t, it, d->pactive, max_iter, s); }
    hipError_t early_syn(int it) { return ldpc::launch_phys_tile_syn(P, st, t, it, s); }
    hipError_t last_syn() { return ldpc::launch_phys_tile_cn(P, st, t, max_iter, true, s, rule); }
};

int phys_tile_decode(ldpc_decoder *d, const DevGraph &P, int max_iter, bool from_ch, hipStream_t s,
                     unsigned long long *ctr, const PhysRule &rule, const ldpc::McStats &ms = ldpc::McStats{}) {
    return phys_tile_sweeps(d, max_iter, s,
                            PhysTileOps{{d, P, d->st, max_iter, s, ctr, ms}, phys_tile(d), from_ch, rule});
}

// Whether a rule phys_rule filled runs one LDS kernel on graph P, not the HBM tile kernels.
bool phys_on_lds(const PhysRule &rule, const DevGraph &P, uint32_t flags) {
    return rule.layer_ptr ? !rule.layered_tile : phys_use_lds(P, flags);
}

// A one-shot decode on the tiles: chunks of 1024 frames through a temporary
// decoder's workspace and staging.  `decode(d)` decodes the chunk bound in
// d->st (channel LLRs in d->ch) and returns an rc; `out(d, z, post)` launches
// the kernel that writes the hard decisions and posteriors to device memory.
template <class Post, class Decode, class Out>
int phys_decode_chunks(const ldpc_graph *g, int32_t batch, const double *llr, uint32_t flags, uint8_t *z_out,
                       int32_t *conv_out, int32_t *status_out, int32_t *iters_out, Post *post_out, hipStream_t s,
                       Decode &&decode, Out &&out) {
    const DevGraph &G = g->dg;
    const bool dev_ptrs = flags & LDPC_F_DEVICE_PTRS;
    const int chunk = std::min<int>(batch, 1024);
    ldpc_decoder *d = nullptr;
    if (int rc = ldpc_decoder_create(g, chunk, &d)) return rc;
    struct Free {
        ldpc_decoder *d;
        ~Free() { ldpc_decoder_destroy(d); }
    } guard{d};
    if (int rc = ensure_phys_tile(d, G)) return rc;
    const size_t n = (size_t)G.n;
    for (int start = 0; start < batch; start += chunk) {
        const int cnt = std::min(chunk, batch - start);
        state_bind(d, (cnt + kTile - 1) / kTile, cnt);
        const DevState &st = d->st;
        const double *src = llr + (size_t)start * n;
        if (!dev_ptrs) {
            HIP_TRY(hipMemcpyAsync(d->llr_stage, src, sizeof(double) * cnt * n, hipMemcpyHostToDevice, s));
            src = d->llr_stage;
        }
        HIP_TRY(ldpc::launch_load_llr(G, st, src, s));
        if (int rc = decode(d)) return rc;
        uint8_t *zd = z_out ? (dev_ptrs ? z_out + (size_t)start * n : d->z_stage) : nullptr;
        Post *pd = post_out ? (dev_ptrs ? post_out + (size_t)start * n : (Post *)d->post_stage) : nullptr;
        HIP_TRY(out(d, zd, pd));
        const hipMemcpyKind kind = dev_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (conv_out) HIP_TRY(hipMemcpyAsync(conv_out + start, st.conv, sizeof(int) * cnt, kind, s));
        if (status_out) HIP_TRY(hipMemcpyAsync(status_out + start, st.status, sizeof(int) * cnt, kind, s));
        if (iters_out) HIP_TRY(hipMemcpyAsync(iters_out + start, st.iters, sizeof(int) * cnt, kind, s));
        if (!dev_ptrs) {
            if (z_out) HIP_TRY(hipMemcpyAsync(z_out + (size_t)start * n, zd, cnt * n, hipMemcpyDeviceToHost, s));
            if (post_out)
                HIP_TRY(hipMemcpyAsync(post_out + (size_t)start * n, pd, sizeof(Post) * cnt * n,
                                       hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s));  // staging and workspace are reused / freed
    }
    return LDPC_OK;
}

int phys_decode_any(const char *fn, const ldpc_graph *g, int32_t batch, const double *llr, int32_t max_iter,
                    uint32_t flags, int32_t cn_rule, int32_t schedule, float param, uint8_t *z_out, int32_t *conv_out,
                    int32_t *status_out, int32_t *iters_out, float *post_out, void *stream) {
    if (!g) return ldpc_fail(LDPC_EINVAL, "%s: NULL graph", fn);
    if (batch < 0 || max_iter < 1 || (batch > 0 && !llr))
        return ldpc_fail(LDPC_EINVAL, "%s: bad arguments (batch=%d max_iter=%d)", fn, batch, max_iter);
    DeviceGuard dg(g->device);
    PhysRule rule;
    if (int rc = phys_rule(fn, g, flags, cn_rule, schedule, param, &rule)) return rc;
    if (batch == 0) return LDPC_OK;
    hipStream_t s = (hipStream_t)stream;
    const DevGraph &G = g->dg;
    if (phys_on_lds(rule, G, flags))  // flooding (any rule) or, with a layer table, the layered kernel
        return phys_decode_staged(
            fn, G, batch, llr, flags, z_out, {conv_out, status_out, iters_out}, post_out, s,
            [&](const double *in, uint8_t *z, int *const *iv, float *post) {
                if (rule.layer_ptr)
                    return ldpc::launch_phys_layered(G, in, nullptr, 0, batch, max_iter, z, iv[0], iv[1], iv[2], post,
                                                     nullptr, nullptr, std::min(phys_layered_grid(G, rule), batch), s,
                                                     rule);
                return ldpc::launch_phys(G, in, nullptr, 0, batch, max_iter, z, iv[0], iv[1], iv[2], post, nullptr,
                                         nullptr, std::min(phys_grid(G), batch), s, rule);
            });
    return phys_decode_chunks(
        g, batch, llr, flags, z_out, conv_out, status_out, iters_out, post_out, s,
        [&](ldpc_decoder *d) { return phys_tile_decode(d, G, max_iter, true, s, nullptr, rule); },
        [&](ldpc_decoder *d, uint8_t *z, float *post) {
            return ldpc::launch_phys_tile_out(G, d->st, phys_tile(d).L, z, post, s);
        });
}

// The argument checks every physical-mode Monte-Carlo entry shares; they touch
// no device.  d decodes graph gp (P below) on frames of its own graph (G).
int phys_mc_check(const char *fn, const ldpc_decoder *d, const ldpc_graph *gp, int32_t n_points, const double *sigmas,
                  int64_t frames_per_point, int64_t frame0, int32_t max_iter, const int64_t *counters_out) {
    if (!gp) return ldpc_fail(LDPC_EINVAL, "%s: NULL graph", fn);
    if (!d || n_points <= 0 || !sigmas || frames_per_point < 0 || frame0 < 0 || max_iter < 1 || !counters_out)
        return ldpc_fail(LDPC_EINVAL, "%s: bad arguments", fn);
    const DevGraph &G = d->g->dg;
    const DevGraph &P = gp->dg;
    if (!G.std_form && !(G.ira && d->g == gp))
        return ldpc_fail(LDPC_EINVAL,
                         "%s: the decoder's graph must be the code's H_std = [A | I_m], or the "
                         "IRA graph itself", fn);
    if (P.n != G.n || P.k != G.k)
        return ldpc_fail(LDPC_EINVAL, "%s: physical graph shape %dx%d != %dx%d", fn, P.m, P.n, G.m, G.n);
    for (int p = 0; p < n_points; ++p)
        if (!(sigmas[p] > 0.0)) return ldpc_fail(LDPC_EINVAL, "%s: sigma[%d] <= 0", fn, p);
    return channel_frames_check(fn, d, 0);
}

// A physical-mode Monte-Carlo run on a decoder phys_mc_check passed, its
// device current, in chunks of the decoder's capacity.  The frames go straight
// to the family's decoder as fp32 Lambda: kFramesRowLambda (rows, contiguous
// per frame) for an LDS kernel, kFramesTileLambda (pLam) for the HBM tile
// kernels (tiles).  `chunk(st, cnt, rows, ctr, ms)` decodes the cnt frames
// bound in st and counts them into the point's counters ctr; it returns an rc.
template <class Chunk>
int phys_mc_drive(ldpc_decoder *d, uint64_t seed, int32_t n_points, const double *sigmas, int64_t frames_per_point,
                  int64_t frame0, int32_t max_iter, int64_t *counters_out, hipStream_t s, ldpc::FramesOut layout,
                  bool tiles, Chunk &&chunk) {
    const DevGraph &G = d->g->dg;
    if (int rc = ensure_pbits(d, G)) return rc;
    ldpc::RateMatchDev rm;
    if (int rc = rate_match_dev(d, s, &rm)) return rc;
    ldpc::HarqDev hq;
    if (int rc = harq_dev(d, s, &hq)) return rc;
    if (int rc = counters_begin(d, n_points, s)) return rc;
    if (int rc = mc_stats_begin(d, n_points, max_iter, tiles, s)) return rc;
    const int64_t cap = (int64_t)d->cap_tiles * kTile;
    for (int p = 0; p < n_points; ++p) {
        unsigned long long *ctr = d->counters + (size_t)p * LDPC_MC_NCOUNT;
        for (int64_t start = 0; start < frames_per_point; start += cap) {
            const int cnt = (int)std::min<int64_t>(cap, frames_per_point - start);
            state_bind(d, (cnt + kTile - 1) / kTile, cnt);
            const DevState st = d->st;
            ldpc::McStats ms;
            mc_stats_point(d, p, frame0 + start, &ms);
            float *rows = (float *)d->llr_stage;  // cap x n doubles: room for cap x n floats
            HIP_TRY(timed(d, LDPC_K_GEN, s, [&] {
                return ldpc::launch_frames(G, st, phys_tile(d), seed, p, sigmas[p], frame0 + start, layout, rows,
                                           frame_channel(d), s, rm, hq);
            }));
            if (tiles && ms.hist) HIP_TRY(ldpc::launch_mc_stats_slots(ms.slot_frame, ms.frame_base, cnt, s));
            if (int rc = chunk(st, cnt, rows, ctr, ms)) return rc;
        }
    }
    if (int rc = counters_read(d, n_points, counters_out, s)) return rc;
    if (d->ms_on) d->ms_state = 1;
    return LDPC_OK;
}

int phys_mc_any(const char *fn, ldpc_decoder *d, const ldpc_graph *gp, uint64_t seed, int32_t n_points,
                const double *sigmas, int64_t frames_per_point, int64_t frame0, int32_t max_iter, uint32_t flags,
                int32_t cn_rule, int32_t schedule, float param, int64_t *counters_out, void *stream) {
    if (int rc = phys_mc_check(fn, d, gp, n_points, sigmas, frames_per_point, frame0, max_iter, counters_out))
        return rc;
    const DevGraph &P = gp->dg;
    DeviceGuard dg(d->g->device);
    PhysRule rule;
    if (int rc = phys_rule(fn, gp, flags, cn_rule, schedule, param, &rule)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool lds = phys_on_lds(rule, P, flags);
    if (!lds)
        if (int rc = ensure_phys_tile(d, P)) return rc;
    return phys_mc_drive(
        d, seed, n_points, sigmas, frames_per_point, frame0, max_iter, counters_out, s,
        lds ? ldpc::kFramesRowLambda : ldpc::kFramesTileLambda, !lds,
        [&](const DevState &st, int cnt, const float *rows, unsigned long long *ctr, const ldpc::McStats &ms) -> int {
            if (!lds) return phys_tile_decode(d, P, max_iter, false, s, ctr, rule, ms);
            HIP_TRY(timed(d, LDPC_K_PHYS, s, [&] {
                if (rule.layer_ptr)
                    return ldpc::launch_phys_layered(P, nullptr, rows, 2, cnt, max_iter, nullptr, nullptr, nullptr,
                                                     nullptr, nullptr, st.ubits, ctr,
                                                     std::min(phys_layered_grid(P, rule), cnt), s, rule, ms);
                return ldpc::launch_phys(P, nullptr, rows, 2, cnt, max_iter, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, st.ubits, ctr, std::min(phys_grid(P), cnt), s, rule, ms);
            }));
            return LDPC_OK;
        });
}

}  // namespace
}  // extern "C++"

int ldpc_phys_decode(const ldpc_graph *g, int32_t batch, const double *llr, int32_t max_iter, uint32_t flags,
                     uint8_t *z_out, int32_t *conv_out, int32_t *status_out, int32_t *iters_out, float *post_out,
                     void *stream) {
    return phys_decode_any("ldpc_phys_decode", g, batch, llr, max_iter, flags, LDPC_CN_SPA, LDPC_SCHED_FLOODING, 0.0f,
                           z_out, conv_out, status_out, iters_out, post_out, stream);
}

int ldpc_phys_decode_ex(const ldpc_graph *g, int32_t batch, const double *llr, int32_t max_iter, uint32_t flags,
                        int32_t cn_rule, int32_t schedule, float param, uint8_t *z_out, int32_t *conv_out,
                        int32_t *status_out, int32_t *iters_out, float *post_out, void *stream) {
    return phys_decode_any("ldpc_phys_decode_ex", g, batch, llr, max_iter, flags, cn_rule, schedule, param, z_out,
                           conv_out, status_out, iters_out, post_out, stream);
}

int ldpc_phys_mc_run(ldpc_decoder *d, const ldpc_graph *gp, uint64_t seed, int32_t n_points, const double *sigmas,
                     int64_t frames_per_point, int64_t frame0, int32_t max_iter, uint32_t flags, int64_t *counters_out,
                     void *stream) {
    return phys_mc_any("ldpc_phys_mc_run", d, gp, seed, n_points, sigmas, frames_per_point, frame0, max_iter, flags,
                       LDPC_CN_SPA, LDPC_SCHED_FLOODING, 0.0f, counters_out, stream);
}

int ldpc_phys_mc_run_ex(ldpc_decoder *d, const ldpc_graph *gp, uint64_t seed, int32_t n_points, const double *sigmas,
                        int64_t frames_per_point, int64_t frame0, int32_t max_iter, uint32_t flags, int32_t cn_rule,
                        int32_t schedule, float param, int64_t *counters_out, void *stream) {
    return phys_mc_any("ldpc_phys_mc_run_ex", d, gp, seed, n_points, sigmas, frames_per_point, frame0, max_iter, flags,
                       cn_rule, schedule, param, counters_out, stream);
}

// ------------------------------------- physical mode, fixed-point min-sum
namespace {

// Padded message bytes of a frame: every row's messages start 4-byte aligned.
int quant_epad(const ldpc_graph *g) {
    int64_t epad = 0;
    for (int r = 0; r < g->dg.m; ++r) epad += (g->h_row_ptr[r + 1] - g->h_row_ptr[r] + 3) & ~3;
    return (int)std::min<int64_t>(epad, INT_MAX / 2);
}

// Whether the quantized state of a frame fits LDS (and 16-bit column indices).
bool quant_fits(const ldpc_graph *g, bool layered) {
    return g->dg.n < 65535 && ldpc::phys_quant_lds_bytes(g->dg, quant_epad(g), layered) <= kLdsLimit;
}

// Whether the fixed-point entries run the HBM tile kernels (phys_qtile.hip): on
// request, and for a graph whose quantized state does not fit LDS.
bool quant_use_tile(const ldpc_graph *g, uint32_t flags, int32_t schedule) {
    return (flags & LDPC_F_QUANT_TILE) || !quant_fits(g, schedule == LDPC_SCHED_LAYERED);
}

// The argument checks of the quantized entries; they touch no device.
int quant_check(const char *fn, const ldpc_graph *g, uint32_t flags, int32_t cn_rule, int32_t schedule, int32_t qbits,
                float llr_scale, int32_t param_q) {
    if (cn_rule == LDPC_CN_SPA)
        return ldpc_fail(LDPC_EINVAL, "%s: cn_rule LDPC_CN_SPA has no fixed-point form (use LDPC_CN_NMS or "
                                      "LDPC_CN_OMS)", fn);
    if (cn_rule != LDPC_CN_NMS && cn_rule != LDPC_CN_OMS)
        return ldpc_fail(LDPC_EINVAL, "%s: unknown cn_rule %d", fn, cn_rule);
    if (schedule != LDPC_SCHED_FLOODING && schedule != LDPC_SCHED_LAYERED)
        return ldpc_fail(LDPC_EINVAL, "%s: unknown schedule %d", fn, schedule);
    if (qbits < 4 || qbits > 8) return ldpc_fail(LDPC_EINVAL, "%s: qbits must be in 4..8, got %d", fn, qbits);
    if (!(llr_scale > 0.0f) || !(llr_scale <= FLT_MAX))
        return ldpc_fail(LDPC_EINVAL, "%s: llr_scale must be finite and > 0, got %g", fn, (double)llr_scale);
    const int qmax = (1 << (qbits - 1)) - 1;
    if (cn_rule == LDPC_CN_NMS && (param_q < 1 || param_q > 16))
        return ldpc_fail(LDPC_EINVAL, "%s: param_q (alpha_q, sixteenths) must be in 1..16, got %d", fn, param_q);
    if (cn_rule == LDPC_CN_OMS && (param_q < 0 || param_q > qmax))
        return ldpc_fail(LDPC_EINVAL, "%s: param_q (beta_q, quantizer steps) must be in 0..%d at qbits %d, got %d",
                         fn, qmax, qbits, param_q);
    if (g->min_row_deg < 2)
        return ldpc_fail(LDPC_EINVAL, "%s: min-sum needs every check row to have at least 2 edges (a row has %d)",
                         fn, g->min_row_deg);
    if (flags & (LDPC_F_PHYS_HBM | LDPC_F_LAYERED_TILE))
        return ldpc_fail(LDPC_ERANGE, "%s: LDPC_F_PHYS_HBM and LDPC_F_LAYERED_TILE select the fp32 tile kernels; "
                                      "the fixed-point decoder's HBM path is LDPC_F_QUANT_TILE", fn);
    return LDPC_OK;
}

// The graph's padded message layout on its device, built on the first call (any thread).
int graph_quant_tab(const ldpc_graph *g, ldpc::QuantTab *tab) {
    std::call_once(g->qtab_once, [g] {
        const DevGraph &G = g->dg;
        const int epad = quant_epad(g);
        std::vector<int> row(2 * (size_t)G.m), csc(G.nnz), fill(G.n + 1, 0);
        std::vector<uint16_t> col((size_t)epad, (uint16_t)G.n);  // padding: the dummy posterior L[n]
        for (int e = 0; e < G.nnz; ++e) fill[g->h_col_idx[e] + 1]++;
        for (int j = 0; j < G.n; ++j) fill[j + 1] += fill[j];  // = csc_ptr; rows ascending within a column below
        int off = 0;
        for (int r = 0; r < G.m; ++r) {
            const int b = g->h_row_ptr[r], deg = g->h_row_ptr[r + 1] - b;
            row[2 * (size_t)r] = off;
            row[2 * (size_t)r + 1] = deg;
            for (int i = 0; i < deg; ++i) {
                const int c = g->h_col_idx[b + i];
                col[off + i] = (uint16_t)c;
                csc[fill[c]++] = off + i;
            }
            off += (deg + 3) & ~3;
        }
        // the column table right after the rows: it is read 8 bytes at a time (hipMalloc aligns to 256
        // bytes, row_bytes is a multiple of 8 and a row's slots start at a multiple of 4)
        const size_t row_bytes = sizeof(int) * row.size(), col_bytes = sizeof(uint16_t) * col.size();
        char *d = nullptr;
        hipError_t e = hipMalloc((void **)&d, row_bytes + col_bytes + sizeof(int) * csc.size());
        if (e == hipSuccess) e = hipMemcpy(d, row.data(), row_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d + row_bytes, col.data(), col_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(d + row_bytes + col_bytes, csc.data(), sizeof(int) * csc.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            g->qtab_rc = LDPC_EDEVICE;
            g->qtab_err = std::string("quantized layout upload failed: ") + hipGetErrorString(e);
            return;
        }
        g->d_qtab = d;
        g->qtab.row = reinterpret_cast<const int2 *>(d);
        g->qtab.col = reinterpret_cast<const uint16_t *>(d + row_bytes);
        g->qtab.csc = reinterpret_cast<const int *>(d + row_bytes + col_bytes);
        g->qtab.epad = epad;
    });
    if (g->qtab_rc) return ldpc_fail(g->qtab_rc, "%s", g->qtab_err.c_str());
    *tab = g->qtab;
    return LDPC_OK;
}

// Fill the kernel's rule (device tables: call with g's device current, after quant_check).
int quant_rule(const ldpc_graph *g, uint32_t flags, int32_t cn_rule, int32_t schedule, int32_t qbits, float llr_scale,
               int32_t param_q, ldpc::QuantRule *rule) {
    *rule = ldpc::QuantRule{};
    rule->cn = cn_rule;
    rule->qbits = qbits;
    rule->scale = llr_scale;
    rule->param_q = param_q;
    rule->tile = quant_use_tile(g, flags, schedule);
    // the tile path reads the graph's CSR / CSC itself: no padded table
    if (!rule->tile)
        if (int rc = graph_quant_tab(g, &rule->tab)) return rc;
    if (schedule == LDPC_SCHED_LAYERED) {
        PhysRule pr;
        if (int rc = graph_layers(g, &pr)) return rc;
        rule->layer_ptr = pr.layer_ptr;
        rule->layer_rows = pr.layer_rows;
        rule->n_layers = pr.n_layers;
        rule->max_layer = pr.max_layer;
        rule->h_layer_ptr = pr.h_layer_ptr;
    }
    return LDPC_OK;
}

// LDPC_PHYS_Q_GRID=<workgroups> (read per launch) caps the grid launch_phys_quant
// picks (the workgroups the device holds at once): one workgroup then decodes
// many frames in sequence (tests of LDS reuse, A/B).
int phys_quant_max_grid() {
    if (const char *e = getenv("LDPC_PHYS_Q_GRID")) {
        const int cap = atoi(e);
        if (cap > 0) return cap;
    }
    return INT_MAX;
}

// The fixed-point state on the tiles, in the bytes of the fp32 tile path's
// workspace (ensure_phys_tile; nothing more is allocated): E8 in pE (a quarter
// of it), L16 in the first half of pL and Lam8 in its third quarter.  pLam
// stays free for the generator's fp32 Lambda tiles, which the load reads.
ldpc::QTile quant_tile(ldpc_decoder *d, const ldpc::QuantRule &rule) {
    const size_t cap = (size_t)d->cap_tiles * kTile, n = (size_t)d->g->dg.n;
    ldpc::QTile qt{};
    qt.E = reinterpret_cast<int8_t *>(d->pE);
    qt.L = reinterpret_cast<int16_t *>(d->pL);
    qt.Lam = rule.layer_ptr ? nullptr : reinterpret_cast<int8_t *>(d->pL) + 2 * cap * n;  // flooding only
    qt.bad = d->pbad;
    qt.cap = (int)cap;
    qt.qmax = (1 << (rule.qbits - 1)) - 1;
    qt.pmax = (1 << (rule.qbits + 1)) - 1;
    qt.param_q = rule.param_q;
    qt.scale = rule.scale;
    return qt;
}

// TileOps on the fixed-point tile kernels (phys_qtile.hip); lam32: the
// generator's fp32 Lambda tiles, or null: the channel LLRs in d->ch.  Both
// flooding syndromes are read from L16.
struct QTileOps : TileOps<QTileOps> {
    ldpc::QTile t;
    const float *lam32;
    const ldpc::QuantRule &rule;

    hipError_t init() { return ldpc::launch_phys_qtile_init(P, st, t, lam32, !rule.layer_ptr, s); }
    hipError_t layer(int it, int lbeg, int lrows) {
        return ldpc::launch_phys_qlayer_tile(P, st, t, rule.cn, it, lbeg, lrows, rule.layer_rows, s);
    }
    hipError_t cn(int it) { return ldpc::launch_phys_qtile_cn(P, st, t, rule.cn, it, s); }
    hipError_t vn(int it) { return ldpc::launch_phys_qtile_vn(P, st, t, it, d->pactive, max_iter, s); }
    hipError_t early_syn(int it) { return ldpc::launch_phys_tile_lsyn(P, st, t.L, t.bad, t.cap, (it + 1) & 1, s); }
    hipError_t last_syn() { return ldpc::launch_phys_tile_lsyn(P, st, t.L, t.bad, t.cap, max_iter & 1, s); }
};

int phys_qtile_decode(ldpc_decoder *d, const DevGraph &P, int max_iter, const float *lam32, hipStream_t s,
                      unsigned long long *ctr, const ldpc::QuantRule &rule,
                      const ldpc::McStats &ms = ldpc::McStats{}) {
    return phys_tile_sweeps(d, max_iter, s,
                            QTileOps{{d, P, d->st, max_iter, s, ctr, ms}, quant_tile(d, rule), lam32, rule});
}

}  // namespace

const char *ldpc_phys_kernel_name_q(const ldpc_graph *g, uint32_t flags, int32_t cn_rule, int32_t schedule,
                                    int32_t qbits) {
    if (!g || (cn_rule != LDPC_CN_NMS && cn_rule != LDPC_CN_OMS) ||
        (schedule != LDPC_SCHED_FLOODING && schedule != LDPC_SCHED_LAYERED) || qbits < 4 || qbits > 8 ||
        g->min_row_deg < 2 || (flags & (LDPC_F_PHYS_HBM | LDPC_F_LAYERED_TILE)))
        return "";
    const bool layered = schedule == LDPC_SCHED_LAYERED;
    if (quant_use_tile(g, flags, schedule)) return layered ? "phys_qlayer_tile_kernel" : "phys_qcn_tile_kernel";
    return ldpc::phys_quant_reg_shape(g->dg, quant_epad(g), layered) >= 0 ? "phys_quant_reg_kernel" : "phys_quant_kernel";
}

int64_t ldpc_phys_q_lds_bytes(const ldpc_graph *g, int32_t schedule) {
    if (!g || (schedule != LDPC_SCHED_FLOODING && schedule != LDPC_SCHED_LAYERED)) return -1;
    return (int64_t)ldpc::phys_quant_lds_bytes(g->dg, quant_epad(g), schedule == LDPC_SCHED_LAYERED);
}

int ldpc_phys_decode_q(const ldpc_graph *g, int32_t batch, const double *llr, int32_t max_iter, uint32_t flags,
                       int32_t cn_rule, int32_t schedule, int32_t qbits, float llr_scale, int32_t param_q,
                       uint8_t *z_out, int32_t *conv_out, int32_t *status_out, int32_t *iters_out, int16_t *post_out,
                       void *stream) {
    const char *fn = "ldpc_phys_decode_q";
    if (!g) return ldpc_fail(LDPC_EINVAL, "%s: NULL graph", fn);
    if (batch < 0 || max_iter < 1 || (batch > 0 && !llr))
        return ldpc_fail(LDPC_EINVAL, "%s: bad arguments (batch=%d max_iter=%d)", fn, batch, max_iter);
    if (int rc = quant_check(fn, g, flags, cn_rule, schedule, qbits, llr_scale, param_q)) return rc;
    if (batch == 0) return LDPC_OK;
    DeviceGuard dg(g->device);
    ldpc::QuantRule rule;
    if (int rc = quant_rule(g, flags, cn_rule, schedule, qbits, llr_scale, param_q, &rule)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const DevGraph &G = g->dg;
    if (rule.tile)  // int16 posteriors
        return phys_decode_chunks(
            g, batch, llr, flags, z_out, conv_out, status_out, iters_out, post_out, s,
            [&](ldpc_decoder *d) { return phys_qtile_decode(d, G, max_iter, nullptr, s, nullptr, rule); },
            [&](ldpc_decoder *d, uint8_t *z, int16_t *post) {
                return ldpc::launch_phys_tile_out(G, d->st, quant_tile(d, rule).L, z, post, s);
            });
    return phys_decode_staged(
        fn, G, batch, llr, flags, z_out, {conv_out, status_out, iters_out}, post_out, s,
        [&](const double *in, uint8_t *z, int *const *iv, int16_t *post) {
            return ldpc::launch_phys_quant(G, in, nullptr, batch, max_iter, z, iv[0], iv[1], iv[2], post, nullptr,
                                           nullptr, phys_quant_max_grid(), s, rule);
        });
}

int ldpc_phys_mc_run_q(ldpc_decoder *d, const ldpc_graph *gp, uint64_t seed, int32_t n_points, const double *sigmas,
                       int64_t frames_per_point, int64_t frame0, int32_t max_iter, uint32_t flags, int32_t cn_rule,
                       int32_t schedule, int32_t qbits, float llr_scale, int32_t param_q, int64_t *counters_out,
                       void *stream) {
    const char *fn = "ldpc_phys_mc_run_q";
    if (int rc = phys_mc_check(fn, d, gp, n_points, sigmas, frames_per_point, frame0, max_iter, counters_out))
        return rc;
    if (int rc = quant_check(fn, gp, flags, cn_rule, schedule, qbits, llr_scale, param_q)) return rc;
    const DevGraph &P = gp->dg;
    DeviceGuard dg(d->g->device);
    ldpc::QuantRule rule;
    if (int rc = quant_rule(gp, flags, cn_rule, schedule, qbits, llr_scale, param_q, &rule)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (rule.tile)
        if (int rc = ensure_phys_tile(d, P)) return rc;
    return phys_mc_drive(
        d, seed, n_points, sigmas, frames_per_point, frame0, max_iter, counters_out, s,
        rule.tile ? ldpc::kFramesTileLambda : ldpc::kFramesRowLambda, rule.tile,
        [&](const DevState &st, int cnt, const float *rows, unsigned long long *ctr, const ldpc::McStats &ms) -> int {
            if (rule.tile) return phys_qtile_decode(d, P, max_iter, d->pLam, s, ctr, rule, ms);
            HIP_TRY(timed(d, LDPC_K_PHYS, s, [&] {
                return ldpc::launch_phys_quant(P, nullptr, rows, cnt, max_iter, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, st.ubits, ctr, phys_quant_max_grid(), s, rule, ms);
            }));
            return LDPC_OK;
        });
}

// ------------------------------------------- physical mode, bit flipping
namespace {

enum BfKernel { kBfNone = 0, kBfSliced, kBfGeneric };

// The kernel a bit-flipping launch on graph P runs (stats: the run collects
// Monte-Carlo statistics, which only the per-frame kernel does).
BfKernel bf_kernel(const DevGraph &P, uint32_t flags, float weight, bool stats) {
    if (weight == 0.0f && !(flags & LDPC_F_BF_GENERIC) && !stats && ldpc::bitflip_sliced_applies(P) &&
        ldpc::bitflip_sliced_lds_bytes(P) + 1024 <= kLdsLimit)
        return kBfSliced;
    return ldpc::bitflip_lds_bytes(P) + 64 <= kLdsLimit ? kBfGeneric : kBfNone;
}

size_t bf_lds(const DevGraph &P, BfKernel k) {
    return k == kBfSliced ? ldpc::bitflip_sliced_lds_bytes(P) + 1024 : ldpc::bitflip_lds_bytes(P) + 64;
}

// workgroups the device holds at once (as phys_grid), at most `work` (frames, or 64-frame tiles)
int bf_grid(const DevGraph &P, BfKernel k, int work) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) cus = p.multiProcessorCount;
    }
    const int waves = ldpc::bitflip_threads() / 64;
    int per_cu = (int)std::min<size_t>(32 / waves, kLdsLimit / bf_lds(P, k));
    if (per_cu < 1) per_cu = 1;
    return (int)std::min<int64_t>((int64_t)cus * per_cu, work);
}

int bf_check(const char *fn, uint32_t flags, uint32_t allowed, float weight, float theta) {
    if (flags & ~allowed) return ldpc_fail(LDPC_EINVAL, "%s: unsupported flags 0x%x", fn, flags & ~allowed);
    if (!std::isfinite(weight) || weight < 0.0f)
        return ldpc_fail(LDPC_EINVAL, "%s: weight must be finite and >= 0, got %g", fn, (double)weight);
    if (!std::isfinite(theta)) return ldpc_fail(LDPC_EINVAL, "%s: theta must be finite, got %g", fn, (double)theta);
    return LDPC_OK;
}

int bf_no_fit(const char *fn, const DevGraph &P) {
    return ldpc_fail(LDPC_ERANGE, "%s: a frame's bit-flipping state (%zu bytes for n = %d, m = %d) does not fit LDS; "
                                  "an HBM path for bit flipping is not implemented", fn, ldpc::bitflip_lds_bytes(P),
                     P.n, P.m);
}

hipError_t bf_launch(const DevGraph &P, BfKernel k, const double *llr, const float *lam, int layout, int count,
                     int max_iter, uint8_t *z, int *conv, int *status, int *iters, int *synw, const uint32_t *ubits,
                     unsigned long long *ctr, hipStream_t s, float weight, float theta,
                     const ldpc::McStats &ms = ldpc::McStats{}) {
    ldpc::BitflipRule rule;
    rule.weight = weight;
    rule.theta = theta;
    rule.sliced = k == kBfSliced;
    const int work = rule.sliced ? (count + kTile - 1) / kTile : count;
    return ldpc::launch_bitflip(P, llr, lam, layout, count, max_iter, z, conv, status, iters, synw, ubits, ctr,
                                bf_grid(P, k, work), s, rule, ms);
}

}  // namespace

const char *ldpc_bf_kernel_name(const ldpc_graph *g, uint32_t flags, float weight) {
    if (!g || (flags & ~(uint32_t)(LDPC_F_DEVICE_PTRS | LDPC_F_BF_GENERIC)) || !std::isfinite(weight) || weight < 0.0f)
        return "";
    switch (bf_kernel(g->dg, flags, weight, false)) {
    case kBfSliced: return "bitflip_sliced_kernel";
    case kBfGeneric: return "bitflip_kernel";
    default: return "";
    }
}

int64_t ldpc_bf_lds_bytes(const ldpc_graph *g, uint32_t flags, float weight) {
    if (!g || (flags & ~(uint32_t)(LDPC_F_DEVICE_PTRS | LDPC_F_BF_GENERIC)) || !std::isfinite(weight) || weight < 0.0f)
        return -1;
    const BfKernel k = bf_kernel(g->dg, flags, weight, false);
    return (int64_t)(k == kBfSliced ? ldpc::bitflip_sliced_lds_bytes(g->dg) : ldpc::bitflip_lds_bytes(g->dg));
}

int ldpc_bf_decode(const ldpc_graph *g, int32_t batch, const double *llr, int32_t max_iter, uint32_t flags,
                   float weight, float theta, uint8_t *z_out, int32_t *conv_out, int32_t *status_out,
                   int32_t *iters_out, int32_t *synw_out, void *stream) {
    const char *fn = "ldpc_bf_decode";
    if (!g) return ldpc_fail(LDPC_EINVAL, "%s: NULL graph", fn);
    if (batch < 1 || max_iter < 1 || !llr)
        return ldpc_fail(LDPC_EINVAL, "%s: bad arguments (batch=%d max_iter=%d)", fn, batch, max_iter);
    if (int rc = bf_check(fn, flags, LDPC_F_DEVICE_PTRS | LDPC_F_BF_GENERIC, weight, theta)) return rc;
    const DevGraph &G = g->dg;
    const BfKernel k = bf_kernel(G, flags, weight, false);
    if (k == kBfNone) return bf_no_fit(fn, G);
    DeviceGuard dg(g->device);
    hipStream_t s = (hipStream_t)stream;
    // bit flipping has no posterior: a fourth integer per frame, the syndrome weight
    return phys_decode_staged(
        fn, G, batch, llr, flags, z_out, {conv_out, status_out, iters_out, synw_out}, (float *)nullptr, s,
        [&](const double *in, uint8_t *z, int *const *iv, float *) {
            return bf_launch(G, k, in, nullptr, 0, batch, max_iter, z, iv[0], iv[1], iv[2], iv[3], nullptr, nullptr, s,
                             weight, theta);
        });
}

int ldpc_bf_mc_run(ldpc_decoder *d, const ldpc_graph *gp, uint64_t seed, int32_t n_points, const double *sigmas,
                   int64_t frames_per_point, int64_t frame0, int32_t max_iter, uint32_t flags, float weight,
                   float theta, int64_t *counters_out, void *stream) {
    const char *fn = "ldpc_bf_mc_run";
    if (int rc = phys_mc_check(fn, d, gp, n_points, sigmas, frames_per_point, frame0, max_iter, counters_out))
        return rc;
    if (int rc = bf_check(fn, flags, LDPC_F_BF_GENERIC, weight, theta)) return rc;
    const DevGraph &P = gp->dg;
    // the statistics are the per-frame kernel's
    const BfKernel k = bf_kernel(P, flags, weight, d->ms_on);
    if (k == kBfNone) return bf_no_fit(fn, P);
    DeviceGuard dg(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    // the frames as fp32 Lambda rows, as ldpc_phys_mc_run's LDS path
    return phys_mc_drive(
        d, seed, n_points, sigmas, frames_per_point, frame0, max_iter, counters_out, s, ldpc::kFramesRowLambda, false,
        [&](const DevState &st, int cnt, const float *rows, unsigned long long *ctr, const ldpc::McStats &ms) -> int {
            HIP_TRY(timed(d, LDPC_K_PHYS, s, [&] {
                return bf_launch(P, k, nullptr, rows, 2, cnt, max_iter, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 st.ubits, ctr, s, weight, theta, ms);
            }));
            return LDPC_OK;
        });
}

// ------------------------------------------------------- channel models
int ldpc_channel_set(ldpc_decoder *d, const ldpc_channel *ch) {
    const char *fn = "ldpc_channel_set";
    ldpc::FrameChannel c{};
    if (ch) {
        if (ch->model != LDPC_CH_REFERENCE && ch->model != LDPC_CH_AWGN && ch->model != LDPC_CH_RAYLEIGH)
            return ldpc_fail(LDPC_EINVAL, "%s: model %d is none of LDPC_CH_REFERENCE, LDPC_CH_AWGN, LDPC_CH_RAYLEIGH", fn,
                             ch->model);
        if (ch->modulation != 1 && ch->modulation != 2 && ch->modulation != 4 && ch->modulation != 6)
            return ldpc_fail(LDPC_EINVAL, "%s: modulation %d bits per symbol is none of 1 (BPSK), 2 (QPSK), 4 (16-QAM), "
                                          "6 (64-QAM)", fn, ch->modulation);
        if (ch->demap != LDPC_DEMAP_EXACT && ch->demap != LDPC_DEMAP_MAXLOG)
            return ldpc_fail(LDPC_EINVAL, "%s: demap %d is neither LDPC_DEMAP_EXACT nor LDPC_DEMAP_MAXLOG", fn,
                             ch->demap);
        if (ch->reserved != 0) return ldpc_fail(LDPC_EINVAL, "%s: reserved must be 0, got %d", fn, ch->reserved);
        if (ch->model == LDPC_CH_REFERENCE && ch->modulation != 1)
            return ldpc_fail(LDPC_EINVAL, "%s: the reference channel is BPSK only (modulation 1), got %d", fn,
                             ch->modulation);
        c.model = ch->model;
        c.bps = ch->modulation;
        c.demap = ch->demap;
    }
    if (!d) return ldpc_fail(LDPC_EINVAL, "%s: NULL decoder", fn);
    c.fade_block = d->chan.fade_block;  // ldpc_fading_set's, a setting of its own
    d->chan = c;
    return LDPC_OK;
}

int ldpc_channel_get(const ldpc_decoder *d, ldpc_channel *out) {
    if (!d) return ldpc_fail(LDPC_EINVAL, "ldpc_channel_get: NULL decoder");
    if (!out) return ldpc_fail(LDPC_EINVAL, "ldpc_channel_get: NULL out");
    *out = ldpc_channel{d->chan.model, d->chan.bps, d->chan.demap, 0};
    return LDPC_OK;
}

// ------------------------------------------------------- rate matching
int ldpc_rate_match_set(ldpc_decoder *d, int32_t n_punct, const int32_t *punct_cols, int32_t n_short,
                        const int32_t *short_cols) {
    const char *fn = "ldpc_rate_match_set";
    if (!d) return ldpc_fail(LDPC_EINVAL, "%s: NULL decoder", fn);
    const DevGraph &G = d->g->dg;
    const std::string err = ldpc::rate_match_validate(G.n, G.k, n_punct, punct_cols, n_short, short_cols);
    if (!err.empty()) return ldpc_fail(LDPC_EINVAL, "%s: %s", fn, err.c_str());
    d->rm_punct.assign(punct_cols, punct_cols + n_punct);
    d->rm_short.assign(short_cols, short_cols + n_short);
    std::sort(d->rm_punct.begin(), d->rm_punct.end());
    std::sort(d->rm_short.begin(), d->rm_short.end());
    d->rm_stale = true;
    return LDPC_OK;
}

int ldpc_rate_match_get(const ldpc_decoder *d, int32_t *n_punct, int32_t *n_short, int32_t *punct_out,
                        int32_t punct_cap, int32_t *short_out, int32_t short_cap) {
    const char *fn = "ldpc_rate_match_get";
    if (!d) return ldpc_fail(LDPC_EINVAL, "%s: NULL decoder", fn);
    if (!n_punct || !n_short || punct_cap < 0 || short_cap < 0 || (punct_cap > 0 && !punct_out) ||
        (short_cap > 0 && !short_out))
        return ldpc_fail(LDPC_EINVAL, "%s: bad arguments", fn);
    *n_punct = (int32_t)d->rm_punct.size();
    *n_short = (int32_t)d->rm_short.size();
    if (punct_out || short_out) {
        if ((punct_out && punct_cap < *n_punct) || (short_out && short_cap < *n_short))
            return ldpc_fail(LDPC_EINVAL, "%s: capacities %d / %d are too small for %d punctured and %d shortened "
                                          "columns", fn, punct_cap, short_cap, *n_punct, *n_short);
        if (punct_out) std::copy(d->rm_punct.begin(), d->rm_punct.end(), punct_out);
        if (short_out) std::copy(d->rm_short.begin(), d->rm_short.end(), short_out);
    }
    return LDPC_OK;
}

// ------------------------------------- bit interleaver and block fading
int ldpc_interleaver_set(ldpc_decoder *d, int32_t len, const int32_t *perm) {
    const char *fn = "ldpc_interleaver_set";
    if (!d) return ldpc_fail(LDPC_EINVAL, "%s: NULL decoder", fn);
    const std::string err = ldpc::interleaver_validate(len, perm);
    if (!err.empty()) return ldpc_fail(LDPC_EINVAL, "%s: %s", fn, err.c_str());
    if (len > 0)
        d->il_perm.assign(perm, perm + len);
    else
        d->il_perm.clear();
    d->rm_stale = true;
    return LDPC_OK;
}

int ldpc_interleaver_get(const ldpc_decoder *d, int32_t *len, int32_t *perm_out, int32_t cap) {
    const char *fn = "ldpc_interleaver_get";
    if (!d) return ldpc_fail(LDPC_EINVAL, "%s: NULL decoder", fn);
    if (!len || cap < 0 || (cap > 0 && !perm_out)) return ldpc_fail(LDPC_EINVAL, "%s: bad arguments", fn);
    *len = (int32_t)d->il_perm.size();
    if (perm_out) {
        if (cap < *len)
            return ldpc_fail(LDPC_EINVAL, "%s: capacity %d is too small for a permutation of length %d", fn, cap, *len);
        std::copy(d->il_perm.begin(), d->il_perm.end(), perm_out);
    }
    return LDPC_OK;
}

int ldpc_fading_set(ldpc_decoder *d, int32_t block_len) {
    const char *fn = "ldpc_fading_set";
    if (!d) return ldpc_fail(LDPC_EINVAL, "%s: NULL decoder", fn);
    if (block_len < 1) return ldpc_fail(LDPC_EINVAL, "%s: block_len %d < 1 (1 is a fade per symbol)", fn, block_len);
    d->chan.fade_block = block_len;
    return LDPC_OK;
}

int ldpc_fading_get(const ldpc_decoder *d, int32_t *block_len) {
    if (!d) return ldpc_fail(LDPC_EINVAL, "ldpc_fading_get: NULL decoder");
    if (!block_len) return ldpc_fail(LDPC_EINVAL, "ldpc_fading_get: NULL block_len");
    *block_len = d->chan.fade_block;
    return LDPC_OK;
}

// ------------------------------------------------------------------ HARQ
int ldpc_harq_set(ldpc_decoder *d, int32_t n_tx, const int32_t *tx_len, const int32_t *cols) {
    const char *fn = "ldpc_harq_set";
    if (!d) return ldpc_fail(LDPC_EINVAL, "%s: NULL decoder", fn);
    const std::string err = ldpc::harq_validate(d->g->dg.n, n_tx, tx_len, cols);
    if (!err.empty()) return ldpc_fail(LDPC_EINVAL, "%s: %s", fn, err.c_str());
    size_t total = 0;
    for (int32_t r = 0; r < n_tx; ++r) total += (size_t)tx_len[r];
    if (n_tx > 0) {
        d->hq_len.assign(tx_len, tx_len + n_tx);
        d->hq_cols.assign(cols, cols + total);
    } else {
        d->hq_len.clear();
        d->hq_cols.clear();
    }
    d->hq_stale = true;
    return LDPC_OK;
}

int ldpc_harq_get(const ldpc_decoder *d, int32_t *n_tx, int32_t *tx_len_out, int32_t *cols_out, int32_t cols_cap) {
    const char *fn = "ldpc_harq_get";
    if (!d) return ldpc_fail(LDPC_EINVAL, "%s: NULL decoder", fn);
    if (!n_tx || cols_cap < 0 || (cols_cap > 0 && !cols_out)) return ldpc_fail(LDPC_EINVAL, "%s: bad arguments", fn);
    *n_tx = (int32_t)d->hq_len.size();
    if (tx_len_out)
        for (int r = 0; r < LDPC_HARQ_MAX_TX; ++r) tx_len_out[r] = r < *n_tx ? d->hq_len[(size_t)r] : 0;
    if (cols_out) {
        if ((size_t)cols_cap < d->hq_cols.size())
            return ldpc_fail(LDPC_EINVAL, "%s: capacity %d is too small for a plan of %zu positions", fn, cols_cap,
                             d->hq_cols.size());
        std::copy(d->hq_cols.begin(), d->hq_cols.end(), cols_out);
    }
    return LDPC_OK;
}

// --------------------------------------------------------- constellations
int ldpc_constellation_set(ldpc_decoder *d, int32_t bps, const double *points) {
    const char *fn = "ldpc_constellation_set";
    if (!d) return ldpc_fail(LDPC_EINVAL, "%s: NULL decoder", fn);
    const std::string err = ldpc::constellation_validate(bps, points);
    if (!err.empty()) return ldpc_fail(LDPC_EINVAL, "%s: %s", fn, err.c_str());
    d->ctab.assign(bps, points);
    return LDPC_OK;
}

int ldpc_constellation_get(const ldpc_decoder *d, int32_t *bps, double *points_out, int32_t cap) {
    const char *fn = "ldpc_constellation_get";
    if (!d) return ldpc_fail(LDPC_EINVAL, "%s: NULL decoder", fn);
    if (!bps) return ldpc_fail(LDPC_EINVAL, "%s: NULL bps", fn);
    *bps = d->ctab.bps;
    if (const int need = d->ctab.copy_to(points_out, cap))
        return ldpc_fail(LDPC_EINVAL, "%s: capacity %d is too small for the %d doubles of a table with bps = %d", fn, cap,
                         need, d->ctab.bps);
    return LDPC_OK;
}

// ------------------------------------------------- Monte-Carlo statistics
int ldpc_mc_stats_enable(ldpc_decoder *d, int32_t enable, int32_t max_failed) {
    if (max_failed < 0) return ldpc_fail(LDPC_EINVAL, "ldpc_mc_stats_enable: max_failed %d < 0", max_failed);
    if (!d) return ldpc_fail(LDPC_EINVAL, "ldpc_mc_stats_enable: NULL decoder");
    d->ms_on = enable != 0;
    d->ms_max_failed = d->ms_on ? max_failed : 0;
    d->ms_state = 0;  // what an earlier run left is gone
    return LDPC_OK;
}

int ldpc_mc_stats_read(ldpc_decoder *d, int32_t point, int64_t *hist_out, int32_t hist_len, int64_t *undetected_out,
                       int64_t *failed_out, int32_t failed_cap, int64_t *n_failed_out) {
    const char *fn = "ldpc_mc_stats_read";
    if (!d) return ldpc_fail(LDPC_EINVAL, "%s: NULL decoder", fn);
    if (!hist_out || !undetected_out || !n_failed_out || failed_cap < 0 || (failed_cap > 0 && !failed_out))
        return ldpc_fail(LDPC_EINVAL, "%s: bad arguments", fn);
    if (!d->ms_on) return ldpc_fail(LDPC_EINVAL, "%s: statistics are not enabled (ldpc_mc_stats_enable)", fn);
    if (d->ms_state == 2)
        return ldpc_fail(LDPC_EINVAL, "%s: the last run was ldpc_mc_run, which collects no statistics", fn);
    if (d->ms_state != 1)
        return ldpc_fail(LDPC_EINVAL, "%s: no physical-mode Monte-Carlo run since statistics were enabled", fn);
    if (point < 0 || point >= d->ms_points)
        return ldpc_fail(LDPC_EINVAL, "%s: point %d out of range (the run had %d)", fn, point, d->ms_points);
    if (hist_len != d->ms_T + 1)
        return ldpc_fail(LDPC_EINVAL, "%s: hist_len %d != max_iter + 1 = %d of the last run", fn, hist_len,
                         d->ms_T + 1);
    DeviceGuard dg(d->g->device);
    const size_t pw = ldpc::mc_stats_point_words(d->ms_T);
    std::vector<unsigned long long> head(pw);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(head.data(), d->ms_buf + (size_t)point * pw, sizeof(unsigned long long) * pw,
                      hipMemcpyDeviceToHost));
    const int64_t stored = ldpc::mc_stats_stored(head[2], d->ms_run_failed);
    if (failed_cap < stored)
        return ldpc_fail(LDPC_EINVAL, "%s: failed_cap %d < %lld stored records", fn, failed_cap, (long long)stored);
    if (stored > 0) {
        std::vector<int64_t> rec(2 * (size_t)stored);
        const unsigned long long *src =
            d->ms_buf + (size_t)d->ms_points * pw + (size_t)point * 2 * (size_t)d->ms_run_failed;
        HIP_TRY(hipMemcpy(rec.data(), src, sizeof(int64_t) * rec.size(), hipMemcpyDeviceToHost));
        ldpc::mc_stats_sort_records(rec.data(), stored, failed_out);
    }
    undetected_out[0] = (int64_t)head[0];
    undetected_out[1] = (int64_t)head[1];
    for (int t = 0; t <= d->ms_T; ++t) hist_out[t] = (int64_t)head[ldpc::kMcStatsHead + t];
    n_failed_out[0] = stored;
    n_failed_out[1] = (int64_t)head[2] - stored;
    return LDPC_OK;
}

// -------------------------------------------------------------- profiling
int ldpc_profile_enable(ldpc_decoder *d, int enable) {
    if (!d) return ldpc_fail(LDPC_EINVAL, "ldpc_profile_enable: NULL decoder");
    d->prof = enable != 0;
    return LDPC_OK;
}

int ldpc_profile_read(ldpc_decoder *d, double *ms_out, int64_t *launches_out) {
    if (!d) return ldpc_fail(LDPC_EINVAL, "ldpc_profile_read: NULL decoder");
    DeviceGuard dg(d->g->device);
    double ms[LDPC_K_NKINDS] = {};
    int64_t cnt[LDPC_K_NKINDS] = {};
    for (auto &sp : d->spans) {
        HIP_TRY(hipEventSynchronize(sp.b));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, sp.a, sp.b));
        ms[sp.kind] += t;
        cnt[sp.kind] += 1;
        d->pool.push_back(sp.a);
        d->pool.push_back(sp.b);
    }
    d->spans.clear();
    for (int i = 0; i < LDPC_K_NKINDS; ++i) {
        if (ms_out) ms_out[i] = ms[i];
        if (launches_out) launches_out[i] = cnt[i];
    }
    return LDPC_OK;
}

}  // extern "C"
