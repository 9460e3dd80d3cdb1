// tile_sub.hip -- the tile-resident parity decoder for long codes (gfx950).
//
// tile_kernels.hip decodes 64 frames per workgroup with the column sums
// S_j = ((0 + E_r0j) + E_r1j) + ... (rows ascending: scipy csr_matvec of E^T,
// the reference's rounding order, python_ldpc_app/spa_decoder.py:173-185)
// kept in LDS: k x 64 x 8 B, which holds only for k <= ~300.  The WiMAX 2304
// codes (k = 1152, 1728) fit when a workgroup decodes a SUB-tile of F = 16 or
// 8 frames (S = k x F x 8 B: 147 KB / 110 KB).  A wavefront instruction then
// covers Q = 64/F edges of F frames: lane = j*F + f (lane group j, frame f).
//
// Row r's edges are split into 16 contiguous wavefront chunks as in
// tile_kernel (wavefront w: positions [w*C, w*C + C), C = ceil(deg/16)), and a
// chunk into Q contiguous lane-group pieces of CS = ceil(C/Q) edges: lane group
// j holds positions j*CS .. j*CS + CS - 1 of the chunk in register slots
// 0..CS-1.  The left-to-right product P = t0 * t1 * ... (:151-152) crosses lane
// groups inside the wavefront: starting from the prefix P of the wavefront
// before it, every lane multiplies its own slots in order; lane group j's
// result is the prefix through group j, moved to group j+1 (permlane swaps;
// ds_bpermute for Q = 8)
// before group j+1's turn.  Groups with no edges are skipped.  Each wavefront
// runs the hop-first pipeline
//
//   body(r):  hop(r)   this wavefront's piece of row r's product;
//             P3(r-1)  E_new = 2 atanh(clip(P/t)) (:159-168), stored, added
//                      into S (LDS, per lane: column of its edge, its frame)
//                      after the overlapping wavefronts' P3(r-2) (sub_p3);
//             P1(r+1)  L[col], E_old, t = tanh((L - E_old)/2) (:138-146,
//                      :260-268).
//
// The default decoder of wimax_2304_0.5 (F = 16, Q = 4: the product crosses
// lane groups with v_permlane16/32_swap); bit-identical to the split path.
// Iteration 0 of the static decoder does not run this pipeline where it need
// not: its rows and columns are independent of each other (sub_pass0_cols).
// (An F = 8 form of this kernel for the r3/4 codes was retired in round 3:
// tile8.hip decodes them, with E in 8-frame blocks.)
//
// Per edge and iteration the HBM traffic is the algorithmic 16 B (E_old read,
// E_new write) plus the L[col] gather (8 B, L2/MALL): the split CN/VN
// launches this replaces move 24 + 8 B plus the gathers.  The identity column
// k+r of a [A | I] graph has row r's last edge only; its posterior
// ch + (0 + E) is final when row r is.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "cn_common.h"
#include "frame_source.h"
#include "spa_device.h"
#include "spa_math.h"
#include "tile_common.h"

namespace ldpc {
namespace {

// wavefronts per workgroup: kSubWaves (16, spa_device.h; 12 wavefronts with
// 168 registers each spilled less but measured 6 % slower, profiles/r4z_ab)
constexpr int kSW = kSubWaves;
// -DLDPC_SUB_TIMERS: diagnostic build (never the product) -- s_memtime phase
// timers per wavefront, printed for two workgroups at the end of the launch:
// hop wait, hop, P3 chain wait, P3 math + stores, P3 order wait, P3 adds, P1
#ifdef LDPC_SUB_TIMERS
#define SUB_NT 7
#define SUB_STAMP(v) const uint64_t v = __builtin_amdgcn_s_memtime()
#define SUB_ADD(c, i, a, b) ((c).tm[i] += (b) - (a))
#else
#define SUB_STAMP(v)
#define SUB_ADD(c, i, a, b)
#endif
constexpr size_t kSubLdsMax = 163840;


template <int Q>
struct SubCfg {
    static constexpr int F = kTile / Q;           // frames per workgroup
    static constexpr int K = Q == 4 ? 10 : 8;  // slots per lane: row degree <= kSW * Q * K
};

// The product crosses lane groups by v_permlane16/32_swap (Q = 4) or
// ds_bpermute (Q = 8); the wavefront carrying the chain runs at raised issue
// priority; the message stream E (read once, written once per pass) is
// non-temporal, as in tile_kernels.hip.  Pipeline: body(r) = hop(r), P3(r-1),
// P1(r+1) -- the chain of row r runs while the other wavefronts are still in
// P3(r-1); the S additions of a row wait on the per-row P3 completion counts,
// and the chain slots are reused every 4 rows.
constexpr int kSR = 4;  // chain slots
// P1 loads and evaluates tanh for all K slots of a lane, branch-free: slots
// past the chunk's CS hold clamped, valid data (their t ends as 1.0 and is never
// used), and the straight-line code lets each slot's math wait only for its own
// loads (+2.7 % over a per-slot branch, profiles r2x logs); the hop multiplies
// all K slots of every lane group (the padded 1.0s are exact no-ops).  P3
// reads clamped column indices for every slot and adds each slot's E_new into
// its column sum with one ds_add_f64 (slots past the piece add into `dummy`):
// the same IEEE add of the same operands as read / add / write, rows ordered
// by the p3dep waits; ds_add_f64 rounds to nearest even and, unlike the other
// LDS float atomics, never flushes denormals (LLVM SIISelLowering emits it for
// workgroup-scope fadd only on that basis; +2 %, profiles/r4za_ab).  A fresh
// streaming frame's lanes read no E_old: M = L - 0.0 == L; iteration 0 of the
// static decoder reads neither E_old nor ch: its t comes from sub_tanh_table.
// Measured and not kept (profiles/ READMEs; git history has the code): tanh
// groups of 2-3 slots in lockstep (spills), guarded per-slot P1/P3 forms,
// skipping the padded slot K-1 (0.4375), sc1 E_new stores (0.436), uint16
// index staging (0.417), 12 wavefronts per workgroup (0.426).
// Logical wavefront (chunk position in a row) of hardware wavefront hw: the
// four wavefronts of one SIMD (hw = s, s+4, s+8, s+12) take four consecutive
// chunk positions, so each SIMD holds one contiguous quarter of every row's
// chain and its P3 neighbours.  +1.3 % over the identity map, static and
// streaming (profiles/r2at_wave_map; pairs of positions per SIMD measured the
// same, spin waits at a lower issue priority +0.2 %).
__device__ __forceinline__ int sub_wave(int hw) { return (hw & 3) * (kSW / 4) + (hw >> 2); }
// E_new stores through a buffer resource: a slot past the lane's piece (or a
// frame-less lane) stores at kSubOOB, past num_records, which the hardware
// drops -- no branch per slot, so every memory operation of the row loop is
// unconditional and the compiler's vmcnt waits count exactly (with branches
// it waited for this row's stores before P1's first request)
typedef unsigned int sub_u2 __attribute__((ext_vector_type(2)));
constexpr uint32_t kSubOOB = 0xfffffff0u;
__device__ __forceinline__ void st_sub_msg(__amdgpu_buffer_rsrc_t r, uint32_t off, double v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(sub_u2, v), r, off, 0, 2 /* nt */);
}
// E_old loads the same way: at kSubOOB (a fresh frame, a masked slot) the
// hardware returns 0 without a memory request
__device__ __forceinline__ double ld_sub_msg(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 2 /* nt */));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sub_rsrc(const void *base, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, (int)min(bytes, (size_t)0x7fffffff),
                                            0x00020000);
}

// Column indices of the rows in flight, staged per wavefront in LDS as 16-bit
// values one row ahead of their P1 (a ring of 3 rows: P3(r-1), P1(r+1) and the
// staging of row r+2 in body(r)), so neither P1's posterior gather nor P3 waits
// on an index load from L2.
constexpr int kCRing = 3;
struct SubLayout {
    size_t S, math, slot, zb, ib, lane_i, flags, dummy, cidx, total;
};
__host__ __device__ constexpr int sub_k(int F) { return F == 16 ? SubCfg<4>::K : 0; }
__host__ __device__ inline SubLayout sub_layout(int k, int m, int F) {
    SubLayout t;
    size_t o = 0;
    t.S = o;  // [k][F] column sums
    o = al16(o + (size_t)k * F * sizeof(double));
    t.math = o;
    o = al16(o + sizeof(MathLds));
    t.slot = o;  // [kSR][F] chain slots
    o = al16(o + kSR * (size_t)F * sizeof(double));
    t.zb = o;  // [kw][F] z^1 bits of the A columns
    o = al16(o + (size_t)((k + 31) / 32) * F * sizeof(uint32_t));
    t.ib = o;  // [mw][F] z^1 bits of the identity columns (adjacent to zb)
    o = al16(o + (size_t)((m + 31) / 32) * F * sizeof(uint32_t));
    t.lane_i = o;  // bad[F], nllr count[F], live[F]
    o = al16(o + 3 * (size_t)F * sizeof(int));
    t.flags = o;  // chain flag[kSR], tiny[kSR], tiny sequence, running, P3 rows done[kSW]
    o = al16(o + (2 * kSR + 2 + kSW) * sizeof(int));
    t.dummy = o;  // [F] target of the identity lane's masked-off S update
    o = al16(o + (size_t)F * sizeof(double));
    t.cidx = o;  // [kCRing][kSW][64/F * K] uint16 column indices (one wavefront chunk per row)
    o = al16(o + (size_t)kCRing * kSW * (64 / F) * sub_k(F) * sizeof(uint16_t));
    t.total = o;
    return t;
}

struct SubChunk {
    int deg, c0, cnt, CS;
};
__device__ __forceinline__ SubChunk sub_chunk(const int *__restrict__ row_ptr, int r, int wave, int Q) {
    SubChunk c;
    const int beg = row_ptr[r];
    c.deg = row_ptr[r + 1] - beg;
    const int C = (c.deg + kSW - 1) / kSW;
    c.c0 = beg + wave * C;
    c.cnt = max(0, min(c.deg - wave * C, C));
    c.CS = (C + Q - 1) / Q;
    return c;
}

template <int Q>
struct SubCtx {
    static constexpr int F = SubCfg<Q>::F;
    static constexpr int K = SubCfg<Q>::K;
    const int *__restrict__ col_idx;
    const int *__restrict__ row_ptr;
    // per-lane bases: element (item) of this lane's frame at [item * 64]
    double *Eb;
    double *Lb;
    const double *Cb;
    double *Tb;     // rare-row scratch of this workgroup, element (pos) at [pos * F]; two buffers
    size_t tbuf;    // doubles between them (rare rows alternate: tile_kernels.hip)
    double *S;      // LDS, element (col) at [col * F]
    double *dummy;  // LDS, this lane's frame
    double *slot;   // LDS, chain slot s at [s * F]
    uint32_t *ib;   // LDS, word w at [w * F]
    uint16_t *cidx; // LDS, this wavefront's index ring: row slot s, position p at [s * kSW * Q * K + p]
    int m;
    int *flag, *tinyf, *tseq, *p3row;
    const int *p3dep;
    LdsTanh ttab;
    LdsAtanh ltab;
    AtanhCoef ac;   // kernel-argument coefficients (when coef_arg)
    bool coef_arg;  // P3 uses ac instead of coef_load() (compile-time per kernel)
    // uniform (SGPR) tile bases + this lane's byte offset: every access is a
    // 32-bit per-lane offset from a scalar base (global_load ... v_off, s_base)
    const char *Eu, *Lu, *Cu;
    __amdgpu_buffer_rsrc_t rE;  // the tile's E for masked stores without a branch (sub_p3_body)
    uint32_t lo8;
    int k, wave, j, f;
    int ep0;
    bool first, live;
    bool fresh;  // streaming: this lane's frame is on its first pass (M = L - 0, L = ch)
    bool verify;  // static decoder: this pass verifies a fixed point (sub_p3_body compares E_new with E_old)
    bool prove;   // ... and runs the next-pass proof where a message differed
    int *mdiff;   // LDS [F]: verifying pass, bit 0: a message of frame f differed; bit 1: its next-pass proof failed
                  // or went untested; bit 2: some frame's proof failed in this pass
    int ntiny;
#ifdef LDPC_SUB_TIMERS
    mutable uint64_t tm[SUB_NT];
#endif
};

// this lane's edge count in chunk rc, and the edge of its slot i (clamped
// into the chunk: slots past the piece load the chunk's last edge again)
template <int Q>
__device__ __forceinline__ int sub_nj(const SubCtx<Q> &c, const SubChunk &rc) {
    return max(0, min(rc.cnt - c.j * rc.CS, rc.CS));
}
template <int Q>
__device__ __forceinline__ int sub_edge(const SubCtx<Q> &c, const SubChunk &rc, int i) {
    return rc.c0 + min(c.j * rc.CS + i, rc.cnt - 1);
}
// element (item, this lane's frame) of a tile array: item * 64 * 8 + lane * 8 bytes
template <int Q>
__device__ __forceinline__ uint32_t sub_off(const SubCtx<Q> &c, int item) {
    return ((uint32_t)item << 9) + c.lo8;
}
template <int Q>
__device__ __forceinline__ double *sub_l(const SubCtx<Q> &c, int col) {
    return (double *)(c.Lu + sub_off(c, col));
}
template <int Q>
__device__ __forceinline__ const double *sub_c(const SubCtx<Q> &c, int col) {
    return (const double *)(c.Cu + sub_off(c, col));
}
template <int Q>
__device__ __forceinline__ int sub_col(const SubCtx<Q> &c, int edge) {
    return *(const int *)((const char *)c.col_idx + ((uint32_t)edge << 2));
}
// This lane's piece of row r's staged column indices: slot i at [i].  The
// staging wrote every position < Q*K (past the chunk: the clamped last
// column), and j*CS + i < Q*K for every slot, so no clamp is needed here and
// each slot's read is an immediate offset from one address per row.
template <int Q>
__device__ __forceinline__ const uint16_t *sub_lcols(const SubCtx<Q> &c, int r, const SubChunk &rc) {
    return c.cidx + (r % kCRing) * kSW * Q * SubCfg<Q>::K + c.j * rc.CS;
}
// Byte offset of this lane's slot 0 of chunk rc in the tile's E; slot i is at
// + i * 512.  Slots past the lane's piece are NOT clamped: their loads read
// other edges (past the tile's last edge: the buffer returns 0) and their
// values are discarded (t = 1.0, the store dropped at kSubOOB).
template <int Q>
__device__ __forceinline__ uint32_t sub_eoff(const SubCtx<Q> &c, const SubChunk &rc) {
    return ((uint32_t)(rc.c0 + c.j * rc.CS) << 9) + c.lo8;
}
// Staging of row q's indices into the ring: issue (one index per lane, lanes <
// the chunk size) early, commit to LDS once the wavefront has waited on its
// other loads anyway.
template <int Q>
__device__ __forceinline__ int sub_stage_issue(const SubCtx<Q> &c, int q) {
    // always one load (an in-range edge): a conditional load into a register
    // also written with 0 makes the compiler wait for every outstanding
    // memory operation (this row's E_new stores) before P1's first request
    const SubChunk rc = sub_chunk(c.row_ptr, min(q, c.m - 1), c.wave, Q);
    const int L = threadIdx.x & 63;
    return sub_col(c, min(max(rc.c0 + min(L, rc.cnt - 1), 0), c.row_ptr[c.m] - 1));
}
template <int Q>
__device__ __forceinline__ void sub_stage_commit(const SubCtx<Q> &c, int q, int v) {
    if (q >= c.m) return;
    constexpr int W = Q * SubCfg<Q>::K;  // positions per wavefront chunk (40 / 64)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if ((int)(threadIdx.x & 63) < W) c.cidx[(q % kCRing) * kSW * W + (threadIdx.x & 63)] = (uint16_t)v;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// P1: t = tanh((L[col] - E_old)/2) for this lane's slots; returns whether
// some lane's own edge has |t| <= 1e-10 (:159).  E_old is requested first
// (independent of the column indices), then the indices, then the posterior
// gather that needs them.
template <int Q>
__device__ __forceinline__ bool sub_p1(const SubCtx<Q> &c, int r, const SubChunk &rc, double (&t)[SubCfg<Q>::K]) {
    constexpr int K = SubCfg<Q>::K;
    bool tiny = false;
    const int sv = sub_stage_issue(c, r + 1);  // row r+1's indices, committed below
    if (rc.cnt > 0 && c.first) {
        // Iteration 0 of the static decoder (uniform): E_old = 0 and M = ch, so
        // t depends on (column, frame) only and sub_tanh_table has left it in
        // L[col] -- one gather per slot where the other passes gather the
        // posterior, no E_old request, no tanh.  A frame-less lane's L holds
        // no table (it may hold a finished frame's outputs): its slots are 1.0.
        const int njt = c.live ? sub_nj(c, rc) : 0;
        const uint16_t *lc = sub_lcols(c, r, rc);
        int col[K];
#pragma unroll
        for (int i = 0; i < K; ++i) col[i] = lc[i];
#pragma unroll
        for (int i = 0; i < K; ++i) t[i] = ld_l2((const double *)(c.Lu + sub_off(c, col[i])));
#pragma unroll
        for (int i = 0; i < K; ++i) {
            tiny |= i < njt && !(fabs(t[i]) > kTiny);
            t[i] = i < njt ? t[i] : 1.0;
        }
    } else if (rc.cnt > 0) {
        const int nj = sub_nj(c, rc);
        const int njt = c.live ? nj : 0;  // the |t| <= 1e-10 vote: frame-less lanes abstain
        const uint16_t *lc = sub_lcols(c, r, rc);
        const uint32_t eoff = sub_eoff(c, rc);
        // a fresh streaming frame: M = L
        const bool noE = c.fresh;
        int col[K];
        double eo[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            // a fresh frame's lanes read no E_old (on a streaming pass most
            // slots hold fresh frames)
            eo[i] = ld_sub_msg(c.rE, noE ? kSubOOB : eoff + (uint32_t)i * (kTile * sizeof(double)));
            col[i] = lc[i];
        }
#pragma unroll
        for (int i = 0; i < K; ++i) t[i] = ld_l2((const double *)(c.Lu + sub_off(c, col[i])));
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const double M = noE ? t[i] : t[i] - eo[i];  // :85-90 / :260-268
            const double d = M * 0.5;
            // :138-146 as np_tanh of M/2 clamped to +-17.5 (spa_math.h
            // tanh_half_clipped: equal to the reference's clip for every M)
            double th[1] = {dfrom(dbits(fmin(fabs(d), 17.5)) | (dbits(d) & 0x8000000000000000ull))};
            np_tanh_n<1, LdsTanh, true>(th, c.ttab);
            const double tv = th[0];
            tiny |= i < njt && !(fabs(tv) > kTiny);
            // slots past this lane's piece: 1.0, an exact no-op in the chain product
            t[i] = i < nj ? tv : 1.0;
        }
    }
    sub_stage_commit(c, r + 1, sv);
    return __ballot(tiny) != 0ull;
}

// Iteration 0's tanh, once per column and frame instead of once per edge (575
// edges per column of wimax_2304_0.5): T[col][f] = np_tanh(clamp(ch[col][f]/2))
// by sub_p1's own expression, so the bits are the ones its per-edge evaluation
// gives.  T lives in the tile's L, which the static decoder does not read in
// iteration 0 (the column sweep compares with ch) and overwrites column by
// column for every live frame: the A columns in the column sweep after the row
// loop, the identity column k + r in P3(r) -- read before that only by P1(r) of
// the same wavefront, the one that holds the row's last edge.  Frame-less lanes
// leave L alone.  The whole workgroup, (wavefront, lane group) pair `me` of
// `nthr` taking every nthr-th column; the caller makes the stores visible.
// Returns whether a table value of this lane's live frame has |t| <= 1e-10
// (sub_p1's rare-row predicate; a NaN LLR too): the column form of iteration 0
// (sub_pass0_cols) has no rare rows and leaves such a sub-tile to the row loop.
// The columns below `kl` (the A columns, or 0: none) are staged in the S region
// of LDS as well, [col][F], for phase A of the column form: every lane of a
// lane group writes its element, a frame-less lane 1.0, so all kl x F are
// initialised.  A caller that then takes the row loop zeroes S again.
template <int Q>
__device__ __forceinline__ bool sub_tanh_table(const SubCtx<Q> &c, int n, int me, int nthr, int kl) {
    constexpr int F = SubCfg<Q>::F;
    bool tiny = false;
    for (int col = me; col < n; col += nthr) {
        const double d = *sub_c(c, col) * 0.5;
        double th[1] = {dfrom(dbits(fmin(fabs(d), 17.5)) | (dbits(d) & 0x8000000000000000ull))};
        np_tanh_n<1, LdsTanh, true>(th, c.ttab);
        tiny |= !(fabs(th[0]) > kTiny);
        if (c.live) *sub_l(c, col) = th[0];
        if (col < kl) c.S[(size_t)col * F] = c.live ? th[0] : 1.0;
    }
    return tiny && c.live;
}

// Lane-group hand-over for Q = 4 (lane = j*16 + f: group j is DPP row j) with
// gfx950's v_permlane16_swap / v_permlane32_swap (VALU, no LDS round trip):
// permlane16_swap(x, x) -> {[x0 x0 x2 x2], [x1 x1 x3 x3]} (rows),
// permlane32_swap(x, x) -> {[x0 x1 x0 x1], [x2 x3 x2 x3]}.
__device__ __forceinline__ uint32_t p16(uint32_t x, int which) {
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    return which ? r[1] : r[0];
}
__device__ __forceinline__ uint32_t p32(uint32_t x, int which) {
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return which ? r[1] : r[0];
}
// value of group jj moved into group jj+1 (other groups: don't care)
__device__ __forceinline__ double group_up4(double v, int jj) {
    const uint64_t u = dbits(v);
    uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
    if (jj == 1) {  // row 1 -> row 2: [x0 x1 x0 x1] then its odd rows
        lo = p16(p32(lo, 0), 1);
        hi = p16(p32(hi, 0), 1);
    } else {  // row 0 -> 1, row 2 -> 3
        lo = p16(lo, 0);
        hi = p16(hi, 0);
    }
    return dfrom(((uint64_t)hi << 32) | lo);
}


// P * t[0] * ... * t[n-1] as exactly n dependent multiplies (a uniform branch
// on n selects a straight-line sequence; slots past a lane's piece hold 1.0)
template <int K, int N>
struct SubMul {
    static __device__ __forceinline__ double run(double P, const double (&t)[K], int n) {
        if (n == N) {
#pragma unroll
            for (int i = 0; i < N; ++i) P = P * t[i];
            return P;
        }
        return SubMul<K, N - 1>::run(P, t, n);
    }
};
template <int K>
struct SubMul<K, 0> {
    static __device__ __forceinline__ double run(double P, const double (&)[K], int) { return P; }
};

// hop: this wavefront's chunk of row r's left-to-right product.  Round jj
// multiplies lane group jj's slots into the running product (every lane
// computes; group jj's lanes hold the value that matters) and moves it to
// group jj+1.
template <int Q>
__device__ __forceinline__ void sub_hop(const SubCtx<Q> &c, int r, const double (&t)[SubCfg<Q>::K], bool tiny) {
    constexpr int F = SubCfg<Q>::F, K = SubCfg<Q>::K;
    const SubChunk rc = sub_chunk(c.row_ptr, r, c.wave, Q);
    if (rc.deg == 0) return;  // spa_decoder.py:115-122
    const int s = r & (kSR - 1);
    const int ep = ((c.ep0 + r) & 0x3ffffff) * 32;
    double *sl = c.slot + s * F;
    double P = 1.0;  // 1.0 * t0 == t0 exactly
    SUB_STAMP(h0);
    if (c.wave != 0) {
        wait_flag<false>(c.flag + s, ep + c.wave);
        P = *sl;
    }
    SUB_STAMP(h1);
    SUB_ADD(c, 0, h0, h1);
    __builtin_amdgcn_s_setprio(2);
    int last = -1;
    if (Q == 4 && rc.cnt > 0) {
        // branch-free: every lane group multiplies all K slots (slots past its
        // piece and every slot of a group past the chunk hold 1.0, sub_p1:
        // exact no-ops), so the product ends in group 3 -- no uniform
        // branches between the dependent multiplies
#pragma unroll
        for (int jj = 0; jj < Q; ++jj) {
#pragma unroll
            for (int i = 0; i < K; ++i) P = P * t[i];
            if (jj + 1 < Q) P = group_up4(P, jj);
        }
        last = Q - 1;
    } else {
#pragma unroll
        for (int jj = 0; jj < Q; ++jj) {
            if (jj * rc.CS < rc.cnt) {  // lane group jj holds edges of this chunk (uniform)
                const double Pl = SubMul<K, K>::run(P, t, rc.CS);
                last = jj;
                if (jj + 1 < Q && (jj + 1) * rc.CS < rc.cnt)
                    P = group_up4(Pl, jj);
                else
                    P = Pl;
            }
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (c.wave == 0)
            lds_st(c.tinyf + s, tiny ? 1 : 0);
        else if (tiny)
            lds_st(c.tinyf + s, 1);
    }
    if (c.j == last) *sl = P;
    lds_release();
    if ((threadIdx.x & 63) == 0) lds_st(c.flag + s, ep + c.wave + 1);
    __builtin_amdgcn_s_setprio(0);
    SUB_STAMP(h2);
    SUB_ADD(c, 1, h1, h2);
}

// P3: E_new of this lane's slots of row r, stored and folded into S; the
// identity column's posterior and z^1 bit.
// row r-1's P3 by the wavefronts whose column spans overlap this one's (sub_p3)
template <int Q>
__device__ __forceinline__ void sub_order(const SubCtx<Q> &c, int r) {
    if (r > 0) {
        const int d = ld_table(c.p3dep, r * kSW + c.wave);
        for (int v = d & 0xff; v <= (d >> 8); ++v) wait_ge<false>(c.p3row + v, r);
    }
}
template <int Q>
__device__ __forceinline__ void sub_p3_body(SubCtx<Q> &c, int r, double (&t)[SubCfg<Q>::K]) {
    constexpr int F = SubCfg<Q>::F, K = SubCfg<Q>::K;
    const SubChunk rc = sub_chunk(c.row_ptr, r, c.wave, Q);
    if (rc.deg == 0) return;
    const int s = r & (kSR - 1);
    const int ep = ((c.ep0 + r) & 0x3ffffff) * 32;
    // the identity column k + r is the row's last edge (an [A | I] graph):
    // the lane whose piece ends there requests its channel LLR now, ahead of
    // the chain wait (+1 % with the late S-order wait below, profiles/r5n_ab)
    // (every lane requests it: a conditional load leaves the compiler's
    // vmcnt count inexact; the 16 frames' 128 B are one line for all lanes)
    const double chI = *sub_c(c, c.k + r);
    SUB_STAMP(q0);
    wait_flag<false>(c.flag + s, ep + kSW);
    SUB_STAMP(q1);
    SUB_ADD(c, 2, q0, q1);
    const bool tiny_row = uniform(lds_ld(c.tinyf + s)) != 0;
    if (rc.cnt == 0) {  // no edges here (short rows): still take part in a rare row's parking count
        sub_order(c, r);
        if (tiny_row) {
            c.ntiny += 1;
            if ((threadIdx.x & 63) == 0)
                __hip_atomic_fetch_add(c.tseq, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            wait_flag<false>(c.tseq, c.ntiny * kSW);
        }
        return;
    }
    const double P = c.slot[s * F];
    const int nj = sub_nj(c, rc);
    const uint16_t *lc = sub_lcols(c, r, rc);
    int col[K];
#pragma unroll
    for (int i = 0; i < K; ++i)
        col[i] = lc[i];  // clamped copy past the chunk: a valid column
    if (!tiny_row) {
        // q = P/t (div_nr: the IEEE quotient without the scaling steps,
        // cn_common.h), then E_new = 2 atanh(clip(q)) (:159-168) -- or 2q when
        // every quotient of the wavefront is below 2^-27, where that is exact
        // (spa_math.h kAtanhIdent; the common case on long rows at low SNR)
        bool big = false;
        const double lim = c.live ? kAtanhIdent : INFINITY;  // frame-less lanes do not vote
        if (div_nr_ok(c.live ? P : 1.0)) {
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (i < rc.CS) {
                    t[i] = div_nr(P, t[i]);
                    big |= !(fabs(t[i]) < lim);
                }
        } else {
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (i < rc.CS) {
                    t[i] = P / t[i];
                    big |= !(fabs(t[i]) < lim);
                }
        }
        if (__ballot(big) == 0ull) {
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (i < rc.CS) t[i] = 2.0 * t[i];
        } else {
            const AtanhCoef ac = c.coef_arg ? c.ac : coef_load();  // scalar loads here (cn_common.h)
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (i < rc.CS) t[i] = 2.0 * atanh_f(clip_cl(t[i]), c.ltab, ac);
        }
    } else {
        // rare: q = in-order product of the others (np.prod(np.delete(...)),
        // :164) for an edge with |t| <= 1e-10; t parked at row positions
        const int rb = c.row_ptr[r];
        double *tb = c.Tb + (c.ntiny & 1) * c.tbuf;  // the next rare row parks in the other buffer
#pragma unroll
        for (int i = 0; i < K; ++i)
            if (i < rc.CS && i < nj) tb[(size_t)(sub_edge(c, rc, i) - rb) * F] = t[i];
        __builtin_amdgcn_s_waitcnt(0);  // scratch stores have reached L2
        c.ntiny += 1;
        if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(c.tseq, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        wait_flag<false>(c.tseq, c.ntiny * kSW);
        const AtanhCoef ac = c.coef_arg ? c.ac : coef_load();  // scalar loads here (cn_common.h)
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (i < rc.CS) {
                const double ti = t[i];
                double q;
                if (fabs(ti) > kTiny || i >= nj) {
                    q = P / ti;
                } else {
                    const int pos = sub_edge(c, rc, i) - rb;
                    q = 1.0;
                    bool fst = true;
                    for (int p = 0; p < rc.deg; ++p) {
                        if (p == pos) continue;
                        const double t2 = ld_l2(tb + (size_t)p * F);
                        q = fst ? t2 : q * t2;
                        fst = false;
                    }
                }
                t[i] = 2.0 * atanh_f(clip_cl(q), c.ltab, ac);
            }
        }
    }
    if (c.verify) {
        // The verifying pass of the static decoder's fixed-point exit
        // (tile_sub_kernel; uniform, false on every other pass): the E_old that
        // each own E_new store replaces is loaded again through the buffer
        // resource (masked slots at kSubOOB request nothing) and compared with
        // E_new bit for bit; a difference sets the frame's flag.  The loads
        // are compared, so they have returned, before the stores issue.
        // Here and not ahead of the chain wait: E_old held from there costs 20
        // registers of every pass's row loop, this block none outside itself.
        // Only the slots that differ are stored: memory holds E_new either
        // way, and at a fixed point no slot differs -- the pass writes no
        // message at all, and a wavefront none of whose lanes found a
        // difference (nearly every one of such a pass) skips the rest of this
        // block.
        // The others run the next-pass proof before they store (c.prove).
        // The posterior of each own slot's column is gathered, half of the
        // slots at a time.  (Issued with the E_old reloads in every wavefront,
        // the gathers spilled values of every pass's row loop and cost more
        // than the exit won.)  During the row loop memory still holds L_old:
        // the column sweep writes the A columns after it, this P3 the identity
        // column k + r further down.  The variable-to-check value that this
        // pass formed, L_old - E_old, is compared bit for bit with the one the
        // next pass would form from E_new, and the identity column's new
        // posterior, which the next pass would gather, with L_old.  A slot
        // whose message repeated passes both tests as it stands (for iteration
        // >= 1 the identity column's L = ch + (0 + E) repeats if E does);
        // frame-less lanes and padded slots abstain.
        // One failure anywhere in the workgroup ends the proof for this pass
        // (bit 2 of every frame's flag; bit 1: this frame's own proof failed,
        // or a difference of its went untested): the sub-tile runs on for the
        // failing frame whatever the others prove, so the exit then takes no
        // frame by the proof and the remaining rows gather nothing (where
        // frames drift, that is after a row or two).
        const uint32_t eoff = sub_eoff(c, rc);
        const int njv = c.live ? nj : 0;
        double eold[K];
#pragma unroll
        for (int i = 0; i < K; ++i)
            eold[i] = ld_sub_msg(c.rE, i < njv ? eoff + (uint32_t)i * (kTile * sizeof(double)) : kSubOOB);
        bool d = false;
#pragma unroll
        for (int i = 0; i < K; ++i) d |= i < njv && dbits(eold[i]) != dbits(t[i]);
        if (__builtin_expect(__ballot(d) != 0ull, 0)) {
            constexpr int H = (K + 1) / 2;
            bool nx = false;
            // the flag only gains bits: a stale read costs one more test;
            // without c.prove no frame is tested, and an untested difference
            // counts as a failure
            const bool open = c.prove && d && (lds_ld(c.mdiff + (threadIdx.x & (F - 1))) & 6) == 0;
            if (__ballot(open) != 0ull) {
#pragma unroll
                for (int h = 0; h < K; h += H) {
                    __builtin_amdgcn_sched_barrier(0);  // one half's gathers at a time
                    double lo[H];
#pragma unroll
                    for (int i = 0; i < H; ++i)
                        lo[i] = ld_l2((const double *)(c.Lu + sub_off(c, col[min(h + i, K - 1)])));
#pragma unroll
                    for (int i = 0; i < H; ++i)
                        if (h + i < K) {
                            const int q = h + i;
                            nx |= q < njv && dbits(lo[i] - eold[q]) != dbits(lo[i] - t[q]);
                            nx |= q < njv && col[q] >= c.k && dbits(chI + (0.0 + t[q])) != dbits(lo[i]);
                        }
                }
            }
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const bool di = i < njv && dbits(eold[i]) != dbits(t[i]);
                st_sub_msg(c.rE, di ? eoff + (uint32_t)i * (kTile * sizeof(double)) : kSubOOB, t[i]);
            }
            if (d) atomicOr((uint32_t *)c.mdiff + (threadIdx.x & (F - 1)), (nx || !open) ? 3u : 1u);
            // a failure: the proof of this pass is over for every frame of the workgroup
            if (__ballot(nx) != 0ull && (threadIdx.x & 63) < F) atomicOr((uint32_t *)c.mdiff + (threadIdx.x & 63), 4u);
        }
    } else {
        const uint32_t eoff = sub_eoff(c, rc);
#pragma unroll
        for (int i = 0; i < K; ++i)  // nj <= CS
            st_sub_msg(c.rE, (i < nj && c.live) ? eoff + (uint32_t)i * (kTile * sizeof(double)) : kSubOOB, t[i]);
    }
    // S_col += E_new, rows ascending (a column occurs once per row: no two
    // lanes of a row share (col, frame)); the identity edge goes to `dummy`
    double EnI = 0.0;
    int colI = -1;
    double *sp[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const bool own = i < nj;  // nj <= CS
        const bool a = own && col[i] < c.k;
        sp[i] = a ? c.S + (size_t)col[i] * F : c.dummy;
        if (own && !a) {
            EnI = t[i];
            colI = col[i];
        }
    }
    // S order: only the additions wait for the overlapping wavefronts' row
    // r-1 (the math and the E_new stores above run meanwhile)
    SUB_STAMP(q2);
    SUB_ADD(c, 3, q1, q2);
    sub_order(c, r);
    SUB_STAMP(q3);
    SUB_ADD(c, 4, q2, q3);
#pragma unroll
    for (int i = 0; i < K; ++i)  // one ds_add_f64 per slot; slots past the piece add into `dummy` (never read)
        __hip_atomic_fetch_add(sp[i], t[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (colI >= 0) {  // identity column: L = ch + (0 + E) (:173-185)
        const double Lj = chI + (0.0 + EnI);
        if (c.live) *sub_l(c, colI) = Lj;
        if (!(Lj < 0.0)) {
            const int q = colI - c.k;
            atomicOr(c.ib + (q >> 5) * F, 1u << (q & 31));
        }
    }
    SUB_STAMP(q4);
    SUB_ADD(c, 5, q3, q4);
}

// P3 of row r.  S_col must take its additions rows ascending.  Wavefront w's
// chunk of row r spans columns [first, last]; extended to the gap before it,
// the chunks of a row partition the columns, so waiting for row r-1's P3 by
// exactly the wavefronts whose extended spans overlap w's (g.p3dep, built on
// the host: ldpc_api.cpp sub_p3_deps) orders every column's additions by
// induction over the rows -- the neighbours, not all 16 wavefronts (the full
// row barrier this replaces cost early wavefronts up to 39 % of their time,
// profiles/r2an_phase_timers).  p3row[v] = 1 + the last row r of THIS pass
// whose P3 wavefront v finished; sub_p3_reset zeroes it between passes (after
// the barrier that ends a pass's rows), so the count never exceeds m + 1 however
// many passes a streaming launch makes.
template <int Q>
__device__ __forceinline__ void sub_p3(SubCtx<Q> &c, int r, double (&t)[SubCfg<Q>::K]) {
    sub_p3_body<Q>(c, r, t);
    lds_release();  // this row's S additions before the count
    if ((threadIdx.x & 63) == 0)
        lds_st(c.p3row + c.wave, r + 1);
}
// Between passes: every wavefront has finished (and waited on) the pass's
// P3s -- call after the barrier that ends the row loop, before the next one.
__device__ __forceinline__ void sub_p3_reset(int *p3row) {
    if (threadIdx.x < kSW) p3row[threadIdx.x] = 0;
}
// Chain-flag epoch of a pass: (pass * m) mod 2^26, so ep0 + r (masked again
// where used) neither overflows nor breaks the sequence of epochs across passes.
__device__ __forceinline__ int sub_epoch0(int pass, int m) {
    return (int)(((uint32_t)pass * (uint32_t)m) & 0x3ffffffu);
}

template <int Q>
__device__ __forceinline__ void sub_body(SubCtx<Q> &c, int r, int m, double (&tcur)[SubCfg<Q>::K], bool ycur,
                                         double (&toth)[SubCfg<Q>::K], bool &yoth) {
    if (r < m) sub_hop(c, r, tcur, ycur);
    if (r >= 1) sub_p3<Q>(c, r - 1, toth);
    SUB_STAMP(p0);
    if (r + 1 < m) yoth = sub_p1<Q>(c, r + 1, sub_chunk(c.row_ptr, r + 1, c.wave, Q), toth);
    SUB_STAMP(p1);
    SUB_ADD(c, 6, p0, p1);
}

// Iteration 0 of the static decoder column by column, in place of its row loop
// and A-column sweep (bit 2 of fp; LDPC_PASS0_COLS=0 keeps the row loop).  There
// E_old = 0 and M = ch, so with T = sub_tanh_table's values in L
//   P_r        = ((1.0 * T[c0]) * T[c1]) * ...   row r's columns ascending, the
//                identity column last: sub_hop's multiplies (its padded 1.0s
//                are exact no-ops),
//   E0(r, col) = g(P_r / T[col])                 sub_p3_body's quotient, vote and atanh,
//   S_col      = ((0.0 + E0(r0, col)) + E0(r1, col)) + ...   rows ascending.
// Rows are independent of each other and so are columns: no chain, no flags,
// no order waits, no LDS additions -- three phases between workgroup barriers.
//   A  lane = (row, frame), 64 rows per step: each lane walks its row's
//      col_idx and multiplies the gathered table values in order; P_r goes to
//      LDS as [m][F] in the S region (unused until pass 1: the caller checks
//      m <= k).  A frame-less lane's P is 1.0.
//      With `lds` (bit 3 of fp; LDPC_PASS0_LDS=0 switches it off) the A
//      columns' factors come from LDS: sub_tanh_table has staged T[col][f],
//      col < k, in the S region (k x F doubles: all of it), which ends the
//      gather of 8 B per edge and frame from L (the same 147 KB about 575
//      times over for wimax_2304_0.5; L2 served most of it).  The row's last
//      factor, its identity column's, is gathered from L once per row; the
//      multiplies and their order are the same.  P_r cannot go to S while the
//      table is there: it is stored in the row's identity-edge slot of E (CSR
//      position row_ptr[r+1] - 1, private to the row; frame-less lanes at
//      kSubOOB), the workgroup meets at a barrier (release / acquire around
//      it), each lane reads its products back and places them in S as above,
//      and a second barrier starts phase B, which is unchanged and overwrites
//      the slot with E0(r, k + r) when it reaches the identity columns.
//   B  lane = (column, frame), 64 columns per step, the A columns and then the
//      identity columns: each lane walks its column's CSC list (rows
//      ascending, DevGraph::csc_*), forms E0 from P_r (LDS) and its own T,
//      stores it at the edge's CSR position (non-temporal; frame-less lanes at
//      kSubOOB) and adds it to S in a register; then L = ch + S, the
//      normalized-LLR count and the fixed-point trigger against ch (A columns
//      only, as the sweep), the z^1 bit.  L[col] overwrites T[col] after its
//      only reader in this phase.  div_nr and the 2q short cut are voted per
//      wavefront step as in sub_p3_body; both are exact where they apply, so
//      which lanes share a vote does not change a bit.  The wavefronts meet at
//      a barrier every kP0Step list positions, so the workgroup's stores stay
//      within a window of rows.
// No table value is tiny here (the caller's vote), so no row is rare.  S is
// left zero for pass 1; the caller adds my_cnt / pd into LDS as after the sweep.
constexpr int kP0Step = 128;
__device__ __forceinline__ int sub_group_max(int v) {  // max over the lane groups' first lanes (Q = 4)
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
template <int Q>
__device__ __forceinline__ void sub_pass0_cols(const SubCtx<Q> &c, const DevGraph &g, double *S0, uint32_t *zb,
                                               int nllr, int me, int nthr, bool lds, int &my_cnt, bool &pd) {
    static_assert(Q == 4, "lane groups of 16");
    constexpr int F = SubCfg<Q>::F;
    // Edges per step of a lane: phase A's gathers in flight, phase B's index loads.  Larger steps measured
    // the same pass 0 (profiles/r10_pass0_cols) and some of them move this kernel's spills into the row
    // loop of the other passes.
#ifndef LDPC_P0_UA
#define LDPC_P0_UA 4
#define LDPC_P0_UB 4
#endif
    constexpr int UA = LDPC_P0_UA, UB = LDPC_P0_UB;
    static_assert(kP0Step % UB == 0, "a barrier window is whole steps");
    const int m = c.m, n = g.n;
    // A: row products
    for (int r0 = 0; r0 < m; r0 += nthr) {
        const int row = r0 + me, rr = min(row, m - 1);
        const int beg = c.row_ptr[rr];
        const int deg = row < m ? c.row_ptr[rr + 1] - beg : 0;
        const int last = min(beg + max(deg, 1), g.nnz) - 1;  // std_form: deg >= 1
        const int nmax = sub_group_max(deg);
        double P = 1.0;  // 1.0 * t0 == t0 exactly
        int cn[UA];
#pragma unroll
        for (int u = 0; u < UA; ++u) cn[u] = sub_col(c, min(beg + u, last));
        if (lds) {
            // the row's last factor, its identity column's, is not staged: one gather from L per row
            const double tI = ld_l2((const double *)(c.Lu + sub_off(c, sub_col(c, last))));
            for (int i = 0; i < nmax; i += UA) {
                double t[UA];
#pragma unroll
                for (int u = 0; u < UA; ++u) t[u] = c.S[(size_t)min(cn[u], c.k - 1) * F];
#pragma unroll
                for (int u = 0; u < UA; ++u) {
                    t[u] = cn[u] < c.k ? t[u] : tI;
                    cn[u] = sub_col(c, min(beg + i + UA + u, last));  // the next step's
                }
#pragma unroll
                for (int u = 0; u < UA; ++u) P = P * ((i + u < deg && c.live) ? t[u] : 1.0);
            }
            // held in the row's identity-edge slot of E (its last CSR position: private to the row, and
            // phase B writes E0(r, k + r) there after everything else) while the table occupies S
            st_sub_msg(c.rE, (row < m && c.live) ? ((uint32_t)last << 9) + c.lo8 : kSubOOB, P);
        } else {
            for (int i = 0; i < nmax; i += UA) {
                double t[UA];
#pragma unroll
                for (int u = 0; u < UA; ++u) t[u] = ld_l2((const double *)(c.Lu + sub_off(c, cn[u])));
#pragma unroll
                for (int u = 0; u < UA; ++u) cn[u] = sub_col(c, min(beg + i + UA + u, last));  // the next step's
#pragma unroll
                for (int u = 0; u < UA; ++u) P = P * ((i + u < deg && c.live) ? t[u] : 1.0);
            }
            if (row < m) c.S[(size_t)row * F] = P;
        }
    }
    if (lds) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();  // the staged table is dead: every row product formed and on its way to E
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        for (int row = me; row < m; row += nthr) {
            const uint32_t last = (uint32_t)c.row_ptr[row + 1] - 1u;
            const double P = ld_sub_msg(c.rE, c.live ? (last << 9) + c.lo8 : kSubOOB);
            c.S[(size_t)row * F] = c.live ? P : 1.0;  // a frame-less lane held nothing
        }
    }
    __syncthreads();  // every P_r in LDS, every gather of the table done
    // B: columns
    const int lastp = g.nnz - 1;
    for (int c0 = 0; c0 < n; c0 += nthr) {
        const int col = c0 + me, cc = min(col, n - 1);
        const int beg = g.csc_ptr[cc];
        const int deg = col < n ? g.csc_ptr[cc + 1] - beg : 0;
        const int nmax = sub_group_max(deg);
        const double chj = *sub_c(c, cc);
        const double Tl = ld_l2(sub_l(c, cc));
        const double T = c.live ? Tl : 1.0;  // a frame-less lane's L holds no table
        double S = 0.0;
        for (int i0 = 0; i0 < g.max_col_deg; i0 += kP0Step) {
            const int iend = min(i0 + kP0Step, nmax);
            for (int i = i0; i < iend; i += UB) {
                int e[UB], r[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const int p = min(beg + i + u, lastp);
                    e[u] = g.csc_edge[p];
                    r[u] = g.csc_row[p];
                }
                double Pr[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u) Pr[u] = c.S[(size_t)r[u] * F];
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const bool act = i + u < deg;
                    const bool own = act && c.live;  // abstains from the votes and stores nothing otherwise
                    const double P = own ? Pr[u] : 1.0;
                    double q;
                    if (div_nr_ok(P))
                        q = div_nr(P, T);
                    else
                        q = P / T;
                    const bool big = own && !(fabs(q) < kAtanhIdent);
                    double E;
                    if (__ballot(big) == 0ull) {
                        E = 2.0 * q;
                    } else {
                        const AtanhCoef ac = c.coef_arg ? c.ac : coef_load();
                        E = 2.0 * atanh_f(clip_cl(q), c.ltab, ac);
                    }
                    st_sub_msg(c.rE, own ? ((uint32_t)e[u] << 9) + c.lo8 : kSubOOB, E);
                    S = act ? S + E : S;
                }
            }
            __syncthreads();
        }
        if (col < n) {
            const double Lj = chj + S;  // an identity column: ch + (0.0 + E)
            if (col < c.k) {
                if (nllr) my_cnt += (fabs(Lj) <= 7.0 && chj * Lj < 0.0) ? 1 : 0;
                pd |= dbits(chj) != dbits(Lj);
                if (!(Lj < 0.0)) atomicOr(zb + (col >> 5) * F + c.f, 1u << (col & 31));
            } else if (!(Lj < 0.0)) {
                const int q = col - c.k;
                atomicOr(c.ib + (q >> 5) * F, 1u << (q & 31));
            }
            if (c.live) *sub_l(c, col) = Lj;
        }
    }
    // the last barrier above: every P_r read (with `lds`, S held k x F table values: m <= k)
    for (int i = threadIdx.x; i < (lds ? c.k : m) * F; i += blockDim.x) S0[i] = 0.0;
}

// Fixed-point exit (fp != 0; LDPC_FIXED_POINT=0 switches it off).  A pass is a
// deterministic function of (E, L) and ch, its summation order fixed by the
// p3dep waits, so a frame whose pass reproduced E and L bit for bit repeats
// that state on every later pass: it stops there with the outputs of pass
// max_iter (failed frames at low SNR: the headline's frames stop after 3 of
// 50 passes).  Nothing approximate:
//   trigger  the column sweep compares each A-column posterior with the
//            previous one (ch on iteration 0) bit for bit: pdiffl[f];
//   verify   a pass at iteration >= 1, when some running frame's posteriors
//            repeated in the pass before, compares every own E_new with the
//            E_old it replaces (c.verify, sub_p3_body): bit 0 of mdiffl[f], and
//            stores only the ones that differ (at a fixed point: none).  The
//            identity columns need no check: for iteration >= 1
//            L = ch + (0 + E) of the row's last edge repeats if E does;
//   proof    (bit 1 of fp; LDPC_FP_NEXT=0 switches this rule alone off) a
//            verifying pass whose messages differed can still prove that the
//            NEXT pass reproduces its output.  Pass `it` maps (E_old, L_old) to
//            (E_new, L_new).  If L_new == L_old bit for bit on every column
//            and, for every edge, fl(L_old[col] - E_new) has the bits of
//            fl(L_old[col] - E_old), pass it + 1 forms exactly the
//            variable-to-check values M that pass `it` formed, and everything
//            after M -- the clamp, tanh, the chain product, the rare-row
//            branch, the division, atanh, the S additions in p3dep order -- is
//            a function of M in a fixed order: E and L after pass it + 1 are
//            E_new and L_new, a fixed point from there on.  (A message far
//            below its posterior's last bit moves without moving M: the
//            headline's stragglers, whose sub-tiles ran a 4th pass for one or
//            two frames.)  The A columns' half of "L_new == L_old" is the
//            trigger's pdiffl[f]; sub_p3_body tests the rest where a message
//            differed.  "No message differed" is the special case
//            E_new == E_old.  The first failure in the workgroup (bit 2 of every
//            frame's mdiffl) ends the proof for that pass: the sub-tile
//            runs on for the failing frame whatever the others prove, so the
//            rest of the pass gathers nothing and the pass takes no frame by
//            the proof (the same frames whichever wavefront saw the flag when);
//   exit     after a verifying pass, a running frame with no posterior
//            difference in that pass and either no message difference or a
//            proof that stood (syndrome non-zero: a zero one took the OK exit)
//            stops as DATA_TRANSFER_NOT_OK after max_iter iterations, memory
//            holding E_new and L_new; its normalized-LLR history continues
//            with the 0 that every later pass would count (ap == Lj);
//   back-off a verifying pass that stopped no frame is followed by a gap of
//            1, 2, 4, ... passes before the next: at most 6 such verifying
//            passes (iterations 1, 3, 6, 11, 20, 37) at T = 50.
// The proof runs inside the verifying passes only, and those are scheduled as
// before it existed.  (It holds for most headline frames after pass 1 already;
// a verifying pass at iteration 1 happens only where a frame's posteriors
// equalled ch after pass 0.)
// st.fp_count: frames stopped this way, frame-passes not executed.
template <int Q>
__global__ __launch_bounds__(64 * kSW, 1) void tile_sub_kernel(DevGraph g, DevState st, int max_iter, int nllr,
                                                               const int *__restrict__ col_idx,
                                                               const int *__restrict__ row_ptr, AtanhCoef ac, int fp) {
    constexpr int F = SubCfg<Q>::F, K = SubCfg<Q>::K;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    // per frame: a posterior differed in this pass / the bits of SubCtx::mdiff
    __shared__ int pdiffl[F], mdiffl[F];
    const SubLayout ly = sub_layout(g.k, g.m, F);
    double *S = (double *)(lds + ly.S);
    MathLds &mlds = *(MathLds *)(lds + ly.math);
    uint32_t *zb = (uint32_t *)(lds + ly.zb);
    uint32_t *ib = (uint32_t *)(lds + ly.ib);
    int *bad = (int *)(lds + ly.lane_i);
    int *cntl = bad + F;
    int *livel = cntl + F;
    int *flags = (int *)(lds + ly.flags);
    const int kw = (g.k + 31) >> 5, mw = (g.m + 31) >> 5;
    const int tile = blockIdx.x / Q, sub = blockIdx.x % Q;
    if (tile >= st.ntiles) return;  // block-uniform

    fill_math_lds(mlds);
    for (int i = threadIdx.x; i < g.k * F; i += blockDim.x) S[i] = 0.0;
    for (int i = threadIdx.x; i < (kw + mw) * F; i += blockDim.x) zb[i] = 0u;
    for (int i = threadIdx.x; i < 2 * F; i += blockDim.x) bad[i] = 0;
    if (threadIdx.x < 2 * kSR) flags[threadIdx.x] = -1;
    if (threadIdx.x >= 2 * kSR && threadIdx.x < 2 * kSR + 2 + kSW) flags[threadIdx.x] = 0;
    const int lane = threadIdx.x & 63;
    const int wave = uniform(sub_wave(threadIdx.x >> 6));
    const int j = lane / F, f = lane % F;
    const int fr = tile * kTile + sub * F + f;  // this lane's frame
    if (wave == 0 && j == 0) {
        livel[f] = st.done[fr] == 0 ? 1 : 0;
        pdiffl[f] = 0;
        mdiffl[f] = 0;
    }
    __syncthreads();
    if (!st.tile_active[tile]) return;
    {  // a sub-tile with no live frame (a ragged batch's last tile) has nothing to do
        int any = 0;
#pragma unroll
        for (int ff = 0; ff < F; ++ff) any |= livel[ff];
        if (!any) return;  // block-uniform: LDS after the barrier
    }

    SubCtx<Q> c;
    c.col_idx = col_idx;
    c.row_ptr = row_ptr;
    const size_t lo = (size_t)sub * F + f;
    c.Eb = st.E + (size_t)tile * g.nnz * kTile + lo;
    c.Lb = st.L + (size_t)tile * g.n * kTile + lo;
    c.Cb = st.ch + (size_t)tile * g.n * kTile + lo;
    c.Eu = (const char *)(st.E + (size_t)tile * g.nnz * kTile);
    c.rE = sub_rsrc(c.Eu, (size_t)g.nnz * kTile * sizeof(double));
    c.Lu = (const char *)(st.L + (size_t)tile * g.n * kTile);
    c.Cu = (const char *)(st.ch + (size_t)tile * g.n * kTile);
    c.lo8 = (uint32_t)lo * 8u;
    c.Tb = st.T + (size_t)blockIdx.x * 2 * g.max_row_deg * F + f;
    c.tbuf = (size_t)g.max_row_deg * F;
    c.S = S + f;
    c.dummy = (double *)(lds + ly.dummy) + f;
    c.slot = (double *)(lds + ly.slot) + f;
    c.ib = ib + f;
    c.cidx = (uint16_t *)(lds + ly.cidx) + wave * Q * K;
    c.m = g.m;
    c.flag = flags;
    c.tinyf = flags + kSR;
    c.tseq = flags + 2 * kSR;
    c.p3row = flags + 2 * kSR + 2;
    c.p3dep = g.p3dep;
    c.ttab = LdsTanh{mlds.tanh};
    c.ltab = LdsAtanh{mlds.atanh};
    c.coef_arg = false;  // the static decoder loads them (1 dB: atanh on few rows)
    c.ac = ac;
    c.k = g.k;
    c.wave = wave;
    c.j = j;
    c.f = f;
    c.ntiny = 0;
    c.fresh = false;
    c.mdiff = mdiffl;
#ifdef LDPC_SUB_TIMERS
    for (int i = 0; i < SUB_NT; ++i) c.tm[i] = 0;
#endif
    const int m = g.m;
    const int nthr = kSW * Q;       // (wavefront, lane group) pairs
    const int me = wave * Q + j;    // this lane's pair

    // fixed-point exit, uniform over the workgroup: ctl = the word wavefront 0
    // left after the last pass (1: a frame still runs, 2: a running frame's
    // posteriors repeated, 4: a frame stopped at a fixed point, 8: one of them
    // by the next-pass proof -- nothing reads 8, but without the ballot behind
    // it this compiler spills two loop-invariant values of the normal passes'
    // row loop: 19 scratch reloads per row pair there instead of none); the
    // next verifying pass is allowed at iteration vnext, after a gap of vgap
    // passes
    int ctl = 1, vnext = 1, vgap = 1;
    const bool fpn = (fp & 2) != 0;  // the verifying passes also run the next-pass proof (LDPC_FP_NEXT)
    // iteration 0 runs column by column (sub_pass0_cols): bit 2 of fp, P_r fits the S region, and no live
    // frame's table value is tiny (the vote below, in the control word that pass 0 rewrites)
    bool cols0 = (fp & 4) != 0 && m <= g.k;
    // ... and its phase A gathers the A columns' table values from LDS (bit 3 of fp, LDPC_PASS0_LDS):
    // staged only where the column form can still follow
    const bool lds0 = cols0 && (fp & 8) != 0;
    fp &= 3;  // the exit's bits
    if (max_iter > 0) {  // iteration 0's tanh table, in L (sub_tanh_table); the other wavefronts gather it with ld_l2
        c.live = livel[f] != 0;
        if (sub_tanh_table<Q>(c, g.n, me, nthr, lds0 ? g.k : 0)) lds_st(flags + 2 * kSR + 1, 1);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        cols0 = cols0 && uniform(flags[2 * kSR + 1]) == 0;
        if (lds0 && !cols0) {  // the vote is lost: the row loop sums into S
            for (int i = threadIdx.x; i < g.k * F; i += blockDim.x) S[i] = 0.0;
            __syncthreads();
        }
    }
    int it0 = 0;
    if (max_iter > 0 && cols0) {
        // Iteration 0 column by column, then its syndrome and exits as in the
        // loop below (iteration 0 never verifies: no fixed-point stop here,
        // only the trigger for the next pass).  Ahead of the loop and not a
        // branch of its body: there this compiler reloads ten doubles from
        // scratch in the normal passes' P1 (profiles/r10_pass0_cols).
        int my_cnt = 0;
        bool pd = false;
        sub_pass0_cols<Q>(c, g, S, zb, nllr, me, nthr, lds0, my_cnt, pd);
        if (nllr && my_cnt) atomicAdd(cntl + f, my_cnt);
        if (fp && pd && c.live) atomicOr((uint32_t *)pdiffl + f, 1u);
        __syncthreads();
        uint32_t acc = 0u;
        for (int r = me; r < m; r += nthr) {
            const uint32_t *ar = g.a_packed + (size_t)r * kw;
            uint32_t par = ib[(r >> 5) * F + f] >> (r & 31);
            for (int w = 0; w < kw; ++w) par += __builtin_popcount(ar[w] & zb[w * F + f]);
            acc |= par & 1u;
        }
        if (acc) atomicOr((uint32_t *)bad + f, 1u);
        __syncthreads();
        if (wave == 0) {
            bool still = false;
            if (j == 0 && c.live) {
                if (nllr) {
                    const int cn = cntl[f];
                    st.nllr_cnt[fr] = cn;
                    if (st.nllr_hist) st.nllr_hist[(size_t)fr * st.hist_stride] = g.k > 0 ? (double)cn / g.k : 0.0;
                }
                const bool ok = bad[f] == 0;  // Result.OK at iteration 0, or DATA_TRANSFER_NOT_OK after the only one
                if (ok || max_iter == 1) {
                    st.done[fr] = 1;
                    st.conv[fr] = ok ? 0 : -1;
                    st.status[fr] = ok ? 0 : 1;
                    st.iters[fr] = 1;
                } else {
                    still = true;
                }
            }
            const unsigned long long any = __ballot(still);
            const unsigned long long trig = __ballot(still && fp && pdiffl[f] == 0);
            if (j == 0) {
                livel[f] = still ? 1 : 0;
                bad[f] = 0;
                cntl[f] = 0;
                pdiffl[f] = 0;
            }
            if (lane == 0) flags[2 * kSR + 1] = (any != 0ull ? 1 : 0) | (trig != 0ull ? 2 : 0);
        }
        for (int i = threadIdx.x; i < (kw + mw) * F; i += blockDim.x) zb[i] = 0u;
        __syncthreads();
        ctl = uniform(flags[2 * kSR + 1]);
        it0 = (ctl & 1) ? 1 : max_iter;
    }
    for (int it = it0; it < max_iter; ++it) {
        c.first = it == 0;
        c.live = livel[f] != 0;
        c.ep0 = sub_epoch0(it, m);
        const bool verify = fp != 0 && it >= vnext && (ctl & 2) != 0;
        c.verify = verify;
        c.prove = verify && fpn;
        double tA[K], tB[K];
        bool yA = false, yB = false;
        if (m > 0) {
            sub_stage_commit(c, 0, sub_stage_issue(c, 0));
            yA = sub_p1<Q>(c, 0, sub_chunk(row_ptr, 0, wave, Q), tA);
        }
        for (int r = 0; r <= m; r += 2) {
            sub_body<Q>(c, r, m, tA, yA, tB, yB);
            if (r + 1 <= m) sub_body<Q>(c, r + 1, m, tB, yB, tA, yA);
        }
        __syncthreads();  // every P3 done: S complete, identity bits set
        sub_p3_reset(c.p3row);

        // posteriors of the A columns (channel added after the sum), the
        // normalized-LLR count against the previous posterior (:210-228),
        // z^1 bits
        int my_cnt = 0;
        bool pd = false;  // the fixed-point trigger: a posterior of this pass differs from the previous one
        for (int col = me; col < g.k; col += nthr) {
            double *sp = c.S + (size_t)col * F;
            const double Sj = *sp;
            *sp = 0.0;
            const double chj = *sub_c(c, col);
            const double Lj = chj + Sj;
            if (nllr || fp) {
                const double ap = c.first ? chj : ld_l2(sub_l(c, col));
                if (nllr) my_cnt += (fabs(Lj) <= 7.0 && ap * Lj < 0.0) ? 1 : 0;
                pd |= dbits(ap) != dbits(Lj);
            }
            if (c.live) *sub_l(c, col) = Lj;
            if (!(Lj < 0.0)) atomicOr(zb + (col >> 5) * F + f, 1u << (col & 31));
        }
        if (nllr && my_cnt) atomicAdd(cntl + f, my_cnt);
        if (fp && pd && c.live) atomicOr((uint32_t *)pdiffl + f, 1u);
        __syncthreads();

        // syndrome (:191-204): parity of row r = popcount(A_r & (z^1)_A) +
        // (z^1)_{k+r}, A_r bit-packed
        uint32_t acc = 0u;
        for (int r = me; r < m; r += nthr) {
            const uint32_t *ar = g.a_packed + (size_t)r * kw;
            uint32_t par = ib[(r >> 5) * F + f] >> (r & 31);
            for (int w = 0; w < kw; ++w) par += __builtin_popcount(ar[w] & zb[w * F + f]);
            acc |= par & 1u;
        }
        if (acc) atomicOr((uint32_t *)bad + f, 1u);
        __syncthreads();

        if (wave == 0) {  // per-frame exits, as vn_kernel (static schedule)
            bool still = false, fixed = false, proven = false;
            if (j == 0 && c.live) {
                if (nllr) {
                    const int cn = cntl[f];
                    st.nllr_cnt[fr] = cn;
                    if (st.nllr_hist)
                        st.nllr_hist[(size_t)fr * st.hist_stride + it] = g.k > 0 ? (double)cn / g.k : 0.0;
                }
                if (bad[f] == 0) {  // syndrome zero: Result.OK at this iteration (:231-241)
                    st.done[fr] = 1;
                    st.conv[fr] = it;
                    st.status[fr] = 0;
                    st.iters[fr] = it + 1;
                } else if (it == max_iter - 1) {  // Result.DATA_TRANSFER_NOT_OK (:244-253)
                    st.done[fr] = 1;
                    st.conv[fr] = -1;
                    st.status[fr] = 1;
                    st.iters[fr] = it + 1;
                } else if (verify && pdiffl[f] == 0 && ((mdiffl[f] & 1) == 0 || (mdiffl[f] & 6) == 0)) {
                    // a fixed point, reached in this pass (no message differed) or proven for the next one
                    // (every difference of the frame tested, and no frame's test failed in this pass): every
                    // pass up to max_iter - 1 would leave E, L and z as memory holds them now,
                    // count 0 sign changes and end as DATA_TRANSFER_NOT_OK
                    st.done[fr] = 1;
                    st.conv[fr] = -1;
                    st.status[fr] = 1;
                    st.iters[fr] = max_iter;
                    if (nllr && st.nllr_hist)
                        for (int i = it + 1; i < max_iter; ++i) st.nllr_hist[(size_t)fr * st.hist_stride + i] = 0.0;
                    fixed = true;
                    proven = mdiffl[f] != 0;
                } else {
                    still = true;
                }
            }
            const unsigned long long any = __ballot(still);
            const unsigned long long trig = __ballot(still && fp && pdiffl[f] == 0);
            const int nfix = __popcll(__ballot(fixed));
            const unsigned long long nprv = __ballot(proven);
            if (j == 0) {
                livel[f] = still ? 1 : 0;
                bad[f] = 0;
                cntl[f] = 0;
                pdiffl[f] = 0;
                mdiffl[f] = 0;
            }
            if (lane == 0) {
                flags[2 * kSR + 1] = (any != 0ull ? 1 : 0) | (trig != 0ull ? 2 : 0) | (nfix ? 4 : 0) | (nprv != 0ull ? 8 : 0);
                if (nfix) {
                    atomicAdd(&st.fp_count[0], (unsigned long long)nfix);
                    atomicAdd(&st.fp_count[1], (unsigned long long)nfix * (unsigned long long)(max_iter - 1 - it));
                }
            }
        }
        for (int i = threadIdx.x; i < (kw + mw) * F; i += blockDim.x) zb[i] = 0u;
        __syncthreads();
        ctl = uniform(flags[2 * kSR + 1]);
        if (!(ctl & 1)) break;
        if (verify && !(ctl & 4)) {  // nothing confirmed: back off
            vnext = it + 1 + vgap;
            vgap *= 2;
        }
    }
    count_rare_rows(st, c.tseq, kSW);
#ifdef LDPC_SUB_TIMERS
    if ((blockIdx.x == 0 || blockIdx.x == 777) && (threadIdx.x & 63) == 0)
        printf("SUB b=%d w=%d hopw=%llu hop=%llu p3f=%llu p3m=%llu p3o=%llu p3s=%llu p1=%llu\n", (int)blockIdx.x,
               c.wave, (unsigned long long)c.tm[0], (unsigned long long)c.tm[1], (unsigned long long)c.tm[2],
               (unsigned long long)c.tm[3], (unsigned long long)c.tm[4], (unsigned long long)c.tm[5],
               (unsigned long long)c.tm[6]);
#endif
}

// Streaming Monte-Carlo on sub-tiles (tile_kernels.hip's tile_stream_kernel,
// at 16 frames per workgroup): every frame slot f is at its own iteration;
// after each pass a slot whose frame stopped adds that frame's counters
// (count_kernel's definitions, main.py:130-138) and takes the next frame
// index from one device counter; the frame is generated in place (gen_slots:
// ch and L = ch, so its next pass forms M = L - 0, its iteration 0).  Each
// frame decodes exactly as in the static schedule, so the counters are
// identical.  A workgroup exits once the supply is out and its slots drained.
template <int Q>
__global__ __launch_bounds__(64 * kSW, 1) void tile_sub_stream_kernel(
    DevGraph g, DevState st, int max_iter, int nllr, const int *__restrict__ col_idx,
    const int *__restrict__ row_ptr, AtanhCoef ac, uint64_t seed, int snr_point, double sigma, int64_t frame0,
    int64_t total, unsigned long long *next, unsigned long long *ctr, int64_t handoff) {
    constexpr int F = SubCfg<Q>::F, K = SubCfg<Q>::K;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int itl[F], freshl[F];
    __shared__ long long gidx[F];  // refill: slot f's new frame index (< 0: none)
    __shared__ int nref;           // refill: some slot took a frame this pass
    const SubLayout ly = sub_layout(g.k, g.m, F);
    double *S = (double *)(lds + ly.S);
    MathLds &mlds = *(MathLds *)(lds + ly.math);
    uint32_t *zb = (uint32_t *)(lds + ly.zb);
    uint32_t *ib = (uint32_t *)(lds + ly.ib);
    int *bad = (int *)(lds + ly.lane_i);
    int *cntl = bad + F;
    int *livel = cntl + F;
    int *flags = (int *)(lds + ly.flags);
    const int kw = (g.k + 31) >> 5, mw = (g.m + 31) >> 5;
    const int tile = blockIdx.x / Q, sub = blockIdx.x % Q;
    if (tile >= st.ntiles) return;  // block-uniform

    fill_math_lds(mlds);
    for (int i = threadIdx.x; i < g.k * F; i += blockDim.x) S[i] = 0.0;
    for (int i = threadIdx.x; i < (kw + mw) * F; i += blockDim.x) zb[i] = 0u;
    for (int i = threadIdx.x; i < 2 * F; i += blockDim.x) bad[i] = 0;
    if (threadIdx.x < 2 * kSR) flags[threadIdx.x] = -1;
    if (threadIdx.x >= 2 * kSR && threadIdx.x < 2 * kSR + 2 + kSW) flags[threadIdx.x] = 0;
    const int lane = threadIdx.x & 63;
    const int wave = uniform(sub_wave(threadIdx.x >> 6));
    const int j = lane / F, f = lane % F;
    const int lane64 = sub * F + f;
    const bool slot_lane = wave == 0 && j == 0;  // the lane that owns frame slot f
    bool want = slot_lane;
    if (slot_lane) {
        livel[f] = 0;
        itl[f] = 0;
        freshl[f] = 0;
    }

    SubCtx<Q> c;
    c.col_idx = col_idx;
    c.row_ptr = row_ptr;
    const size_t lo = (size_t)lane64;
    c.Eb = st.E + (size_t)tile * g.nnz * kTile + lo;
    c.Lb = st.L + (size_t)tile * g.n * kTile + lo;
    c.Cb = st.ch + (size_t)tile * g.n * kTile + lo;
    c.Eu = (const char *)(st.E + (size_t)tile * g.nnz * kTile);
    c.rE = sub_rsrc(c.Eu, (size_t)g.nnz * kTile * sizeof(double));
    c.Lu = (const char *)(st.L + (size_t)tile * g.n * kTile);
    c.Cu = (const char *)(st.ch + (size_t)tile * g.n * kTile);
    c.lo8 = (uint32_t)lo * 8u;
    c.Tb = st.T + (size_t)blockIdx.x * 2 * g.max_row_deg * F + f;
    c.tbuf = (size_t)g.max_row_deg * F;
    c.S = S + f;
    c.dummy = (double *)(lds + ly.dummy) + f;
    c.slot = (double *)(lds + ly.slot) + f;
    c.ib = ib + f;
    c.cidx = (uint16_t *)(lds + ly.cidx) + wave * Q * K;
    c.m = g.m;
    c.flag = flags;
    c.tinyf = flags + kSR;
    c.tseq = flags + 2 * kSR;
    c.p3row = flags + 2 * kSR + 2;
    c.p3dep = g.p3dep;
    c.ttab = LdsTanh{mlds.tanh};
    c.ltab = LdsAtanh{mlds.atanh};
    c.coef_arg = kStreamCoefArg;
    c.ac = ac;
    c.k = g.k;
    c.wave = wave;
    c.j = j;
    c.f = f;
    c.ntiny = 0;
    c.first = false;
    c.verify = false;  // the fixed-point exit is the static decoder's
    c.prove = false;
    c.mdiff = nullptr;
    const int m = g.m;
    const int nthr = kSW * Q;
    const int me = wave * Q + j;
    const uint32_t *Ut = st.ubits + (size_t)tile * kw * kTile + lane64;

    for (int pass = 0;; ++pass) {
        if (wave == 0) {  // refill: slots without a frame take the next indices (generated below)
            // hand-off: once the supply is out and at most `handoff` frames
            // are still running anywhere, stop here and leave them to the
            // column-parallel tail (ldpc_api.cpp mc_stream_point): a running
            // frame costs this workgroup a full pass per iteration
            int stop = 0;
            if (handoff > 0 && lane == 0) {
                const long long nx = (long long)__hip_atomic_load(next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const long long fin = (long long)__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                stop = nx >= total && total - fin <= handoff ? 1 : 0;
            }
            stop = uniform(stop);
            if (stop) want = false;
            const unsigned long long w = __ballot(want);
            bool have = false;
            if (w != 0ull) {
                const int first = __ffsll((long long)w) - 1;
                unsigned long long base = 0ull;
                if (lane == first) base = atomicAdd(next, (unsigned long long)__popcll(w));
                base = __shfl(base, first);
                const unsigned long long below = lane ? (w & (~0ull >> (64 - lane))) : 0ull;
                const int64_t idx = (int64_t)(base + (unsigned long long)__popcll(below));
                have = want && idx < total;
                if (slot_lane) gidx[f] = have ? supply_frame(st, frame0, idx) : -1ll;
                if (want) {
                    livel[f] = have ? 1 : 0;
                    freshl[f] = have ? 1 : 0;
                    itl[f] = 0;
                }
            }
            const bool gen = __ballot(have) != 0ull;
            want = false;
            const unsigned long long any = __ballot(slot_lane && livel[f] != 0);
            const bool go = any != 0ull && !stop;
            if (!go && slot_lane) {  // the slots' state, in the split path's terms
                const int fr = tile * kTile + lane64;
                st.done[fr] = livel[f] != 0 ? 0 : 1;
                st.iters[fr] = itl[f];
                st.fresh[fr] = freshl[f];
                st.refill[fr] = 0;
            }
            if (lane == 0) {
                flags[2 * kSR + 1] = go ? 1 : 0;
                nref = go && gen ? 1 : 0;
            }
        }
        __syncthreads();
        if (!flags[2 * kSR + 1]) break;  // supply exhausted, every slot drained
        // the new frames, generated by the whole workgroup (u bits staged in
        // zb, which is zero here and again after)
        if (nref) gen_slots<F>(g, st, tile, sub * F, gidx, zb, seed, snr_point, sigma);
        c.live = livel[f] != 0;
        c.fresh = freshl[f] != 0;
        c.ep0 = sub_epoch0(pass, m);
        double tA[K], tB[K];
        bool yA = false, yB = false;
        if (m > 0) {
            sub_stage_commit(c, 0, sub_stage_issue(c, 0));
            yA = sub_p1<Q>(c, 0, sub_chunk(row_ptr, 0, wave, Q), tA);
        }
        for (int r = 0; r <= m; r += 2) {
            sub_body<Q>(c, r, m, tA, yA, tB, yB);
            if (r + 1 <= m) sub_body<Q>(c, r + 1, m, tB, yB, tA, yA);
        }
        __syncthreads();
        sub_p3_reset(c.p3row);

        int my_cnt = 0;
        for (int col = me; col < g.k; col += nthr) {
            double *sp = c.S + (size_t)col * F;
            const double Sj = *sp;
            *sp = 0.0;
            const double chj = *sub_c(c, col);
            const double Lj = chj + Sj;  // channel added after the sum (:173,185)
            if (nllr) {
                const double ap = ld_l2(sub_l(c, col));  // previous L (= ch on a frame's first pass)
                my_cnt += (fabs(Lj) <= 7.0 && ap * Lj < 0.0) ? 1 : 0;
            }
            if (c.live) *sub_l(c, col) = Lj;
            if (!(Lj < 0.0)) atomicOr(zb + (col >> 5) * F + f, 1u << (col & 31));
        }
        if (nllr && my_cnt) atomicAdd(cntl + f, my_cnt);
        __syncthreads();

        uint32_t acc = 0u;  // syndrome (:191-204)
        for (int r = me; r < m; r += nthr) {
            const uint32_t *ar = g.a_packed + (size_t)r * kw;
            uint32_t par = ib[(r >> 5) * F + f] >> (r & 31);
            for (int w = 0; w < kw; ++w) par += __builtin_popcount(ar[w] & zb[w * F + f]);
            acc |= par & 1u;
        }
        if (acc) atomicOr((uint32_t *)bad + f, 1u);
        __syncthreads();

        if (wave == 0) {  // per-slot exits and counters (vn_kernel's stream variant)
            unsigned long long cv[7] = {0, 0, 0, 0, 0, 0, 0};
            bool fin = false;
            if (slot_lane && c.live) {
                const int it = itl[f];
                const bool ok = bad[f] == 0;  // Result.OK at this iteration (:231-241)
                fin = ok || it == max_iter - 1;  // else DATA_TRANSFER_NOT_OK (:244-253)
                if (fin) {
                    int err = 0;
                    if (!ok)  // main.py:130-138: u vs z^1 of a failed frame
                        for (int w = 0; w < kw; ++w) err += __builtin_popcount(Ut[w * kTile] ^ zb[w * F + f]);
                    cv[0] = 1;
                    cv[1] = ok ? 0 : 1;
                    cv[2] = (unsigned long long)err;
                    cv[3] = ok ? (unsigned long long)it : 0;
                    cv[4] = ok ? 1 : 0;
                    cv[5] = nllr ? (unsigned long long)cntl[f] : 0;
                    cv[6] = (unsigned long long)(it + 1);
                    livel[f] = 0;
                    want = true;
                } else {
                    itl[f] = it + 1;
                }
                freshl[f] = 0;
            }
            if (__ballot(fin) != 0ull) {
#pragma unroll
                for (int i = 0; i < 7; ++i) {
                    const unsigned long long sm = wave_sum(cv[i]);
                    if (lane == 0 && sm) atomicAdd(&ctr[i], sm);
                }
            }
            if (slot_lane) {
                bad[f] = 0;
                cntl[f] = 0;
            }
        }
        __syncthreads();  // wave 0 has read zb (error bits) before it is cleared
        for (int i = threadIdx.x; i < (kw + mw) * F; i += blockDim.x) zb[i] = 0u;
        __syncthreads();
    }
    count_rare_rows(st, c.tseq, kSW);
}

template <int Q>
size_t sub_lds_bytes_q(const DevGraph &g) {
    constexpr int F = SubCfg<Q>::F, K = SubCfg<Q>::K;
    if (!g.std_form || !g.a_packed || g.k <= 0 || g.max_row_deg > kSW * Q * K || Q * K > 64 || g.n > 65535)
        return 0;
    const size_t b = sub_layout(g.k, g.m, F).total;
    // + the static kernel's own 2 x F ints (tile_sub_kernel: pdiffl, mdiffl)
    return b + 2 * F * sizeof(int) <= kSubLdsMax ? b : 0;
}

}  // namespace

// Frames per workgroup of the sub-tile decoder for this graph: 16, or 0
// (does not apply).
int sub_frames(const DevGraph &g) { return sub_lds_bytes_q<4>(g) ? 16 : 0; }
size_t sub_lds_bytes(const DevGraph &g) { return sub_lds_bytes_q<4>(g); }

hipError_t launch_tile_sub_stream(const DevGraph &g, const DevState &st, int max_iter, bool nllr, uint64_t seed,
                                  int snr_point, double sigma, int64_t frame0, int64_t total,
                                  unsigned long long *next, unsigned long long *ctr, int64_t handoff, hipStream_t s) {
    const size_t lds = sub_lds_bytes_q<4>(g);
    // the 16-frame form only (+ static LDS: 2 x 16 ints, 16 frame indices, the refill flag)
    if (!lds || !g.a_packed || !st.ubits || 2 * st.ntiles > st.nslots ||
        lds + 2 * 16 * sizeof(int) + 16 * sizeof(long long) + 16 > kSubLdsMax)
        return hipErrorInvalidValue;
    tile_sub_stream_kernel<4><<<st.ntiles * 4, 64 * kSW, lds, s>>>(g, st, max_iter, nllr ? 1 : 0, g.col_idx, g.row_ptr,
                                                                   kAtanhCoef, seed, snr_point, sigma, frame0, total,
                                                                   next, ctr, handoff);
    return hipGetLastError();
}

hipError_t launch_tile_sub(const DevGraph &g, const DevState &st, int max_iter, bool nllr, hipStream_t s) {
    const size_t lds = sub_lds_bytes(g);
    if (!lds || 2 * st.ntiles > st.nslots) return hipErrorInvalidValue;  // two rare-row buffers per workgroup
    // LDPC_FIXED_POINT=0 (read per launch): no fixed-point exit, every frame makes its passes (A/B, diagnosis)
    // LDPC_FP_NEXT=0 (bit 1 of fp): a frame stops only where no message differed, not on the next-pass proof
    const char *e = getenv("LDPC_FIXED_POINT");
    const char *en = getenv("LDPC_FP_NEXT");
    // LDPC_PASS0_COLS=0 (bit 2 of fp, no part of the exit): iteration 0 by the row loop, not column by column
    // LDPC_PASS0_LDS=0 (bit 3 of fp, neither): the column form's row products gather the table from L, not from LDS
    const char *ec = getenv("LDPC_PASS0_COLS");
    const char *el = getenv("LDPC_PASS0_LDS");
    const int fp = ((!e || atoi(e) != 0) ? (1 | ((!en || atoi(en) != 0) ? 2 : 0)) : 0) | ((!ec || atoi(ec) != 0) ? 4 : 0) |
                   ((!el || atoi(el) != 0) ? 8 : 0);
    tile_sub_kernel<4><<<st.ntiles * 4, 64 * kSW, lds, s>>>(g, st, max_iter, nllr ? 1 : 0, g.col_idx, g.row_ptr,
                                                            kAtanhCoef, fp);
    return hipGetLastError();
}

}  // namespace ldpc
