"""Python handles over the C ABI: the graph on a GPU and a decoder workspace.

``Graph``   wraps ldpc_graph_create (H_std uploaded once per device, cached by
            content and process so repeated SPA_Decoder constructions --
            main.py:221 builds one per SNR point, main.py:78 one per frame --
            do not re-upload, and a forked worker never gets its parent's
            device handle).
``Decoder`` wraps ldpc_decoder_create / ldpc_decode_f64 / ldpc_mc_run.
Every call here goes through _lib.gpu() (fork check, _lib's docstring); a
handle is only released by the process that created it.
"""
import ctypes
import hashlib
import os
import threading

import numpy as np
from scipy import sparse

from . import _lib
from ._lib import (LDPC_EINVAL, LDPC_ERANGE, LDPC_F_BF_GENERIC, LDPC_F_DEVICE_PTRS, LDPC_F_LAYERED_TILE, LDPC_F_NLLR,
                   LDPC_F_PHYS_HBM, LDPC_F_QUANT_TILE, LDPC_F_SPLIT, LDPC_F_STATIC, LDPC_MC_NCOUNT, LdpcError, as_i32, check)


def _csr_arrays(H):
    H = sparse.csr_matrix(H)
    if not H.has_sorted_indices:
        H = H.sorted_indices()
    return H.shape[0], H.shape[1], as_i32(H.indptr), as_i32(H.indices)


def validate_csr(m, n, indptr, indices):
    """ldpc_graph_create's argument checks (csrc/ldpc_api.cpp), HIP-free, so a
    bad H fails where it is handed over (SPA_Decoder.__init__ in the parent
    process, as the reference's constructor would) rather than on the first
    decode() inside a forked worker.  Raises LdpcError with the C codes."""
    fn = "ldpc_graph_create"
    if m <= 0 or n <= 0 or m > n:
        raise LdpcError(fn, LDPC_EINVAL, f"bad shape m={m} n={n}")
    indptr = np.asarray(indptr)
    indices = np.asarray(indices)
    if len(indptr) != m + 1 or indptr[0] != 0:
        raise LdpcError(fn, LDPC_EINVAL, "row_ptr[0] != 0")
    nnz = int(indptr[-1])
    lim = (2 ** 31 - 1) // 64  # within-tile offsets are 32-bit: e * 64 must fit
    if nnz <= 0 or nnz > lim or n > lim:
        raise LdpcError(fn, LDPC_ERANGE, f"nnz={nnz} outside 32-bit tile indexing")
    d = np.diff(indptr)
    if (d < 0).any():
        raise LdpcError(fn, LDPC_EINVAL, f"row_ptr not monotone at {int(np.argmax(d < 0))}")
    if len(indices) < nnz or (indices[:nnz] < 0).any() or (indices[:nnz] >= n).any():
        raise LdpcError(fn, LDPC_EINVAL, "column out of range")
    c = indices[:nnz].astype(np.int64)
    step = np.diff(c)
    same_row = np.ones(max(nnz - 1, 0), bool)
    same_row[(indptr[1:-1][(indptr[1:-1] > 0) & (indptr[1:-1] < nnz)] - 1)] = False
    bad = (step <= 0) & same_row
    if bad.any():
        r = int(np.searchsorted(indptr, int(np.argmax(bad)) + 1, side="right") - 1)
        raise LdpcError(fn, LDPC_EINVAL, f"row {r} columns not strictly ascending "
                                         "(the reference's check_to_var order is required)")


class Graph:
    """H_std (CSR, ascending columns) resident on one GPU."""

    _cache = {}
    _cache_lock = threading.Lock()

    def __init__(self, H, device=-1):
        m, n, indptr, indices = _csr_arrays(H)
        self.m, self.n, self.k = m, n, n - m
        self.indptr, self.indices = indptr, indices
        self.nnz = int(indptr[-1])
        h = ctypes.c_void_p()
        check("ldpc_graph_create", _lib.gpu().ldpc_graph_create(
            m, n, _lib.i32p(indptr), _lib.i32p(indices), int(device), ctypes.byref(h)))
        self._h = h
        self._pid = os.getpid()
        mr, mc = ctypes.c_int32(), ctypes.c_int32()
        check("ldpc_graph_info", _lib.gpu().ldpc_graph_info(h, None, None, None, ctypes.byref(mr), ctypes.byref(mc)))
        self.max_row_deg, self.max_col_deg = mr.value, mc.value

    @property
    def handle(self):
        return self._h

    @classmethod
    def cached(cls, H, device=-1):
        m, n, indptr, indices = _csr_arrays(H)
        key = (os.getpid(), m, n, int(device), hashlib.sha1(indptr.tobytes() + indices.tobytes()).hexdigest())
        with cls._cache_lock:
            g = cls._cache.get(key)
            if g is None:
                g = cls(sparse.csr_matrix((np.ones(len(indices), np.int32), indices, indptr), shape=(m, n)), device)
                cls._cache[key] = g
        return g

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib._lib is not None and getattr(self, "_pid", None) == os.getpid():
            _lib._lib.ldpc_graph_destroy(h)
        self._h = None


CN_RULES = {"spa": _lib.LDPC_CN_SPA, "nms": _lib.LDPC_CN_NMS, "oms": _lib.LDPC_CN_OMS}
SCHEDULES = {"flooding": _lib.LDPC_SCHED_FLOODING, "layered": _lib.LDPC_SCHED_LAYERED}


def phys_rule_args(cn="spa", schedule="flooding", alpha=0.75, beta=0.5):
    """(cn_rule, schedule, param) of the C ABI for the physical-mode options:
    cn "spa" (sum-product), "nms" (normalized min-sum, alpha in (0, 1]) or
    "oms" (offset min-sum, beta >= 0); schedule "flooding" or "layered".
    Raises ValueError for anything else -- before any device call."""
    if cn not in CN_RULES:
        raise ValueError(f"cn must be one of {sorted(CN_RULES)}, got {cn!r}")
    if schedule not in SCHEDULES:
        raise ValueError(f"schedule must be one of {sorted(SCHEDULES)}, got {schedule!r}")
    alpha, beta = float(alpha), float(beta)
    if cn == "nms" and not (0.0 < alpha <= 1.0):
        raise ValueError(f"alpha must be in (0, 1], got {alpha}")
    if cn == "oms" and not beta >= 0.0:
        raise ValueError(f"beta must be >= 0, got {beta}")
    if cn == "spa" and schedule == "layered":
        raise ValueError("the layered schedule needs a min-sum rule (cn='nms' or 'oms'): "
                         "sum-product layered is not implemented")
    return CN_RULES[cn], SCHEDULES[schedule], {"spa": 0.0, "nms": alpha, "oms": beta}[cn]


def phys_flags(hbm=False, tile=False, schedule="flooding", qtile=False):
    """The physical-mode flags: hbm forces the flooding HBM tile path, tile the
    layered schedule's (LDPC_F_LAYERED_TILE), qtile the fixed-point decoder's
    (LDPC_F_QUANT_TILE; either schedule).  tile without schedule="layered"
    raises ValueError -- before any device call."""
    if tile and schedule != "layered":
        raise ValueError(f"tile=True needs schedule='layered', got {schedule!r}")
    return (LDPC_F_PHYS_HBM if hbm else 0) | (LDPC_F_LAYERED_TILE if tile else 0) | \
        (LDPC_F_QUANT_TILE if qtile else 0)


def _need_qbits(qtile, qbits):
    """qtile selects the fixed-point decoder's tile kernels: without qbits it
    has no meaning (ValueError -- before any device call)."""
    if qtile and qbits is None:
        raise ValueError("qtile=True needs qbits (the fixed-point decoder)")


def phys_quant_args(cn, alpha=0.75, beta=0.5, qbits=6, llr_scale=4.0):
    """(qbits, llr_scale, param_q) of the fixed-point entries (ldpc_phys_decode_q):
    qbits in 4..8, llr_scale finite and > 0, and the float alpha / beta as the
    integers the decoder computes with -- alpha_q = round(16 alpha) in 1..16
    (sixteenths) for "nms", beta_q = round(beta llr_scale) in 0..Qmax (quantizer
    steps, Qmax = 2^(qbits-1) - 1) for "oms".  Raises ValueError otherwise --
    before any device call."""
    if cn not in ("nms", "oms"):
        raise ValueError(f"qbits needs a min-sum rule (cn='nms' or 'oms'), got cn={cn!r}")
    if isinstance(qbits, bool) or int(qbits) != qbits or not 4 <= int(qbits) <= 8:
        raise ValueError(f"qbits must be an integer in 4..8, got {qbits!r}")
    qbits, llr_scale = int(qbits), float(llr_scale)
    if not (np.isfinite(llr_scale) and llr_scale > 0.0 and np.isfinite(np.float32(llr_scale))
            and np.float32(llr_scale) > 0.0):
        raise ValueError(f"llr_scale must be finite and > 0 (in fp32), got {llr_scale}")
    qmax = (1 << (qbits - 1)) - 1
    if cn == "nms":
        param_q = int(round(16.0 * float(alpha)))
        if not 1 <= param_q <= 16:
            raise ValueError(f"alpha = {alpha} gives alpha_q = round(16 alpha) = {param_q}, outside 1..16")
    else:
        param_q = int(round(float(beta) * llr_scale))
        if not 0 <= param_q <= qmax:
            raise ValueError(f"beta = {beta} gives beta_q = round(beta llr_scale) = {param_q}, outside 0..{qmax} "
                             f"(Qmax at qbits = {qbits})")
    return qbits, llr_scale, param_q


def phys_kernel_name(graph, hbm=False, cn="spa", schedule="flooding", qbits=None, llr_scale=4.0, tile=False,
                     qtile=False):
    """Measurement label: the kernel phys_decode runs for these options."""
    _need_qbits(qtile, qbits)
    rule, sched, _ = phys_rule_args(cn, schedule)
    flags = phys_flags(hbm, tile, schedule, qtile)
    if qbits is not None:
        qbits, _, _ = phys_quant_args(cn, qbits=qbits, llr_scale=llr_scale)
        return _lib.gpu().ldpc_phys_kernel_name_q(graph.handle, flags, rule, sched, qbits).decode()
    return _lib.gpu().ldpc_phys_kernel_name_ex(graph.handle, flags, rule, sched).decode()


def phys_decode(graph, llr, max_iter, post=False, hbm=False, cn="spa", schedule="flooding", alpha=0.75, beta=0.5,
                ex=False, qbits=None, llr_scale=4.0, tile=False, qtile=False):
    """Physical-mode decode of [B, n] LLRs on a sparse graph (H[:, perm]).

    State in LDS when a frame fits, else in HBM (hbm=True forces HBM).
    cn / schedule / alpha / beta: phys_rule_args; the defaults are the
    sum-product flooding decoder (ldpc_phys_decode), anything else goes through
    ldpc_phys_decode_ex (ex=True: the defaults too -- the library takes the
    same path for them either way; tests).  Layered runs with the state in LDS
    when it fits, else on the HBM tiles (tile=True forces them; it needs
    schedule="layered"); hbm=True with layered is refused.
    qbits=4..8: the fixed-point min-sum decoder (ldpc_phys_decode_q;
    phys_quant_args turns alpha / beta into its integers) on LLRs scaled by
    llr_scale; post is then the integer posterior, int16, in units of
    1 / llr_scale.  Its state is in LDS when it fits, else on the HBM tiles
    (qtile=True forces them, either schedule; it needs qbits).  qbits=None:
    the fp32 decoders, llr_scale unused."""
    _need_qbits(qtile, qbits)
    rule, sched, param = phys_rule_args(cn, schedule, alpha, beta)
    flags = phys_flags(hbm, tile, schedule, qtile)
    if qbits is not None:
        qbits, llr_scale, param_q = phys_quant_args(cn, alpha, beta, qbits, llr_scale)
    llr = np.ascontiguousarray(np.atleast_2d(np.asarray(llr, dtype=np.float64)))
    B, n = llr.shape
    if n != graph.n:
        raise ValueError(f"llr must be [batch, {graph.n}]")
    z = np.empty((B, n), np.uint8)
    conv = np.empty(B, np.int32)
    status = np.empty(B, np.int32)
    iters = np.empty(B, np.int32)
    Lp = np.empty((B, n), np.float32 if qbits is None else np.int16) if post else None
    if qbits is not None:
        check("ldpc_phys_decode_q", _lib.gpu().ldpc_phys_decode_q(
            graph.handle, B, _lib.ptr(llr), int(max_iter), flags, rule, sched, qbits, llr_scale, param_q,
            _lib.ptr(z), _lib.ptr(conv), _lib.ptr(status), _lib.ptr(iters), _lib.ptr(Lp), None))
    elif (cn, schedule) == ("spa", "flooding") and not ex:
        check("ldpc_phys_decode", _lib.gpu().ldpc_phys_decode(
            graph.handle, B, _lib.ptr(llr), int(max_iter), flags, _lib.ptr(z), _lib.ptr(conv), _lib.ptr(status),
            _lib.ptr(iters), _lib.ptr(Lp), None))
    else:
        check("ldpc_phys_decode_ex", _lib.gpu().ldpc_phys_decode_ex(
            graph.handle, B, _lib.ptr(llr), int(max_iter), flags, rule, sched, param, _lib.ptr(z), _lib.ptr(conv),
            _lib.ptr(status), _lib.ptr(iters), _lib.ptr(Lp), None))
    return DecodeResult(z=z, conv=conv, status=status, iters=iters, post=Lp)


class DecodeResult(dict):
    __getattr__ = dict.__getitem__


def bitflip_args(weight=0.0, theta=0.0):
    """(weight, theta) of the bit-flipping entries (ldpc_bf_decode) as floats:
    weight finite and >= 0, theta finite, both also as the fp32 values the
    decoder computes with.  Raises ValueError otherwise -- before any device
    call."""
    try:
        weight, theta = float(weight), float(theta)
    except (TypeError, ValueError):
        raise ValueError(f"weight and theta must be numbers, got {weight!r}, {theta!r}")
    with np.errstate(over="ignore"):
        w32, t32 = np.float32(weight), np.float32(theta)
    if not (np.isfinite(weight) and np.isfinite(w32) and weight >= 0.0):
        raise ValueError(f"weight must be finite and >= 0 (in fp32), got {weight}")
    if not (np.isfinite(theta) and np.isfinite(t32)):
        raise ValueError(f"theta must be finite (in fp32), got {theta}")
    return weight, theta


def bitflip_kernel_name(graph, weight=0.0, generic=False):
    """Measurement label: the kernel bitflip_decode runs for these options
    ("bitflip_sliced_kernel", "bitflip_kernel", or "" when the state does not
    fit LDS)."""
    weight, _ = bitflip_args(weight)
    return _lib.gpu().ldpc_bf_kernel_name(graph.handle, LDPC_F_BF_GENERIC if generic else 0, weight).decode()


def bitflip_decode(graph, llr, max_iter, weight=0.0, theta=0.0, generic=False):
    """Bit-flipping decode of [B, n] LLRs on a sparse graph (H[:, perm]):
    parallel gradient-descent bit flipping with Delta_j = weight * c_j +
    (d_j - 2 u_j), flip where Delta_j < theta (include/ldpc_hip.h
    "bit-flipping decoders"); weight = 0 is plain hard-decision flipping, with
    theta = 0 the majority rule.  generic=True runs the per-frame kernel even
    where the bit-sliced one applies.  Returns DecodeResult(z, conv, status,
    iters, synw); synw is the syndrome weight at exit."""
    weight, theta = bitflip_args(weight, theta)
    llr = np.ascontiguousarray(np.atleast_2d(np.asarray(llr, dtype=np.float64)))
    B, n = llr.shape
    if n != graph.n:
        raise ValueError(f"llr must be [batch, {graph.n}]")
    z = np.empty((B, n), np.uint8)
    conv, status, iters, synw = (np.empty(B, np.int32) for _ in range(4))
    check("ldpc_bf_decode", _lib.gpu().ldpc_bf_decode(
        graph.handle, B, _lib.ptr(llr), int(max_iter), LDPC_F_BF_GENERIC if generic else 0, weight, theta,
        _lib.ptr(z), _lib.ptr(conv), _lib.ptr(status), _lib.ptr(iters), _lib.ptr(synw), None))
    return DecodeResult(z=z, conv=conv, status=status, iters=iters, synw=synw)


class Decoder:
    """Device workspace for chunks of up to `max_frames` frames."""

    def __init__(self, graph, max_frames=4096):
        self.graph = graph
        h = ctypes.c_void_p()
        check("ldpc_decoder_create", _lib.gpu().ldpc_decoder_create(graph.handle, int(max_frames), ctypes.byref(h)))
        self._h = h
        self._pid = os.getpid()
        self.capacity = int(_lib.gpu().ldpc_decoder_capacity(h))
        self._max_failed = 0  # record capacity mc_stats_read offers: the max_failed of the last mc_stats()

    @staticmethod
    def workspace_bytes(graph, max_frames):
        return int(_lib.gpu().ldpc_decoder_bytes(graph.handle, int(max_frames)))

    # HBM the Monte-Carlo drivers let one decoder take (of 288 GB per MI355X);
    # LDPC_HBM_BUDGET_GB overrides
    HBM_BUDGET = 160e9

    @classmethod
    def fit_slots(cls, graph, frames, budget=None):
        """Slots (resident frames, a multiple of 64) for a workspace of at most
        `budget` bytes, and no more than `frames`: fp64 messages are 8 B per
        edge per frame, 5.3 MB for wimax_2304_0.5, so its 65,536-frame batch
        (348 GB) streams through ~30k slots instead."""
        if budget is None:
            budget = float(os.environ.get("LDPC_HBM_BUDGET_GB", cls.HBM_BUDGET / 1e9)) * 1e9
        # workspace = fixed (rare-row scratch, graph-sized buffers) + per-frame state
        a, b = 64 * 64, 2 * 64 * 64
        wa, wb = cls.workspace_bytes(graph, a), cls.workspace_bytes(graph, b)
        per = (wb - wa) / (b - a)
        fixed = wa - per * a
        fit = max(64, int((budget - fixed) // per) // 64 * 64)
        return max(1, min(int(frames), fit))

    def decode(self, llr, max_iter, nllr=False, post=False, hist=False, msgs=False, split=False):
        """Decode [B, n] channel LLRs (H_std column order).  Returns numpy arrays.

        split=True forces the per-iteration CN/VN launches where the
        tile-resident decoder would run (same results; A/B and tests)."""
        g = self.graph
        llr = np.ascontiguousarray(np.asarray(llr, dtype=np.float64))
        if llr.ndim == 1:
            llr = llr[None, :]
        if llr.ndim != 2 or llr.shape[1] != g.n:
            raise ValueError(f"llr must be [batch, {g.n}], got {llr.shape}")
        B = llr.shape[0]
        T = int(max_iter)
        z = np.empty((B, g.n), np.uint8)
        conv = np.empty(B, np.int32)
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        nl = np.zeros(B, np.float64) if nllr else None
        Lp = np.empty((B, g.n), np.float64) if post else None
        hi = np.empty((B, T), np.float64) if (hist and nllr) else None
        E = np.empty((B, g.nnz), np.float64) if msgs else None
        flags = (LDPC_F_NLLR if nllr else 0) | (LDPC_F_SPLIT if split else 0)
        check("ldpc_decode_f64", _lib.gpu().ldpc_decode_f64(
            self._h, B, _lib.ptr(llr), T, flags, _lib.ptr(z), _lib.ptr(conv), _lib.ptr(status),
            _lib.ptr(Lp), _lib.ptr(nl), _lib.ptr(hi), _lib.ptr(iters), _lib.ptr(E), None))
        return DecodeResult(z=z, conv=conv, status=status, iters=iters, nllr=nl, post=Lp, hist=hi, msgs=E)

    def decode_device(self, llr, max_iter, z=None, conv=None, status=None, post=None, nllr=None, hist=None,
                      iters=None, split=False, stream=None):
        """LDPC_F_DEVICE_PTRS: every buffer is device memory (anything with a
        data_ptr(), e.g. a torch CUDA tensor: llr [B, n] f64, z [B, n] u8,
        conv / status / iters [B] i32, post [B, n] f64, nllr [B] f64, hist
        [B, max_iter] f64), and the call is asynchronous on `stream` (a
        hipStream_t handle as int; None = the null stream) unless nllr or hist
        is requested.  Same results as decode()."""
        def dp(t):
            return None if t is None else ctypes.c_void_p(int(t.data_ptr()))
        B, n = int(llr.shape[0]), int(llr.shape[1])
        if n != self.graph.n:
            raise ValueError(f"llr must be [batch, {self.graph.n}]")
        flags = LDPC_F_DEVICE_PTRS | (LDPC_F_NLLR if (nllr is not None or hist is not None) else 0) | \
            (LDPC_F_SPLIT if split else 0)
        check("ldpc_decode_f64", _lib.gpu().ldpc_decode_f64(
            self._h, B, dp(llr), int(max_iter), flags, dp(z), dp(conv), dp(status), dp(post), dp(nllr), dp(hist),
            dp(iters), None, ctypes.c_void_p(int(stream)) if stream else None))

    def set_channel(self, spec):
        """The frame source's channel for generate() and phys_mc_run() on this
        decoder from now on (ldpc_channel_set): a channel.ChannelSpec, or None
        for the reference channel.  No device work."""
        from .channel import ChannelSpec
        if spec is None:
            check("ldpc_channel_set", _lib.lib().ldpc_channel_set(self._h, None))
            return
        if not isinstance(spec, ChannelSpec):
            raise ValueError(f"set_channel takes a ChannelSpec or None, got {type(spec).__name__}")
        model, bps, demap = spec.codes()
        c = _lib.Channel(model, bps, demap, 0)
        check("ldpc_channel_set", _lib.lib().ldpc_channel_set(self._h, ctypes.byref(c)))

    @property
    def channel(self):
        """The channel in force, as a channel.ChannelSpec (ldpc_channel_get)."""
        from .channel import ChannelSpec
        c = _lib.Channel()
        check("ldpc_channel_get", _lib.lib().ldpc_channel_get(self._h, ctypes.byref(c)))
        return ChannelSpec.from_codes(c.model, c.modulation, c.demap)

    def set_rate_match(self, rm):
        """The frame source's rate-matching pattern for generate() and
        phys_mc_run() on this decoder from now on (ldpc_rate_match_set): a
        ratematch.RateMatch; None or an empty one clears it.  Validated here
        (ValueError) and by the library; no device work."""
        from .ratematch import RateMatch
        if rm is None:
            rm = RateMatch()
        if not isinstance(rm, RateMatch):
            raise ValueError(f"set_rate_match takes a RateMatch or None, got {type(rm).__name__}")
        rm.validate(self.graph.n, self.graph.k)
        p, s = _lib.as_i32(rm.punctured), _lib.as_i32(rm.shortened)
        check("ldpc_rate_match_set", _lib.lib().ldpc_rate_match_set(
            self._h, len(p), _lib.i32p(p) if len(p) else None, len(s), _lib.i32p(s) if len(s) else None))

    @property
    def rate_match(self):
        """The pattern in force, as a ratematch.RateMatch (ldpc_rate_match_get)."""
        from .ratematch import RateMatch
        npu, nsh = _lib.c_i32(), _lib.c_i32()
        check("ldpc_rate_match_get", _lib.lib().ldpc_rate_match_get(
            self._h, ctypes.byref(npu), ctypes.byref(nsh), None, 0, None, 0))
        p, s = np.zeros(max(npu.value, 1), np.int32), np.zeros(max(nsh.value, 1), np.int32)
        check("ldpc_rate_match_get", _lib.lib().ldpc_rate_match_get(
            self._h, ctypes.byref(npu), ctypes.byref(nsh), _lib.i32p(p), len(p), _lib.i32p(s), len(s)))
        return RateMatch(tuple(int(x) for x in p[:npu.value]), tuple(int(x) for x in s[:nsh.value]))

    def set_interleaver(self, il):
        """The frame source's bit interleaver for generate(), phys_mc_run() and
        bitflip_mc_run() on this decoder from now on (ldpc_interleaver_set): an
        interleave.Interleaver; None clears it.  Its length must be the E of the
        pattern in force when frames are generated.  No device work."""
        from .interleave import Interleaver
        if il is None:
            check("ldpc_interleaver_set", _lib.lib().ldpc_interleaver_set(self._h, 0, None))
            return
        if not isinstance(il, Interleaver):
            raise ValueError(f"set_interleaver takes an Interleaver or None, got {type(il).__name__}")
        p = _lib.as_i32(il.perm)
        check("ldpc_interleaver_set", _lib.lib().ldpc_interleaver_set(self._h, len(p), _lib.i32p(p) if len(p) else None))

    @property
    def interleaver(self):
        """The interleaver in force as an interleave.Interleaver (kind "custom":
        the library keeps the permutation only), None without one."""
        from .interleave import Interleaver
        n = _lib.c_i32()
        check("ldpc_interleaver_get", _lib.lib().ldpc_interleaver_get(self._h, ctypes.byref(n), None, 0))
        if n.value == 0:
            return None
        p = np.zeros(n.value, np.int32)
        check("ldpc_interleaver_get", _lib.lib().ldpc_interleaver_get(self._h, ctypes.byref(n), _lib.i32p(p), len(p)))
        return Interleaver(tuple(int(x) for x in p))

    def set_fading_block(self, block_len):
        """The Rayleigh channel's coherence length from now on (ldpc_fading_set):
        block_len symbols (BPSK: bits) share a fade; 1 is a fade each (the
        default), anything >= the symbols of a frame is one fade per frame."""
        if isinstance(block_len, bool) or int(block_len) != block_len or not 1 <= block_len <= 2 ** 31 - 1:
            raise ValueError(f"set_fading_block takes an integer in [1, 2^31 - 1], got {block_len!r}")
        check("ldpc_fading_set", _lib.lib().ldpc_fading_set(self._h, int(block_len)))

    @property
    def fading_block(self):
        """The coherence length in force (ldpc_fading_get)."""
        n = _lib.c_i32()
        check("ldpc_fading_get", _lib.lib().ldpc_fading_get(self._h, ctypes.byref(n)))
        return int(n.value)

    def set_harq(self, plan):
        """The frame source's HARQ plan for generate(), phys_mc_run() and
        bitflip_mc_run() on this decoder from now on (ldpc_harq_set): a
        harq.HarqPlan; None clears it.  Every transmission's LLRs are added
        per column before the decoders see the frame.  No device work."""
        from .harq import HarqPlan
        if plan is None:
            check("ldpc_harq_set", _lib.lib().ldpc_harq_set(self._h, 0, None, None))
            return
        if not isinstance(plan, HarqPlan):
            raise ValueError(f"set_harq takes a HarqPlan or None, got {type(plan).__name__}")
        plan.validate(self.graph.n)
        lens = _lib.as_i32(plan.lengths)
        cols = _lib.as_i32([c for t in plan.tx for c in t])
        check("ldpc_harq_set", _lib.lib().ldpc_harq_set(self._h, len(lens), _lib.i32p(lens), _lib.i32p(cols)))

    @property
    def harq(self):
        """The plan in force as a harq.HarqPlan (kind "custom": the library
        keeps the lists only), None without one."""
        from .harq import MAX_TX, HarqPlan
        n = _lib.c_i32()
        lens = np.zeros(MAX_TX, np.int32)
        check("ldpc_harq_get", _lib.lib().ldpc_harq_get(self._h, ctypes.byref(n), _lib.i32p(lens), None, 0))
        if n.value == 0:
            return None
        cols = np.zeros(int(lens.sum()), np.int32)
        check("ldpc_harq_get", _lib.lib().ldpc_harq_get(self._h, ctypes.byref(n), _lib.i32p(lens), _lib.i32p(cols),
                                                        len(cols)))
        offs = np.concatenate([[0], np.cumsum(lens[:n.value])])
        return HarqPlan(tuple(tuple(int(x) for x in cols[offs[r]:offs[r + 1]]) for r in range(n.value)))

    def set_constellation(self, c):
        """The frame source's constellation table for generate(), phys_mc_run()
        and bitflip_mc_run() on this decoder from now on
        (ldpc_constellation_set): a constellation.Constellation, which replaces
        the channel model's modulation while it is set; None clears it.  No
        device work."""
        from .constellation import Constellation
        if c is None:
            check("ldpc_constellation_set", _lib.lib().ldpc_constellation_set(self._h, 0, None))
            self._constellation_name = "custom"
            return
        if not isinstance(c, Constellation):
            raise ValueError(f"set_constellation takes a Constellation or None, got {type(c).__name__}")
        xy = (ctypes.c_double * (2 * len(c.points)))(*c.flat())
        check("ldpc_constellation_set", _lib.lib().ldpc_constellation_set(self._h, c.bps, xy))
        self._constellation_name = c.name

    @property
    def constellation(self):
        """The table in force as a constellation.Constellation (the library
        stores the points; the name is the one last set here), None without one
        (ldpc_constellation_get)."""
        from .constellation import Constellation
        bps = ctypes.c_int32(0)
        check("ldpc_constellation_get", _lib.lib().ldpc_constellation_get(self._h, ctypes.byref(bps), None, 0))
        if bps.value == 0:
            return None
        xy = (ctypes.c_double * (2 << bps.value))()
        check("ldpc_constellation_get", _lib.lib().ldpc_constellation_get(self._h, ctypes.byref(bps), xy, len(xy)))
        return Constellation(getattr(self, "_constellation_name", "custom"),
                             tuple(complex(xy[2 * i], xy[2 * i + 1]) for i in range(1 << bps.value)))

    def generate(self, seed, snr_point, sigma, frame0, count, test_zero=False):
        """On-device synthetic frames (u bits, channel LLRs) copied back for testing.
        test_zero: the frame source's test-only erasures (LDPC_F_TEST_ZERO)."""
        g = self.graph
        u = np.empty((count, g.k), np.uint8)
        llr = np.empty((count, g.n), np.float64)
        check("ldpc_generate_frames", _lib.gpu().ldpc_generate_frames(
            self._h, int(seed), int(snr_point), float(sigma), int(frame0), int(count),
            _lib.LDPC_F_TEST_ZERO if test_zero else 0, _lib.ptr(u), _lib.ptr(llr), None))
        return u, llr

    def mc_run(self, seed, sigmas, frames_per_point, frame0, max_iter, nllr=False, static=False, split=False,
               test_zero=False):
        """Generate + decode + count on the GPU; returns int64 [n_points, 7] counters.

        Default schedule streams frames through the decoder's slots (a slot is
        refilled as soon as its frame stops); static=True decodes chunks of
        capacity frames to completion.  Same frames, identical counters.
        test_zero: the frame source's test-only erasures (LDPC_F_TEST_ZERO)."""
        sig = np.ascontiguousarray(np.asarray(sigmas, dtype=np.float64))
        out = np.zeros((len(sig), LDPC_MC_NCOUNT), np.int64)
        flags = (LDPC_F_NLLR if nllr else 0) | (LDPC_F_STATIC if static else 0) | (LDPC_F_SPLIT if split else 0) | \
            (_lib.LDPC_F_TEST_ZERO if test_zero else 0)
        check("ldpc_mc_run", _lib.gpu().ldpc_mc_run(
            self._h, int(seed), len(sig), sig.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            int(frames_per_point), int(frame0), int(max_iter), flags,
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None))
        return out

    def frame_order(self, seed, snr_point, sigma, frame0, count):
        """The streaming schedule's supply order of a point (ldpc_frame_order):
        local frame indices by descending syndrome weight of their channel hard
        decisions, ties in index order."""
        out = np.empty(int(count), np.int32)
        check("ldpc_frame_order", _lib.gpu().ldpc_frame_order(
            self._h, int(seed), int(snr_point), float(sigma), int(frame0), int(count), _lib.ptr(out), None))
        return out

    def phys_mc_run(self, phys_graph, seed, sigmas, frames_per_point, frame0, max_iter, hbm=False, cn="spa",
                    schedule="flooding", alpha=0.75, beta=0.5, qbits=None, llr_scale=4.0, tile=False, qtile=False):
        """Physical mode (§8 f4): same on-device frames, decoded on the sparse graph.

        This decoder's graph is the code's H_std (frame source) or, for an IRA
        code, phys_graph itself.  hbm=True forces the HBM-resident tile path,
        tile=True the layered schedule's (it needs schedule="layered").
        cn / schedule / alpha / beta as phys_decode (the defaults are
        ldpc_phys_mc_run, anything else ldpc_phys_mc_run_ex); qbits /
        llr_scale / qtile as phys_decode (ldpc_phys_mc_run_q)."""
        _need_qbits(qtile, qbits)
        rule, sched, param = phys_rule_args(cn, schedule, alpha, beta)
        flags = phys_flags(hbm, tile, schedule, qtile)
        if qbits is not None:
            qbits, llr_scale, param_q = phys_quant_args(cn, alpha, beta, qbits, llr_scale)
        sig = np.ascontiguousarray(np.asarray(sigmas, dtype=np.float64))
        out = np.zeros((len(sig), LDPC_MC_NCOUNT), np.int64)
        head = (self._h, phys_graph.handle, int(seed), len(sig), sig.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                int(frames_per_point), int(frame0), int(max_iter), flags)
        tail = (out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None)
        if qbits is not None:
            check("ldpc_phys_mc_run_q", _lib.gpu().ldpc_phys_mc_run_q(*head, rule, sched, qbits, llr_scale, param_q,
                                                                      *tail))
        elif (cn, schedule) == ("spa", "flooding"):
            check("ldpc_phys_mc_run", _lib.gpu().ldpc_phys_mc_run(*head, *tail))
        else:
            check("ldpc_phys_mc_run_ex", _lib.gpu().ldpc_phys_mc_run_ex(*head, rule, sched, param, *tail))
        return out

    def bitflip_mc_run(self, phys_graph, seed, sigmas, frames_per_point, frame0, max_iter, weight=0.0, theta=0.0,
                       generic=False):
        """phys_mc_run with a bit-flipping decoder (ldpc_bf_mc_run): the same
        on-device frames, channel and rate-matching pattern, the same seven
        counters.  weight / theta / generic as bitflip_decode; with mc_stats on
        the run uses the per-frame kernel."""
        weight, theta = bitflip_args(weight, theta)
        sig = np.ascontiguousarray(np.asarray(sigmas, dtype=np.float64))
        out = np.zeros((len(sig), LDPC_MC_NCOUNT), np.int64)
        check("ldpc_bf_mc_run", _lib.gpu().ldpc_bf_mc_run(
            self._h, phys_graph.handle, int(seed), len(sig), sig.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            int(frames_per_point), int(frame0), int(max_iter), LDPC_F_BF_GENERIC if generic else 0, weight, theta,
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None))
        return out

    KINDS = ("cn", "vn", "generate", "count", "phys", "phys_cn", "phys_vn", "tile", "cn_edge", "vn_edge",
             "vn_cols")

    def profile(self, enable=True):
        check("ldpc_profile_enable", _lib.gpu().ldpc_profile_enable(self._h, 1 if enable else 0))

    def profile_read(self):
        """{kind: (total_ms, launches)} of this decoder's launches since the last read."""
        ms = (ctypes.c_double * len(self.KINDS))()
        n = (ctypes.c_int64 * len(self.KINDS))()
        check("ldpc_profile_read", _lib.gpu().ldpc_profile_read(self._h, ms, n))
        return {k: (ms[i], n[i]) for i, k in enumerate(self.KINDS)}

    def rare_rows(self):
        """(rows queued to cn_rare_kernel, rare rows the tile decoders took in-kernel)
        since the last call (ldpc_rare_rows_read)."""
        out = (ctypes.c_int64 * 2)()
        check("ldpc_rare_rows_read", _lib.gpu().ldpc_rare_rows_read(self._h, out))
        return int(out[0]), int(out[1])

    def fixed_point(self):
        """(frames the static sub-tile decoder stopped at a bitwise fixed point,
        frame-passes those frames did not execute) since the last call
        (ldpc_fixed_point_read; LDPC_FIXED_POINT=0 switches the exit off)."""
        out = (ctypes.c_int64 * 2)()
        check("ldpc_fixed_point_read", _lib.gpu().ldpc_fixed_point_read(self._h, out))
        return int(out[0]), int(out[1])

    def mc_stats(self, enable=True, max_failed=0):
        """Collect the Monte-Carlo statistics of every phys_mc_run on this
        decoder from now on (ldpc_mc_stats_enable): the histogram of the
        convergence iteration, the undetected errors and up to max_failed
        failed-frame records per SNR point.  The counters do not change."""
        if int(max_failed) < 0:
            raise ValueError(f"max_failed must be >= 0, got {max_failed}")
        check("ldpc_mc_stats_enable", _lib.gpu().ldpc_mc_stats_enable(self._h, 1 if enable else 0, int(max_failed)))
        self._max_failed = int(max_failed) if enable else 0

    def mc_stats_read(self, point, max_iter):
        """Statistics of SNR point `point` of the last phys_mc_run (max_iter as
        in that run): {"hist": int64 [max_iter + 1] -- frames by convergence
        iteration, the last bin the failed ones; "undetected_frames",
        "undetected_bit_errors": frames that converged to other info bits than
        were sent, and those bits; "failed": int64 [n, 2] (global frame index,
        info-bit errors) sorted by index, at most max_failed; "failed_dropped":
        failures beyond max_failed}.  Decoder.generate(seed, point, sigma,
        index, 1) regenerates a listed frame."""
        T = int(max_iter)
        cap = self._max_failed
        hist = np.zeros(T + 1, np.int64)
        und = np.zeros(2, np.int64)
        rec = np.zeros((cap, 2), np.int64)
        nf = np.zeros(2, np.int64)
        check("ldpc_mc_stats_read", _lib.gpu().ldpc_mc_stats_read(
            self._h, int(point), _lib.ptr(hist), T + 1, _lib.ptr(und), _lib.ptr(rec) if cap else None, cap,
            _lib.ptr(nf)))
        return {"hist": hist, "undetected_frames": int(und[0]), "undetected_bit_errors": int(und[1]),
                "failed": rec[:int(nf[0])].copy(), "failed_dropped": int(nf[1])}

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib._lib is not None and getattr(self, "_pid", None) == os.getpid():
            _lib._lib.ldpc_decoder_destroy(h)
        self._h = None

    def __del__(self):
        self.close()
