"""Tensor-level wrappers over the C-ABI (include/mvlt_hip.h).

PyTorch is plumbing here: device memory (caching allocator), the current HIP
stream and dtype bookkeeping.  Every function launches hand-written gfx950
kernels on torch's current stream; nothing falls back to eager torch math.
"""
import ctypes as C
import os

import torch

from . import _lib as L

_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16}
_ws = {}
_ws_need = {}     # (dtype, M, N, K, a_kmajor, b_kmajor, split_k) -> split-K workspace bytes
GEMM_TIMER = None   # bench.py: callable(flops, key) -> (start_event, end_event) or None; .layout = (a_kmajor, b_kmajor) it watches


_stream_cache = [None, None]

# ----------------------------------------------------------------------------- native host path (csrc/host.cpp)
# One native call per SwinTransformerBlock / BertLayer forward or backward pass (torch C++ extension over the same
# C-ABI).  MVLT_NATIVE_HOST=0 keeps every launch on the Python + ctypes path below (same kernels, same results).
NATIVE = os.environ.get("MVLT_NATIVE_HOST", "1") != "0"
_host = None


def host():
    global _host
    if _host is None:
        import importlib.util
        L.lib()                                   # same libmvlt_hip.so the extension binds by rpath
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_mvlt_host.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with `make -C medical-vision-langauge-transformer_amd/csrc` "
                               "(python __graft_entry__.py); there is no fallback")
        spec = importlib.util.spec_from_file_location("_mvlt_host", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        # abi_version() / struct_sizes() are compile-time constants of the extension: a stale _mvlt_host.so (built
        # against an older header) fails here instead of handing truncated structs to the kernels
        if mod.abi_version() != L.ABI_VERSION or list(mod.struct_sizes()) != [C.sizeof(s) for s in L.STRUCTS]:
            raise RuntimeError(f"_mvlt_host.so was compiled against ABI {mod.abi_version()}, libmvlt_hip.so / _lib.py are "
                               f"at ABI {L.ABI_VERSION} (or a struct size differs): rebuild both (make -C .../csrc)")
        _host = mod
    return _host


def stream_int():
    """Handle of the stream the current pass launches on, as a plain int (0 = the null stream)."""
    return int(_stream().value or 0)


def side_int(device):
    return int(side_stream(device).cuda_stream)


def s64(v):
    """64-bit unsigned seed -> the int64 the extension takes (two's complement, cast back in C++)."""
    return v - (1 << 64) if v >= (1 << 63) else v


def _stream():
    # torch.cuda.current_stream() costs ~5 us; engines pin it for the duration of a pass (pin_stream)
    if _stream_cache[0] is not None:
        return _stream_cache[0]
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_side = {}


def side_stream(device):
    """One extra HIP stream per device for work that is off the critical path (weight gradients)."""
    st = _side.get(device.index)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _side[device.index] = st
    return st


class on_side:
    """Launch the enclosed kernels on the side stream once everything queued on the main stream so
    far is done; tensors read there must be passed so the caching allocator keeps them alive."""

    def __init__(self, device, *tensors):
        self.dev, self.tensors = device, tensors

    def __enter__(self):
        side = side_stream(self.dev)
        side.wait_stream(torch.cuda.current_stream())
        # keep the operands alive until the side stream has been joined (cheaper than record_stream per
        # tensor, and also correct under hipGraph capture where the allocator cannot see stream use)
        _side_keepalive.append(self.tensors)
        self.prev = (_stream_cache[0], _stream_cache[1])
        _stream_cache[0], _stream_cache[1] = C.c_void_p(side.cuda_stream), "side"

    def __exit__(self, *a):
        _stream_cache[0], _stream_cache[1] = self.prev


_side_keepalive = []
_opt = {}


def opt_stream(device):
    """Third HIP stream: AdamW of finished gradient buckets runs here while the backward pass continues."""
    st = _opt.get(device.index)
    if st is None:
        st = _opt[device.index] = torch.cuda.Stream(device=device)
    return st


class on_stream:
    """Context manager: launch the enclosed ops on ``stream`` (ordering is the caller's business)."""

    def __init__(self, stream, tag):
        self.stream, self.tag = stream, tag

    def __enter__(self):
        self.prev = (_stream_cache[0], _stream_cache[1])
        _stream_cache[0], _stream_cache[1] = C.c_void_p(self.stream.cuda_stream), self.tag

    def __exit__(self, *a):
        _stream_cache[0], _stream_cache[1] = self.prev


def join_side(device):
    """Main stream waits for the side stream (end of a backward pass / before communication).
    The operands kept alive for the side stream are released to the main-stream allocator only now:
    anything that reuses their memory is ordered after this join."""
    st = _side.get(device.index)
    if st is not None:
        torch.cuda.current_stream().wait_stream(st)
    _side_keepalive.clear()
    if _host is not None:
        _host.side_release()


_pinned_scratch = []


def pin_scratch():
    """A HIP graph is about to record (or has recorded) the addresses of the scratch workspaces: never free them.
    Idempotent (a buffer is pinned once, by address) and limited to the buffers a capture can have seen: the "graph"-tagged
    Python workspaces and the native host path's scratch (the training pass's split-K workspaces used to be pinned
    again at every capture)."""
    have = {b.data_ptr() for b in _pinned_scratch}
    for key, buf in _ws.items():
        if key[2] == "graph" and buf.data_ptr() not in have:
            _pinned_scratch.append(buf)
            have.add(buf.data_ptr())
    if _host is not None:
        _host.scratch_pin()


class pin_stream:
    """Context manager: resolve torch's current stream once for a whole forward/backward pass."""

    def __enter__(self):
        self.prev = (_stream_cache[0], _stream_cache[1])
        # (inside a HIP-graph capture the scratch buffers keep their "graph" tag: their addresses are recorded)
        _stream_cache[0], _stream_cache[1] = C.c_void_p(torch.cuda.current_stream().cuda_stream), ("graph" if self.prev[1] == "graph" else None)

    def __exit__(self, *a):
        _stream_cache[0], _stream_cache[1] = self.prev


_ws_graph_keep = []


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype} (float32 / bfloat16 only)")


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("mvlt_amd ops run on the GPU only (no CPU fallback)")


def workspace(name, nbytes, device):
    key = (name, device.index, _stream_cache[1])      # the side stream gets its own scratch buffers
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None and _stream_cache[1] == "graph":
            _ws_graph_keep.append(buf)                 # a captured HIP graph has this pointer baked in: never free it
        if buf is not None and _stream_cache[1] == "side":
            buf.record_stream(side_stream(device))     # a queued side-stream kernel may still be using it
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        if _stream_cache[1] == "side":
            buf.record_stream(side_stream(device))
        _ws[key] = buf
    return buf


# ----------------------------------------------------------------------------- GEMM
def _ld(t):
    """Row stride of a 2-D operand; torch leaves the stride of a size-1 dimension arbitrary (a one-row matrix
    sliced out of a batch, B = 1 decode), so one-row matrices report their width."""
    return t.stride(0) if t.shape[0] != 1 else max(t.shape[1], 1)


def gemm(A, B, *, a_kmajor=False, b_kmajor=False, out=None, out_f32=False, bias=None, gelu=False,
         save_pre=None, dropout=None, rowscale=None, residual=None, rowmap=None, mul_gelu_grad=None,
         accumulate=False, split_k=0, ldc=None, a_colsum=None, m_dev=None, prefetch=None, tail=False):
    """C = epilogue(A @ B); see MvltGemm.  A: [M,K] (or [K,M] if a_kmajor);
    B: [N,K] torch-Linear layout (or [K,N] if b_kmajor).
    (Written for a short host path: ~330 calls per training step; pointers go into the struct as plain ints.)"""
    if not (A.is_cuda and B.is_cuda):
        raise RuntimeError("mvlt_amd ops run on the GPU only (no CPU fallback)")
    dtA = A.dtype
    sa, sb = A.shape, B.shape
    assert len(sa) == 2 and len(sb) == 2 and dtA == B.dtype and A.stride(1) == 1 and B.stride(1) == 1
    if a_kmajor:
        K, M = sa
    else:
        M, K = sa
    if b_kmajor:
        Kb, N = sb
    else:
        N, Kb = sb
    assert K == Kb, f"inner dims differ: {K} vs {Kb}"
    odt = torch.float32 if out_f32 else dtA
    if out is None:
        rows = M if rowmap is None else int(rowmap.numel())
        out = torch.empty((rows, N if ldc is None else ldc), dtype=odt, device=A.device)
    assert out.dtype == odt and out.stride(-1) == 1
    p = L.MvltGemm()
    p.dtype = dti = _DT[dtA]
    p.M, p.N, p.K = M, N, K
    p.A, p.lda = A.data_ptr(), (A.stride(0) if sa[0] != 1 else sa[1])
    p.B, p.ldb = B.data_ptr(), (B.stride(0) if sb[0] != 1 else sb[1])
    if a_kmajor:
        p.a_kmajor = 1
    if b_kmajor:
        p.b_kmajor = 1
    p.C = out.data_ptr()
    p.ldc = pldc = (_ld(out) if out.dim() == 2 else N)
    epi = 0
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N
        epi |= L.EPI_BIAS
        p.bias = bias.data_ptr()
    if gelu:
        epi |= L.EPI_GELU
        if save_pre is not None:
            assert save_pre.dtype == dtA and _ld(save_pre) == pldc
            epi |= L.EPI_SAVE_PRE
            p.pre = save_pre.data_ptr()
    if dropout is not None and dropout[0] > 0.0:
        epi |= L.EPI_DROPOUT
        p.dropout_p, p.seed, p.tag = float(dropout[0]), int(dropout[1]), int(dropout[2])
    if rowscale is not None:
        epi |= L.EPI_ROWSCALE
        p.rowscale, p.rows_per_scale = rowscale[0].data_ptr(), int(rowscale[1])
    if residual is not None:
        assert residual.dtype == dtA and residual.stride(-1) == 1
        epi |= L.EPI_RESIDUAL
        p.residual, p.ldr = residual.data_ptr(), _ld(residual)
    if rowmap is not None:
        assert rowmap.dtype == torch.int32
        epi |= L.EPI_ROWMAP
        p.rowmap = rowmap.data_ptr()
    if mul_gelu_grad is not None:
        assert mul_gelu_grad.dtype == dtA and _ld(mul_gelu_grad) == pldc
        epi |= L.EPI_MUL_GELU_GRAD
        p.aux = mul_gelu_grad.data_ptr()
    if out_f32:
        epi |= L.EPI_OUT_F32
    if accumulate:
        epi |= L.EPI_ACCUM
    if tail:                       # MVLT_EPI_TAIL: rows at or beyond *m_dev run the epilogue on a zero accumulator (k-slices refuse it)
        assert m_dev is not None and not a_kmajor
        epi |= L.EPI_TAIL
        split_k = split_k or 1
    p.epilogue = epi
    p.split_k = split_k
    if m_dev is not None:          # valid storage rows of A on the device (ragged batch planned on the GPU)
        p.m_dev = m_dev.data_ptr()
    if prefetch is not None:             # weights of the product that runs next: pulled towards the caches by this launch
        p.prefetch, p.prefetch_bytes = prefetch.data_ptr(), prefetch.numel() * prefetch.element_size()
    if a_colsum is not None:
        assert a_kmajor and a_colsum.dtype == torch.float32 and a_colsum.numel() == M
        p.a_colsum = a_colsum.data_ptr()
    lib = L.lib()
    wkey = (dti, M, N, K, a_kmajor, b_kmajor, split_k)
    need = _ws_need.get(wkey)
    if need is None:
        need = _ws_need[wkey] = lib.mvlt_gemm_workspace_bytes(C.byref(p))       # pure function of the key
    if need:
        ws = workspace("gemm", need, A.device)
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    if GEMM_TIMER is not None and GEMM_TIMER.layout == (int(a_kmajor), int(b_kmajor)):
        # bench.py: bracket the launch with HIP events on the stream it is launched on
        bm, bn, sp = C.c_int(), C.c_int(), C.c_int()
        lib.mvlt_gemm_plan(C.byref(p), C.byref(bm), C.byref(bn), C.byref(sp))
        evs = GEMM_TIMER(2.0 * M * N * K, (p.dtype, bm.value, bn.value, int(a_kmajor), int(b_kmajor)))
        if evs is not None:
            st = side_stream(A.device) if _stream_cache[1] == "side" else torch.cuda.current_stream()
            if not getattr(evs[1], "_mvlt_created", False):
                evs[1].record(st)                       # creates the underlying hipEvent_t; re-recorded by the library
                evs[1]._mvlt_created = True
            p.event_after_main = C.c_void_p(evs[1].cuda_event)
            evs[0].record(st)
            L.check(lib.mvlt_gemm(C.byref(p), _stream()), "mvlt_gemm")
            return out
    L.check(lib.mvlt_gemm(C.byref(p), _stream()), "mvlt_gemm")
    return out


def _head_gemm(A, W, bias, lda=None):
    """The MvltGemm of an MLM-head product (A: [M, K], W: [N, K], f32 bias or None) -> (p, M, N), without an output matrix: the decode
    heads (M <= 64, checked by their entry points) have none, mlm_head_ce (any M) sets C / ldc itself when logits are wanted.
    ``lda``: row stride of A when its rows are read in place out of a wider buffer."""
    _need_cuda(A, W)
    M, K = A.shape
    N = W.shape[0]
    p = L.MvltGemm()
    p.dtype, p.M, p.N, p.K = _dt(A), M, N, K
    p.A, p.lda, p.B, p.ldb = _p(A), _ld(A) if lda is None else lda, _p(W), _ld(W)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N
        p.epilogue, p.bias = L.EPI_BIAS, _p(bias)
    return p, M, N


# scratch of the head products, one part per row and 16 columns: planes x [M, nblk] f32 values + [M, nblk] int32 indices
_head_parts_cache = {}


def _head_parts(planes, M, N, device, tag=None):
    nblk = (N + 15) // 16
    key = (planes, M, nblk, device.index, tag)
    buf = _head_parts_cache.get(key)
    if buf is None:
        shape = (M, nblk) if planes == 1 else (planes, M, nblk)
        buf = _head_parts_cache[key] = (torch.empty(shape, dtype=torch.float32, device=device),
                                        torch.empty((M, nblk), dtype=torch.int32, device=device))
    return buf


class LogitRules:
    """The logit rules of constrained decoding over ``rows`` rows of a V-column head (mvlt_hip.h MvltLogitRules): the two bitmaps
    [rows, ceil(V / 32)] the plan kernel rebuilds per token from ``ids[:, :col]`` (int64 [rows, ld], the history as stored) and
    ``col`` (int64 [1], the number of generated tokens) -- both device tensors this object keeps alive -- and the prepared structs.
    ``struct(row0)``: the view of rows row0 .. of it (the entry points take at most 64 rows: larger batches go in chunks)."""

    def __init__(self, V, penalty, ngram, min_length, eos, ids, col):
        assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.stride(1) == 1 and col.dtype == torch.int64
        self.rows, self.V, self.ids, self.col = ids.shape[0], V, ids, col
        self.ld_words = (V + 31) // 32
        self.maps = torch.zeros((2, self.rows, self.ld_words), dtype=torch.int32, device=ids.device)
        self.args = (float(penalty), int(ngram), int(min_length), eos)
        self._structs = {}

    def struct(self, row0=0):
        r = self._structs.get(row0)
        if r is None:
            r = self._structs[row0] = L.MvltLogitRules()
            penalty, ngram, min_length, eos = self.args
            r.seen, r.banned, r.ld_words = _p(self.maps[0, row0:]), _p(self.maps[1, row0:]), self.ld_words
            r.penalty, r.ngram, r.min_length = penalty, ngram, min_length
            r.ids, r.ld_ids, r.col = _p(self.ids[row0:]), self.ids.stride(0), _p(self.col)
            r.eos_id, r.has_eos = (eos if eos is not None else -1), int(eos is not None)
        return r

    def plan(self):
        """Rebuild the bitmaps of every row from the history (mvlt_decode_rules_plan, a launch per 64 rows)."""
        for r0 in range(0, self.rows, 64):
            L.check(L.lib().mvlt_decode_rules_plan(C.byref(self.struct(r0)), min(64, self.rows - r0), self.V, _stream()),
                    "mvlt_decode_rules_plan")


def _head_call(name, args, rules):
    """Launch the head entry point ``name`` on ``args`` and the stream -- with ``rules`` (a prepared ``L.MvltLogitRules``) its
    ``_rules`` form, which takes the same arguments with the rules ahead of the stream."""
    if rules is not None:
        name, args = name + "_rules", args + (C.byref(rules),)
    L.check(getattr(L.lib(), name)(*args, _stream()), name)


def gemm_argmax(A, W, bias=None, rules=None):
    """argmax_n (A @ W^T + bias) and its value, without materialising the logits (greedy decoding).
    A: [M <= 64, K], W: [N, K] -> (int64 [M], f32 [M]).  ``rules`` (here and in the five head functions below): a prepared
    ``L.MvltLogitRules`` whose bitmaps the plan has filled -- the _rules form of the entry point applies them to the raw logits."""
    p, M, N = _head_gemm(A, W, bias)
    nblk = (N + 15) // 16
    pv = torch.empty((M, nblk), dtype=torch.float32, device=A.device)          # a stand-alone call: its scratch lives as long as the call
    pi = torch.empty((M, nblk), dtype=torch.int32, device=A.device)
    idx = torch.empty(M, dtype=torch.int64, device=A.device)
    val = torch.empty(M, dtype=torch.float32, device=A.device)
    _head_call("mvlt_gemm_argmax", (C.byref(p), _p(pv), _p(pi), _p(idx), _p(val)), rules)
    return idx, val


def gemm_argmax_greedy(A, W, bias, state, rules=None):
    """Decoder GEMM + greedy pick + the per-token bookkeeping of greedy_search in two launches (mvlt_gemm_argmax_greedy).
    A: [M <= 64, K] (rows may be strided), W: [N, K]; ``state``: a prepared ``L.MvltGreedyState`` (decode._GreedyGraph)."""
    # A.stride(0), not _ld(A): the head reads the [MASK] rows in place, at row stride 2 H of the step's hidden states
    p, M, N = _head_gemm(A, W, bias, lda=A.stride(0))
    pv, pi = _head_parts(1, M, N, A.device)
    _head_call("mvlt_gemm_argmax_greedy", (C.byref(p), _p(pv), _p(pi), C.byref(state)), rules)


def _sample_parts(M, N, device):
    # keyed by the stream tag: a captured graph keeps a scratch of its own (it records addresses)
    return _head_parts(4, M, N, device, tag=_stream_cache[1])


def gemm_sample(A, W, bias, seed, tag, temperature=1.0, rules=None):
    """One draw per row from softmax((A @ W^T + bias) / temperature) by Gumbel-max and its log-probability, without
    materialising the logits (mvlt_gemm_sample; the noise is a pure function of (seed, tag, row, column)).
    A: [M <= 64, K] (rows may be strided), W: [N, K] -> (int64 [M], f32 [M])."""
    p, M, N = _head_gemm(A, W, bias)
    pv, pi = _sample_parts(M, N, A.device)
    idx = torch.empty(M, dtype=torch.int64, device=A.device)
    lp = torch.empty(M, dtype=torch.float32, device=A.device)
    _head_call("mvlt_gemm_sample", (C.byref(p), _p(pv), _p(pi), _p(idx), _p(lp), int(seed) & ((1 << 64) - 1), int(tag) & 0xFFFFFFFF,
                                    1.0 / float(temperature)), rules)
    return idx, lp


def gemm_sample_step(A, W, bias, state, rules=None):
    """Decoder GEMM + sampled pick + the per-token bookkeeping of greedy_search in two launches (mvlt_gemm_sample_step).
    ``state``: a prepared ``L.MvltSampleState`` (decode._GreedyGraph, mode 'sample')."""
    p, M, N = _head_gemm(A, W, bias)
    pv, pi = _sample_parts(M, N, A.device)
    _head_call("mvlt_gemm_sample_step", (C.byref(p), _p(pv), _p(pi), C.byref(state)), rules)


def _pick_rows_tables(M, noise_row, inv_t):
    assert noise_row.dtype == torch.int32 and noise_row.is_cuda and noise_row.is_contiguous() and noise_row.numel() == M
    assert inv_t.dtype == torch.float32 and inv_t.is_cuda and inv_t.is_contiguous() and inv_t.numel() == M


def gemm_pick_rows(A, W, bias, noise_row, inv_t, seed, tag, rules=None):
    """The MLM head with a per-row pick over any number of rows (mvlt_gemm_pick_rows).  ``noise_row`` int32 [M]: >= 0 draws the
    row by Gumbel-max with the noise gemm_sample gives row ``noise_row[r]``, < 0 picks it greedily; ``inv_t`` f32 [M]: the
    row's inverse temperature (0 < inv_t < inf, not checked: device data).  Every row returns its token and the token's
    log-probability at its temperature -- for a greedy row too, where gemm_argmax returns the raw logit.
    ``rules``: a prepared ``L.MvltLogitRules`` over all M rows (``LogitRules.struct()``).
    A: [M, K] (rows may be strided), W: [N, K] -> (int64 [M], f32 [M])."""
    p, M, N = _head_gemm(A, W, bias)
    _pick_rows_tables(M, noise_row, inv_t)
    pv, pi = _sample_parts(M, N, A.device)
    idx = torch.empty(M, dtype=torch.int64, device=A.device)
    lp = torch.empty(M, dtype=torch.float32, device=A.device)
    seed, tag = int(seed) & ((1 << 64) - 1), int(tag) & 0xFFFFFFFF
    _head_call("mvlt_gemm_pick_rows", (C.byref(p), _p(pv), _p(pi), _p(noise_row), _p(inv_t), _p(idx), _p(lp), seed, tag), rules)
    return idx, lp


def gemm_pick_rows_step(A, W, bias, state, noise_row, inv_t, rules=None):
    """gemm_pick_rows with the per-token bookkeeping of gemm_sample_step over the M rows of ``state``, a prepared
    ``L.MvltSampleState`` (mvlt_gemm_pick_rows_step; decode._MultiSampleGraph).  The tables are read at their address every
    call: a captured graph keeps them alive."""
    p, M, N = _head_gemm(A, W, bias)
    _pick_rows_tables(M, noise_row, inv_t)
    pv, pi = _sample_parts(M, N, A.device)
    _head_call("mvlt_gemm_pick_rows_step", (C.byref(p), _p(pv), _p(pi), _p(noise_row), _p(inv_t), C.byref(state)), rules)


def check_sample_filter(top_k, top_p):
    """(int top_k, float top_p) of a sampled pick, or ValueError: top_k >= 0 (0 = off), top_p > 0 (>= 1 = off), no NaN."""
    if isinstance(top_k, float) and top_k != top_k:
        raise ValueError("top_k must be a non-negative integer")
    k, p = int(top_k), float(top_p)
    if k < 0 or k != top_k:
        raise ValueError("top_k must be a non-negative integer (0 switches the filter off)")
    if not p > 0.0:
        raise ValueError("top_p must lie in (0, 1] (1 switches the filter off)")
    return k, p


_filter_ws_cache = {}


def _sample_filter(M, N, device, top_k, top_p, row0):
    """MvltSampleFilter with its [M, ldx] f32 logit workspace, keyed like the part buffers by the stream tag (a captured graph
    keeps a workspace of its own: it records the address)."""
    ldx = (N + 3) // 4 * 4
    key = (M, ldx, device.index, _stream_cache[1])
    ws = _filter_ws_cache.get(key)
    if ws is None:
        ws = _filter_ws_cache[key] = torch.empty((M, ldx), dtype=torch.float32, device=device)
    f = L.MvltSampleFilter()
    f.top_k, f.top_p, f.x, f.ldx, f.row0 = min(int(top_k), 2 ** 31 - 1), float(top_p), _p(ws), ldx, int(row0)
    return f, ws


def gemm_sample_filtered(A, W, bias, seed, tag, temperature=1.0, top_k=0, top_p=1.0, row0=0, rules=None):
    """gemm_sample behind a top-k / top-p filter (mvlt_gemm_sample_filtered): per row, keep the top_k largest logits (ties at
    the threshold all kept; 0 = off), then the tokens whose mass strictly above is below top_p of what is left (1.0 = off), draw
    among them by Gumbel-max and return the log-probability under the renormalised distribution.  ``row0``: index of row 0
    within the batch the noise is indexed by, so a batch issued in row chunks draws what one call would.
    A: [M <= 64, K], W: [N, K] -> (int64 [M], f32 [M])."""
    top_k, top_p = check_sample_filter(top_k, top_p)
    p, M, N = _head_gemm(A, W, bias)
    pv, pi = _sample_parts(M, N, A.device)
    f, _ = _sample_filter(M, N, A.device, top_k, top_p, row0)
    idx = torch.empty(M, dtype=torch.int64, device=A.device)
    lp = torch.empty(M, dtype=torch.float32, device=A.device)
    _head_call("mvlt_gemm_sample_filtered", (C.byref(p), _p(pv), _p(pi), C.byref(f), _p(idx), _p(lp), int(seed) & ((1 << 64) - 1),
                                             int(tag) & 0xFFFFFFFF, 1.0 / float(temperature)), rules)
    return idx, lp


def gemm_sample_filtered_step(A, W, bias, state, top_k=0, top_p=1.0, rules=None):
    """gemm_sample_step with the filtered pick as its finish (mvlt_gemm_sample_filtered_step); ``state``: a prepared
    ``L.MvltSampleState`` (decode._GreedyGraph, mode 'sample' with a filter)."""
    top_k, top_p = check_sample_filter(top_k, top_p)
    p, M, N = _head_gemm(A, W, bias)
    pv, pi = _sample_parts(M, N, A.device)
    f, _ = _sample_filter(M, N, A.device, top_k, top_p, 0)
    _head_call("mvlt_gemm_sample_filtered_step", (C.byref(p), _p(pv), _p(pi), C.byref(f), C.byref(state)), rules)


BEAM_MAX_BEAMS, BEAM_MAX_CAND = 8, 16          # limits of mvlt_gemm_beam_candidates (csrc/skinny.hip BEAM_MAXB / BEAM_MAXC)


def beam_rules_plan(rules, seq, rows, V):
    """Rebuild the bitmaps of ``rules`` (a prepared ``L.MvltLogitRules``; its ids / ld_ids are not read) for the first ``rows`` rows
    from the int32 live sequences ``seq`` [>= rows, ld] of beam search and ``rules.col`` (mvlt_beam_rules_plan: one launch, any
    number of rows)."""
    assert seq.dtype == torch.int32 and seq.dim() == 2 and seq.stride(1) == 1 and seq.shape[0] >= rows
    L.check(L.lib().mvlt_beam_rules_plan(C.byref(rules), _p(seq), seq.stride(0), int(rows), int(V), _stream()), "mvlt_beam_rules_plan")


class BeamLogitRules:
    """The logit rules of a beam search over ``seq.shape[0]`` = B * num_beams hypotheses of a V-column head: the two bitmaps
    [rows, ceil(V / 32)], the history ``seq`` (int32 [rows, max_length]: the hypotheses' own tokens after the beam reorder, the layout
    of MvltBeamStep.seq) and ``col`` (int64 [1], the number of generated tokens) -- device tensors this object keeps alive -- and
    the prepared struct.  ``plan(rows)`` before every candidate call (step 0 scores one row per sample: rows = B, col = 0)."""

    def __init__(self, V, penalty, ngram, min_length, eos, seq, col):
        assert seq.dtype == torch.int32 and seq.dim() == 2 and seq.stride(1) == 1 and col.dtype == torch.int64
        self.rows, self.V, self.seq, self.col = seq.shape[0], V, seq, col
        self.ld_words = (V + 31) // 32
        self.maps = torch.zeros((2, self.rows, self.ld_words), dtype=torch.int32, device=seq.device)
        r = self.struct = L.MvltLogitRules()
        r.seen, r.banned, r.ld_words = _p(self.maps[0]), _p(self.maps[1]), self.ld_words
        r.penalty, r.ngram, r.min_length = float(penalty), int(ngram), int(min_length)
        r.ids, r.ld_ids, r.col = None, 0, _p(col)
        r.eos_id, r.has_eos = (eos if eos is not None else -1), int(eos is not None)

    def plan(self, rows=None):
        beam_rules_plan(self.struct, self.seq, self.rows if rows is None else rows, self.V)


def gemm_beam_candidates(A, W, bias, beam_scores, num_beams, n_cand, want_lse=False, out=None, ws=None, rules=None):
    """The candidate step of beam search without the logits round trip (mvlt_gemm_beam_candidates): A: [G * num_beams, K] (the
    beams of sample g are the rows g * num_beams .. + num_beams; any number of rows), W: [N, K], beam_scores f32 [G * num_beams].
    Per sample the n_cand largest log_softmax(A @ W^T + bias) + beam score over (beam, token), sorted descending, ties by the
    lower beam * N + token.  Returns ``(out, lse)``: ``out`` one int32 tensor [3, G, n_cand] -- out[0] viewed as f32 holds the
    scores, out[1] the beams, out[2] the tokens (one buffer: one read-back) -- and lse f32 [rows] or None.
    ``out`` / ``ws``: caller-owned buffers for the lists (int32 [3, G, n_cand], contiguous) and the f32 logits workspace (at least
    rows * ldx elements, ldx = N rounded up to 4) -- a replayed decode loop reads the lists at a fixed address.
    ``rules``: a prepared ``L.MvltLogitRules`` whose bitmaps ``beam_rules_plan`` has filled for these rows -- the rules act on the
    log-probabilities ahead of the beam score, banned entries are never listed (mvlt_gemm_beam_candidates_rules); a sample with
    fewer than n_cand unbanned entries ends its list with (-inf, 0, 0)."""
    p, M, N = _head_gemm(A, W, bias)
    assert beam_scores.dtype == torch.float32 and beam_scores.is_contiguous() and beam_scores.numel() == M
    ldx = (N + 3) // 4 * 4
    if ws is None:
        ws = workspace("beam_logits", M * ldx * 4, A.device)
    else:
        assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= M * ldx
    G = M // max(int(num_beams), 1)
    if out is None:
        out = torch.empty((3, G, n_cand), dtype=torch.int32, device=A.device)
    else:
        assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (3, G, n_cand)
    lse = torch.empty(M, dtype=torch.float32, device=A.device) if want_lse else None
    c = L.MvltBeamCand()
    c.num_beams, c.n_cand, c.beam_scores, c.x, c.ldx = int(num_beams), int(n_cand), _p(beam_scores), _p(ws), ldx
    c.cand_score, c.cand_beam, c.cand_tok, c.lse = _p(out[0]), _p(out[1]), _p(out[2]), (_p(lse) if want_lse else None)
    _head_call("mvlt_gemm_beam_candidates", (C.byref(p), C.byref(c)), rules)
    return out, lse


def beam_step(state, src_beams=None):
    """One token of beam-search bookkeeping on the device (mvlt_beam_step): consumes the candidate lists ``state`` points at and
    advances pool, live sequences, slot table, beam scores, next ids and the counters.  ``state``: a prepared ``L.MvltBeamStep``
    (decode.BeamDeviceState); ``src_beams``: the num_beams of the candidate call that made the lists (1 at step 0), when given."""
    if src_beams is not None:
        state.src_beams = int(src_beams)
    L.check(L.lib().mvlt_beam_step(C.byref(state), _stream()), "mvlt_beam_step")


def mlm_head_ce(t2, W, bias, labels, V, rows_dev=None, want_logits=True):
    """MLM decoder product with the cross-entropy forward in its epilogue (mvlt_mlm_head_ce): t2 [M, K], W [V, K], f32 bias [V],
    int64 labels [M] (negative = ignored), rows_dev (int32 device scalar): only the first *rows_dev rows exist.
    Returns ``(acc, lse, x_label, logits)``: acc f32 [2] = (sum of nll over the labelled rows, their number) as ce_fwd returns
    it, lse f32 [M], x_label f32 [M] (the logit at the label; untouched where the label is ignored), and the logits in the
    storage dtype ([M, ld] with ld = V rounded up to 64, as the head's plain product lays them out) or None with
    ``want_logits=False`` -- then no logits exist anywhere."""
    _need_cuda(t2, W, bias, labels)
    assert W.shape[0] == V and t2.dtype == W.dtype and t2.stride(1) == 1 and W.stride(1) == 1
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == t2.shape[0]
    p, M, _ = _head_gemm(t2, W, bias)
    dev = t2.device
    logits = None
    if want_logits:
        ld = (V + 63) // 64 * 64
        logits = torch.empty((M, ld), dtype=t2.dtype, device=dev)
        p.C, p.ldc = _p(logits), ld
    if rows_dev is not None:
        p.m_dev = _p(rows_dev)
    out = torch.empty(2 * M + 2, dtype=torch.float32, device=dev)
    lse, x_label, acc = out[:M], out[M:2 * M], out[2 * M:]
    h = L.MvltHeadCE()
    h.labels, h.lse, h.x_label, h.acc = _p(labels), _p(lse), _p(x_label), _p(acc)
    need = L.lib().mvlt_mlm_head_ce_workspace_bytes(M, V)
    ws = workspace("head_ce", need, dev)
    h.workspace, h.workspace_bytes = _p(ws), ws.numel()
    L.check(L.lib().mvlt_mlm_head_ce(C.byref(p), C.byref(h), _stream()), "mvlt_mlm_head_ce")
    return acc, lse, x_label, logits


def retrieval_head_supported(dtype, H):
    """True when mvlt_retrieval_head covers this compute dtype and width (bf16, H % 64 == 0, H <= 1024)."""
    return dtype in _DT and bool(L.lib().mvlt_retrieval_head_supported(_DT[dtype], int(H)))


def retrieval_head(hidden, row_start, w_pool, b_pool, w_tr, b_tr, gamma, beta, eps, w_out, b_out, out_index, scores, *,
                   p_dev=None, want=False):
    """Scoring head of MVLBertForRetrieval in one launch (mvlt_retrieval_head): hidden [R, H] packed encoder rows, row_start int32
    [P] (the [CLS] rows), out_index int64 [P] flat positions in ``scores`` (f32, written in place).  ``want=True`` also returns
    ``(pooled [P, H], t1 [P, H], logits f32 [P, 2])``; p_dev (int32 device scalar): only the first *p_dev pairs exist."""
    _need_cuda(hidden, row_start, w_pool, w_tr, w_out, out_index, scores)
    P, H = row_start.numel(), hidden.shape[1]
    assert hidden.dim() == 2 and hidden.stride(1) == 1 and row_start.dtype == torch.int32 and row_start.is_contiguous()
    assert out_index.dtype == torch.int64 and out_index.is_contiguous() and out_index.numel() == P
    assert scores.dtype == torch.float32 and scores.is_contiguous()
    for w in (w_pool, w_tr, w_out):
        assert w.dtype == hidden.dtype and w.is_contiguous() and w.shape[1] == H
    assert w_pool.shape[0] == H and w_tr.shape[0] == H and w_out.shape[0] == 2
    for b in (b_pool, b_tr, gamma, beta, b_out):
        assert b.dtype == torch.float32 and b.is_contiguous()
    h = L.MvltRetrievalHead()
    h.dtype, h.P, h.H = _dt(hidden), P, H
    h.hidden, h.ld_hidden, h.row_start, h.p_dev = _p(hidden), _ld(hidden), _p(row_start), _p(p_dev)
    h.w_pool, h.b_pool, h.w_tr, h.b_tr = _p(w_pool), _p(b_pool), _p(w_tr), _p(b_tr)
    h.ln_gamma, h.ln_beta, h.ln_eps, h.w_out, h.b_out = _p(gamma), _p(beta), float(eps), _p(w_out), _p(b_out)
    h.out_index, h.scores = _p(out_index), _p(scores)
    extra = None
    if want:
        extra = (torch.empty((P, H), dtype=hidden.dtype, device=hidden.device),
                 torch.empty((P, H), dtype=hidden.dtype, device=hidden.device),
                 torch.empty((P, 2), dtype=torch.float32, device=hidden.device))
        h.pooled, h.t1, h.logits = _p(extra[0]), _p(extra[1]), _p(extra[2])
    L.check(L.lib().mvlt_retrieval_head(C.byref(h), _stream()), "mvlt_retrieval_head")
    return extra


def recall_ranks(scores, image_group, caption_group):
    """(i2t_rank int32 [Ni], t2i_rank int32 [Nc]) of a f32 score matrix [Ni, Nc] (row stride >= Nc); see mvlt_recall_ranks."""
    _need_cuda(scores, image_group, caption_group)
    assert scores.dim() == 2 and scores.dtype == torch.float32 and scores.stride(1) == 1
    Ni, Nc = scores.shape
    assert image_group.dtype == torch.int64 and image_group.is_contiguous() and image_group.numel() == Ni
    assert caption_group.dtype == torch.int64 and caption_group.is_contiguous() and caption_group.numel() == Nc
    ranks = torch.empty(Ni + Nc, dtype=torch.int32, device=scores.device)
    i2t, t2i = ranks[:Ni], ranks[Ni:]
    L.check(L.lib().mvlt_recall_ranks(_p(scores), _ld(scores) if Ni > 1 else max(scores.stride(0), Nc), Ni, Nc, _p(image_group),
                                      _p(caption_group), _p(i2t), _p(t2i), _stream()), "mvlt_recall_ranks")
    return i2t, t2i


def recall_counts(rank, ks, out=None):
    """int32 [len(ks)] on the device: the number of ranks below each threshold (mvlt_recall_counts)."""
    _need_cuda(rank)
    assert rank.dtype == torch.int32 and rank.is_contiguous()
    nk = len(ks)
    if out is None:
        out = torch.empty(nk, dtype=torch.int32, device=rank.device)
    arr = (C.c_int * nk)(*[int(k) for k in ks])
    L.check(L.lib().mvlt_recall_counts(_p(rank), rank.numel(), arr, nk, _p(out), _stream()), "mvlt_recall_counts")
    return out


REPORT_MAX_PIECES = 512          # a row of mvlt_report_ngram_keys / mvlt_report_stats (BERT's position limit)


def _report_rows(ids, what):
    assert ids.dim() == 2 and ids.dtype == torch.int64 and ids.stride(1) == 1 and ids.shape[0] > 0, f"{what}: int64 [rows, T]"
    if not 0 < ids.shape[1] <= REPORT_MAX_PIECES:
        raise ValueError(f"{what}: a row holds {ids.shape[1]} pieces, the kernels take 1 .. {REPORT_MAX_PIECES}")


def _report_common(flags, stop_ids):
    if flags is not None:
        assert flags.dtype == torch.uint8 and flags.dim() == 1 and flags.is_contiguous() and flags.numel() > 0
    stops = [int(s) for s in stop_ids]
    if len(stops) > 8:
        raise ValueError("at most 8 stop ids")
    return (C.c_int64 * max(len(stops), 1))(*stops), len(stops), (flags.numel() if flags is not None else 0)


def report_ngram_keys(ids, flags, stop_ids):
    """(keys int64 [rows, 4, T], n_words int32 [rows]): the distinct n-grams of every row as 64-bit keys, INT64_MAX elsewhere
    (mvlt_report_ngram_keys)."""
    _need_cuda(ids, flags)
    _report_rows(ids, "ids")
    arr, ns, V = _report_common(flags, stop_ids)
    rows, T = ids.shape
    keys = torch.empty((rows, 4, T), dtype=torch.int64, device=ids.device)
    n_words = torch.empty(rows, dtype=torch.int32, device=ids.device)
    L.check(L.lib().mvlt_report_ngram_keys(_p(ids), _ld(ids), rows, T, _p(flags), V, arr, ns, _p(keys), _p(n_words), _stream()),
            "mvlt_report_ngram_keys")
    return keys, n_words


def report_stats(hyp, ref, index, flags, stop_ids, df_keys, df_counts):
    """(stats int32 [rows, 11], cider f64 [rows]) of hyp [rows, Th] against ref[index] (ref [N, Tr]; index int32 [rows] or None:
    row i against reference i); see mvlt_report_stats."""
    _need_cuda(hyp, ref, index, flags, df_keys, df_counts)
    _report_rows(hyp, "hyp")
    _report_rows(ref, "ref")
    arr, ns, V = _report_common(flags, stop_ids)
    rows, N = hyp.shape[0], ref.shape[0]
    if index is None:
        if rows > N:
            raise ValueError(f"{rows} hypotheses for {N} references: pass index")
    else:
        assert index.dtype == torch.int32 and index.is_contiguous() and index.numel() == rows
    assert df_keys.dtype == torch.int64 and df_counts.dtype == torch.int32 and df_keys.is_contiguous() and df_counts.is_contiguous()
    assert df_keys.numel() == df_counts.numel()
    stats = torch.empty((rows, 11), dtype=torch.int32, device=hyp.device)
    cider = torch.empty(rows, dtype=torch.float64, device=hyp.device)
    K = df_keys.numel()
    L.check(L.lib().mvlt_report_stats(_p(hyp), _ld(hyp), rows, hyp.shape[1], _p(ref), _ld(ref), N, ref.shape[1], _p(index), _p(flags),
                                      V, arr, ns, _p(df_keys) if K else None, _p(df_counts) if K else None, K, _p(stats), _p(cider),
                                      _stream()), "mvlt_report_stats")
    return stats, cider


def gumbel_noise(seed, tag, rows, N, device):
    """The noise of gemm_sample as the kernel computes it, f32 [rows, N] (tests)."""
    out = torch.empty((rows, N), dtype=torch.float32, device=device)
    L.check(L.lib().mvlt_gumbel_noise(int(seed) & ((1 << 64) - 1), int(tag) & 0xFFFFFFFF, rows, N, _p(out), _stream()), "mvlt_gumbel_noise")
    return out


def gemm_skinny_accum(A, W, acc, k_splits):
    """acc[s] (f32 [k_splits, M, N]) = A[:, k-slice s] @ W[:, k-slice s]^T: the reduction split over k_splits workgroups per
    column tile, every slice in a slab of its own (no atomics; layernorm_acc_fwd adds them in slice order)."""
    _need_cuda(A, W)
    M, K = A.shape
    N = W.shape[0]
    assert acc.dtype == torch.float32 and acc.shape == (k_splits, M, N) and acc.is_contiguous() and A.stride(1) == 1 and W.stride(1) == 1
    p = L.MvltGemm()
    p.dtype, p.M, p.N, p.K = _dt(A), M, N, K
    p.A, p.lda, p.B, p.ldb = A.data_ptr(), _ld(A), W.data_ptr(), _ld(W)
    L.check(L.lib().mvlt_gemm_skinny_accum(C.byref(p), _p(acc), int(k_splits), _stream()), "mvlt_gemm_skinny_accum")
    return acc


def layernorm_acc_fwd(acc, bias, residual, gamma, beta, eps, dtype, out=None):
    """LayerNorm(sum_s acc[s] + bias + residual); acc: the f32 slabs [nsplit, rows, C] of gemm_skinny_accum."""
    nsplit, rows, Cn = acc.shape
    y = out if out is not None else torch.empty((rows, Cn), dtype=dtype, device=acc.device)
    L.check(L.lib().mvlt_layernorm_acc_fwd(_DT[dtype], _p(acc), int(nsplit), _p(bias), _p(residual), _p(gamma), _p(beta), float(eps),
                                           rows, Cn, _p(y), _stream()), "mvlt_layernorm_acc_fwd")
    return y


_GROUP_LONG_K = 8192
# MVLT_DETERMINISTIC=1: no float-atomic k-slices in the GEMM path (the 4-wave fallback of the Swin stage-0/1 weight
# gradients takes split-K slabs + the deterministic reduce).  Greedy decoding needs no flag since round 5: its split
# reductions meet in slabs summed in slice order.  Still
# accumulated with float atomics under the flag: the relative-position-bias-table gradient (swin_attn_bwd2_kernel) and the
# word-embedding gradient (embed_bwd); tests/test_model_gpu.py::test_config2_step_is_bit_reproducible_* lists them.  The
# flag is read once at import: set it before importing the package.
DETERMINISTIC = os.environ.get("MVLT_DETERMINISTIC", "0") == "1"


def wgrad_group(items):
    """Weight gradients of one layer: items = [(dY [R,No], X [R,Ni], dW f32 [No,Ni], dbias f32 [No] | None), ...]
    -> dW_i = dY_i^T X_i (and dbias_i = column sums of dY_i).  When the items qualify (mvlt_gemm_group) and
    their 64-row tiles together fill the GPU, they go out as ONE launch without split-K -- instead of
    len(items) split-K launches plus their reduce kernels; with few tiles but >= 8192 reduction rows (Swin stages
    0/1) still one launch, cut into k-slices that meet in the zeroed f32 output by atomicAdd; otherwise one gemm() each."""
    lib = L.lib()
    n = len(items)
    m_dev = None
    if items and len(items[0]) == 5:          # (dy, x, dw, db, m_dev): the reduction length lives on the device
        m_dev = items[0][4]
        items = [it[:4] for it in items]
    bn = 128 if all(x.shape[1] % 128 == 0 for _, x, _, _ in items) else (96 if all(x.shape[1] % 96 == 0 for _, x, _, _ in items) else 0)
    tiles = sum(((dy.shape[1] + 63) // 64) * ((x.shape[1] + bn - 1) // bn) for dy, x, _, _ in items) if bn else 0
    # few tiles but a long reduction (Swin stages 0/1): still one launch, cut into k-slices inside mvlt_gemm_group
    slices_ok = items[0][0].dtype == torch.bfloat16      # bf16: k-slices through the 8-wave engine's deterministic slab reduce
    if not (1 < n <= 8 and bn and (tiles >= 200 or (slices_ok and items[0][0].shape[0] >= _GROUP_LONG_K))):
        for dy, x, dw, db in items:
            gemm(dy, x, a_kmajor=True, b_kmajor=True, out=dw, out_f32=True, a_colsum=db, m_dev=m_dev)
        return
    arr = (L.MvltGemm * n)()
    flops = 0.0
    for i, (dy, x, dw, db) in enumerate(items):
        _need_cuda(dy, x)
        assert dy.dtype == x.dtype and dy.stride(1) == 1 and x.stride(1) == 1 and dy.shape[0] == x.shape[0]
        assert dw.dtype == torch.float32 and dw.shape == (dy.shape[1], x.shape[1]) and dw.stride(1) == 1
        p = arr[i]
        p.dtype, p.M, p.N, p.K = _dt(dy), dy.shape[1], x.shape[1], dy.shape[0]
        p.A, p.lda, p.a_kmajor = _p(dy), dy.stride(0), 1
        p.B, p.ldb, p.b_kmajor = _p(x), x.stride(0), 1
        p.C, p.ldc = _p(dw), dw.stride(0)
        p.epilogue, p.split_k = L.EPI_OUT_F32, 1
        if m_dev is not None:
            p.m_dev = m_dev.data_ptr()
        if db is not None:
            assert db.dtype == torch.float32 and db.numel() == dy.shape[1]
            p.a_colsum = _p(db)
        flops += 2.0 * p.M * p.N * p.K
    need = lib.mvlt_gemm_group_workspace_bytes(arr, n)          # k-slice slabs of the 8-wave engine (0: none)
    if need:
        ws = workspace("gemm_group", need, items[0][0].device)
        arr[0].workspace, arr[0].workspace_bytes = ws.data_ptr(), ws.numel()
    evs = GEMM_TIMER(flops, ("group", arr[0].dtype, 64, bn)) if GEMM_TIMER is not None else None
    st = None
    if evs is not None:
        st = side_stream(items[0][0].device) if _stream_cache[1] == "side" else torch.cuda.current_stream()
        evs[0].record(st)
    L.check(lib.mvlt_gemm_group(arr, n, _stream()), "mvlt_gemm_group")
    if evs is not None:
        evs[1].record(st)


def prefetch(tensors):
    """Pull up to 8 read-only tensors (weights about to be used) towards the GPU's caches: one launch, nothing written."""
    arr = (L.MvltRange * len(tensors))()
    for i, t in enumerate(tensors):
        assert t.is_cuda and t.is_contiguous()
        arr[i].ptr, arr[i].bytes = t.data_ptr(), t.numel() * t.element_size()
    L.check(L.lib().mvlt_prefetch(arr, len(tensors), _stream()), "mvlt_prefetch")


def zero_batch(tensors):
    """Zero several small f32 tensors in one launch."""
    arr = (L.MvltZeroItem * len(tensors))()
    for i, t in enumerate(tensors):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
        arr[i].ptr, arr[i].n = t.data_ptr(), t.numel()
    L.check(L.lib().mvlt_zero_batch(arr, len(tensors), _stream()), "mvlt_zero_batch")


def colsum(x, out=None, accumulate=False):
    """out[n] = sum_m x[m,n] (f32) -- bias gradients."""
    _need_cuda(x)
    M, N = x.shape
    lib = L.lib()
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = workspace("colsum", lib.mvlt_colsum_workspace_rows(M) * N * 4, x.device)
    L.check(lib.mvlt_colsum(_dt(x), _p(x), x.stride(0), M, N, _p(out), int(accumulate), _p(ws), _stream()),
            "mvlt_colsum")
    return out


# ----------------------------------------------------------------------------- LayerNorm
def layernorm_fwd(x, gamma, beta, eps, *, rows=None, C_=None, out=None, out_rowmap=None, merge=None, gelu=False,
                  save_pre=False, save_stats=True, rows_dev=None):
    """x: [..., C] contiguous (or the un-merged [B,H*W,C/4] tensor when merge=(H,W))."""
    _need_cuda(x)
    assert x.is_contiguous() and gamma.dtype == torch.float32
    Cn = gamma.numel()
    if merge is None:
        nrows = x.numel() // Cn
        oshape = x.shape
    else:
        H, W = merge
        nrows = x.numel() // Cn
        oshape = (x.shape[0], (H // 2) * (W // 2), Cn)
    y = out if out is not None else torch.empty(oshape, dtype=x.dtype, device=x.device)
    p = L.MvltLayerNorm()
    p.dtype, p.rows, p.C, p.eps = _DT[x.dtype], nrows, Cn, eps
    p.x, p.gamma, p.beta, p.y = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr()
    mean = rstd = ypre = None
    if save_stats:
        mean, rstd = torch.empty((2, nrows), dtype=torch.float32, device=x.device).unbind(0)
        p.mean = pm = mean.data_ptr()
        p.rstd = pm + 4 * nrows
    if gelu:
        p.gelu = 1
        if save_pre:
            ypre = torch.empty_like(y)
            p.y_pre = _p(ypre)
    if out_rowmap is not None:
        assert out_rowmap.dtype == torch.int32 and out_rowmap.numel() == nrows
        p.out_rowmap = _p(out_rowmap)
    if merge is not None:
        p.merge_H, p.merge_W = merge
    if rows_dev is not None:
        p.rows_dev = rows_dev.data_ptr()
    L.check(L.lib().mvlt_layernorm_fwd(C.byref(p), _stream()), "mvlt_layernorm_fwd")
    return y, mean, rstd, ypre


def layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, *, dy_rowmap=None, y_pre=None, dres=None, merge=None,
                  accumulate=False, dx=None, branch=None, defer=None, rows_dev=None, dy_parts=False):
    """branch=dict(rowmap=, rowscale=(t, rps), dropout=(p, seed, tag)) also returns the branch gradient dz.
    defer=LnReduceQueue: the dgamma/dbeta partial rows are reduced later in one batched launch.
    dy_parts=True: dy is [parts, rows, C], 1 .. 4 partial tensors whose sum is the gradient (swin_wmsa2_bwd's dxn_parts)."""
    _need_cuda(dy, x)
    if accumulate and defer is not None:
        # the batched reduce writes dgamma / dbeta and has no accumulate form: the flag would be dropped silently
        raise ValueError("layernorm_bwd: accumulate=True cannot be combined with defer (the batched parameter reduce overwrites)")
    Cn = gamma.numel()
    nrows = mean.numel()
    if dx is None:
        dx = torch.empty_like(x)
    lib = L.lib()
    if defer is not None:
        ws = defer.take(2 * lib.mvlt_layernorm_bwd_workspace_rows() * Cn, x.device)
        defer.items.append((ws, lib.mvlt_layernorm_bwd_nparts(nrows, Cn), Cn, dgamma, dbeta))
        if defer not in LnReduceQueue._active:
            LnReduceQueue._active.append(defer)
    else:
        ws = workspace("ln_bwd", 2 * lib.mvlt_layernorm_bwd_workspace_rows() * Cn * 4, x.device)
    p = L.MvltLayerNormBwd()
    p.dtype, p.rows, p.C = _dt(x), nrows, Cn
    p.dy, p.x, p.mean, p.rstd, p.gamma = _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma)
    if dy_parts:
        assert dy.dim() == 3 and dy.is_contiguous() and dy.shape[1:] == (nrows, Cn)
        if dy.shape[0] > 1:
            p.dy_parts, p.dy_part_stride = dy.shape[0], dy.stride(0)
    if dy_rowmap is not None:
        p.dy_rowmap = _p(dy_rowmap)
    if y_pre is not None:
        p.y_pre, p.gelu = _p(y_pre), 1
    if dres is not None:
        p.dres = _p(dres)
    p.dx = _p(dx)
    if merge is not None:
        p.merge_H, p.merge_W = merge
    p.dgamma, p.dbeta, p.accumulate, p.workspace = _p(dgamma), _p(dbeta), int(accumulate), _p(ws)
    p.defer_param_reduce = int(defer is not None)
    if rows_dev is not None:
        p.rows_dev = rows_dev.data_ptr()
    dz = None
    if branch is not None:
        dz = torch.empty((nrows, Cn), dtype=x.dtype, device=x.device)
        p.dz = _p(dz)
        if branch.get("rowmap") is not None:
            p.dz_rowmap = _p(branch["rowmap"])
        if branch.get("rowscale") is not None:
            p.dz_rowscale, p.dz_rows_per_scale = _p(branch["rowscale"][0]), int(branch["rowscale"][1])
        if branch.get("dropout") is not None and branch["dropout"][0] > 0:
            p.dz_dropout_p, p.seed, p.tag = float(branch["dropout"][0]), int(branch["dropout"][1]), int(branch["dropout"][2])
    L.check(lib.mvlt_layernorm_bwd(C.byref(p), _stream()), "mvlt_layernorm_bwd")
    return dx if branch is None else (dx, dz)


class LnReduceQueue:
    """Partial dgamma/dbeta rows of every LayerNorm of one backward pass live in one pool and are
    reduced by ceil(n/96) launches at the end (instead of one launch per LayerNorm)."""
    _pool = {}
    _active = []          # queues with pending items (flushed early by the DDP bucket launcher)

    def __init__(self):
        self.items, self.off = [], 0

    @staticmethod
    def flush_all():
        """Write every pending dgamma/dbeta now: a gradient bucket is about to be communicated."""
        for q in list(LnReduceQueue._active):
            q.flush()
        if _host is not None and _host.lnq_pending():
            _host.lnq_flush(stream_int())

    def take(self, nfloats, device):
        pool = LnReduceQueue._pool.get(device.index)
        need = self.off + nfloats
        if pool is None or pool.numel() < need:
            newp = torch.empty(max(need, 48 << 20), dtype=torch.float32, device=device)
            if pool is not None:            # keep earlier slices valid: they are still referenced by self.items
                self._keep = getattr(self, "_keep", []) + [pool]
                self.off = 0
            LnReduceQueue._pool[device.index] = pool = newp
        ws = pool[self.off:self.off + nfloats]
        self.off += nfloats
        return ws

    def flush(self):
        if self in LnReduceQueue._active:
            LnReduceQueue._active.remove(self)
        if not self.items:
            return
        arr = (L.MvltLnReduceItem * len(self.items))()
        for i, (ws, nparts, Cn, dg, db) in enumerate(self.items):
            arr[i].workspace, arr[i].nparts, arr[i].C, arr[i].dgamma, arr[i].dbeta = ws.data_ptr(), nparts, Cn, dg.data_ptr(), db.data_ptr()
        L.check(L.lib().mvlt_layernorm_param_reduce_batch(arr, len(self.items), _stream()), "mvlt_layernorm_param_reduce_batch")
        self.items, self.off = [], 0


# ----------------------------------------------------------------------------- attention
def _attn_struct(qkv, out, lse, mode, nseq, Lq, nH, hd, scale, *, bias_table=None, nW=0, win_res=0, shift=0,
                 text_ids=None, image_mask=None, obj_end=0, dropout=None, pack=None):
    p = L.MvltAttn()
    if pack is not None:          # (row_start int32 [nseq], seq_len int32 [nseq], total rows): packed activations
        assert pack[0].dtype == torch.int32 and pack[1].dtype == torch.int32 and pack[0].numel() == nseq
        p.row_start, p.seq_len = _p(pack[0]), _p(pack[1])
    p.dtype, p.mode, p.nseq, p.L, p.nH, p.hd = _dt(qkv), mode, nseq, Lq, nH, hd
    p.qkv, p.out, p.lse, p.scale = _p(qkv), _p(out), _p(lse), float(scale)
    if bias_table is not None:
        assert bias_table.dtype == torch.float32
        p.bias_table, p.nW, p.win_res, p.shift = _p(bias_table), nW, win_res, shift
    if text_ids is not None:
        assert text_ids.dtype == torch.int64 and text_ids.is_contiguous()
        p.text_ids, p.T = _p(text_ids), text_ids.shape[1]
    if image_mask is not None:
        p.image_mask = _p(image_mask)
    p.obj_end = obj_end
    if dropout is not None and dropout[0] > 0.0:
        p.dropout_p, p.seed, p.tag = float(dropout[0]), int(dropout[1]), int(dropout[2])
    return p


def attn_fwd(qkv, mode, nseq, Lq, nH, hd, scale, out=None, lse=None, **kw):
    """qkv: [nseq*L, 3*nH*hd] -> (out [nseq*L, nH*hd], lse [nseq,nH,L]); with pack= the rows are packed
    ([R, ...], sequence s at rows row_start[s] .. +seq_len[s]).  out / lse: optional caller buffers."""
    _need_cuda(qkv)
    rows = nseq * Lq if kw.get("pack") is None else kw["pack"][2]
    assert qkv.is_contiguous() and qkv.shape == (rows, 3 * nH * hd)
    if out is None:
        out = torch.empty((rows, nH * hd), dtype=qkv.dtype, device=qkv.device)
    if lse is None:
        lse = torch.empty((nseq, nH, Lq), dtype=torch.float32, device=qkv.device)
    assert out.is_contiguous() and out.dtype == qkv.dtype and out.shape == (rows, nH * hd)
    assert lse.is_contiguous() and lse.dtype == torch.float32 and lse.shape == (nseq, nH, Lq)
    p = _attn_struct(qkv, out, lse, mode, nseq, Lq, nH, hd, scale, **kw)
    L.check(L.lib().mvlt_attn_fwd(C.byref(p), _stream()), "mvlt_attn_fwd")
    return out, lse


def attn_probs(qkv, lse, mode, nseq, Lq, nH, hd, scale, q_range, k_range, head_mean=False, renorm=False, out=None, **kw):
    """Attention maps (mvlt_attn_probs): f32 [nseq, nH or 1, nq, nk], exp(scale q.k + mask - lse) for the queries
    q_range = (q0, nq) and the keys k_range = (k0, nk) of every sequence, from the qkv / lse of an eval-mode attn_fwd call with
    the same mode and keywords (text_ids, image_mask, obj_end, pack).  head_mean: the mean over heads; renorm: every output row
    divided by its sum over the selected keys.  out: optional caller buffer (one allocation can hold every layer)."""
    _need_cuda(qkv, lse)
    rows = nseq * Lq if kw.get("pack") is None else kw["pack"][2]
    assert qkv.is_contiguous() and qkv.shape == (rows, 3 * nH * hd)
    assert lse.is_contiguous() and lse.dtype == torch.float32 and lse.shape == (nseq, nH, Lq)
    (q0, nq), (k0, nk) = (int(v) for v in q_range), (int(v) for v in k_range)
    shape = (nseq, 1 if head_mean else nH, nq, nk)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=qkv.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.shape == shape
    p = _attn_struct(qkv, None, lse, mode, nseq, Lq, nH, hd, scale, **kw)
    flags = (L.ATTNMAP_HEAD_MEAN if head_mean else 0) | (L.ATTNMAP_RENORM if renorm else 0)
    L.check(L.lib().mvlt_attn_probs(C.byref(p), q0, nq, k0, nk, flags, _p(out), _stream()), "mvlt_attn_probs")
    return out


def swin_bwd_proj_supported(dtype, nseq, nH, hd, shift):
    """MvltAttn.dout_weight (the output projection's dgrad inside the Swin attention backward): what the dispatch itself answers."""
    return bool(L.lib().mvlt_swin_bwd_proj_supported(_DT[dtype], nseq, nH, hd, shift))


def _attn_bwd_struct(dout, qkv, out, lse, mode, nseq, Lq, nH, hd, scale, dbias_table, dout_weight, dqkv, delta_ws, kw):
    p = _attn_struct(qkv, out, lse, mode, nseq, Lq, nH, hd, scale, **kw)
    p.dout, p.dqkv = _p(dout), _p(dqkv)
    if dout_weight is not None:
        assert mode == L.ATTN_SWIN and dout_weight.dtype == qkv.dtype and dout_weight.is_contiguous() and dout_weight.shape == (nH * hd, nH * hd)
        p.dout_weight = _p(dout_weight)
    if mode != L.ATTN_SWIN and delta_ws:
        delta = torch.empty_like(lse)          # delta_q hand-over between the two backward launches
        p.delta_ws = _p(delta)
    if dbias_table is not None:
        assert dbias_table.dtype == torch.float32
        p.dbias_table = _p(dbias_table)
    return p


def attn_route(qkv, mode, nseq, Lq, nH, hd, scale, bwd=False, dout_weight=None, delta_ws=True, **kw):
    """The kernel mvlt_attn_fwd / mvlt_attn_bwd would launch for these arguments (a name of _lib.ATTN_ROUTES), nothing
    launched.  Same keywords as attn_fwd / attn_bwd."""
    rows = qkv.shape[0]
    out = torch.empty((rows, nH * hd), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((nseq, nH, Lq), dtype=torch.float32, device=qkv.device)
    if bwd:
        p = _attn_bwd_struct(out, qkv, out, lse, mode, nseq, Lq, nH, hd, scale, None, dout_weight, qkv, delta_ws, kw)
    else:
        p = _attn_struct(qkv, out, lse, mode, nseq, Lq, nH, hd, scale, **kw)
    r = L.lib().mvlt_attn_route(C.byref(p), int(bool(bwd)))
    L.check(min(r, 0), "mvlt_attn_route")
    return L.ATTN_ROUTES[r]


def attn_bwd(dout, qkv, out, lse, mode, nseq, Lq, nH, hd, scale, dbias_table=None, event=None, dout_weight=None,
             dqkv=None, delta_ws=True, **kw):
    """event: a hipEvent_t handle (int) that completes with the call's last kernel (mvlt_attn_bwd_ev: the fork of the
    weight-gradient stream without a marker packet on this stream).  dout_weight (Swin only): `dout` is the gradient of the output
    projection's OUTPUT and the kernel applies proj.weight's transpose per head itself (MvltAttn.dout_weight).
    dqkv: optional caller buffer.  delta_ws=False (MVLBert modes): no delta_q workspace, which leaves the two-launch
    backward out and takes the generic one (MVLT_ERR_UNSUPPORTED where that does not apply)."""
    _need_cuda(qkv, dout)
    assert dout.is_contiguous() and dout.shape == out.shape
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    assert dqkv.is_contiguous() and dqkv.dtype == qkv.dtype and dqkv.shape == qkv.shape
    p = _attn_bwd_struct(dout, qkv, out, lse, mode, nseq, Lq, nH, hd, scale, dbias_table, dout_weight, dqkv, delta_ws, kw)
    if event is not None:
        L.check(L.lib().mvlt_attn_bwd_ev(C.byref(p), _stream(), C.c_void_p(event)), "mvlt_attn_bwd_ev")
    else:
        L.check(L.lib().mvlt_attn_bwd(C.byref(p), _stream()), "mvlt_attn_bwd")
    return dqkv


# ----------------------------------------------------------------------------- fused Swin W-MSA
def swin_wmsa_supported(dtype, C_, nH):
    return bool(L.lib().mvlt_swin_wmsa_supported(_DT[dtype], C_, nH))


def _wmsa_struct(x, w2n, B, res, nH, shift, gamma, beta, eps, wqkv, bqkv, wproj, bproj, table, scale, rowscale):
    Cn = x.shape[1]
    assert x.is_contiguous() and x.shape[0] == B * res * res and w2n.dtype == torch.int32 and w2n.numel() == x.shape[0]
    assert wqkv.dtype == x.dtype and wproj.dtype == x.dtype and wqkv.shape == (3 * Cn, Cn) and wproj.shape == (Cn, Cn)
    assert wqkv.is_contiguous() and wproj.is_contiguous() and table.dtype == torch.float32 and table.shape == (169, nH)
    p = L.MvltSwinWmsa()
    p.dtype, p.B, p.res, p.C, p.nH, p.shift = _DT[x.dtype], B, res, Cn, nH, shift
    p.x, p.w2n = x.data_ptr(), w2n.data_ptr()
    p.ln_gamma, p.ln_beta, p.ln_eps = gamma.data_ptr(), beta.data_ptr(), eps
    p.wqkv, p.bqkv, p.wproj, p.bproj = wqkv.data_ptr(), bqkv.data_ptr(), wproj.data_ptr(), bproj.data_ptr()
    p.bias_table, p.scale = table.data_ptr(), float(scale)
    if rowscale is not None:
        assert rowscale.dtype == torch.float32 and rowscale.numel() == B and rowscale.is_contiguous()
        p.rowscale = rowscale.data_ptr()
    return p


def swin_wmsa_fwd(x, w2n, B, res, nH, shift, gamma, beta, eps, wqkv, bqkv, wproj, bproj, table, scale,
                  rowscale=None, save=False, head_split=False):
    """y = x + rowscale * proj(window_attention(qkv(norm1(x))))  (MvltSwinWmsa): one launch.
    save=True also returns (xn_win, qkv_win, attn_out, lse, mean, rstd) for the backward pass.
    head_split=True: one workgroup per (window, head group), no output projection: returns (attn_out, saved)."""
    _need_cuda(x)
    p = _wmsa_struct(x, w2n, B, res, nH, shift, gamma, beta, eps, wqkv, bqkv, wproj, bproj, table, scale, rowscale)
    if head_split:
        p.head_split = 1
        ao = torch.empty_like(x)
        p.attn_out = ao.data_ptr()
        saved = None
        if save:
            rows, Cn = x.shape
            xn = torch.empty_like(x)
            qkv = torch.empty((rows, 3 * Cn), dtype=x.dtype, device=x.device)
            lse = torch.empty((rows // 49, nH, 49), dtype=torch.float32, device=x.device)
            mean, rstd = torch.empty((2, rows), dtype=torch.float32, device=x.device).unbind(0)
            p.xn_win, p.lse, p.mean, p.rstd, p.qkv_win = xn.data_ptr(), lse.data_ptr(), mean.data_ptr(), rstd.data_ptr(), qkv.data_ptr()
            saved = (xn, qkv, ao, lse, mean, rstd)
        L.check(L.lib().mvlt_swin_wmsa_fwd(C.byref(p), _stream()), "mvlt_swin_wmsa_fwd")
        return ao, saved
    y = torch.empty_like(x)
    p.y = y.data_ptr()
    saved = None
    if save:
        rows, Cn = x.shape
        xn, ao = torch.empty_like(x), torch.empty_like(x)
        qkv = torch.empty((rows, 3 * Cn), dtype=x.dtype, device=x.device)
        lse = torch.empty((rows // 49, nH, 49), dtype=torch.float32, device=x.device)
        mean, rstd = torch.empty((2, rows), dtype=torch.float32, device=x.device).unbind(0)
        p.xn_win, p.attn_out, p.lse, p.mean, p.rstd = xn.data_ptr(), ao.data_ptr(), lse.data_ptr(), mean.data_ptr(), rstd.data_ptr()
        p.qkv_win = qkv.data_ptr()
        saved = (xn, qkv, ao, lse, mean, rstd)
    L.check(L.lib().mvlt_swin_wmsa_fwd(C.byref(p), _stream()), "mvlt_swin_wmsa_fwd")
    return y, saved


def swin_wmsa2_supported(dtype, B, res, C_, nH):
    return bool(L.lib().mvlt_swin_wmsa2_supported(_DT[dtype], B, res, C_, nH))


_WMSA2_SYNC = {}          # (device, stream) -> int32 hand-off workspace
_WMSA2_PINNED = {}        # key -> (pinned int32 [1], event): asynchronous copies of the error count


def wmsa2_sync_ws(device, words):
    """The int32 hand-off workspace of mvlt_swin_wmsa2_fwd for the CURRENT stream of `device`: zeroed once here, every
    launch leaves its counters zeroed; word 0 is the sticky error count (include/mvlt_hip.h).  One workspace per (device,
    stream): launches of one stream are serialised, launches of different streams never share counters."""
    st = _stream_cache[0]          # (pinned by the engines for the duration of a pass: torch.cuda.current_stream costs ~5 us)
    if _stream_cache[1] == "graph":
        # ONE workspace for every captured inference graph of the device (replays are serialised on the caller's stream): it is
        # allocated and zeroed by the eager warm-up run that precedes a capture (runtime.GraphedEval._capture), so no memset is
        # ever captured -- a replay must not clear the sticky error count -- and it is never reallocated under a graph that has
        # its address baked in (a larger one is a NEW buffer; the old one is kept alive)
        key = (torch.device(device), "graph")
    else:
        key = (torch.device(device), (st.value or 0) if st is not None else torch.cuda.current_stream(device).cuda_stream)
    ws = _WMSA2_SYNC.get(key)
    if ws is None or ws.numel() < words:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("mvlt_amd: the W-MSA hand-off workspace must exist before a HIP-graph capture (run the call once "
                               "eagerly under ops.on_stream(stream, 'graph') first, as runtime.GraphedEval does)")
        if ws is not None and key[1] == "graph":
            _ws_graph_keep.append(ws)
        ws = torch.zeros(max(words, 4096), dtype=torch.int32, device=device)
        _WMSA2_SYNC[key] = ws
    return ws


class DeviceHandoffError(RuntimeError):
    """A bounded in-launch wait of mvlt_swin_wmsa2_fwd ran out: the head groups of a window pair were not co-resident
    (something else held the CUs / the LDS).  The affected rows of the block output are NaN."""


def _wmsa2_raise(n):
    raise DeviceHandoffError(
        f"mvlt_swin_wmsa2_fwd: {n} hand-off wait(s) between head-group workgroups ran out (the groups of a window pair were "
        "not resident together -- another kernel or process was holding CUs / LDS).  The affected rows of the block output "
        "were written as NaN.  A training step that ran on them has applied NaN gradients (reload the last checkpoint) unless its "
        "optimizer was built with skip_nonfinite=True, which refused that step: training can then continue.  "
        "Set MVLT_WMSA2=0 to use the kernels without an in-launch hand-off.")


def wmsa2_sync_errors():
    """Sum of the sticky error counts of all hand-off workspaces (0 = no bounded wait ever ran out).  Forces a device sync."""
    return sum(int(ws[0].item()) for ws in _WMSA2_SYNC.values())


def wmsa2_check(sync=True):
    """Raise DeviceHandoffError if a hand-off wait ran out.  sync=True reads the error counts now (a device sync: use it
    where the caller synchronises anyway -- loss.item(), save_pretrained).  sync=False costs no sync: it looks at the copies
    queued by the PREVIOUS call (pinned host memory, ready when their event has completed) and queues fresh ones behind
    the work issued so far, so a failure surfaces one call late."""
    if sync:
        n = wmsa2_sync_errors()
        if n:
            _wmsa2_raise(n)
        return
    for key, ws in _WMSA2_SYNC.items():
        slot = _WMSA2_PINNED.get(key)
        if slot is None:
            slot = _WMSA2_PINNED[key] = [torch.zeros(1, dtype=torch.int32).pin_memory(), None]
        host, ev = slot
        if ev is not None and ev.query() and int(host[0]):
            _wmsa2_raise(int(host[0]))
        if ev is None or ev.query():          # (never rewrite the pinned word while a copy into it is in flight)
            host.copy_(ws[:1], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(key[0]))
            slot[1] = ev


def wmsa2_error_tensor(device):
    """f32 [1] on `device`: the sum of the sticky error counts of its hand-off workspaces (no sync), or None if the fused W-MSA
    kernel has not run there.  ddp.GradReducer sends it along with the label count so that EVERY rank learns of a time-out."""
    dev = torch.device(device)
    ws = [w for k, w in _WMSA2_SYNC.items() if k[0] == dev]
    if not ws:
        return None
    return torch.stack([w[0] for w in ws]).sum().to(torch.float32).reshape(1)


def wmsa2_clear_errors():
    """Zero the error counts and the counters (after a reported failure; the caller has synchronised)."""
    torch.cuda.synchronize()
    for ws in _WMSA2_SYNC.values():
        ws.zero_()
    for slot in _WMSA2_PINNED.values():
        slot[0].zero_()
        slot[1] = None


def wmsa2_set_timeout_ms(ms):
    L.check(L.lib().mvlt_swin_wmsa2_set_timeout_ms(int(ms)), "mvlt_swin_wmsa2_set_timeout_ms")


def debug_stream_copy(dst, src, blocks=32, inflight=2, stream=None):
    """Diagnostic: copy src -> dst (same byte count, may alias) with the launch geometry of a ring collective's kernel."""
    _need_cuda(dst, src)
    nbytes = src.numel() * src.element_size()
    assert dst.numel() * dst.element_size() == nbytes and nbytes % 16 == 0
    st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    L.check(L.lib().mvlt_debug_stream_copy(_p(dst), _p(src), nbytes, int(blocks), int(inflight), st), "mvlt_debug_stream_copy")


def debug_hold_cus(blocks, lds_bytes, usec, stream=None):
    """Diagnostic: occupy CUs with spinning workgroups on `stream` (default: the current one)."""
    st = stream.cuda_stream if stream is not None else _stream()
    L.check(L.lib().mvlt_debug_hold_cus(int(blocks), int(lds_bytes), int(usec), st), "mvlt_debug_hold_cus")


def swin_wmsa2_fwd(x, w2n, B, res, nH, shift, gamma, beta, eps, wqkv, bqkv, wproj, bproj, table, scale,
                   rowscale=None, save=False):
    """Second design of the fused forward (csrc/wmsa2.hip): same result as swin_wmsa_fwd, two windows per workgroup,
    head groups across workgroups.  save=True also returns (xn_win, qkv_win, attn_out, lse, mean, rstd)."""
    _need_cuda(x)
    p = _wmsa_struct(x, w2n, B, res, nH, shift, gamma, beta, eps, wqkv, bqkv, wproj, bproj, table, scale, rowscale)
    y = torch.empty_like(x)
    ao = torch.empty_like(x)
    p.y, p.attn_out = y.data_ptr(), ao.data_ptr()
    saved = None
    if save:
        rows, Cn = x.shape
        xn = torch.empty_like(x)
        qkv = torch.empty((rows, 3 * Cn), dtype=x.dtype, device=x.device)
        lse = torch.empty((rows // 49, nH, 49), dtype=torch.float32, device=x.device)
        mean, rstd = torch.empty((2, rows), dtype=torch.float32, device=x.device).unbind(0)
        p.xn_win, p.lse, p.mean, p.rstd, p.qkv_win = xn.data_ptr(), lse.data_ptr(), mean.data_ptr(), rstd.data_ptr(), qkv.data_ptr()
        saved = (xn, qkv, ao, lse, mean, rstd)
    ws = wmsa2_sync_ws(x.device, L.lib().mvlt_swin_wmsa2_sync_words(B, res))
    L.check(L.lib().mvlt_swin_wmsa2_fwd(C.byref(p), ws.data_ptr(), _stream()), "mvlt_swin_wmsa2_fwd")
    return y, saved


def swin_wmsa2_bwd_parts(dtype, B, res, C_, nH):
    """Number of partial dXn tensors the one-launch backward of the second design writes (nH / 3); 0 = shape not covered."""
    return int(L.lib().mvlt_swin_wmsa2_bwd_parts(_DT[dtype], B, res, C_, nH))


def swin_dbias_reduce(items):
    """items: [(ws f32 [nwg, 3 * 169], nH, dtable f32 [169, nH])]: the per-workgroup sums of mvlt_swin_wmsa2_bwd launches added
    into their tables, one launch for all of them (mvlt_swin_wmsa2_bwd_dbias)."""
    arr = (L.MvltSwinDbiasItem * len(items))()
    for i, (ws, nH, dtable) in enumerate(items):
        assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.shape[1] == 507 and dtable.dtype == torch.float32 and dtable.shape == (169, nH)
        arr[i].ws, arr[i].nwg, arr[i].nH, arr[i].dbias_table = ws.data_ptr(), ws.shape[0], nH, dtable.data_ptr()
    L.check(L.lib().mvlt_swin_wmsa2_bwd_dbias(arr, len(items), _stream()), "mvlt_swin_wmsa2_bwd_dbias")


def swin_wmsa2_bwd(dy_win, qkv_win, lse, B, res, nH, shift, wproj, wqkv, table, scale, dtable, event=None, dbias_defer=None):
    """Output-projection dgrad + window-attention backward + qkv dgrad in one launch, second design (mvlt_swin_wmsa2_bwd).
    dy_win [rows, C] window order (DropPath scale applied); wproj [C, C], wqkv [3C, C] as stored (compute dtype).
    Returns (dqkv [rows, 3C], dxn_parts [nH / 3, rows, C]): the qkv dgrad is the SUM of the parts (layernorm_bwd adds them
    while it loads: dy_parts); dtable (f32 [169, nH]) is accumulated -- by a second small launch here, or later together with
    other blocks' when dbias_defer (a list) is given: it receives (ws, nH, dtable) for swin_dbias_reduce."""
    _need_cuda(dy_win)
    rows, Cn = dy_win.shape
    nparts = swin_wmsa2_bwd_parts(dy_win.dtype, B, res, Cn, nH)
    assert nparts > 0, "mvlt_swin_wmsa2_bwd: shape not covered"
    assert dy_win.is_contiguous() and qkv_win.is_contiguous() and qkv_win.shape == (rows, 3 * Cn) and rows == B * res * res
    assert wproj.is_contiguous() and wproj.shape == (Cn, Cn) and wqkv.is_contiguous() and wqkv.shape == (3 * Cn, Cn)
    assert wproj.dtype == dy_win.dtype and wqkv.dtype == dy_win.dtype
    assert lse.dtype == torch.float32 and table.dtype == torch.float32 and dtable.dtype == torch.float32
    p = L.MvltSwinWmsa()
    p.dtype, p.B, p.res, p.C, p.nH, p.shift = _DT[dy_win.dtype], B, res, Cn, nH, shift
    p.dy_win, p.qkv_win, p.lse = dy_win.data_ptr(), qkv_win.data_ptr(), lse.data_ptr()
    p.wproj, p.wqkv, p.bias_table, p.scale = wproj.data_ptr(), wqkv.data_ptr(), table.data_ptr(), float(scale)
    dqkv = torch.empty_like(qkv_win)
    dxn = torch.empty((nparts, rows, Cn), dtype=dy_win.dtype, device=dy_win.device)
    p.dqkv, p.dxn_win = dqkv.data_ptr(), dxn.data_ptr()
    ws = None
    if dtable is not None:
        nwg = int(L.lib().mvlt_swin_wmsa2_bwd_workgroups(p.dtype, B, res, Cn, nH))
        ws = torch.empty((nwg, 507), dtype=torch.float32, device=dy_win.device)
        p.dbias_ws = ws.data_ptr()
    if event is not None:
        L.check(L.lib().mvlt_swin_wmsa2_bwd_ev(C.byref(p), _stream(), C.c_void_p(event)), "mvlt_swin_wmsa2_bwd_ev")
    else:
        L.check(L.lib().mvlt_swin_wmsa2_bwd(C.byref(p), _stream()), "mvlt_swin_wmsa2_bwd")
    if ws is not None:
        if dbias_defer is not None:
            dbias_defer.append((ws, nH, dtable))
        else:
            swin_dbias_reduce([(ws, nH, dtable)])
    return dqkv, dxn


# ----------------------------------------------------------------------------- data movement
def im2col_patch(img, dtype, patch):
    _need_cuda(img)
    assert img.dtype == torch.float32 and img.is_contiguous() and img.dim() == 4 and img.shape[2] == img.shape[3]
    B, Cin, S, _ = img.shape
    G = S // patch
    cols = torch.empty((B * G * G, Cin * patch * patch), dtype=dtype, device=img.device)
    L.check(L.lib().mvlt_im2col_patch(_DT[dtype], _p(img), _p(cols), B, Cin, S, patch, _stream()), "mvlt_im2col_patch")
    return cols


def pack_plan(text_ids, labels, n_img):
    """Packing plan of a ragged caption batch, computed on the device (mvlt_pack_plan, no host sync).
    -> (row_start i32 [B], seq_len i32 [B], total i32 [1], row_start i64 [B], text_row i64 [B*T])"""
    _need_cuda(text_ids)
    assert text_ids.dtype == torch.int64 and text_ids.is_contiguous() and text_ids.dim() == 2
    B, T = text_ids.shape
    if labels is not None:
        assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == B * T
    dev = text_ids.device
    i32buf = torch.empty(2 * B + 1, dtype=torch.int32, device=dev)
    i64buf = torch.empty(B + B * T, dtype=torch.int64, device=dev)
    rs, sl, tot = i32buf[:B], i32buf[B:2 * B], i32buf[2 * B:]
    rs64, trow = i64buf[:B], i64buf[B:]
    L.check(L.lib().mvlt_pack_plan(_p(text_ids), _p(labels), B, T, n_img, _p(rs), _p(sl), _p(tot), _p(rs64), _p(trow),
                                   _stream()), "mvlt_pack_plan")
    return rs, sl, tot, rs64, trow


def label_plan(labels, text_row):
    """Labelled caption positions first (mvlt_label_plan) -> (gather_row i32 [N], sel_labels i64 [N], count i32 [1])."""
    _need_cuda(labels)
    assert labels.dtype == torch.int64 and labels.is_contiguous()
    N = labels.numel()
    dev = labels.device
    gr = torch.empty(N + 1, dtype=torch.int32, device=dev)
    sel = torch.empty(N, dtype=torch.int64, device=dev)
    L.check(L.lib().mvlt_label_plan(_p(labels), _p(text_row), N, _p(gr), _p(sel), C.c_void_p(gr.data_ptr() + 4 * N), _stream()),
            "mvlt_label_plan")
    return gr[:N], sel, gr[N:]


def rows_scatter(x, rowmap, count, out):
    """out[rowmap[i]] = x[i] for i < count (device scalar)."""
    L.check(L.lib().mvlt_rows_scatter(_dt(x), _p(x), _p(out), x.shape[0], x.shape[1], _p(rowmap), _p(count), _stream()),
            "mvlt_rows_scatter")
    return out


def _embed_struct(dtype, B, n_img, T, H, text_ids, word, pos, typ, cls_id, sep_id, pos_offset, type_override):
    p = L.MvltEmbed()
    p.dtype, p.B, p.n_img, p.T, p.H = _DT[dtype], B, n_img, T, H
    if text_ids is not None:
        assert text_ids.dtype == torch.int64 and text_ids.is_contiguous()
        p.text_ids = _p(text_ids)
    p.word_emb, p.pos_emb, p.type_emb = _p(word), _p(pos), _p(typ)
    if torch.is_tensor(pos_offset):          # position kept on the device (replayed decode step)
        assert pos_offset.dtype == torch.int32 and pos_offset.is_cuda
        p.pos_offset, p.pos_offset_dev = 0, _p(pos_offset)
    else:
        p.pos_offset = pos_offset
    p.cls_id, p.sep_id, p.type_override = cls_id, sep_id, type_override
    return p


def embed_fwd(text_ids, image_feature, word, pos, typ, cls_id, sep_id, *, dtype=None, pos_offset=0,
              type_override=-1, pack=None, out=None, row_shift=None):
    """MVLBert.get_embedding sum.  image_feature None -> cached-step (text only) layout.
    ``row_shift`` (int32 [B], device; None: the entry point without it): the position of batch row b is shifted by row_shift[b]
    and clamped into the position table (mvlt_embed_fwd_rows)."""
    if image_feature is not None:
        B, n_img, H = image_feature.shape
        dtype = image_feature.dtype
        assert image_feature.is_contiguous()
    else:
        B, n_img, H = text_ids.shape[0], -1, word.shape[1]
    T = 0 if text_ids is None else text_ids.shape[1]
    Lq = T if n_img < 0 else n_img + 2 + T
    if out is None:
        out = torch.empty((B, Lq, H) if pack is None else (pack[2], H), dtype=dtype, device=word.device)
    p = _embed_struct(dtype, B, n_img, T, H, text_ids, word, pos, typ, cls_id, sep_id, pos_offset, type_override)
    p.image_feature, p.out = _p(image_feature), _p(out)
    if pack is not None:
        p.row_start, p.seq_len = _p(pack[0]), _p(pack[1])
    if row_shift is not None:
        assert row_shift.dtype == torch.int32 and row_shift.is_cuda and row_shift.is_contiguous() and row_shift.numel() == B
        p.pos_rows = pos.shape[0]
        L.check(L.lib().mvlt_embed_fwd_rows(C.byref(p), _p(row_shift), _stream()), "mvlt_embed_fwd_rows")
        return out
    L.check(L.lib().mvlt_embed_fwd(C.byref(p), _stream()), "mvlt_embed_fwd")
    return out


def embed_bwd(dout, text_ids, n_img, word, pos, typ, cls_id, sep_id, dword, dpos, dtype_emb, *, want_dimage=True,
              pos_offset=0, type_override=-1, pack=None, B=None):
    if pack is None:
        B, Lq, H = dout.shape
    else:
        H = dout.shape[1]            # dout: packed [R, H]; B given by the caller
    T = 0 if text_ids is None else text_ids.shape[1]
    dimg = torch.empty((B, n_img, H), dtype=dout.dtype, device=dout.device) if (want_dimage and n_img > 0) else None
    p = _embed_struct(dout.dtype, B, n_img, T, H, text_ids, word, pos, typ, cls_id, sep_id, pos_offset, type_override)
    assert dout.is_contiguous()
    p.dout, p.dimage, p.dword, p.dpos, p.dtype_emb = _p(dout), _p(dimg), _p(dword), _p(dpos), _p(dtype_emb)
    # the position / type table gradients are OVERWRITTEN with ordered batch sums and their unused rows zeroed (no atomics);
    # dword is accumulated: the caller clears it
    p.pos_rows = 0 if dpos is None else dpos.shape[0]
    p.type_rows = 0 if dtype_emb is None else dtype_emb.shape[0]
    if pack is not None:
        p.row_start, p.seq_len = _p(pack[0]), _p(pack[1])
    L.check(L.lib().mvlt_embed_bwd(C.byref(p), _stream()), "mvlt_embed_bwd")
    return dimg


def rows_transform(x, *, rowmap=None, rowscale=None, dropout=None, out=None):
    """out[i] = scale * mask(x[rowmap[i]]) (DropPath / dropout backward, window gathers)."""
    _need_cuda(x)
    assert x.is_contiguous() and x.dim() == 2
    rows = x.shape[0] if rowmap is None else rowmap.numel()
    if out is None:
        out = torch.empty((rows, x.shape[1]), dtype=x.dtype, device=x.device)
    dp, seed, tag = (dropout if dropout is not None else (0.0, 0, 0))
    rs, rps = (rowscale if rowscale is not None else (None, 1))
    L.check(L.lib().mvlt_rows_transform(_dt(x), _p(x), _p(out), rows, x.shape[1], _p(rowmap), _p(rs), rps,
                                        float(dp), int(seed), int(tag), _stream()), "mvlt_rows_transform")
    return out


def cast(x, dtype, out=None):
    _need_cuda(x)
    assert x.is_contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=dtype, device=x.device)
    L.check(L.lib().mvlt_cast(_dt(x), _p(x), _DT[dtype], _p(out), x.numel(), _stream()), "mvlt_cast")
    return out


def gelu(x):
    y = torch.empty_like(x)
    L.check(L.lib().mvlt_gelu_fwd(_dt(x), _p(x), _p(y), x.numel(), _stream()), "mvlt_gelu_fwd")
    return y


def tanh_fwd(x):
    y = torch.empty_like(x)
    L.check(L.lib().mvlt_tanh_fwd(_dt(x), _p(x), _p(y), x.numel(), _stream()), "mvlt_tanh_fwd")
    return y


def tanh_bwd(y, dy):
    dx = torch.empty_like(y)
    L.check(L.lib().mvlt_tanh_bwd(_dt(y), _p(y), _p(dy), _p(dx), y.numel(), _stream()), "mvlt_tanh_bwd")
    return dx


def dropout_mask(n, p, seed, tag, device):
    keep = torch.empty(n, dtype=torch.uint8, device=device)
    L.check(L.lib().mvlt_dropout_mask(_p(keep), n, float(p), int(seed), int(tag), _stream()), "mvlt_dropout_mask")
    return keep


def droppath_scale(B, p, seed, tag, device):
    s = torch.empty(B, dtype=torch.float32, device=device)
    L.check(L.lib().mvlt_droppath_scale(_p(s), B, float(p), int(seed), int(tag), _stream()), "mvlt_droppath_scale")
    return s


def droppath_scales(probs, B, seed, tag=0):
    """probs: f32 [rows] on the device -> [rows, B] scales (1/(1-p) kept, 0 dropped), one launch for a whole forward pass."""
    _need_cuda(probs)
    assert probs.dtype == torch.float32 and probs.is_contiguous()
    s = torch.empty((probs.numel(), B), dtype=torch.float32, device=probs.device)
    L.check(L.lib().mvlt_droppath_scales(_p(s), _p(probs), probs.numel(), B, int(seed), int(tag), _stream()), "mvlt_droppath_scales")
    return s


def droppath_plan(scales, row0, row_step, lt, B, ld):
    """Row plans (mvlt_droppath_plan) of the len(lt) blocks whose DropPath scales are rows row0, row0 + row_step, ... of `scales`
    ([*, B] f32); lt: int32 [nblk] on the device, tokens per sample (0: no plan).  -> perm, inv int32 [nblk, ld], count int32
    [nblk].  One launch, nothing read back; rows of perm / inv beyond B * lt[i] and the rows of skipped blocks stay unwritten."""
    _need_cuda(scales)
    assert scales.dtype == torch.float32 and scales.is_contiguous() and lt.dtype == torch.int32 and lt.is_contiguous()
    n = lt.numel()
    assert scales.numel() >= (row0 + (n - 1) * row_step + 1) * B
    buf = torch.empty(n * (2 * ld + 1), dtype=torch.int32, device=scales.device)
    perm, inv, count = buf[:n * ld].view(n, ld), buf[n * ld:2 * n * ld].view(n, ld), buf[2 * n * ld:]
    L.check(L.lib().mvlt_droppath_plan(_p(scales), int(row0), int(row_step), _p(lt), n, B, ld, _p(perm), _p(inv), _p(count), _stream()),
            "mvlt_droppath_plan")
    return perm, inv, count


# ----------------------------------------------------------------------------- loss / optimizer / decode
def ce_fwd(logits, V, labels, rows_dev=None):
    """logits [rows, ld>=V]; returns (loss_sum, count, lse) device tensors (mean = sum/count).
    rows_dev (int32 device scalar): only the first *rows_dev rows exist."""
    _need_cuda(logits)
    rows = logits.shape[0]
    assert labels.dtype == torch.int64 and labels.numel() == rows and labels.is_contiguous()
    acc = torch.zeros(2, dtype=torch.float32, device=logits.device)
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    L.check(L.lib().mvlt_ce_fwd_ragged(_dt(logits), _p(logits), logits.stride(0), rows, V, _p(labels), _p(lse),
                                       C.c_void_p(acc.data_ptr()), C.c_void_p(acc.data_ptr() + 4), _p(rows_dev), _stream()),
            "mvlt_ce_fwd")
    return acc, lse


def ce_bwd(logits, V, labels, lse, acc, grad_scale=1.0, out=None, grad_scale_dev=None, rows_dev=None):
    if out is None:
        out = logits
    if grad_scale_dev is not None:
        assert grad_scale_dev.dtype == torch.float32 and grad_scale_dev.numel() == 1
    L.check(L.lib().mvlt_ce_bwd_ragged(_dt(logits), _p(logits), logits.stride(0), logits.shape[0], V, _p(labels), _p(lse),
                                       C.c_void_p(acc.data_ptr() + 4), float(grad_scale), _p(grad_scale_dev), _p(out),
                                       _p(rows_dev), _stream()), "mvlt_ce_bwd")
    return out


SEQ_LOSS_MAX_B, SEQ_LOSS_MAX_T = 4096, 512          # one workgroup plans the batch (mvlt_seq_loss_plan)


def seq_loss_plan(ids, eos, weights, row0, row_step):
    """Decoded id rows -> the labelled-row plan of the sequence loss (mvlt_seq_loss_plan).  ids int64 [B, T] (unit column stride),
    eos (None / negative: only PAD ends a row), weights f32 [B] or [B, T] (any strides), row0 / row_step: the encoder row of
    position (b, t) is row0 + b * row_step + t.  Returns ``(len i32 [B], tf_ids i64 [B, T], gather_row i32 [B T], sel_labels i64
    [B T], row_weight f32 [B T], rows_dev i32 [1])`` -- the last four as ``label_plan`` lays them out."""
    _need_cuda(ids, weights)
    assert ids.dim() == 2 and ids.dtype == torch.int64 and ids.stride(1) == 1
    B, T = ids.shape
    if not (0 < B <= SEQ_LOSS_MAX_B and 0 < T <= SEQ_LOSS_MAX_T):
        raise ValueError(f"sequences [{B}, {T}]: the plan takes 1 .. {SEQ_LOSS_MAX_B} rows of 1 .. {SEQ_LOSS_MAX_T} ids")
    assert weights.dtype == torch.float32 and tuple(weights.shape) in ((B,), (B, T))
    wsb, wst = weights.stride(0), (weights.stride(1) if weights.dim() == 2 else 0)
    assert wsb >= 0 and wst >= 0
    dev = ids.device
    N = B * T
    i32buf = torch.empty(B + N + 1, dtype=torch.int32, device=dev)
    i64buf = torch.empty(2 * N, dtype=torch.int64, device=dev)
    rw = torch.empty(N, dtype=torch.float32, device=dev)
    ln, gr, rd = i32buf[:B], i32buf[B:B + N], i32buf[B + N:]
    tf, sel = i64buf[:N].view(B, T), i64buf[N:]
    L.check(L.lib().mvlt_seq_loss_plan(_p(ids), ids.stride(0) if B > 1 else max(ids.stride(0), T), B, T,
                                       -1 if eos is None else int(eos), _p(weights), wsb, wst, int(row0), int(row_step), _p(ln),
                                       _p(tf), _p(gr), _p(sel), _p(rw), _p(rd), _stream()), "mvlt_seq_loss_plan")
    return ln, tf, gr, sel, rw, rd


def seq_loss_fwd(lse, x_label, row_weight, rows_dev=None):
    """acc f32 [2] = (sum of row_weight * (lse - x_label) over the first *rows_dev rows, their number), in a fixed order."""
    _need_cuda(lse, x_label, row_weight)
    rows = lse.numel()
    for t in (lse, x_label, row_weight):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == rows
    acc = torch.empty(2, dtype=torch.float32, device=lse.device)
    L.check(L.lib().mvlt_seq_loss_fwd(_p(lse), _p(x_label), _p(row_weight), rows, _p(rows_dev), _p(acc), _stream()),
            "mvlt_seq_loss_fwd")
    return acc


def ce_bwd_weighted(logits, V, labels, lse, row_weight, acc, grad_scale=1.0, out=None, grad_scale_dev=None, rows_dev=None):
    """ce_bwd with a weight per row (mvlt_ce_bwd_weighted): dlogits = (grad_scale * grad_scale_dev / max(acc[1], 1)) *
    row_weight[i] * (softmax - onehot), in place over the logits unless ``out`` is given."""
    if out is None:
        out = logits
    if grad_scale_dev is not None:
        assert grad_scale_dev.dtype == torch.float32 and grad_scale_dev.numel() == 1
    assert row_weight.dtype == torch.float32 and row_weight.is_contiguous() and row_weight.numel() == logits.shape[0]
    assert out.stride(0) == logits.stride(0) and out.dtype == logits.dtype
    L.check(L.lib().mvlt_ce_bwd_weighted(_dt(logits), _p(logits), logits.stride(0), logits.shape[0], V, _p(labels), _p(lse),
                                         _p(row_weight), C.c_void_p(acc.data_ptr() + 4), float(grad_scale), _p(grad_scale_dev),
                                         _p(out), _p(rows_dev), _stream()), "mvlt_ce_bwd_weighted")
    return out


def gelu_bwd(x, dy, out=None):
    dx = torch.empty_like(x) if out is None else out
    L.check(L.lib().mvlt_gelu_bwd(_dt(x), _p(x), _p(dy), _p(dx), x.numel(), _stream()), "mvlt_gelu_bwd")
    return dx


def softmax_rows(logits, V):
    out = torch.empty((logits.shape[0], V), dtype=torch.float32, device=logits.device)
    L.check(L.lib().mvlt_softmax_rows(_dt(logits), _p(logits), logits.stride(0), logits.shape[0], V, _p(out),
                                      _stream()), "mvlt_softmax_rows")
    return out


def adamw(param, grad, exp_avg, exp_avg_sq, shadow, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    _need_cuda(param)
    L.check(L.lib().mvlt_adamw(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(shadow), param.numel(),
                               float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                               float(grad_scale), _stream()), "mvlt_adamw")


def adamw_guarded(param, grad, exp_avg, exp_avg_sq, shadow, lr, beta1, beta2, eps, weight_decay, step, grad_scale, coef, skip):
    """adamw with the gradient scale ``grad_scale * coef[0]`` (f32 on the device) that writes nothing when ``skip[0] != 0``
    (int32 on the device): the consumer of grad_norm_finish."""
    _need_cuda(param, coef, skip)
    assert coef.dtype == torch.float32 and skip.dtype == torch.int32
    L.check(L.lib().mvlt_adamw_guarded(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(shadow), param.numel(),
                                       float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                                       float(grad_scale), _p(coef), _p(skip), _stream()), "mvlt_adamw_guarded")


def adamw_groups_block():
    return int(L.lib().mvlt_adamw_groups_block())


def adamw_groups(param, grad, exp_avg, exp_avg_sq, shadow, block_group, lr_scale, weight_decay, lr, beta1, beta2, eps, step,
                 grad_scale=1.0, coef=None, skip=None):
    """adamw with the parameter groups resolved inside the launch: ``block_group`` (uint8, one per 64 elements of ``param``) names
    the group of each block, group g runs with lr * lr_scale[g] and weight_decay[g] (f32 tables on the device).  ``coef`` / ``skip``
    both None: plain; both given: adamw_guarded's semantics."""
    _need_cuda(param, block_group, lr_scale, weight_decay)
    n = param.numel()
    assert block_group.dtype == torch.uint8 and block_group.is_contiguous() and block_group.numel() * 64 == n, (block_group.shape, n)
    assert lr_scale.dtype == torch.float32 and weight_decay.dtype == torch.float32 and lr_scale.numel() == weight_decay.numel()
    assert lr_scale.is_contiguous() and weight_decay.is_contiguous()
    if coef is not None or skip is not None:
        _need_cuda(coef, skip)
        assert coef.dtype == torch.float32 and skip.dtype == torch.int32
    L.check(L.lib().mvlt_adamw_groups(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(shadow), n, _p(block_group),
                                      _p(lr_scale), _p(weight_decay), lr_scale.numel(), float(lr), float(beta1), float(beta2),
                                      float(eps), int(step), float(grad_scale), _p(coef), _p(skip), _stream()), "mvlt_adamw_groups")


def grad_sumsq_parts():
    return int(L.lib().mvlt_grad_sumsq_parts())


def grad_sumsq(g, partial=None, accumulate=False):
    """partial[b] (f64 [grad_sumsq_parts()]) = or += the sum of squares workgroup b takes of the f32 range ``g``, every element
    widened to f64 before it is squared.  The sum of ``partial`` is the squared L2 norm; no float atomics, bit-reproducible."""
    _need_cuda(g)
    assert g.dtype == torch.float32 and g.is_contiguous()
    if partial is None:
        assert not accumulate
        partial = torch.empty(grad_sumsq_parts(), dtype=torch.float64, device=g.device)
    assert partial.dtype == torch.float64 and partial.is_contiguous() and partial.numel() == grad_sumsq_parts()
    L.check(L.lib().mvlt_grad_sumsq(_p(g), g.numel(), _p(partial), 1 if accumulate else 0, _stream()), "mvlt_grad_sumsq")
    return partial


def grad_norm_finish(partial, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False, out=None, flags=None):
    """out (f32 [2]) = (norm, clip coefficient), flags (int32 [2]) = (skip this step, running count of skipped steps) from the
    partial sums of grad_sumsq; ``flags`` must be initialised (the count is added to)."""
    _need_cuda(partial)
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=partial.device)
    if flags is None:
        flags = torch.zeros(2, dtype=torch.int32, device=partial.device)
    assert partial.dtype == torch.float64 and out.dtype == torch.float32 and flags.dtype == torch.int32
    assert out.numel() >= 2 and flags.numel() >= 2
    L.check(L.lib().mvlt_grad_norm_finish(_p(partial), partial.numel(), float(grad_scale), float(max_norm),
                                          1 if skip_nonfinite else 0, _p(out), _p(flags), _stream()), "mvlt_grad_norm_finish")
    return out, flags


def attn_cached(qkv_new, k_cache, v_cache, past, scale, out=None, row_shift=None):
    """past: int, or an int32 device tensor [1] (position kept on the GPU by a replayed decode loop).
    ``row_shift`` (int32 [B], device; None: the entry point without it): batch row b sits at ``past + row_shift[b]``, clamped
    into its cache (mvlt_attn_cached_rows: hd = 64, n_new <= 4)."""
    B, nH, cap, hd = k_cache.shape
    n_new = qkv_new.shape[0] // B
    if out is None:
        out = torch.empty((B * n_new, nH * hd), dtype=qkv_new.dtype, device=qkv_new.device)
    p = L.MvltAttnCached()
    p.dtype, p.B, p.nH, p.hd, p.n_new, p.cache_cap = _dt(qkv_new), B, nH, hd, n_new, cap
    if torch.is_tensor(past):
        assert past.dtype == torch.int32 and past.is_cuda
        p.past_dev = _p(past)
    else:
        p.past = past
    p.qkv_new, p.k_cache, p.v_cache, p.out, p.scale = _p(qkv_new), _p(k_cache), _p(v_cache), _p(out), float(scale)
    if row_shift is not None:
        assert row_shift.dtype == torch.int32 and row_shift.is_cuda and row_shift.is_contiguous() and row_shift.numel() == B
        L.check(L.lib().mvlt_attn_cached_rows(C.byref(p), _p(row_shift), _stream()), "mvlt_attn_cached_rows")
        return out
    L.check(L.lib().mvlt_attn_cached(C.byref(p), _stream()), "mvlt_attn_cached")
    return out


def attn_cached_beam(qkv_new, k_cache, v_cache, past, scale, num_beams, prefix, slot, out=None):
    """attn_cached over the hypotheses of a beam search whose cache is never reordered (mvlt_attn_cached_beam): key positions
    < prefix come from the first cache row of the row's sample, generated positions from the row ``slot[r, k - prefix]`` (int32
    [rows, ld]) names within the sample, the new rows are appended to the row's own cache row.  hd = 64, n_new <= 4."""
    rows, nH, cap, hd = k_cache.shape
    n_new = qkv_new.shape[0] // rows
    assert slot.dtype == torch.int32 and slot.is_cuda and slot.dim() == 2 and slot.shape[0] == rows and slot.stride(1) == 1
    if out is None:
        out = torch.empty((rows * n_new, nH * hd), dtype=qkv_new.dtype, device=qkv_new.device)
    p = L.MvltAttnCachedBeam()
    p.dtype, p.rows, p.nH, p.hd, p.n_new, p.cache_cap = _dt(qkv_new), rows, nH, hd, n_new, cap
    if torch.is_tensor(past):
        assert past.dtype == torch.int32 and past.is_cuda
        p.past_dev = _p(past)
    else:
        p.past = past
    p.qkv_new, p.k_cache, p.v_cache, p.out, p.scale = _p(qkv_new), _p(k_cache), _p(v_cache), _p(out), float(scale)
    p.num_beams, p.prefix, p.slot, p.ld_slot = int(num_beams), int(prefix), _p(slot), slot.stride(0)
    L.check(L.lib().mvlt_attn_cached_beam(C.byref(p), _stream()), "mvlt_attn_cached_beam")
    return out


def argmax(logits, V):
    out = torch.empty(logits.shape[0], dtype=torch.int64, device=logits.device)
    L.check(L.lib().mvlt_argmax(_dt(logits), _p(logits), logits.stride(0), logits.shape[0], V, _p(out), _stream()),
            "mvlt_argmax")
    return out
