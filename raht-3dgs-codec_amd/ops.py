"""Host-side mirror of the reference's operator interface for the RAHT hot path.

Same names, argument meaning and return shapes as the reference's L3 operators, so that the
three-entry dispatch table of its drivers (reference python/encode_3dgs.py:23-27) can be replaced by

    from raht_3dgs_codec_amd import raht_fn      # {"RAHT", "iRAHT", "RAHT_param"}

Everything below runs on the MI355X through the C ABI of include/raht.h (libraht_hip.so); torch
is only plumbing (device memory, current stream). There is no CPU path: CPU tensors raise.

Differences from the reference, all deliberate:
  * ``RAHT_param_reorder_fast`` returns one opaque plan token per list instead of 3J tensors per
    list; the tokens are real device tensors, so the drivers' ``[t.to(device) for t in ListC]``
    keeps working, and they are handed back opaquely to RAHT / iRAHT exactly as before.
    ``plan_of(ListC).export_lists()`` materialises the reference-shaped List/Flags/weights.
  * unsorted / duplicate / out-of-range voxels raise ``RahtError`` (the reference silently
    mis-pairs them); N == 1 returns order_RAGFT = [0] (the reference returns None).
  * compute dtype follows the input: float32 in -> float32 kernels (the fast path), float64 in ->
    float64 kernels (the reference's own precision). The reference always returns float64.
"""
import collections
import contextlib
import ctypes as C

import torch

from . import _lib
from ._lib import RahtError, check  # noqa: F401

_MAGIC = 0x52414854_504C414E  # "RAHTPLAN"
_plans = collections.OrderedDict()   # id -> RahtPlan (strong refs to the most recent plans)
_PLAN_CACHE = 16
_next_id = [1]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"raht-3dgs-codec_amd: {name} must be a CUDA (HIP) tensor; this package has "
                           "no CPU path for the RAHT hot path")


_VDT = {torch.float32: _lib.RAHT_F32, torch.float64: _lib.RAHT_F64, torch.int32: _lib.RAHT_I32,
        torch.int64: _lib.RAHT_I64}
_STEP_CTYPE = {torch.float32: C.c_float, torch.float64: C.c_double}
_FN_SUFFIX = {torch.float32: "", torch.float64: "_f64"}      # raht_fwd_quant / raht_fwd_quant_f64, ...: one name per precision


def _fn(name, dtype):
    return getattr(_lib.lib(), name + _FN_SUFFIX[dtype])


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _call(fn, device, *args, after=()):
    """one call through the C ABI on ``device``, on its current stream (every entry point's last argument but for ``after``)"""
    with torch.cuda.device(device):
        check(fn(*args, _stream(), *after))


def _host_floats(v):
    """host floats from a tensor (which comes to the host once), list or tuple: a bounding box corner as the caller gives it"""
    return [float(x) for x in (v.detach().cpu().reshape(-1).tolist() if isinstance(v, torch.Tensor) else v)]


def _rows(X, dtype, name):
    """X as a matrix the kernels take: on the GPU, of ``dtype`` (None: float32 or float64 as it comes, anything else float32),
    unit column stride and a row stride of at least D -- column slices of wider matrices pass as they are"""
    _need_cuda(X, name)
    if dtype is None:
        dtype = X.dtype if X.dtype in (torch.float32, torch.float64) else torch.float32
    X = X.to(dtype)
    if X.stride(1) != 1 or X.stride(0) < X.shape[1]:
        X = X.contiguous()
    return X


def _qmat(Q):
    _need_cuda(Q, "Q")
    return Q.to(torch.int32).contiguous()


def to_int32(R):
    """The integers of R = floor(x / step + 0.5) (float32 or float64, any device) by THE out-of-range rule of every quantizer
    (include/raht.h): R itself within [-2^31, 2^31 - 1], INT32_MAX above (+inf included), INT32_MIN below (-inf included), 0 for NaN.
    A bare ``.to(torch.int32)`` of such values differs between the CPU and the GPU. Clamped in R's own type, so that only values in
    range are converted: the largest float32 below 2^31 is 2^31 - 128, whatever lies above it takes INT32_MAX by a select."""
    f64 = R.dtype == torch.float64
    q = torch.nan_to_num(R, nan=0.0).clamp_(-2147483648.0, 2147483647.0 if f64 else 2147483520.0).to(torch.int32)
    return q if f64 else q.masked_fill_(R >= 2147483648.0, 2147483647)


def step_list(steps, D=None):
    """A quantization step argument as a list of Python floats: [step] for a scalar (Python or numpy number, 0-d array or tensor),
    else the entries of a list, tuple, numpy array or tensor (which comes to the host once). With ``D``: one entry or D."""
    if hasattr(steps, "tolist"):
        steps = steps.tolist()
    out = [float(steps)] if isinstance(steps, (int, float)) else [float(x) for x in steps]
    if D is not None and len(out) not in (1, D):
        raise ValueError("steps must be a scalar or have D entries")
    return out


def _step_array(steps, D, ctype):
    st = step_list(steps, D)
    return (ctype * len(st))(*st)


class RahtPlan:
    """Owns a ``raht_plan*`` (device-resident lvl / wl / wr / order_RAGFT and tile schedules)."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = device
        L = _lib.lib()
        self.N = int(L.raht_plan_size(handle))
        self.nbits = int(L.raht_plan_nbits(handle))
        self.id = _next_id[0]
        _next_id[0] += 1
        self._order = None
        self._inv_order = None
        self._roots = None
        self.map_rows = None             # rows of the matrices of a row-mapped plan (set_row_map)

    @property
    def inv_order(self):
        """Inverse permutation of order_RAGFT: position of row i in the reordered coefficient list."""
        if self._inv_order is None:
            o = self.order_RAGFT
            inv = torch.empty_like(o)
            inv[o] = torch.arange(self.N, dtype=torch.int64, device=o.device)
            self._inv_order = inv
        return self._inv_order

    # -- construction ---------------------------------------------------------------------------
    @staticmethod
    def from_coords(V, minV, width, depth):
        _need_cuda(V, "V")
        if V.dim() != 2 or V.shape[1] != 3:
            raise ValueError("V must be (N, 3)")
        if V.dtype not in _VDT:
            V = V.to(torch.float64)
        V = V.contiguous()
        mv = _host_floats(minV)
        if len(mv) != 3:
            raise ValueError("minV must have 3 entries")
        arr = (C.c_double * 3)(*mv)
        h = C.c_void_p()
        with torch.cuda.device(V.device):
            check(_lib.lib().raht_plan_create(C.c_void_p(V.data_ptr()), _VDT[V.dtype], V.shape[0], arr,
                                              float(width), int(depth), _stream(), C.byref(h)))
        return RahtPlan(h, V.device)

    @staticmethod
    def from_keys(keys_sorted, nbits, leaf_weights=None, top_level=None, borrow=False):
        """borrow=True: the plan reads `keys_sorted` in place instead of copying it (the plan keeps a reference to the
        tensor; the caller must not modify it while the plan lives)."""
        _need_cuda(keys_sorted, "keys_sorted")
        k = keys_sorted.contiguous()
        if k.dtype not in (torch.int64, torch.uint64):
            raise ValueError("keys must be int64/uint64")
        lw = None
        if leaf_weights is not None:
            _need_cuda(leaf_weights, "leaf_weights")
            lw = leaf_weights.to(torch.int64).contiguous()
        h = C.c_void_p()
        fn = _lib.lib().raht_plan_create_from_keys_borrowed if borrow else _lib.lib().raht_plan_create_from_keys
        with torch.cuda.device(k.device):
            check(fn(C.c_void_p(k.data_ptr()), k.shape[0], int(nbits),
                     C.c_void_p(lw.data_ptr()) if lw is not None else None, _stream(), C.byref(h)))
        p = RahtPlan(h, k.device)
        if borrow:
            p._keys_ref = k                   # keeps the borrowed array alive as long as the plan
        if top_level is not None:
            p.set_top_level(top_level)
        return p

    # -- truncated trees / roots (Morton-prefix sharded scenes) -----------------------------------
    def set_top_level(self, top_level):
        """Butterflies at binary levels >= top_level are left to the caller's top stage."""
        with torch.cuda.device(self.device):
            check(_lib.lib().raht_plan_set_top_level(self._h, int(top_level), _stream()))
        self._roots = None

    @property
    def root_rows(self):
        """int64 device tensor: rows that still carry a low-pass value after a forward transform."""
        if getattr(self, "_roots", None) is None:
            n = C.c_int64()
            check(_lib.lib().raht_plan_roots(self._h, C.byref(n), None, None))
            r = torch.empty(n.value, dtype=torch.int64, device=self.device)
            with torch.cuda.device(self.device):
                check(_lib.lib().raht_plan_roots(self._h, C.byref(n), C.c_void_p(r.data_ptr()), _stream()))
            self._roots = r
        return self._roots

    @property
    def n_roots(self):
        return int(self.root_rows.shape[0])

    def _set_roots_buffer(self, buf, D, dtype):
        if buf is None:
            check(_lib.lib().raht_plan_set_root_buffer(self._h, None))
            return
        _need_cuda(buf, "roots")
        if buf.dtype != dtype or tuple(buf.shape) != (self.n_roots, D) or not buf.is_contiguous():
            raise ValueError(f"roots buffer must be a contiguous ({self.n_roots}, {D}) {dtype} tensor")
        check(_lib.lib().raht_plan_set_root_buffer(self._h, C.c_void_p(buf.data_ptr())))

    def _set_mixed_roots(self, roots, roots_wide, D, n_wide):
        """the two root buffers of the mixed-precision entries: (n_roots, D) float32 (columns [n_wide, D) meaningful) and
        (n_roots, n_wide) float64; both or neither"""
        if (roots is None) != (roots_wide is None):
            raise ValueError("roots and roots_wide go together: pass both or neither")
        if roots is None:
            return
        _need_cuda(roots_wide, "roots_wide")
        if roots_wide.dtype != torch.float64 or tuple(roots_wide.shape) != (self.n_roots, n_wide) or not roots_wide.is_contiguous():
            raise ValueError(f"roots_wide must be a contiguous ({self.n_roots}, {n_wide}) float64 tensor")
        self._set_roots_buffer(roots, D, torch.float32)
        check(_lib.lib().raht_plan_set_root_buffer_wide(self._h, C.c_void_p(roots_wide.data_ptr())))

    @contextlib.contextmanager
    def _with_roots(self, D, roots, dtype, roots_wide=None, n_wide=None):
        """these root buffers are set for the duration of a call and reset afterwards, also when the call raises: one (n_roots, D)
        buffer of ``dtype``, or with ``n_wide`` the pair of the mixed-precision entries (_set_mixed_roots); None: nothing to set"""
        try:
            if n_wide is None:
                self._set_roots_buffer(roots, D, dtype)
            else:
                self._set_mixed_roots(roots, roots_wide, D, n_wide)
            yield
        finally:
            if roots is not None:
                check(_lib.lib().raht_plan_set_root_buffer(self._h, None))
                check(_lib.lib().raht_plan_set_root_buffer_wide(self._h, None))

    def _quant(self, fn, src, st, *rest):
        """the argument head every quantizing entry point shares: plan, source matrix, its row stride, D, the step array"""
        _call(fn, src.device, self._h, _p(src), src.stride(0), src.shape[1], st, len(st), *rest)

    def __del__(self):
        try:
            if self._h:
                _lib.lib().raht_plan_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # -- views ----------------------------------------------------------------------------------
    @property
    def order_RAGFT(self):
        if self._order is None:
            o = torch.empty(self.N, dtype=torch.int64, device=self.device)
            with torch.cuda.device(self.device):
                check(_lib.lib().raht_plan_order(self._h, C.c_void_p(o.data_ptr()), _stream()))
            self._order = o
        return self._order

    @property
    def levels(self):
        return int(_lib.lib().raht_plan_levels(self._h))

    def set_engine(self, engine="tile", tile_rows=0, tail_rows=0, tail_channels=0, final_rows=0):
        e = {"tile": _lib.ENGINE_TILE, "level": _lib.ENGINE_LEVEL}[engine]
        check(_lib.lib().raht_plan_set_engine(self._h, e, int(tile_rows)))
        check(_lib.lib().raht_plan_set_tail_tile(self._h, int(tail_rows), int(tail_channels), int(final_rows)))

    def export_lists(self):
        """Reference-shaped (List, Flags, weights) as CPU tensors (RAHT_param.py:190-279 outputs)."""
        import numpy as np
        L = _lib.lib()
        List, Flags, weights = [], [], []
        for l in range(self.levels):
            n = C.c_int64()
            check(L.raht_plan_export_level(self._h, l, None, None, None, C.byref(n)))
            a = np.empty(n.value, np.int64)
            f = np.empty(n.value, np.uint8)
            w = np.empty(n.value, np.int64)
            check(L.raht_plan_export_level(self._h, l, a.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p),
                                           w.ctypes.data_as(C.c_void_p), C.byref(n)))
            List.append(torch.from_numpy(a))
            Flags.append(torch.from_numpy(f.astype(bool)))
            weights.append(torch.from_numpy(w))
        return List, Flags, weights

    def keys_tensor(self):
        """The plan's sorted Morton keys as an int64 device tensor (a copy)."""
        t = torch.empty(self.N, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            check(_lib.lib().raht_plan_copy_array(self._h, 0, C.c_void_p(t.data_ptr()), _stream()))
        return t

    def arrays(self):
        """(keys, lvl, wl, wr) copied to CPU numpy arrays (inspection / tests)."""
        import numpy as np
        out = []
        with torch.cuda.device(self.device):
            for which, dt in enumerate((torch.int64, torch.uint8, torch.int32, torch.int32)):
                t = torch.empty(self.N, dtype=dt, device=self.device)
                check(_lib.lib().raht_plan_copy_array(self._h, which, C.c_void_p(t.data_ptr()), _stream()))
                out.append(t.cpu().numpy())
        out[0] = out[0].view(np.uint64)
        return tuple(out)

    def stage_stats(self, elem_size=4, D=59):
        n = C.c_int()
        rows = (C.c_int64 * 32)()
        tr = C.c_int()
        check(_lib.lib().raht_plan_stage_stats(self._h, elem_size, D, C.byref(n), rows, 32, C.byref(tr)))
        k = abs(n.value)
        return dict(valid=n.value > 0, tile_rows=tr.value, rows_per_stage=[int(rows[i]) for i in range(k)])

    # -- transforms -----------------------------------------------------------------------------
    def _xform(self, X, inverse, want_w=False, roots=None, out=None):
        _need_cuda(X, "C" if not inverse else "T")
        rows = self.N if self.map_rows is None else self.map_rows
        if X.dim() != 2 or X.shape[0] != rows:
            raise ValueError(f"expected ({rows}, D) tensor, got {tuple(X.shape)}")
        if X.dtype not in (torch.float32, torch.float64):
            X = X.to(torch.float32)
        if X.stride(1) != 1 or X.stride(0) < X.shape[1]:
            X = X.contiguous()
        D = X.shape[1]
        if out is None:
            out = torch.empty((rows, D), dtype=X.dtype, device=X.device)
        elif out.dtype != X.dtype or tuple(out.shape) != (rows, D) or not out.is_contiguous() or out.device != X.device:
            raise ValueError(f"out must be a contiguous ({rows}, {D}) {X.dtype} tensor on {X.device}")
        w = torch.empty((self.N, 1), dtype=X.dtype, device=X.device) if want_w else None
        L = _lib.lib()
        f64 = X.dtype == torch.float64
        with self._with_roots(D, roots, X.dtype):
            self._run(L, X, out, w, D, inverse, f64)
        return (out, w) if want_w else out

    def _run(self, L, X, out, w, D, inverse, f64):
        with torch.cuda.device(X.device):
            if not inverse:
                fn = L.raht_fwd_f64 if f64 else L.raht_fwd
                check(fn(self._h, C.c_void_p(X.data_ptr()), X.stride(0), D, C.c_void_p(out.data_ptr()), D,
                         C.c_void_p(w.data_ptr()) if w is not None else None, _stream()))
            else:
                fn = L.raht_inv_f64 if f64 else L.raht_inv
                check(fn(self._h, C.c_void_p(X.data_ptr()), X.stride(0), D, C.c_void_p(out.data_ptr()), D,
                         _stream()))

    def forward(self, Cmat, want_w=True, roots=None, out=None):
        """roots: optional (n_roots, D) output buffer receiving the rows that still carry a low-pass;
        out: optional preallocated result matrix."""
        return self._xform(Cmat, False, want_w, roots, out)

    def inverse(self, T, roots=None, out=None):
        """roots: optional (n_roots, D) buffer the root rows are read from instead of T."""
        return self._xform(T, True, False, roots, out)

    def prepare(self, D, dtype=torch.float32):
        """Pre-build schedule + workspaces so later calls only enqueue kernels (hipGraph-safe)."""
        es = 8 if dtype == torch.float64 else 4
        with torch.cuda.device(self.device):
            check(_lib.lib().raht_plan_prepare(self._h, es, int(D), _stream()))

    def set_row_map(self, row_map, n_matrix_rows):
        """Plan row i lives in row ``row_map[i]`` of the (n_matrix_rows, D) matrices given to forward / inverse
        (small plans: the replicated top tree of a sharded scene works in place on the padded all-gather buffer)."""
        with torch.cuda.device(self.device):
            if row_map is None:
                check(_lib.lib().raht_plan_set_row_map(self._h, None, 0, _stream()))
                self.map_rows = None
                return
            m = row_map.to(device=self.device, dtype=torch.int64).contiguous()
            check(_lib.lib().raht_plan_set_row_map(self._h, C.c_void_p(m.data_ptr()), int(n_matrix_rows), _stream()))
        self.map_rows = int(n_matrix_rows)

    def set_concurrent_directions(self, on=True):
        """One workspace set per direction: a forward-direction and an inverse-direction call of this plan may then run at the same
        time on two streams (the drivers' loop over quantization steps: forward of step s + 1 next to the inverse of step s)."""
        with torch.cuda.device(self.device):
            check(_lib.lib().raht_plan_set_concurrent_directions(self._h, 1 if on else 0))

    def set_max_stages(self, max_stages):
        """Bound on the launches per direction of the tile schedule; above it the level engine runs."""
        with torch.cuda.device(self.device):
            check(_lib.lib().raht_plan_set_max_stages(self._h, int(max_stages)))

    def _quant_to(self, name, src, steps, out_dtype, step_dtype, roots=None):
        """``src`` through the entry point ``name`` of ``step_dtype``'s precision -> a new (N, D) matrix of ``out_dtype``"""
        D = src.shape[1]
        st = _step_array(steps, D, _STEP_CTYPE[step_dtype])
        dst = torch.empty((self.N, D), dtype=out_dtype, device=src.device)
        with self._with_roots(D, roots, step_dtype):
            self._quant(_fn(name, step_dtype), src, st, _p(dst), D)
        return dst

    def forward_quant(self, Cmat, steps, roots=None):
        """Forward RAHT + quantize + reorder -> int32 Q. float32 (default): ONE fused pass, T is never
        materialised. float64 input: the same at the reference's precision (encode_3dgs.py:82-83,204): the float64 tile
        kernels with the float64 quantizer in their write-back."""
        X = _rows(Cmat, None, "C")
        return self._quant_to("raht_fwd_quant", X, steps, torch.int32, X.dtype, roots)

    def dequant_inverse(self, Q, steps, roots=None, dtype=torch.float32):
        """Un-reorder + dequantize + inverse RAHT -> C in ONE fused pass (dtype=torch.float64: at the reference's
        precision)."""
        dtype = torch.float64 if dtype == torch.float64 else torch.float32
        return self._quant_to("raht_dequant_inv", _qmat(Q), steps, dtype, dtype, roots)

    def forward_quant_multi(self, Cmat, steps):
        """ONE forward pass, one quantization per (scalar) step: -> [Q_0, ..., Q_{k-1}], each bit-identical to
        ``forward_quant(C, steps[i])`` (the drivers quantize one coefficient matrix at nine steps, python/encode_3dgs.py:28,199-217)."""
        X = _rows(Cmat, torch.float32, "C")
        Qs, st, ptrs = self._multi_out(X, steps, C.c_float)
        self._quant(_lib.lib().raht_fwd_quant_multi, X, st, ptrs, X.shape[1])
        return Qs

    def _multi_out(self, X, steps, ctype):
        """one output matrix per (scalar) step -> (matrices, step array, pointer array)"""
        k = len(steps)
        Qs = [torch.empty((self.N, X.shape[1]), dtype=torch.int32, device=X.device) for _ in range(k)]
        return Qs, (ctype * k)(*[float(s) for s in steps]), (C.c_void_p * k)(*[q.data_ptr() for q in Qs])

    def dequant_inverse_sqdiff(self, Q, steps, C_ref, want_rec=True):
        """Un-reorder + dequantize + inverse RAHT (float32, fused) that also compares its output with the original attributes on the
        way out: -> (C_rec or None, float64[D] per-column sums of (C_rec - C_ref)^2). What the drivers' five PSNR columns are made of
        (python/encode_3dgs.py:274,298-310) without a pass of its own; with ``want_rec=False`` C_rec is never written."""
        Q, X, st, out, ssd = self._sqdiff_args(Q, steps, C_ref, want_rec, C.c_float)
        self._quant(_lib.lib().raht_dequant_inv_sqdiff, Q, st, _p(X), X.stride(0), _p(out), Q.shape[1], _p(ssd))
        return out, ssd

    def _sqdiff_args(self, Q, steps, C_ref, want_rec, ctype):
        _need_cuda(Q, "Q")
        _need_cuda(C_ref, "C_ref")
        Q = _qmat(Q)
        D = Q.shape[1]
        X = _rows(C_ref, torch.float32, "C_ref")
        st = _step_array(steps, D, ctype)
        out = torch.empty((self.N, D), dtype=torch.float32, device=Q.device) if want_rec else None
        return Q, X, st, out, torch.empty(D, dtype=torch.float64, device=Q.device)

    def forward_quant_mixed(self, Cmat, steps, n_wide=3, roots=None, roots_wide=None):
        """Forward RAHT + quantize + reorder of a float32 matrix whose first ``n_wide`` channels (the xyz columns of a
        59-column frame, python/voxelize_pc.py:155) are carried in float64 -- the reference's precision
        (python/encode_3dgs.py:82-83,204) where float32 cannot hold the quotient -- in the same launches as the float32
        channels. Wide columns: bit-identical to the float64 kernels; the others: bit-identical to ``forward_quant``.
        roots / roots_wide (together; a truncated plan needs them): (n_roots, D) float32 and (n_roots, n_wide) float64 buffers
        receiving the roots' low-pass rows -- columns [n_wide, D) in the first (its columns [0, n_wide) are unspecified), columns
        [0, n_wide) unrounded in the second; the roots' Q rows are left to the caller."""
        X = _rows(Cmat, torch.float32, "C")
        D = X.shape[1]
        st = _step_array(steps, D, C.c_double)
        Q = torch.empty((self.N, D), dtype=torch.int32, device=X.device)
        with self._with_roots(D, roots, torch.float32, roots_wide, int(n_wide)):
            self._quant(_lib.lib().raht_fwd_quant_mixed, X, st, int(n_wide), _p(Q), D)
        return Q

    def dequant_inverse_mixed(self, Q, steps, n_wide=3, out=None, roots=None, roots_wide=None):
        """Un-reorder + dequantize + inverse RAHT -> float32 C, the first ``n_wide`` channels computed in float64 and
        rounded once on output (counterpart of ``forward_quant_mixed``). roots / roots_wide: the two root buffers the
        roots' low-pass rows are read from instead of Q (as ``forward_quant_mixed`` writes them)."""
        Q = _qmat(Q)
        D = Q.shape[1]
        st = _step_array(steps, D, C.c_double)
        if out is None:
            out = torch.empty((self.N, D), dtype=torch.float32, device=Q.device)
        with self._with_roots(D, roots, torch.float32, roots_wide, int(n_wide)):
            self._quant(_lib.lib().raht_dequant_inv_mixed, Q, st, int(n_wide), _p(out), out.stride(0))
        return out

    def forward_quant_mixed_multi(self, Cmat, steps, n_wide=3, roots=None, roots_wide=None):
        """ONE mixed-precision forward pass, one quantization per (scalar) step: -> [Q_0, ..., Q_{k-1}], each bit-identical to
        ``forward_quant_mixed(C, steps[i], n_wide)`` -- the nine steps of a frame (python/encode_3dgs.py:28,199-217) with the
        reference's integers on the first ``n_wide`` columns. roots / roots_wide: as for ``forward_quant_mixed``."""
        X = _rows(Cmat, torch.float32, "C")
        D = X.shape[1]
        Qs, st, ptrs = self._multi_out(X, steps, C.c_double)
        with self._with_roots(D, roots, torch.float32, roots_wide, int(n_wide)):
            self._quant(_lib.lib().raht_fwd_quant_mixed_multi, X, st, int(n_wide), ptrs, D)
        return Qs

    def dequant_inverse_mixed_sqdiff(self, Q, steps, C_ref, n_wide=3, want_rec=True, roots=None, roots_wide=None):
        """``dequant_inverse_mixed`` that also compares its output with the original attributes on the way out: -> (C_rec or None,
        float64[D] per-column sums of (C_rec - C_ref)^2, from the float32 values C_rec holds). With ``want_rec=False`` C_rec is
        never written. roots / roots_wide: as for ``dequant_inverse_mixed``."""
        Q, X, st, out, ssd = self._sqdiff_args(Q, steps, C_ref, want_rec, C.c_double)
        D = Q.shape[1]
        with self._with_roots(D, roots, torch.float32, roots_wide, int(n_wide)):
            self._quant(_lib.lib().raht_dequant_inv_mixed_sqdiff, Q, st, int(n_wide), _p(X), X.stride(0), _p(out), D, _p(ssd))
        return out, ssd

    def rate_curve(self, Cmat, steps, n_wide=0, seg_len=2048):
        """The rate-distortion curve of a frame from ONE forward transform and one read of its coefficients: for each of the k
        ``steps`` (scalars, or tables of D entries) the bytes of the attribute container ``bitstream.encode_frame_bytes`` would write
        (``SegmentedCoder.size_bytes`` of ``forward_quant(C, step)``; with ``n_wide`` > 0 of ``forward_quant_mixed(C, step, n_wide)``)
        and the squared quantization error per column, in the coefficient domain -- RAHT is orthonormal, so up to the transform's
        rounding this is the attributes' squared error. Nothing is quantized, coded or written but two small tables
        (rlgr.SegmentedCoder.rate). -> {"bytes": int64 numpy [k], "sse": float64 numpy [k, D]}.
        ``n_wide`` > 0: the first n_wide columns through the float64 transform (the mixed kernels' integers on those columns are
        the float64 path's), the others through the float32 one. Row-mapped and truncated plans raise ``ValueError``."""
        from .rlgr import SegmentedCoder
        _need_cuda(Cmat, "C")
        if self.map_rows is not None or self.n_roots != 1:
            raise ValueError("rate_curve: not available for row-mapped or truncated plans")
        n_wide = int(n_wide)
        if Cmat.dim() != 2 or Cmat.shape[0] != self.N or not 0 <= n_wide <= Cmat.shape[1]:
            raise ValueError(f"rate_curve: expected an ({self.N}, D) matrix and 0 <= n_wide <= D")
        D = int(Cmat.shape[1])
        rows = []
        for st in steps:
            r = step_list(st)
            if len(r) not in (1, D):
                raise ValueError("rate_curve: every step must be a scalar or have D entries")
            rows.append(r * D if len(r) == 1 else r)
        if not rows:
            raise ValueError("rate_curve: no steps")
        k = len(rows)
        scalar = all(len(set(r)) == 1 for r in rows)
        order = self.order_RAGFT
        parts = []                                                   # (column range, coefficients in coded order)
        with torch.cuda.device(self.device):
            # the float32 transform runs over all D columns, as forward_quant_mixed's float32 launches do (tests/test_gpu_rate.py
            # holds the sizes to that path's integers exactly); transforming columns [n_wide, D) alone gives the same bits
            #  but needs a contiguous copy of them first, which moves what it saves: 3 of 59 columns for a frame
            if n_wide:
                Tw = self.forward(Cmat[:, :n_wide].to(torch.float64).contiguous(), want_w=False)
                Twq = torch.empty_like(Tw)
                rows_gather(Tw, order, Twq)
                parts.append((0, n_wide, Twq))
                del Tw
            if n_wide < D:
                T = self.forward(Cmat.to(torch.float32), want_w=False)
                Tq = torch.empty_like(T)
                rows_gather(T, order, Tq)
                parts.append((n_wide, D, Tq[:, n_wide:] if n_wide else Tq))
                del T
            payload = 0
            sse = torch.empty((k, D), dtype=torch.float64, device=self.device)
            G = 0
            for lo, hi, Tp in parts:
                st = [r[lo] for r in rows] if scalar else [r[lo:hi] for r in rows]
                nbytes, seg_bytes, e = SegmentedCoder.rate(Tp, st, seg_len, 1, True)
                Gp = seg_bytes.shape[1]
                payload = payload + (nbytes - SegmentedCoder.container_size(Gp, 0))     # (the padded streams of this part)
                G += Gp
                sse[:, lo:hi] = e
        return {"bytes": SegmentedCoder.container_size(G, payload), "sse": sse.cpu().numpy()}

    def mixed_stats(self, D=59, n_wide=3):
        """Tile rows and rows per stage of the mixed-precision schedule (tile_rows 0: the shape takes the two-pass path)."""
        tr, ns = C.c_int(0), C.c_int(0)
        rows = (C.c_int64 * 64)()
        with torch.cuda.device(self.device):
            check(_lib.lib().raht_plan_mixed_stats(self._h, int(D), int(n_wide), C.byref(tr), C.byref(ns), rows, 64))
        return {"tile_rows": tr.value, "rows_per_stage": [int(rows[i]) for i in range(ns.value)]}

    def quant_reorder(self, T, steps):
        """int32 Q[k] = floor(T[order[k]] / step + 0.5)  (encode_3dgs.py:204,210,215)."""
        T = _rows(T, None, "T")
        return self._quant_to("raht_quant_reorder", T, steps, torch.int32, T.dtype)

    def dequant_unreorder(self, Q, steps, dtype=torch.float32):
        """T[order[k]] = Q[k] * step  (encode_3dgs.py:261,267-268); float32, or float64 like the reference."""
        dtype = torch.float64 if dtype == torch.float64 else torch.float32
        return self._quant_to("raht_dequant_unreorder", _qmat(Q), steps, dtype, dtype)


# ---------------------------------------------------------------------------------------------------
# several scenes in one set of launches (include/raht.h: raht_*_batch)
# ---------------------------------------------------------------------------------------------------
def _batch_arrays(plans, mats, dtype, name):
    n = len(plans)
    if n < 1 or len(mats) != n:
        raise ValueError("batch: one matrix per plan")
    D = int(mats[0].shape[1])
    ms = []
    for p, m in zip(plans, mats):
        _need_cuda(m, name)
        if m.dim() != 2 or m.shape[0] != p.N or m.shape[1] != D:
            raise ValueError(f"batch: expected ({p.N}, {D}) matrices, got {tuple(m.shape)}")
        if m.dtype != dtype:
            m = m.to(dtype)
        if m.stride(1) != 1 or m.stride(0) < D:
            m = m.contiguous()
        ms.append(m)
    hp = (C.c_void_p * n)(*[p._h for p in plans])
    mp = (C.c_void_p * n)(*[m.data_ptr() for m in ms])
    ld = (C.c_int64 * n)(*[m.stride(0) for m in ms])
    return n, D, ms, hp, mp, ld


def _batch_out(plans, D, dtype, device):
    outs = [torch.empty((p.N, D), dtype=dtype, device=device) for p in plans]
    return outs, (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs]), (C.c_int64 * len(outs))(*[D] * len(outs))


@contextlib.contextmanager
def _batch_mixed_roots(plans, roots, roots_wide, D, n_wide):
    """the root buffers of every scene that brings some, set for the duration of a mixed batch call (one entry per scene, None
    allowed) and reset afterwards, also when setting one of them or the call itself raises"""
    n = len(plans)
    roots = [None] * n if roots is None else list(roots)
    wide = [None] * n if roots_wide is None else list(roots_wide)
    if len(roots) != n or len(wide) != n:
        raise ValueError("batch: roots / roots_wide need one entry per plan (None allowed)")
    with contextlib.ExitStack() as stack:
        for p, r, w in zip(plans, roots, wide):
            stack.enter_context(p._with_roots(D, r, torch.float32, w, n_wide))
        yield


def _batch(fn, plans, mats, dtype, name, out_dtype, steps=None, ctype=None, n_wide=None, roots=None, roots_wide=None):
    """one batch entry point: (n, plans, matrices, row strides, D, [steps, n_steps, [n_wide,]] outputs, their row strides);
    with ``n_wide`` (the mixed entries) under the scenes' root buffers"""
    n, D, ms, hp, mp, ld = _batch_arrays(plans, mats, dtype, name)
    mid = []
    if steps is not None:
        st = _step_array(steps, D, ctype)
        mid = [st, len(st)] if n_wide is None else [st, len(st), int(n_wide)]
    outs, op, old = _batch_out(plans, D, out_dtype, ms[0].device)
    with contextlib.nullcontext() if n_wide is None else _batch_mixed_roots(plans, roots, roots_wide, D, int(n_wide)):
        _call(fn, ms[0].device, n, hp, mp, ld, D, *mid, op, old)
    return outs


def forward_batch(plans, Cs):
    """[T_i] = forward RAHT of every scene (plans[i], Cs[i]) in one set of launches; float32."""
    return _batch(_lib.lib().raht_fwd_batch, plans, Cs, torch.float32, "C", torch.float32)


def inverse_batch(plans, Ts):
    return _batch(_lib.lib().raht_inv_batch, plans, Ts, torch.float32, "T", torch.float32)


def forward_quant_batch(plans, Cs, steps):
    """[Q_i] = forward RAHT + quantize + reorder of every scene in one set of launches (bit-identical to
    plans[i].forward_quant(Cs[i], steps))."""
    return _batch(_lib.lib().raht_fwd_quant_batch, plans, Cs, torch.float32, "C", torch.int32, steps, C.c_float)


def dequant_inverse_batch(plans, Qs, steps):
    return _batch(_lib.lib().raht_dequant_inv_batch, plans, Qs, torch.int32, "Q", torch.float32, steps, C.c_float)


def forward_quant_mixed_batch(plans, Cs, steps, n_wide=3, roots=None, roots_wide=None):
    """[Q_i] = ``plans[i].forward_quant_mixed(Cs[i], steps, n_wide)`` of every scene in one set of launches, bit for bit (the
    frames of a 59-column sequence: the reference's xyz integers and the batch's shared tail launches at once). roots /
    roots_wide: optional lists, one entry per scene (None allowed), with the meaning they have in ``forward_quant_mixed``; a
    scene with root buffers (a truncated plan needs them) runs through the single-scene call inside."""
    return _batch(_lib.lib().raht_fwd_quant_mixed_batch, plans, Cs, torch.float32, "C", torch.int32, steps, C.c_double, n_wide, roots,
                  roots_wide)


def dequant_inverse_mixed_batch(plans, Qs, steps, n_wide=3, roots=None, roots_wide=None):
    """[C_i] = ``plans[i].dequant_inverse_mixed(Qs[i], steps, n_wide)`` of every scene in one set of launches, bit for bit
    (counterpart of ``forward_quant_mixed_batch``; roots / roots_wide as there, read instead of written)."""
    return _batch(_lib.lib().raht_dequant_inv_mixed_batch, plans, Qs, torch.int32, "Q", torch.float32, steps, C.c_double, n_wide, roots,
                  roots_wide)


def mixed_batch_stats(plans, D, n_wide, inverse=False):
    """What a mixed batch of these plans launches (a dry run of the grouping; no transform kernel runs): tile launches, top-stage
    launches, and scenes that run through the single-scene call (two-pass shapes, truncated plans, plans with stage-0 events)."""
    n = len(plans)
    if n < 1:
        raise ValueError("batch: at least one plan")
    hp = (C.c_void_p * n)(*[p._h for p in plans])
    t, u, v = C.c_int(0), C.c_int(0), C.c_int(0)
    with torch.cuda.device(plans[0].device):
        check(_lib.lib().raht_mixed_batch_stats(n, hp, int(D), int(n_wide), 1 if inverse else 0, C.byref(t), C.byref(u), C.byref(v)))
    return {"tile_launches": t.value, "top_launches": u.value, "single_scene_calls": v.value}


def _quant_rows(X, steps, pos, Q, dtype):
    _need_cuda(X, "X")
    if X.shape[0] == 0:
        return Q
    if dtype == torch.float64 and X.dtype != dtype:
        raise ValueError("quant_rows_f64: X must be float64")           # (the float32 call casts)
    X = _rows(X, dtype, "X")
    n, D = X.shape
    st = _step_array(steps, D, _STEP_CTYPE[dtype])
    pos = pos.to(torch.int64).contiguous()
    if Q.dtype != torch.int32 or Q.stride(1) != 1:
        raise ValueError("Q must be an int32 matrix with contiguous rows")
    _call(_fn("raht_quant_rows", dtype), X.device, _p(X), X.stride(0), n, D, st, len(st), _p(pos), _p(Q), Q.stride(0))
    return Q


def _dequant_rows(Q, steps, pos, out, dtype):
    _need_cuda(Q, "Q")
    if Q.dtype != torch.int32 or Q.stride(1) != 1:
        raise ValueError("Q must be an int32 matrix with contiguous rows")
    D = Q.shape[1]
    st = _step_array(steps, D, _STEP_CTYPE[dtype])
    pos = pos.to(torch.int64).contiguous()
    X = torch.empty((pos.shape[0], D), dtype=dtype, device=Q.device) if out is None else out
    if X.dtype != dtype or tuple(X.shape) != (pos.shape[0], D) or (X.shape[0] > 0 and (X.stride(1) != 1 or X.stride(0) < D)):
        raise ValueError(f"out must be a {'float64' if dtype == torch.float64 else 'float32'} (n, D) tensor with contiguous rows")
    _call(_fn("raht_dequant_rows", dtype), Q.device, _p(Q), Q.stride(0), _p(pos), pos.shape[0], D, st, len(st), _p(X), max(X.stride(0), D))
    return X


def quant_rows(X, steps, pos, Q):
    """Q[pos[i], :] = floor(X[i, :] / step + 0.5) in place (X float32 (n, D), pos int64 (n,), Q int32). X and Q may be
    column slices of wider matrices (contiguous rows, any row stride)."""
    return _quant_rows(X, steps, pos, Q, torch.float32)


def dequant_rows(Q, steps, pos, out=None):
    """-> float32 (n, D): Q[pos[i], :] * step (written into ``out`` when given: a float32 (n, D) view with contiguous rows)."""
    return _dequant_rows(Q, steps, pos, out, torch.float32)


def quant_rows_f64(X, steps, pos, Q):
    """Q[pos[i], :] = floor(X[i, :] / step + 0.5) in place, in float64 (X float64 (n, D), float64 steps, IEEE double
    division: the reference's arithmetic, python/encode_3dgs.py:204)."""
    return _quant_rows(X, steps, pos, Q, torch.float64)


def dequant_rows_f64(Q, steps, pos, out=None):
    """-> float64 (n, D): Q[pos[i], :] * step in float64 (written into ``out`` when given: a float64 (n, D) view with contiguous rows)."""
    return _dequant_rows(Q, steps, pos, out, torch.float64)


def sqdiff_columns(A, B):
    """-> float64 (D,) device tensor: the per-column sums of (A - B)^2 of two float32 or two float64 (N, D) matrices with
    contiguous rows, in one pass (raht_sqdiff_columns; differences in the matrices' own type, sums in float64)."""
    _need_cuda(A, "A")
    N, D = A.shape
    out = torch.empty(D, dtype=torch.float64, device=A.device)
    _call(_lib.lib().raht_sqdiff_columns, A.device, _p(A), A.stride(0), _p(B), B.stride(0), N, D, _VDT[A.dtype], _p(out))
    return out


def _rows_move(fn, src, pos, dst):
    _need_cuda(src, "src")
    if pos.shape[0] == 0:                     # nothing to move (an empty rank of a sharded scene); empty tensors have no strides to check
        return dst
    if src.dtype != dst.dtype or src.dtype not in (torch.float32, torch.float64, torch.int32) or src.stride(1) != 1 or dst.stride(1) != 1:
        raise ValueError("rows: float32 / float64 / int32 matrices with contiguous rows of one dtype")
    if pos.dtype != torch.int64 or not pos.is_contiguous():
        pos = pos.to(torch.int64).contiguous()
    with torch.cuda.device(src.device):
        check(fn(C.c_void_p(src.data_ptr()), src.stride(0), C.c_void_p(pos.data_ptr()), pos.shape[0], src.shape[1],
                 src.element_size(), C.c_void_p(dst.data_ptr()), dst.stride(0), _stream()))
    return dst


def rows_gather(src, pos, out):
    """out[i, :] = src[pos[i], :] in one launch (pos int64 (n,))."""
    return _rows_move(_lib.lib().raht_rows_gather, src, pos, out)


def rows_scatter(src, pos, out):
    """out[pos[i], :] = src[i, :] in one launch."""
    return _rows_move(_lib.lib().raht_rows_scatter, src, pos, out)


# ---------------------------------------------------------------------------------------------------
# plan tokens: what RAHT_param hands back in place of the reference's List / Flags / weights
# ---------------------------------------------------------------------------------------------------
def _token(plan):
    t = torch.tensor([_MAGIC, plan.id], dtype=torch.int64, device=plan.device)
    t._raht_plan = plan
    return t


def plan_of(lst):
    """Recover the RahtPlan from what the driver passes back as List (or Flags / weights)."""
    if isinstance(lst, RahtPlan):
        return lst
    tok = lst[0] if isinstance(lst, (list, tuple)) else lst
    p = getattr(tok, "_raht_plan", None)
    if p is not None:
        return p
    if isinstance(tok, torch.Tensor) and tok.numel() == 2 and tok.dtype == torch.int64:
        magic, pid = tok.cpu().tolist()          # token was copied: fall back to its contents
        if magic == _MAGIC and pid in _plans:
            return _plans[pid]
    raise RuntimeError("raht-3dgs-codec_amd: List/Flags/weights must be the plan tokens returned by "
                       "RAHT_param_reorder_fast of this package (reference-shaped lists are not accepted; "
                       "build the plan from V with RAHT_param_reorder_fast)")


@torch.no_grad()
def RAHT_param_reorder_fast(V, minV, width, depth):
    """Drop-in for reference python/RAHT_param.py:190-279 (call site encode_3dgs.py:149).

    V: (N, 3) tensor holding integer voxel coordinates, Morton-sorted, unique, on the GPU.
    Returns (List, Flags, weights, order_RAGFT); the three lists hold one opaque plan token each.
    """
    plan = RahtPlan.from_coords(V, minV, width, depth)
    _plans[plan.id] = plan
    while len(_plans) > _PLAN_CACHE:
        _plans.popitem(last=False)
    return [_token(plan)], [_token(plan)], [_token(plan)], plan.order_RAGFT


@torch.no_grad()
def RAHT2_optimized(Cmat, List, Flags, weights, one_based=False):
    """Drop-in for reference python/RAHT.py:252-336 (call site encode_3dgs.py:159). Returns (T, w)."""
    if one_based:
        raise ValueError("one_based lists are a MATLAB convention; plan tokens are index-free")
    return plan_of(List).forward(Cmat, want_w=True)


@torch.no_grad()
def inverse_RAHT_optimized(T, List, Flags, weights, one_based=False):
    """Drop-in for reference python/iRAHT.py:40-114 (call site encode_3dgs.py:274). Returns C."""
    if one_based:
        raise ValueError("one_based lists are a MATLAB convention; plan tokens are index-free")
    return plan_of(List).inverse(T)


raht_fn = {
    "RAHT": RAHT2_optimized,
    "iRAHT": inverse_RAHT_optimized,
    "RAHT_param": RAHT_param_reorder_fast,
}


# ---------------------------------------------------------------------------------------------------
# voxelizer (reference python/voxelize_pc.py)
# ---------------------------------------------------------------------------------------------------
@torch.no_grad()
def get_morton_code(V, J):
    """Drop-in for reference python/voxelize_pc.py:25-59. V: (N, 3) integer tensor on the GPU."""
    _need_cuda(V, "V")
    V = V.to(torch.int64).contiguous()
    out = torch.empty(V.shape[0], dtype=torch.int64, device=V.device)
    with torch.cuda.device(V.device):
        check(_lib.lib().raht_morton(C.c_void_p(V.data_ptr()), V.shape[0], int(J), C.c_void_p(out.data_ptr()),
                                     _stream()))
    return out


@torch.no_grad()
def demorton(keys, J):
    """Inverse of ``get_morton_code``: (N,) int64 / uint64 Morton keys on the GPU -> (N, 3) int64 voxel coordinates."""
    _need_cuda(keys, "keys")
    if keys.dtype not in (torch.int64, torch.uint64) or keys.dim() != 1:
        raise ValueError("keys must be a 1-D int64/uint64 tensor")
    k = keys.contiguous()
    out = torch.empty((k.shape[0], 3), dtype=torch.int64, device=k.device)
    with torch.cuda.device(k.device):
        check(_lib.lib().raht_demorton(C.c_void_p(k.data_ptr()), k.shape[0], int(J), C.c_void_p(out.data_ptr()), _stream()))
    return out


REGION_BUCKETS = 22                                          # RAHT_REGION_BUCKETS


def _region_keys(keys, what):
    _need_cuda(keys, "keys")
    if keys.dtype not in (torch.int64, torch.uint64) or keys.dim() != 1 or keys.shape[0] < 1:
        raise ValueError(f"{what}: keys must be a non-empty 1-D int64/uint64 tensor")
    return keys.contiguous()


@torch.no_grad()
def region_layout(keys_sorted, nbits, row_lo, row_hi):
    """-> (3, 22) int64 device tensor: rows per bucket (a row's bucket: msb(key[i] ^ key[i-1]) / 3, row 0: 21) in the whole frame,
    in [0, row_lo) and in [row_lo, row_hi) (raht_region_layout). Enqueued only."""
    k = _region_keys(keys_sorted, "region_layout")
    table = torch.empty((3, REGION_BUCKETS), dtype=torch.int64, device=k.device)
    with torch.cuda.device(k.device):
        check(_lib.lib().raht_region_layout(C.c_void_p(k.data_ptr()), k.shape[0], int(nbits), int(row_lo), int(row_hi),
                                            C.c_void_p(table.data_ptr()), _stream()))
    return table


@torch.no_grad()
def region_cells(keys_sorted, nbits, top_level, n_cells):
    """The occupied cells of the octree level ``top_level / 3`` bits above the voxels -> (cell_keys (n_cells,) int64: key >>
    top_level, cell_first (n_cells + 1,) int64: every cell's first row, then N) on the keys' device (raht_region_cells).
    ``n_cells``: how many there must be (a geometry header's level count); ``RahtError`` when the keys hold another number.
    Synchronises."""
    k = _region_keys(keys_sorted, "region_cells")
    n_cells = int(n_cells)
    if n_cells < 1:
        raise ValueError("region_cells: n_cells must be at least 1")
    cell_keys = torch.empty(n_cells, dtype=torch.int64, device=k.device)
    cell_first = torch.empty(n_cells + 1, dtype=torch.int64, device=k.device)
    with torch.cuda.device(k.device):
        check(_lib.lib().raht_region_cells(C.c_void_p(k.data_ptr()), k.shape[0], int(nbits), int(top_level), n_cells,
                                           C.c_void_p(cell_keys.data_ptr()), C.c_void_p(cell_first.data_ptr()), _stream()))
    return cell_keys, cell_first


@torch.no_grad()
def region_assemble(src, runs, n_dst_rows):
    """-> (n_dst_rows, D) int32: the runs ``(src_row, dst_row, count)`` (at most 22, destinations ascending and disjoint) of rows of
    the int32 matrix ``src``, every other row 0, in one launch (raht_region_assemble)."""
    _need_cuda(src, "src")
    if src.dtype != torch.int32 or src.dim() != 2 or src.stride(1) != 1 or src.shape[0] < 1:
        raise ValueError("region_assemble: src must be a non-empty int32 matrix with contiguous rows")
    D = int(src.shape[1])
    dst = torch.empty((int(n_dst_rows), D), dtype=torch.int32, device=src.device)
    flat = [int(x) for r in runs for x in r]
    arr = (C.c_int64 * max(len(flat), 1))(*flat)
    with torch.cuda.device(src.device):
        check(_lib.lib().raht_region_assemble(C.c_void_p(src.data_ptr()), src.stride(0), src.shape[0], C.c_void_p(dst.data_ptr()), D,
                                              int(n_dst_rows), D, arr, len(flat) // 3, _stream()))
    return dst


REGION_MAX_RANGES = 512                                      # RAHT_REGION_MAX_RANGES


@torch.no_grad()
def region_layout_set(keys_sorted, nbits, row_bounds):
    """``region_layout`` for R row ranges in one pass over the keys (raht_region_layout_set). row_bounds: (2 R,) int64 on the keys'
    device, lo_0, hi_0, lo_1, ... ascending, R <= 512 -> (1 + 2 R, 22) int64 device tensor: rows per bucket in the whole frame, then
    per range in [0, lo_r) and in [lo_r, hi_r). With R = 1 it is ``region_layout``'s table. Enqueued only."""
    k = _region_keys(keys_sorted, "region_layout_set")
    _need_cuda(row_bounds, "row_bounds")
    if row_bounds.dtype != torch.int64 or row_bounds.dim() != 1 or row_bounds.shape[0] % 2 or row_bounds.device != k.device:
        raise ValueError("region_layout_set: row_bounds must be a 1-D int64 tensor of 2 R entries on the keys' device")
    R = int(row_bounds.shape[0]) // 2
    if not 1 <= R <= REGION_MAX_RANGES:
        raise ValueError(f"region_layout_set: 1 .. {REGION_MAX_RANGES} ranges")
    rb = row_bounds.contiguous()
    table = torch.empty((1 + 2 * R, REGION_BUCKETS), dtype=torch.int64, device=k.device)
    _call(_lib.lib().raht_region_layout_set, k.device, _p(k), k.shape[0], int(nbits), _p(rb), R, _p(table))
    return table


@torch.no_grad()
def region_assemble_set(src, runs, n_dst_rows):
    """``region_assemble`` with any number of runs up to 22 * 512 (raht_region_assemble_set). runs: ``(src_row, dst_row, count)``
    triples, destinations ascending and disjoint -- as a host list or array they are checked here (``RahtError`` for a run that
    leaves a matrix or overlaps the one before it) and uploaded; as a (n, 3) int64 tensor on ``src``'s device they are the caller's
    word, and the kernel clamps every source row into ``src``. -> (n_dst_rows, D) int32, rows no run covers 0. One launch."""
    import numpy as np
    _need_cuda(src, "src")
    if src.dtype != torch.int32 or src.dim() != 2 or src.stride(1) != 1 or src.shape[0] < 1:
        raise ValueError("region_assemble_set: src must be a non-empty int32 matrix with contiguous rows")
    D = int(src.shape[1])
    if isinstance(runs, torch.Tensor) and runs.is_cuda:
        if runs.dtype != torch.int64 or runs.dim() != 2 or runs.shape[1] != 3 or runs.device != src.device:
            raise ValueError("region_assemble_set: a device table is (n, 3) int64 on src's device")
        table, host = runs.contiguous(), None
    else:
        flat = np.ascontiguousarray(np.asarray(runs, np.int64).reshape(-1, 3))
        host = flat.ctypes.data_as(C.POINTER(C.c_int64))
        table = torch.from_numpy(flat).to(src.device)
    dst = torch.empty((int(n_dst_rows), D), dtype=torch.int32, device=src.device)
    _call(_lib.lib().raht_region_assemble_set, src.device, _p(src), src.stride(0), src.shape[0], _p(dst), D, int(n_dst_rows), D,
          C.c_void_p(table.data_ptr()) if table.shape[0] else None, host, int(table.shape[0]))
    return dst


@torch.no_grad()
def region_needs(keys, J, top_level, up, block_first=None, mv=None, block_log2=0, capacity=None):
    """The cells, ``top_level / 3`` octree levels above the voxels, of a reference frame that the predictor of the rows ``keys``
    (strictly ascending int64 Morton keys on the GPU) reaches into (raht_region_needs) -> (n,) int64 on the device,
    ascending and without repeats: ``k' >> top_level`` of every row with a match, k' the row's key shifted by the vector of its
    block (mv (n_blocks, 3) int8, block_first (n_blocks + 1,) int64 rows of ``keys``, as ``predict_mc`` takes them), or the key
    itself without a field. Where ``3 up > top_level`` an entry is the first cell of the aligned group of cells that the
    ``up``-cell covers; widening it to the group is the caller's. ``capacity``: the entries the result may have (default: as many
    as there can be); ``RahtError`` for more. Synchronises."""
    J, tl, up = int(J), int(top_level), int(up)
    if mv is None:
        k = _region_keys(keys, "region_needs")
        bf, field, n_blocks, m = None, None, 0, 0
    else:
        k, J, m = _motion_frame("region_needs", keys, J, block_log2)
        _need_cuda(block_first, "block_first")
        _need_cuda(mv, "mv")
        if block_first.dtype != torch.int64 or block_first.dim() != 1 or not 2 <= block_first.shape[0] <= k.shape[0] + 1:
            raise ValueError("region_needs: block_first must hold n_blocks + 1 int64 rows, 1 <= n_blocks <= N")
        n_blocks = int(block_first.shape[0]) - 1
        if mv.dtype != torch.int8 or tuple(mv.shape) != (n_blocks, 3):
            raise ValueError(f"region_needs: mv must be a ({n_blocks}, 3) int8 tensor")
        bf, field = block_first.contiguous(), mv.contiguous()
    if capacity is None:
        capacity = min(int(k.shape[0]), 8 ** max(J - tl // 3, 0))
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError("region_needs: capacity must be at least 1")
    cells = torch.empty(capacity, dtype=torch.int64, device=k.device)
    n = C.c_int64(0)
    _call(_lib.lib().raht_region_needs, k.device, _p(k), k.shape[0], J, tl, up, _p(bf), n_blocks, _p(field), m, _p(cells), capacity,
          C.byref(n))
    return cells[: n.value]


@torch.no_grad()
def region_needs_bi(keys, J, top_level, up, block_first=None, mv0=None, mv1=None, modes=None, block_log2=0, capacity=None):
    """``region_needs`` for the two references of a B frame from one pass over the keys (raht_region_needs_bi) ->
    (cells0, cells1), each (n_r,) int64 on the device, ascending and without repeats: ``region_needs``' entries for reference r
    under the field ``mv_r``, over the rows whose block's mode uses that reference -- 0: both, 1: reference 0 alone, 2: reference 1
    alone, 3 (or any byte above it): neither. mv0, mv1: (n_blocks, 3) int8, modes: (n_blocks,) uint8, on the device, each may be None
    (a zero field; every block in mode 0); block_first ((n_blocks + 1,) int64 rows of ``keys``) and ``block_log2`` are needed as soon
    as one of them is given. ``capacity``: the entries either list may have (default: as many as there can be); ``RahtError`` for
    more. Synchronises."""
    who = "region_needs_bi"
    J, tl, up = int(J), int(top_level), int(up)
    given = [t for t in (mv0, mv1, modes) if t is not None]
    if not given:
        k = _region_keys(keys, who)
        bf, n_blocks, m = None, 0, 0
    else:
        k, J, m = _motion_frame(who, keys, J, block_log2)
        if block_first is None:
            raise ValueError(f"{who}: a motion field or modes need block_first and block_log2")
        _need_cuda(block_first, "block_first")
        if block_first.dtype != torch.int64 or block_first.dim() != 1 or not 2 <= block_first.shape[0] <= k.shape[0] + 1:
            raise ValueError(f"{who}: block_first must hold n_blocks + 1 int64 rows, 1 <= n_blocks <= N")
        n_blocks = int(block_first.shape[0]) - 1
        for name, t in (("mv0", mv0), ("mv1", mv1)):
            if t is not None:
                _need_cuda(t, name)
                if t.dtype != torch.int8 or tuple(t.shape) != (n_blocks, 3) or t.device != k.device:
                    raise ValueError(f"{who}: {name} must be a ({n_blocks}, 3) int8 tensor on the keys' device")
        if modes is not None:
            _need_cuda(modes, "modes")
            if modes.dtype != torch.uint8 or tuple(modes.shape) != (n_blocks,) or modes.device != k.device:
                raise ValueError(f"{who}: modes must be a ({n_blocks},) uint8 tensor on the keys' device")
        if block_first.device != k.device:
            raise ValueError(f"{who}: block_first must lie on the keys' device")
        bf = block_first.contiguous()
    f0, f1, md = (None if t is None else t.contiguous() for t in (mv0, mv1, modes))
    if capacity is None:
        capacity = min(int(k.shape[0]), 8 ** max(J - tl // 3, 0))
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError(f"{who}: capacity must be at least 1")
    cells = torch.empty((2, capacity), dtype=torch.int64, device=k.device)
    n = (C.c_int64 * 2)(0, 0)
    _call(_lib.lib().raht_region_needs_bi, k.device, _p(k), k.shape[0], J, tl, up, _p(bf), n_blocks, m, _p(f0), _p(f1), _p(md), _p(cells[0]),
          _p(cells[1]), capacity, n)
    return cells[0, : n[0]], cells[1, : n[1]]


def _predict_rows(M, n_rows, D, name):
    """a float32 CUDA matrix of the predictor, as it is: (n_rows, D), unit column stride, a row stride of at least D"""
    _need_cuda(M, name)
    if M.dtype != torch.float32 or M.dim() != 2 or tuple(M.shape) != (n_rows, D) or M.stride(1) != 1 or M.stride(0) < D:
        raise ValueError(f"predict: {name} must be a ({n_rows}, {D}) float32 matrix with contiguous rows")
    return M


def _inter_args(who, keys, ref_keys, C_ref, up, X, blocks=None, result=None):
    """What ``predict``, ``predict_mc`` and ``motion_search`` take in common, checked (``who`` opens a refusal) -> (device, the
    entry point's arguments from the keys on, the tensors behind them -- to be held until the call is made --, out, matched).
    blocks: (J, block_log2, block_first) of ``motion_search``, with mv as a fourth of ``predict_mc``. result: (add, out,
    want_matched) of the two predictors, whose arguments end with out and matched; without it X is required and they end with D."""
    if blocks is None:
        k = _region_keys(keys, who)
    else:
        k, J, m = _motion_frame(who, keys, blocks[0], blocks[1])
    r = _region_keys(ref_keys, who)
    up = int(up)
    if not 0 <= up <= 3:
        raise ValueError(f"{who}: up must be 0 .. 3")
    _need_cuda(C_ref, "C_ref")
    if C_ref.dim() != 2:
        raise ValueError(f"{who}: C_ref must be a matrix")
    N, D = int(k.shape[0]), int(C_ref.shape[1])
    C_ref = _predict_rows(C_ref, int(r.shape[0]), D, "C_ref")
    live, args = [k, r, C_ref], [_p(k), N]
    if blocks is not None:
        _need_cuda(blocks[2], "block_first")
        if blocks[2].dtype != torch.int64 or blocks[2].dim() != 1 or not 2 <= blocks[2].shape[0] <= N + 1:
            raise ValueError(f"{who}: block_first must hold n_blocks + 1 int64 rows, 1 <= n_blocks <= N")
        bf, n_blocks = blocks[2].contiguous(), int(blocks[2].shape[0]) - 1
        live, args = live + [bf], args + [J, m, _p(bf), n_blocks]
        if len(blocks) > 3:
            _need_cuda(blocks[3], "mv")
            if blocks[3].dtype != torch.int8 or tuple(blocks[3].shape) != (n_blocks, 3):
                raise ValueError(f"{who}: mv must be a ({n_blocks}, 3) int8 tensor")
            live.append(blocks[3].contiguous())
            args.append(_p(live[-1]))
    add, out, want_matched = result or (False, None, False)
    if X is not None or result is None:
        X = _predict_rows(X, N, D, "X")
        live.append(X)
    elif add:
        raise ValueError(f"{who}: add needs X")
    args += [_p(r), int(r.shape[0]), 3 * up, _p(C_ref), C_ref.stride(0), _p(X), 0 if X is None else X.stride(0), D]
    matched = torch.empty(1, dtype=torch.int64, device=k.device) if want_matched else None
    if result is not None:
        out = torch.empty((N, D), dtype=torch.float32, device=k.device) if out is None else _predict_rows(out, N, D, "out")
        live.append(out)
        args += [int(bool(add)), _p(out), out.stride(0), _p(matched)]
    if len({t.device for t in live}) != 1:
        raise ValueError(f"{who}: all tensors must be on one device")
    return k.device, args, live, out, matched


@torch.no_grad()
def predict(keys, ref_keys, C_ref, X=None, up=0, add=False, out=None, want_matched=False):
    """The inter-frame predictor (raht_predict). keys (N,), ref_keys (N_ref,): the sorted int64 Morton keys of the frame
    and of its reference, as ``get_morton_code`` returns them; C_ref: (N_ref, D) float32, the reference's reconstruction. P[i] is the
    mean of the reference rows in the cell ``keys[i] >> 3 up`` (summed in row order in float32, divided once; 0 where the cell is
    empty; ``up = 0``: the co-located voxel's row). -> P when ``X`` is None, X - P, or X + P with ``add``; into ``out`` when given
    (``out`` may be ``X``: in place). Column slices of wider matrices pass as they are. ``want_matched``: -> (result, n_matched), a
    (1,) int64 device tensor with the number of rows whose cell is not empty. Enqueued only."""
    dev, args, _live, out, matched = _inter_args("predict", keys, ref_keys, C_ref, up, X, result=(add, out, want_matched))
    _call(_lib.lib().raht_predict, dev, *args)
    return (out, matched) if want_matched else out


# ---- motion compensation (raht_motion_search / raht_predict_mc) -----------------------------------------------------
MOTION_MAX_CANDIDATES = 512


def motion_candidates(radius):
    """-> (K, 3) int32 numpy: every vector of [-radius, radius]^3, radius 1 .. 3, sorted by (dx^2 + dy^2 + dz^2, dx, dy, dz). Index 0
    is (0, 0, 0), and the search gives a tie to the smaller index: to no motion first, to a shorter vector before a longer one."""
    import numpy as np
    r = int(radius)
    if not 1 <= r <= 3:
        raise ValueError("motion_candidates: radius must be 1 .. 3")
    rng = range(-r, r + 1)
    return np.array(sorted(((x, y, z) for x in rng for y in rng for z in rng), key=lambda v: (v[0] ** 2 + v[1] ** 2 + v[2] ** 2,) + v),
                    np.int32)


def _motion_frame(who, keys, J, block_log2):
    k = _region_keys(keys, who)
    J, m = int(J), int(block_log2)
    if not 1 <= J <= 21 or not 1 <= m <= J:
        raise ValueError(f"{who}: J must be 1 .. 21 and block_log2 1 .. J")
    return k, J, m


@torch.no_grad()
def motion_blocks(keys, J, block_log2, n_blocks):
    """-> block_first (n_blocks + 1,) int64 on the keys' device: the first row of every occupied block (a cell of the octree level
    ``block_log2`` above the voxels: ``key >> 3 block_log2``), ascending, then N. ``n_blocks``: the level count n_(J - block_log2)
    of the frame's geometry header; ``RahtError`` when the keys hold another number. This is ``region_cells``' cell walk (one block,
    ``block_log2 == J``, needs none). Synchronises."""
    k, J, m = _motion_frame("motion_blocks", keys, J, block_log2)
    if m == J:
        if int(n_blocks) != 1:
            raise ValueError("motion_blocks: block_log2 == J is one block")
        return torch.tensor([0, k.shape[0]], dtype=torch.int64, device=k.device)
    return region_cells(k, 3 * J, 3 * m, n_blocks)[1]


@torch.no_grad()
def motion_search(keys, ref_keys, C_ref, X, J, block_log2, block_first, candidates, weights, up=0, want_table=False):
    """Block motion search (raht_motion_search): for every block of the frame, the candidate vector under which the
    reference predicts the rows of ``X`` best. keys / ref_keys / C_ref / ``up``: as ``predict`` takes them; X: (N, D) float32;
    block_first: ``motion_blocks``; candidates: (K, 3) integers within +-127, K <= 512 (``motion_candidates``); weights: D finite
    floats >= 0 (checked here, on the host), a column of weight 0 is left out. The cost of a row under a vector v is
    sum_ch w[ch] |X[i, ch] - P_v[i, ch]| in float32 (channels ascending, product rounded before the sum), capped at 2^20 and taken
    to 2^-10 fixed point; a block's cost is the integer sum over its rows; the smallest cost wins, the smallest index among equals.
    -> (mv (n_blocks, 3) int8, best_cost (n_blocks,) int64[, table (n_blocks, K) int64]) on the device; v points from the voxel to
    its reference voxel. Enqueued only, but for the first call with a given table of candidates or weights on a device, which sends
    the table up with a blocking copy and so waits for the current stream (``_device_table``)."""
    dev, args, _live, _, _ = _inter_args("motion_search", keys, ref_keys, C_ref, up, X, blocks=(J, block_log2, block_first))
    n_blocks = int(block_first.shape[0]) - 1
    cand_d, w_d, K = _search_host_args("motion_search", candidates, weights, int(C_ref.shape[1]), dev)
    best_k = torch.empty(n_blocks, dtype=torch.int32, device=dev)
    best_cost = torch.empty(n_blocks, dtype=torch.int64, device=dev)
    table = torch.empty((n_blocks, K), dtype=torch.int64, device=dev) if want_table else None
    _call(_lib.lib().raht_motion_search, dev, *args, _p(w_d), _p(cand_d), K, _p(best_k), _p(best_cost), _p(table))
    mv = cand_d.to(torch.int8)[best_k.long()]
    return (mv, best_cost, table) if want_table else (mv, best_cost)


_TABLE_CACHE = {}


def _device_table(a, dev):
    """a small host table (the candidates or the weights of a search) as a device tensor. The upload is a blocking copy, which waits
    for everything the caller has queued on the current stream; a search is made with the same few tables frame after frame, so the
    copy is made once per (device, table) -- as ``_vmin_tensor`` keeps a bounding box -- and every later call with that table only
    enqueues. The tensor handed out is shared and read-only."""
    key = (str(dev), a.dtype.str, a.shape, a.tobytes())
    t = _TABLE_CACHE.get(key)
    if t is None:
        if len(_TABLE_CACHE) > 64:
            _TABLE_CACHE.clear()
        t = _TABLE_CACHE[key] = torch.from_numpy(a).to(dev)
    return t


def _search_host_args(who, candidates, weights, D, dev):
    """the candidates and weights of a search, checked on the host -> (cand (K, 3) int32, weights (D,) float32 on ``dev``, K)"""
    import numpy as np
    cand = np.asarray(candidates)
    if cand.ndim != 2 or cand.shape[1] != 3 or not 1 <= cand.shape[0] <= MOTION_MAX_CANDIDATES or cand.dtype.kind not in "iu":
        raise ValueError(f"{who}: candidates must be (K, 3) integers, 1 <= K <= {MOTION_MAX_CANDIDATES}")
    if np.abs(cand.astype(np.int64)).max() > 127:
        raise ValueError(f"{who}: a candidate outside +-127 (a vector is stored as int8)")
    return _device_table(np.ascontiguousarray(cand, np.int32), dev), _search_weights(who, weights, D, dev), int(cand.shape[0])


def _search_weights(who, weights, D, dev):
    """the weights of a search, checked on the host -> (D,) float32 on ``dev`` (weights given as a device tensor come to the host
    first, which waits for the stream: pass host numbers to a call that must only enqueue)"""
    import numpy as np
    w = np.ascontiguousarray(np.asarray(weights.detach().cpu() if isinstance(weights, torch.Tensor) else weights, np.float32).reshape(-1))
    if w.shape[0] != D or not bool(np.all(np.isfinite(w) & (w >= 0))):
        raise ValueError(f"{who}: weights must be D finite numbers >= 0")
    return _device_table(w, dev)


# ---- hierarchical motion search (raht_motion_search_around) -------------------------------------------------------------
MOTION_MAX_LEVELS = 3


@torch.no_grad()
def motion_search_around(keys, ref_keys, C_ref, X, J, block_log2, block_first, base, candidates, weights, up=0, want_table=False):
    """``motion_search`` around a base (raht_motion_search_around). base: (n_blocks, 3) int8 on the device; the vector
    of the pair (block b, candidate k) is ``base[b] + candidates[k]``, and its cost is ``motion_search``'s under that vector. A pair
    with a component outside +-127 is invalid: its table entry is -1 (2^64 - 1) and it is never chosen. -> (mv (n_blocks, 3) int8:
    base + the chosen candidate, written by the library; best_cost (n_blocks,) int64; best_k (n_blocks,) int32: the smallest k among
    the valid pairs of the smallest cost[, table (n_blocks, K) int64]). A block with no valid pair has best_k = -1, best_cost = -1
    and mv = 0. With a zero base the table and the choice are ``motion_search``'s. Enqueued only, as ``motion_search`` is: but for
    the first call with a given table."""
    who = "motion_search_around"
    dev, args, _live, _, _ = _inter_args(who, keys, ref_keys, C_ref, up, X, blocks=(J, block_log2, block_first))
    n_blocks = int(block_first.shape[0]) - 1
    _need_cuda(base, "base")
    if base.dtype != torch.int8 or tuple(base.shape) != (n_blocks, 3) or base.device != dev:
        raise ValueError(f"{who}: base must be a ({n_blocks}, 3) int8 tensor on the keys' device")
    base = base.contiguous()
    cand_d, w_d, K = _search_host_args(who, candidates, weights, int(C_ref.shape[1]), dev)
    best_k = torch.empty(n_blocks, dtype=torch.int32, device=dev)
    best_cost = torch.empty(n_blocks, dtype=torch.int64, device=dev)
    mv = torch.empty((n_blocks, 3), dtype=torch.int8, device=dev)
    table = torch.empty((n_blocks, K), dtype=torch.int64, device=dev) if want_table else None
    _call(_lib.lib().raht_motion_search_around, dev, *args, _p(w_d), _p(base), _p(cand_d), K, _p(best_k), _p(best_cost), _p(mv), _p(table))
    return (mv, best_cost, best_k, table) if want_table else (mv, best_cost, best_k)


def _level_counts(who, k, J, levels, counts):
    """the number of occupied cells at depth J - l for l = 1 .. levels: from ``counts`` (a geometry header's level counts, indexed
    by depth 0 .. J), or counted from the keys (which synchronises)"""
    if counts is None:
        return [int(torch.unique_consecutive(k >> (3 * l)).numel()) for l in range(1, levels + 1)]
    if len(counts) != J + 1:
        raise ValueError(f"{who}: counts must hold the J + 1 level counts of the frame")
    return [int(counts[J - l]) for l in range(1, levels + 1)]


def _hier_levels(who, J, block_log2, levels):
    J, L = int(J), int(levels)
    if not 0 <= L <= MOTION_MAX_LEVELS or J - L < 1 or (block_log2 is not None and L > int(block_log2) - 1):
        raise ValueError(f"{who}: levels must be 0 .. min({MOTION_MAX_LEVELS}, block_log2 - 1) with J - levels >= 1")
    return J, L


@torch.no_grad()
def motion_pyramid(keys, C, J, levels, counts=None):
    """The coarse levels of a frame for the hierarchical search -> per level l = 1 .. ``levels`` (keys_l (n_l,) int64:
    the distinct values of ``keys >> 3 l``, ascending -- keys of depth J - l --, C_l (n_l, D) float32: the mean of ``C`` over the rows
    of every cell, as ``predict`` forms it: summed in row order in float32, divided once). counts: the frame's level counts (a
    geometry header's, indexed by depth 0 .. J); None: counted from the keys. The cell walk is ``region_cells``, the means are
    ``predict(keys_l << 3 l, keys, C, up=l)``. Synchronises."""
    who = "motion_pyramid"
    k = _region_keys(keys, who)
    J, L = _hier_levels(who, J, None, levels)
    if k.dtype == torch.uint64:
        k = k.view(torch.int64)
    out = []
    for l, n_l in zip(range(1, L + 1), _level_counts(who, k, J, L, counts)):
        cells = region_cells(k, 3 * J, 3 * l, n_l)[0]
        out.append((cells, predict(cells << (3 * l), k, C, up=l)))
    return out


@torch.no_grad()
def motion_search_hier(keys, ref_keys, C_ref, X, J, block_log2, block_first, levels, radius, weights, up=0, counts=None, ref_counts=None,
                       ref_pyramid=None):
    """Coarse-to-fine block motion search. With L = ``levels`` (0 .. min(3, block_log2 - 1), J - L >= 1) and r =
    ``radius`` (1 .. 3): level L of both frames (``motion_pyramid``) is searched with ``motion_candidates(r)`` and ``up = 0``; then
    every level l below it is searched around twice the vectors of level l + 1 with ``motion_candidates(1)`` -- ``up = 0`` above
    level 0, the caller's ``up`` at level 0. The frame's blocks are the same cells at every level (block_log2 - l at level l). The
    reach is r 2^L + 2^L - 1 voxels; ``levels = 0`` is ``motion_search``. counts / ref_counts: the level counts of the frame and of
    the reference (None: counted from the keys). ref_pyramid: ``info["ref_pyramid"]`` of an earlier call against the same reference,
    which is then not built again. -> (mv (n_blocks, 3) int8, best_cost (n_blocks,) int64 -- of level 0 --, info: "mv": the vectors
    per level 0 .. L, "pyramid" and "ref_pyramid": the levels 1 .. L of the frame and of the reference). Synchronises when L > 0."""
    who = "motion_search_hier"
    J, L = _hier_levels(who, J, block_log2, levels)
    m, top = int(block_log2), motion_candidates(radius)
    if L == 0:
        mv, cost = motion_search(keys, ref_keys, C_ref, X, J, m, block_first, top, weights, up=up)
        return mv, cost, dict(mv=[mv], pyramid=[], ref_pyramid=[])
    n_blocks = int(block_first.shape[0]) - 1
    pyramid = motion_pyramid(keys, X, J, L, counts)
    if ref_pyramid is None:
        ref_pyramid = motion_pyramid(ref_keys, C_ref, J, L, ref_counts)
    elif len(ref_pyramid) != L:
        raise ValueError(f"{who}: ref_pyramid must hold the levels 1 .. {L} of the reference")
    cur, ref = [(keys, X)] + list(pyramid), [(ref_keys, C_ref)] + list(ref_pyramid)
    firsts = [block_first] + [motion_blocks(cur[l][0], J - l, m - l, n_blocks) for l in range(1, L + 1)]
    mv, cost = motion_search(cur[L][0], ref[L][0], ref[L][1], cur[L][1], J - L, m - L, firsts[L], top, weights, up=0)
    per_level, around = [mv], motion_candidates(1)
    for l in range(L - 1, -1, -1):
        mv, cost, _ = motion_search_around(cur[l][0], ref[l][0], ref[l][1], cur[l][1], J - l, m - l, firsts[l], mv * 2, around, weights,
                                           up=up if l == 0 else 0)
        per_level.insert(0, mv)
    return mv, cost, dict(mv=per_level, pyramid=pyramid, ref_pyramid=ref_pyramid)


@torch.no_grad()
def predict_mc(keys, ref_keys, C_ref, mv, block_first, J, block_log2, X=None, up=0, add=False, out=None, want_matched=False):
    """The motion-compensated predictor (raht_predict_mc): ``predict`` with the key of every row shifted by the vector
    of its block before it is looked up in the reference -- P[i] is ``predict``'s P of the voxel x_i + mv[block(i)], 0 where that
    voxel leaves the cube [0, 2^J)^3. mv: (n_blocks, 3) int8 on the device; block_first: ``motion_blocks``. Everything else, the three
    modes and ``out`` / ``want_matched`` included, is ``predict``'s; with mv = 0 so are the bits. Enqueued only."""
    dev, args, _live, out, matched = _inter_args("predict_mc", keys, ref_keys, C_ref, up, X, blocks=(J, block_log2, block_first, mv),
                                                 result=(add, out, want_matched))
    _call(_lib.lib().raht_predict_mc, dev, *args)
    return (out, matched) if want_matched else out


@torch.no_grad()
def predict_bi(keys, ref0, ref1, X=None, up=0, add=False, out=None, want_matched=False, J=None, block_log2=0, block_first=None,
               mv0=None, mv1=None, modes=None):
    """The two-reference predictor of a B frame (raht_predict_bi). ref0, ref1: (ref_keys, C_ref) as ``predict`` takes
    them, of one D. With m_r = ``predict``'s P against reference r (``predict_mc``'s under ``mv_r``: (n_blocks, 3) int8 over the
    FRAME's blocks, with ``J``, ``block_log2`` and ``block_first`` of ``motion_blocks``; a field that is None is all zero), P is m0
    where reference 1 has no run for the row, m1 where reference 0 has none, 0 where neither has, and fl(0.5 fl(m0 + m1)) where
    both have. -> P when ``X`` is None, X - P, or X + P with ``add``; into ``out`` when given (``out`` may be ``X``). Column slices
    pass as they are. ``want_matched``: -> (result, n_matched), a (3,) int64 device tensor: the rows with a run in reference 0, in
    reference 1, in both. Enqueued only.

    ``modes`` (raht_predict_bi_modes): (n_blocks,) uint8 on the device, one per block of the frame (``J``,
    ``block_log2`` and ``block_first`` are then needed with or without fields) -- 0: the rule above, 1: m0 alone (0 where reference
    0 has no run), 2: m1 alone, 3: P = 0. All 0 gives the bits of the call without modes, all 1 or all 2 those of ``predict`` /
    ``predict_mc`` against that reference; n_matched then counts the runs the prediction uses."""
    who = "predict_bi"
    (rk0, C0), (rk1, C1) = _ref_pairs(who, ref0, ref1)
    fields = [f for f in (mv0, mv1) if f is not None]
    if fields and (J is None or block_first is None):
        raise ValueError(f"{who}: a motion field needs J, block_log2 and block_first")
    if modes is not None and (J is None or block_first is None):
        raise ValueError(f"{who}: modes need J, block_log2 and block_first")
    framed = bool(fields) or modes is not None                               # (the blocks are read under a field or under modes)
    blocks0 = (J, block_log2, block_first, *fields[:1]) if framed else None
    blocks1 = (J, block_log2, block_first, *fields[-1:]) if framed else None
    dev, _, live0, out, _ = _inter_args(who, keys, rk0, C0, up, X, blocks=blocks0, result=(add, out, False))
    _, _, live1, _, _ = _inter_args(who, keys, rk1, C1, up, X, blocks=blocks1, result=(add, out, False))
    (k, r0, C0), (r1, C1) = live0[:3], live1[1:3]
    if C1.shape[1] != C0.shape[1] or C1.device != dev:
        raise ValueError(f"{who}: both references must have the same D and lie on one device")
    N, D = int(k.shape[0]), int(C0.shape[1])
    bf = live0[3] if framed else None
    n_blocks = int(bf.shape[0]) - 1 if framed else 0
    f0, f1 = (None if f is None else f.contiguous() for f in (mv0, mv1))
    matched = torch.empty(3, dtype=torch.int64, device=dev) if want_matched else None
    head = [_p(k), N, int(J) if framed else 0, int(block_log2) if framed else 0, _p(bf), n_blocks]
    tail = [_p(f0), _p(f1), _p(r0), int(r0.shape[0]), _p(C0), C0.stride(0), _p(r1), int(r1.shape[0]), _p(C1), C1.stride(0), 3 * int(up),
            _p(X), 0 if X is None else X.stride(0), D, int(bool(add)), _p(out), out.stride(0), _p(matched)]
    if modes is None:
        _call(_lib.lib().raht_predict_bi, dev, *head, *tail)
    else:
        _need_cuda(modes, "modes")
        if modes.dtype != torch.uint8 or tuple(modes.shape) != (n_blocks,) or modes.device != dev:
            raise ValueError(f"{who}: modes must be a ({n_blocks},) uint8 tensor on the keys' device")
        modes = modes.contiguous()
        _call(_lib.lib().raht_predict_bi_modes, dev, *head, _p(modes), *tail)
    return (out, matched) if want_matched else out


def _ref_pairs(who, ref0, ref1):
    try:
        (rk0, C0), (rk1, C1) = ref0, ref1
    except (TypeError, ValueError):
        raise ValueError(f"{who}: ref0 and ref1 are (ref_keys, C_ref) pairs") from None
    return (rk0, C0), (rk1, C1)


# ---- block modes of a B frame (raht_mode_search / raht_predict_bi_modes) ------------------------------------------------
@torch.no_grad()
def mode_search(keys, ref0, ref1, X, J, block_log2, block_first, weights, up=0, mv0=None, mv1=None, want_table=False):
    """The per-block choice among a B frame's predictors (raht_mode_search). keys, ref0, ref1, ``up``, mv0, mv1: as
    ``predict_bi`` takes them; X: (N, D) float32; block_first: ``motion_blocks``; weights: D finite floats >= 0 (checked here, on the
    host), a column of weight 0 is left out. A block is predicted in one of four ways -- 0: ``predict_bi``'s rule, 1: from reference
    0 alone (``predict`` / ``predict_mc`` under mv0; 0 where it has no run), 2: from reference 1 alone, 3: not at all. The cost of a
    row under a mode is ``motion_search``'s row cost against that mode's prediction, a block's cost the integer sum over its rows;
    the smallest cost wins, the smallest mode among equals. -> (mode (n_blocks,) uint8, best_cost (n_blocks,) int64[, table
    (n_blocks, 4) int64]) on the device. One pass over the frame. Enqueued only, as ``motion_search`` is: but for the first call
    with given weights."""
    who = "mode_search"
    (rk0, C0), (rk1, C1) = _ref_pairs(who, ref0, ref1)
    dev, _, live0, _, _ = _inter_args(who, keys, rk0, C0, up, X, blocks=(J, block_log2, block_first, *(() if mv0 is None else (mv0,))))
    _, _, live1, _, _ = _inter_args(who, keys, rk1, C1, up, X, blocks=(J, block_log2, block_first, *(() if mv1 is None else (mv1,))))
    (k, r0, C0, bf), (r1, C1) = live0[:4], live1[1:3]
    if C1.shape[1] != C0.shape[1] or C1.device != dev:
        raise ValueError(f"{who}: both references must have the same D and lie on one device")
    X = live0[-1]
    N, D, n_blocks = int(k.shape[0]), int(C0.shape[1]), int(bf.shape[0]) - 1
    f0, f1 = (None if f is None else f.contiguous() for f in (mv0, mv1))
    w_d = _search_weights(who, weights, D, dev)
    mode = torch.empty(n_blocks, dtype=torch.uint8, device=dev)
    best_cost = torch.empty(n_blocks, dtype=torch.int64, device=dev)
    table = torch.empty((n_blocks, 4), dtype=torch.int64, device=dev) if want_table else None
    _call(_lib.lib().raht_mode_search, dev, _p(k), N, int(J), int(block_log2), _p(bf), n_blocks, _p(f0), _p(f1), _p(r0), int(r0.shape[0]),
          _p(C0), C0.stride(0), _p(r1), int(r1.shape[0]), _p(C1), C1.stride(0), 3 * int(up), _p(X), X.stride(0), D, _p(w_d), _p(mode),
          _p(best_cost), _p(table))
    return (mode, best_cost, table) if want_table else (mode, best_cost)


@torch.no_grad()
def voxel_keys(PC, vmin, width, J):
    """Unsorted 3J-bit Morton keys (int64) of the points of PC (n, >= 3) float32 for a given bounding box: the
    voxelizer's first phase (reference python/voxelize_pc.py:92-100)."""
    _need_cuda(PC, "PC")
    if PC.dtype != torch.float32 or PC.stride(1) != 1:
        PC = PC.to(torch.float32).contiguous()
    out = torch.empty(PC.shape[0], dtype=torch.int64, device=PC.device)
    vm = (C.c_float * 3)(*[float(x) for x in vmin])
    _call(_lib.lib().raht_voxel_keys, PC.device, _p(PC), PC.stride(0), PC.shape[0], vm, float(width), int(J), _p(out))
    return out


@torch.no_grad()
def sort_keys(keys, nbits=64):
    """Stable LSD radix sort of Morton keys on device -> (keys_sorted, idx)."""
    _need_cuda(keys, "keys")
    k = keys.contiguous()
    ko = torch.empty_like(k)
    idx = torch.empty(k.shape[0], dtype=torch.int64, device=k.device)
    _call(_lib.lib().raht_sort_keys, k.device, _p(k), k.shape[0], int(nbits), _p(ko), _p(idx))
    return ko, idx


_VMIN_CACHE = {}


def _vmin_tensor(vmin, dev):
    """info['vmin'] as a device tensor (the reference's is one). The frames of a sequence share their bounding box: the 12-byte
    upload (a synchronising copy, ~30 us of a 0.7 ms call) is made once per (device, box), the tensor handed out is a clone."""
    key = (str(dev), vmin)
    t = _VMIN_CACHE.get(key)
    if t is None:
        if len(_VMIN_CACHE) > 64:
            _VMIN_CACHE.clear()
        t = _VMIN_CACHE[key] = torch.tensor(list(vmin), dtype=torch.float32, device=dev)
    return t.clone()


class _Voxelizer:
    """THE call path of voxelize_pc_batched / voxelize_merge / voxelize_plan. Construction prepares the cloud (on ``device``, float32,
    contiguous) and allocates what all three hand to the library: ``keys``, ``vidx`` (N int64 each) and ``rows`` (N x ld float32);
    ``run`` parses vmin, makes the call -- fn(cloud, ld, N, *head, vmin, width, J, *outs, n_vox, vmin_out, width_out,
    voxel_size_out, stream, *after), every wrapper spelling out its own ``head`` and ``outs`` in the order of its C signature
    -- and returns what the three info dictionaries share (vmin as a tuple)."""

    def __init__(self, PC, device, name):
        PC = PC.to(device)
        _need_cuda(PC, name)
        self.PC = PC.to(torch.float32).contiguous()
        self.N, self.ld = self.PC.shape
        self.dev = self.PC.device
        self.keys, self.vidx, self.rows = self.empty(), self.empty(), self.empty(self.ld, torch.float32)

    def empty(self, cols=None, dtype=torch.int64):
        return torch.empty(self.N if cols is None else (self.N, cols), dtype=dtype, device=self.dev)

    def run(self, fn, head, vmin, width, J, outs, after=()):
        nvox = C.c_int64()
        vmin_out = (C.c_float * 3)()
        w_out, vs_out = C.c_double(), C.c_double()
        vm = None if vmin is None else (C.c_float * 3)(*_host_floats(vmin))
        _call(fn, self.dev, _p(self.PC), self.ld, self.N, *head, vm, -1.0 if width is None else float(width), int(J),
              *[_p(t) for t in outs], C.byref(nvox), vmin_out, C.byref(w_out), C.byref(vs_out), after=after)
        return {"Nvox": nvox.value, "voxel_size": vs_out.value, "vmin": tuple(vmin_out), "width": w_out.value, "N": self.N}


@torch.no_grad()
def voxelize_pc_batched(PC, vmin=None, width=None, J=10, device="cuda", residuals=True, sorted_points=True):
    """Drop-in for reference python/voxelize_pc.py:62-172.

    Returns (PCvox, PCsorted, voxel_indices, DeltaPC, info) like the reference. PCvox,
    voxel_indices, info['sort_idx'] and the sorted Morton keys (info['keys_sorted'], extra) come
    from the HIP voxelizer; PCsorted / DeltaPC are its secondary outputs, produced by the same call (``raht_voxelize_all``:
    the pass that forms the voxel means has every point's row in registers anyway and writes them too -- voxelize_pc.py:103-111,
    147-156; raht_voxelize + raht_voxelize_residuals give the same bits; ``residuals=False`` skips DeltaPC;
    ``sorted_points=False`` skips PCsorted and returns None in its place; the codec path only consumes PCvox).
    """
    v = _Voxelizer(PC, device, "PC")
    idx = v.empty()
    PCsorted = v.empty(v.ld, torch.float32) if sorted_points else None
    DeltaPC = v.empty(v.ld, torch.float32) if residuals else None
    info = v.run(_lib.lib().raht_voxelize_all, (v.ld - 3,), vmin, width, J,
                 (v.keys, idx, v.vidx, v.rows, None, PCsorted, DeltaPC))               # (None: no Vvox)
    nv = info["Nvox"]
    info.update(vmin=_vmin_tensor(info["vmin"], v.dev), sort_idx=idx, keys_sorted=v.keys)
    return v.rows[:nv], PCsorted, v.vidx[:nv], DeltaPC, info


@torch.no_grad()
def voxelize_merge(G, vmin=None, width=None, J=10, device="cuda", weight_by_opacity=True, want_means=True):
    """N whole Gaussians [xyz | quat(4) | scale(3) | opacity | colour(cd)] -> the voxelized frame in ONE call and one pass over the
    rows (raht_voxelize_merge): voxelizer + the reference's per-voxel opacity-weighted merge (python/test_voxelize_3dgs.py:203-257,
    cuda/merge_cluster.cu:2-111), bit-identical to ``voxelize_pc_batched`` followed by ``merge_gaussian_clusters_with_indices``.
    Returns (Gvox (Nvox, 11 + cd): integer voxel coordinates as floats + merged attributes, info: Nvox, voxel_size, vmin, width,
    N, sort_idx, keys_sorted, voxel_indices, merged_means)."""
    v = _Voxelizer(G, device, "G")
    if v.ld < 11:
        raise ValueError("voxelize_merge: rows are [xyz | quat(4) | scale(3) | opacity | colours]: at least 11 columns")
    idx = v.empty()
    mm = v.empty(3, torch.float32) if want_means else None
    info = v.run(_lib.lib().raht_voxelize_merge, (v.ld - 11, 1 if weight_by_opacity else 0), vmin, width, J,
                 (v.keys, idx, v.vidx, v.rows, mm))
    nv = info["Nvox"]
    info.update(vmin=_vmin_tensor(info["vmin"], v.dev), sort_idx=idx, keys_sorted=v.keys, voxel_indices=v.vidx[:nv],
                merged_means=None if mm is None else mm[:nv])
    return v.rows[:nv], info


@torch.no_grad()
def voxelize_plan(PC, vmin=None, width=None, J=10, device="cuda"):
    """Unsorted cloud -> (PCvox, plan, info): the voxelizer's own sorted voxel keys go STRAIGHT into the RAHT plan
    (reference: voxelize_pc_batched, python/voxelize_pc.py:62-172, then -- one script later, through a PLY file --
    RAHT_param_reorder_fast on the voxel coordinates, python/RAHT_param.py:190-279, which re-derives the same Morton keys).
    No key recomputation, no key copy (the plan borrows the key tensor and keeps it alive), one plan build per frame, ONE call
    through the C ABI (raht_voxelize_plan). PCvox[:, 3:] is the attribute matrix in the plan's row order. info: Nvox,
    voxel_size, vmin (HOST tensor), width, N, voxel_keys, voxel_indices."""
    v = _Voxelizer(PC, device, "PC")
    h = C.c_void_p()
    info = v.run(_lib.lib().raht_voxelize_plan, (v.ld - 3,), vmin, width, J, (v.keys, v.vidx, v.rows), after=(C.byref(h),))
    nv = info["Nvox"]
    plan = RahtPlan(h, v.dev)
    vkeys = v.keys[:nv]                                   # (here: the key of every voxel)
    plan._keys_ref = vkeys                                # borrowed by the plan: alive as long as it is
    info.update(vmin=torch.tensor(list(info["vmin"]), dtype=torch.float32), voxel_keys=vkeys, voxel_indices=v.vidx[:nv])
    return v.rows[:nv], plan, info
