"""Host-side mirror of the reference codec interface (ITTC/log_map.cpp), over the C ABI.

Reference                                   here
  TurboCodingInit()          :349-434   ->  TurboCodec(K, f1, f2, iterations, algo, precision, device)
  TurboDecoding(flow,out,n)  :1146-1280 ->  TurboCodec.TurboDecoding(flow)  (host arrays, batched)
                                            TurboCodec.decode(llr_tensor)   (device-resident, batched)
  Log_MAP_decoder(...)       :898-1047  ->  TurboCodec.Log_MAP_decoder(recs, La, terminated)
  TurboCodingRelease()       :1330-1345 ->  TurboCodec.close()
  N_ITERATION (log_map.h:30)            ->  `iterations` (runtime, default 15 like the macro)
  TYPE_DECODER (log_map.h:26)           ->  `algo` ("logmap" = table max*, "maxlog")

Every decode runs on the MI355X through libturbo_mi355x.so; nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

N_ITERATION = 15   # log_map.h:30
TERMINATED = 1     # log_map.h:24

_ALGOS = {"logmap": N.TD_ALGO_LOGMAP, "maxlog": N.TD_ALGO_MAXLOG}
_PRECS = {"f64": N.TD_F64, "f32": N.TD_F32, "fixed": N.TD_FIXED}
_NP_DT = {"f64": np.float64, "f32": np.float32, "fixed": np.int8}
_STOP_RULES = {None: N.TD_STOP_NONE, "hda": N.TD_STOP_HDA, "crc": N.TD_STOP_CRC}


def _maxstar_table(steps_per_unit, shift=None):
    m = N.TdFixedMaxstarParams()
    N.check(N.lib().td_fixed_maxstar_table(float(steps_per_unit), -1 if shift is None else int(shift), C.byref(m)))
    return m


def fixed_maxstar_table(steps_per_unit: float, shift=None):
    """(shift, corr) of td_fixed_maxstar_table: the integer log-MAP correction table for LLRs quantised
    at steps_per_unit steps per unit; shift=None chooses the bucket width.  Host only."""
    m = _maxstar_table(steps_per_unit, shift)
    return int(m.shift), tuple(int(v) for v in m.corr)


def stream_length(K: int) -> int:
    """3K+12: the coded stream length TurboDecoding takes (main.cpp:221)."""
    return 3 * K + 12


class TurboCodec:
    def __init__(self, K: int, f1: int, f2: int, iterations: int = N_ITERATION, algo: str = "logmap",
                 precision: str = "f64", device: int = 0):
        self.K, self.f1, self.f2 = int(K), int(f1), int(f2)
        self.L = self.K + 3
        self.iterations = int(iterations)
        self.algo, self.precision = algo, precision
        self.dtype = _NP_DT[precision]                                 # the channel LLRs
        self.le_dtype = np.int16 if precision == "fixed" else self.dtype   # the extrinsics
        p = N.TdParams(self.K, self.f1, self.f2, self.iterations, _ALGOS[algo], _PRECS[precision], int(device))
        h = C.c_void_p()
        N.check(N.lib().td_create(C.byref(h), C.byref(p)))
        self._h = h
        self.device = int(device)
        self.early_stop = None   # set_early_stop / set_window_early_stop / set_fixed_early_stop
        self._window_stop = False   # the rule in self.early_stop is the windowed schedule's
        self._fixed_window, self._fixed_nii = (0, 0), False   # set_fixed_window's last setting

    # -- lifetime (TurboCodingRelease) -------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            N.lib().td_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reserve(self, B: int) -> None:
        N.check(N.lib().td_reserve(self._h, int(B)))

    def placement(self):
        """(probe ms of each candidate workspace, index kept) of the last reserve that allocated
        (td_debug_placement; ([], -1) for a plain allocation)."""
        pick = C.c_int(-1)
        n = N.lib().td_debug_placement(self._h, None, 0, C.byref(pick))   # the count first
        if n < 0:
            N.check(n)
        ms = (C.c_float * max(n, 1))()
        n = N.lib().td_debug_placement(self._h, ms, n, C.byref(pick))
        return [round(ms[i], 4) for i in range(n)], pick.value

    def placement_cost(self):
        """(wall ms, peak bytes of candidate workspaces held) of that search (td_debug_placement_cost)."""
        if not hasattr(N.lib(), "td_debug_placement_cost"):
            return None, None
        w, b = C.c_double(0), C.c_double(0)
        N.check(N.lib().td_debug_placement_cost(self._h, C.byref(w), C.byref(b)))
        return w.value, b.value

    def workspace_bytes(self) -> int:
        """Bytes of the decode workspace (td_debug_workspace_bytes)."""
        v = C.c_ulonglong(0)
        N.check(N.lib().td_debug_workspace_bytes(self._h, C.byref(v)))
        return int(v.value)

    def debug_fill_workspace(self, byte: int) -> int:
        """Fill every scratch buffer of the handle with `byte` (0..255) and arm it: later allocations of
        scratch get the same byte (td_debug_workspace_fill; tests).  byte=-1 disarms.  Returns the bytes
        this call wrote.  Synchronises the device: never inside a stream capture."""
        v = C.c_ulonglong(0)
        N.check(N.lib().td_debug_workspace_fill(self._h, int(byte), C.byref(v)))
        return int(v.value)

    def _torch_dtypes(self):
        """(LLR dtype, Le dtype) of the device-resident calls."""
        import torch

        return {"f64": (torch.float64, torch.float64), "f32": (torch.float32, torch.float32),
                "fixed": (torch.int8, torch.int16)}[self.precision]

    def set_fixed(self, le_max: int = 255, ext_scale_q: int = 3) -> None:
        """The fixed-point decoder's extrinsic (td_set_fixed; precision="fixed" only):
        Le = clamp(sign(r) * ((|r| * ext_scale_q) >> 2), +-le_max), le_max in [1, 255], ext_scale_q in
        [1, 4] quarters (4 = no scaling)."""
        f = N.TdFixedParams(int(le_max), int(ext_scale_q))
        N.check(N.lib().td_set_fixed(self._h, C.byref(f)))

    def set_fixed_window(self, window: int = 64, overlap: int = 48, nii: bool = False) -> None:
        """The fixed-point decoder's sub-block schedule (td_set_fixed_window; precision="fixed" only):
        sub-blocks of `window` positions (a multiple of 16) that warm up over `overlap` positions on each
        side and run in parallel, for batches that do not fill the chip with a lane per codeword.
        window=0: the exact schedule.  Excludes set_fixed_early_stop (its rule is
        set_fixed_window_early_stop's).  The default overlap is the smallest
        measured one whose bit and frame errors stay within 1.1x the exact schedule's at 0.4, 0.5 and
        0.6 dB (K = 6144; DESIGN.md "Fixed point", profiles/fixed/window_ber.json).
        nii: next-iteration initialisation (td_set_fixed_window_nii): from the second iteration on a
        warm-up starts from the metrics the neighbouring sub-block had there one iteration earlier, which
        lets a smaller overlap do; the overlap must then be a multiple of 16.  Window, overlap and nii are
        set together: on an error the call raises and the handle keeps its previous three.  Call reserve()
        after it: the NII state is part of the workspace only while nii is on."""
        L, new = N.lib(), (int(window), int(overlap))
        on = bool(nii) and new[0] != 0
        prev, prev_on = self._fixed_window, self._fixed_nii

        def put(win, flag):
            N.check(L.td_set_fixed_window(self._h, C.byref(N.TdFixedWindowParams(*win))))
            if flag:
                N.check(L.td_set_fixed_window_nii(self._h, 1))

        try:
            if prev_on and not on:   # off first: the new overlap is then free
                N.check(L.td_set_fixed_window_nii(self._h, 0))
            put(new, on)
        except N.TurboError:
            try:   # back to the previous three (a failed C call changed nothing, an earlier one of this call did)
                put(prev, prev_on)
            except N.TurboError:
                pass
            raise
        self._fixed_window, self._fixed_nii = new if new[0] else (0, 0), on
        if not int(window) and self._window_stop:   # td_set_fixed_window(0) clears the sub-block schedule's rule
            self.early_stop, self._window_stop = None, False

    def set_fixed_maxstar(self, steps_per_unit=8.0, shift=None, table=None) -> None:
        """Integer log-MAP on the fixed-point decoder (td_set_fixed_maxstar; precision="fixed" only): every
        max becomes max + corr[min(|a - b| >> shift, 7)].  The table is fixed_maxstar_table(steps_per_unit,
        shift) -- for LLRs quantised at steps_per_unit steps per unit -- or table=(shift, corr) as is (eight
        entries 0 .. 63, the last 0).  set_fixed_maxstar(None) turns it off (Max-Log-MAP).  It applies to
        every fixed schedule and survives the other setters.  Log-MAP wants set_fixed(255, 4): the default
        3/4 scale compensates Max-Log-MAP."""
        if steps_per_unit is None and table is None:
            N.check(N.lib().td_set_fixed_maxstar(self._h, None))
            return
        if table is not None:
            sh, corr = table
            corr = [int(v) for v in corr]
            if len(corr) != 8 or any(not 0 <= v <= 255 for v in corr):
                raise ValueError("table = (shift, corr): corr is eight entries")
            m = N.TdFixedMaxstarParams(int(sh), (C.c_uint8 * 8)(*corr))
        else:
            m = _maxstar_table(steps_per_unit, shift)
        N.check(N.lib().td_set_fixed_maxstar(self._h, C.byref(m)))

    def set_window_maxstar(self, exact: bool) -> None:
        """max* of the windowed log-MAP schedule (td_set_window_maxstar): exact=False the one-read
        table (default), exact=True log_map.cpp's E_algorithm exactly."""
        N.check(N.lib().td_set_window_maxstar(self._h, N.TD_WMAXSTAR_EXACT if exact else N.TD_WMAXSTAR_FAST))

    def set_window(self, window: int = 64, overlap: int = 30, ext_scale: float = 1.0, nii: bool = False,
                   concurrent: bool = False) -> None:
        """Windowed schedule (td_set_window; BASELINE config 5); window=0: exact.
        The reference GPU decoder with P sub-blocks (turboDecoderBianJieZhi.cu) is
        set_window(6144 // P, 0, 0.77, nii=True, concurrent=True) on a maxlog / f32 codec."""
        w = N.TdWindowParams(int(window), int(overlap), int(bool(nii)), int(bool(concurrent)), float(ext_scale))
        N.check(N.lib().td_set_window(self._h, C.byref(w)))
        self.window = int(window)
        if not self.window and self._window_stop:   # td_set_window(0) clears the windowed schedule's rule
            self.early_stop, self._window_stop = None, False

    def set_early_stop(self, rule=None, min_iters: int = 1, crc_poly: int = N.CRC24B) -> None:
        """Per-codeword early termination of the exact schedule (td_set_early_stop): rule "hda" (a
        codeword stops once its hard decisions repeat), "crc" (once their CRC-24 with `crc_poly` is
        zero; gCRC24B by default) or None (off).  No codeword stops before `min_iters` iterations.
        With all_iters the rows after a codeword's stop are copies of its stop row."""
        if rule not in _STOP_RULES:
            raise ValueError(f"rule must be 'hda', 'crc' or None, got {rule!r}")
        s = N.TdStopParams(_STOP_RULES[rule], int(min_iters), int(crc_poly) & 0xFFFFFFFF)
        N.check(N.lib().td_set_early_stop(self._h, C.byref(s)))
        self.early_stop = rule

    def set_window_early_stop(self, rule=None, min_iters: int = 1, crc_poly: int = N.CRC24B) -> None:
        """Per-codeword early termination of the windowed schedule (td_set_window_stop; after
        set_window): the rules, arguments and frozen-row convention of set_early_stop, judged on the
        windowed decode's own rows.  The rule survives later set_window calls with a window;
        set_window(0) clears it."""
        if rule not in _STOP_RULES:
            raise ValueError(f"rule must be 'hda', 'crc' or None, got {rule!r}")
        s = N.TdStopParams(_STOP_RULES[rule], int(min_iters), int(crc_poly) & 0xFFFFFFFF)
        N.check(N.lib().td_set_window_stop(self._h, C.byref(s)))
        self.early_stop = rule
        self._window_stop = rule is not None

    def set_fixed_early_stop(self, rule=None, min_iters: int = 1, crc_poly: int = N.CRC24B) -> None:
        """Per-codeword early termination of the fixed-point decoder (td_set_fixed_stop; precision="fixed"
        only): the rules, arguments and frozen-row convention of set_early_stop, judged on the fixed
        decode's own rows.  The rule survives set_fixed."""
        if rule not in _STOP_RULES:
            raise ValueError(f"rule must be 'hda', 'crc' or None, got {rule!r}")
        s = N.TdStopParams(_STOP_RULES[rule], int(min_iters), int(crc_poly) & 0xFFFFFFFF)
        N.check(N.lib().td_set_fixed_stop(self._h, C.byref(s)))
        if not self._window_stop:   # (with a window set only None gets here, and leaves the window's rule alone)
            self.early_stop = rule

    def set_fixed_window_early_stop(self, rule=None, min_iters: int = 1, crc_poly: int = N.CRC24B) -> None:
        """Per-codeword early termination of the fixed-point decoder's sub-block schedule
        (td_set_fixed_window_stop; after set_fixed_window): the rules, arguments and frozen-row convention of
        set_early_stop, judged on the windowed fixed decode's own rows.  The rule survives set_fixed and
        later set_fixed_window calls with a window; set_fixed_window(0) clears it."""
        if rule not in _STOP_RULES:
            raise ValueError(f"rule must be 'hda', 'crc' or None, got {rule!r}")
        s = N.TdStopParams(_STOP_RULES[rule], int(min_iters), int(crc_poly) & 0xFFFFFFFF)
        N.check(N.lib().td_set_fixed_window_stop(self._h, C.byref(s)))
        self.early_stop = rule
        self._window_stop = rule is not None

    def debug_window_layout(self, run: int = 0, run_a: int = 0, parts: int = 0) -> None:
        """Windowed kernels' layout for tests and measurements (td_debug_window_layout): sub-blocks
        per lane run (beta and alpha kernels) and batch parts; 0 = the layout's own choice."""
        N.check(N.lib().td_debug_window_layout(self._h, int(run), int(run_a), int(parts)))

    # -- TurboDecoding, host arrays ------------------------------------------------------
    def TurboDecoding(self, flow: np.ndarray, return_le: bool = False, return_iters: bool = False):
        """flow [B, 3K+12] (or one row) -> out int32 [B, iterations, K] (the reference's
        flow_decoded rows); with return_le also Le [B, iterations, 2, K+3]; with return_iters also
        the iterations each codeword used, int32 [B] (all `iterations` unless set_early_stop,
        set_window_early_stop or set_fixed_early_stop)."""
        flow = np.ascontiguousarray(flow, dtype=self.dtype)
        one = flow.ndim == 1
        flow = flow.reshape(-1, stream_length(self.K))
        B = flow.shape[0]
        out = np.zeros((B, self.iterations, self.K), dtype=np.int32)
        le = np.zeros((B, self.iterations, 2, self.L), dtype=self.le_dtype) if return_le else None
        used = np.zeros(B, dtype=np.int32) if return_iters else None
        le_p = le.ctypes.data_as(C.c_void_p) if return_le else None
        if return_iters:
            N.check(N.lib().td_decode_host_stop(self._h, flow.ctypes.data_as(C.c_void_p), B,
                                                out.ctypes.data_as(C.c_void_p), le_p, used.ctypes.data_as(C.c_void_p)))
        else:
            N.check(N.lib().td_decode_host(self._h, flow.ctypes.data_as(C.c_void_p), B,
                                           out.ctypes.data_as(C.c_void_p), le_p))
        if one:
            out, le = out[0], (le[0] if return_le else None)
            used = int(used[0]) if return_iters else None
        res = (out,) + ((le,) if return_le else ()) + ((used,) if return_iters else ())
        return res if len(res) > 1 else out

    # -- device-resident decode (torch tensors as HBM buffers) ---------------------------
    def decode(self, llr, bits=None, all_iters: bool = False, le=None, stream=None, iters_out=None):
        """llr: torch tensor [B, 3K+12] on this codec's device (float64 for f64, float32 for f32, int8
        for fixed; le then int16).
        Returns uint8 bits [B, K] (or [B, iterations, K] with all_iters).  Asynchronous on
        `stream` (default: torch's current stream).  iters_out: None, an int32 [B] tensor that
        receives the iterations each codeword used, or True to have one made: the call then returns
        (bits, iters_out)."""
        import torch

        want, want_le = self._torch_dtypes()
        if llr.dtype != want or not llr.is_cuda or not llr.is_contiguous():
            raise ValueError(f"llr must be a contiguous {want} CUDA tensor")
        if llr.ndim != 2 or llr.shape[1] != stream_length(self.K):
            raise ValueError(f"llr must be [B, {stream_length(self.K)}] (3K+12), got {tuple(llr.shape)}")
        if llr.device.index != self.device:
            raise ValueError(f"llr is on {llr.device}, the codec on cuda:{self.device}")
        B = llr.shape[0]
        shape = (B, self.iterations, self.K) if all_iters else (B, self.K)
        if bits is None:
            bits = torch.empty(shape, dtype=torch.uint8, device=llr.device)
        else:
            self._check_out("bits", bits, torch.uint8, shape, llr.device)
        if le is not None:
            self._check_out("le", le, want_le, (B, self.iterations, 2, self.L), llr.device)
        made = iters_out is True
        if made:
            iters_out = torch.empty((B,), dtype=torch.int32, device=llr.device)
        elif iters_out is not None:
            self._check_out("iters_out", iters_out, torch.int32, (B,), llr.device)
        if stream is None:
            stream = torch.cuda.current_stream(llr.device)
        le_p = C.c_void_p(le.data_ptr()) if le is not None else None
        if iters_out is None:
            N.check(N.lib().td_decode_device(self._h, C.c_void_p(llr.data_ptr()), B, C.c_void_p(bits.data_ptr()),
                                             int(all_iters), le_p, C.c_void_p(stream.cuda_stream)))
            return bits
        N.check(N.lib().td_decode_device_stop(self._h, C.c_void_p(llr.data_ptr()), B, C.c_void_p(bits.data_ptr()),
                                              int(all_iters), le_p, C.c_void_p(iters_out.data_ptr()),
                                              C.c_void_p(stream.cuda_stream)))
        return (bits, iters_out) if made else bits

    @staticmethod
    def _check_out(name, t, dtype, shape, device) -> None:
        """An output buffer the kernels write B*... elements into: its dtype, shape, device and
        layout must be exactly what they assume, or they write past its end."""
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, "
                             f"got {t.dtype} {tuple(t.shape)} on {t.device}")

    def decode_raw(self, llr_ptr: int, B: int, bits_ptr: int, all_iters: bool = False, le_ptr: int = 0,
                   stream_ptr: int = 0, iters_ptr: int = 0) -> None:
        """td_decode_device (td_decode_device_stop with iters_ptr) on raw device pointers (no checks possible here: the caller owns the
        sizes -- llr B*(3K+12), bits B*K or B*iterations*K bytes, le B*iterations*2*(K+3), iters B
        int32 or null)."""
        if B < 0 or not llr_ptr or not bits_ptr:
            raise ValueError("decode_raw: B >= 0 and non-null llr / bits pointers")
        if not iters_ptr:
            N.check(N.lib().td_decode_device(self._h, C.c_void_p(llr_ptr), int(B), C.c_void_p(bits_ptr),
                                             int(all_iters), C.c_void_p(le_ptr) if le_ptr else None,
                                             C.c_void_p(stream_ptr) if stream_ptr else None))
            return
        N.check(N.lib().td_decode_device_stop(self._h, C.c_void_p(llr_ptr), int(B), C.c_void_p(bits_ptr),
                                              int(all_iters), C.c_void_p(le_ptr) if le_ptr else None,
                                              C.c_void_p(iters_ptr), C.c_void_p(stream_ptr) if stream_ptr else None))

    # -- LTE rate matching (36.212 5.1.4.1; td_rm_set / td_rate_match / td_rate_dematch) ---
    def set_rate_matching(self, Ncb: int = 0) -> dict:
        """Build the handle's rate-matching tables for a soft buffer of Ncb entries (0: the whole
        circular buffer Kw; otherwise Kpi <= Ncb <= Kw).  May be called again.  Returns the layout:
        R, Kpi, Kw, Ncb and n_nonnull (the non-NULL entries of the buffer: E above it repeats)."""
        N.check(N.lib().td_rm_set(self._h, int(Ncb)))
        v = [C.c_int() for _ in range(5)]
        N.check(N.lib().td_rm_info(self._h, *[C.byref(x) for x in v]))
        self.rate_matching = dict(zip(("R", "Kpi", "Kw", "Ncb", "n_nonnull"), (x.value for x in v)))
        return self.rate_matching

    def _check_in(self, name, t, dtypes, cols=None) -> None:
        """An input the rate-matching kernels read B * cols elements of."""
        if t.dtype not in dtypes or not t.is_cuda or not t.is_contiguous() or t.ndim != 2:
            raise ValueError(f"{name} must be a contiguous 2-D CUDA tensor of {' / '.join(map(str, dtypes))}, "
                             f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        if cols is not None and t.shape[1] != cols:
            raise ValueError(f"{name} must be [B, {cols}], got {tuple(t.shape)}")
        if t.device.index != self.device:
            raise ValueError(f"{name} is on {t.device}, the codec on cuda:{self.device}")

    def rate_match(self, x, rv: int, E: int, out=None, stream=None):
        """x: uint8 / int8 / float32 / float64 tensor [B, 3K+12] on this codec's device (coded bits, or any
        per-position values) -> the E values a transmission of redundancy version rv carries,
        [B, E] of x's dtype: x[:, rate_match_index(K, Ncb, rv, E)].  After set_rate_matching."""
        import torch

        self._check_in("x", x, (torch.uint8, torch.int8, torch.float32, torch.float64), stream_length(self.K))
        rv, E, B = int(rv), int(E), x.shape[0]
        if E < 1:
            raise ValueError(f"E must be at least 1, got {E}")
        if out is None:
            out = torch.empty((B, E), dtype=x.dtype, device=x.device)
        else:
            self._check_out("out", out, x.dtype, (B, E), x.device)
        if stream is None:
            stream = torch.cuda.current_stream(x.device)
        N.check(N.lib().td_rate_match(self._h, C.c_void_p(x.data_ptr()), x.element_size(), B, rv, E,
                                      C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)))
        return out

    def rate_dematch(self, e, rv: int, out=None, accumulate: bool = False, stream=None):
        """e: the received soft values [B, E] of a transmission of redundancy version rv, in the codec's
        dtype -> LLRs [B, 3K+12] ready for decode: every position gets the sum of the e that were
        selected from it (repetition), punctured positions 0.  With accumulate the sums are added
        into `out` (required then): HARQ combining of a retransmission into the soft buffer.  A fixed
        codec takes and gives int8, and every addition saturates to [-127, 127]."""
        import torch

        want = self._torch_dtypes()[0]
        self._check_in("e", e, (want,))
        B, E = e.shape
        if E < 1:
            raise ValueError("e must have at least one column")
        if out is None:
            if accumulate:
                raise ValueError("accumulate adds into `out`: pass the soft buffer")
            out = torch.empty((B, stream_length(self.K)), dtype=want, device=e.device)
        else:
            self._check_out("out", out, want, (B, stream_length(self.K)), e.device)
        if stream is None:
            stream = torch.cuda.current_stream(e.device)
        N.check(N.lib().td_rate_dematch(self._h, C.c_void_p(e.data_ptr()), B, int(rv), E, C.c_void_p(out.data_ptr()),
                                        int(bool(accumulate)), C.c_void_p(stream.cuda_stream)))
        return out

    def demod_dematch(self, yi, yq, rv: int, E: int, modulation: int, Kf: float, steps_per_unit: float = 8.0,
                      out=None, accumulate: bool = False, stream=None):
        """The receive front end in one pass (td_demod_dematch): yi, yq float64 [B, E / modulation], the
        received symbols of a transmission of redundancy version rv -> LLRs [B, 3K+12] in the codec's dtype,
        byte for byte rate_dematch(convert_llr(demodulate(yi, yq, modulation, Kf).view(B, E), precision,
        steps_per_unit), rv, out, accumulate) without the arrays in between.  steps_per_unit is the
        quantiser's on a fixed codec and ignored otherwise.  After set_rate_matching."""
        import torch

        want = self._torch_dtypes()[0]
        rv, E, M = int(rv), int(E), int(modulation)
        if M not in (1, 2, 3, 4, 6):
            raise ValueError(f"modulation must be 1, 2, 3, 4 or 6 bits per symbol, got {M}")
        if E < 1 or E % M:
            raise ValueError(f"E must be a positive multiple of modulation = {M}, got {E}")
        self._check_in("yi", yi, (torch.float64,), E // M)
        self._check_in("yq", yq, (torch.float64,), E // M)
        if yq.shape != yi.shape:
            raise ValueError(f"yi and yq must have one shape, got {tuple(yi.shape)} and {tuple(yq.shape)}")
        B = yi.shape[0]
        if out is None:
            if accumulate:
                raise ValueError("accumulate adds into `out`: pass the soft buffer")
            out = torch.empty((B, stream_length(self.K)), dtype=want, device=yi.device)
        else:
            self._check_out("out", out, want, (B, stream_length(self.K)), yi.device)
        if stream is None:
            stream = torch.cuda.current_stream(yi.device)
        N.check(N.lib().td_demod_dematch(self._h, C.c_void_p(yi.data_ptr()), C.c_void_p(yq.data_ptr()), B, rv, E, M,
                                         float(Kf), float(steps_per_unit), C.c_void_p(out.data_ptr()),
                                         int(bool(accumulate)), C.c_void_p(stream.cuda_stream)))
        return out

    # -- the transmit side: CRC-24 attach / check and the encoder (td_crc_set / td_crc_attach /
    #    td_crc_check / td_encode_device) ----------------------------------------------------
    def encode(self, info, out=None, stream=None):
        """info: uint8 tensor [B, K] on this codec's device (any non-zero byte is a 1) -> the coded stream
        uint8 [B, 3K+12] of encoderm_turbo, each byte 0 or 1: what rate_match and modulate take."""
        import torch

        self._check_in("info", info, (torch.uint8,), self.K)
        B = info.shape[0]
        if out is None:
            out = torch.empty((B, stream_length(self.K)), dtype=torch.uint8, device=info.device)
        else:
            self._check_out("out", out, torch.uint8, (B, stream_length(self.K)), info.device)
        if stream is None:
            stream = torch.cuda.current_stream(info.device)
        if B:   # (an empty tensor has no address to pass)
            N.check(N.lib().td_encode_device(self._h, C.c_void_p(info.data_ptr()), B, C.c_void_p(out.data_ptr()),
                                             C.c_void_p(stream.cuda_stream)))
        return out

    def set_crc(self, poly: int = N.CRC24B) -> None:
        """The CRC-24 generator of crc_attach / crc_check (td_crc_set): its 24 low-order coefficients,
        gCRC24B by default.  Needs K > 24.  Independent of the early-termination rules' polynomial."""
        N.check(N.lib().td_crc_set(self._h, int(poly) & 0xFFFFFFFF))
        self.crc_poly = int(poly)

    def crc_attach(self, bits, stream=None):
        """bits: uint8 tensor [B, K] on this codec's device.  In place: the last 24 bytes of every row
        become the CRC-24 of the K-24 before them (most significant bit first).  Returns bits.  After set_crc."""
        import torch

        self._check_in("bits", bits, (torch.uint8,), self.K)
        if stream is None:
            stream = torch.cuda.current_stream(bits.device)
        if bits.shape[0]:
            N.check(N.lib().td_crc_attach(self._h, C.c_void_p(bits.data_ptr()), bits.shape[0],
                                          C.c_void_p(stream.cuda_stream)))
        return bits

    def crc_check(self, bits, out=None, stream=None):
        """bits: uint8 tensor [B, K] -> the CRC-24 remainder of every row, a [B] tensor of 32-bit values
        (0 = the block passes; td_crc24_host of the row).  After set_crc."""
        import torch

        self._check_in("bits", bits, (torch.uint8,), self.K)
        B = bits.shape[0]
        if out is None:
            out = torch.empty((B,), dtype=torch.int32, device=bits.device)
        else:
            self._check_out("out", out, torch.int32, (B,), bits.device)
        if stream is None:
            stream = torch.cuda.current_stream(bits.device)
        if B:
            N.check(N.lib().td_crc_check(self._h, C.c_void_p(bits.data_ptr()), B, C.c_void_p(out.data_ptr()),
                                         C.c_void_p(stream.cuda_stream)))
        return out

    # -- measurement ---------------------------------------------------------------------
    def profile(self, on: bool = True) -> None:
        """Bracket the next decodes' kernels with hipEvents (see td_profile_enable)."""
        N.check(N.lib().td_profile_enable(self._h, int(on)))

    def kernel_ms(self):
        """(demux_ms, turbo_ms, launches): average kernel durations over the decodes since the
        last call (synchronises on their events)."""
        a, b, n = C.c_float(), C.c_float(), C.c_int()
        N.check(N.lib().td_profile_read(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def clock(self):
        """(sustained shader clock GHz, workgroup span ms) of the last decode: the exact schedule's
        turbo launch, or a windowed decode's last SISO2 beta workgroup (td_clock_read; waits for
        this handle's last decode).  A windowed decode with early termination takes no sample: an error."""
        g, s = C.c_double(), C.c_double()
        N.check(N.lib().td_clock_read(self._h, C.byref(g), C.byref(s)))
        return g.value, s.value

    # -- frame generator and error counts (main.cpp's channel, on the device) -------------
    def synth_seed(self, seed: int) -> None:
        """srand(seed) for the handle's frame stream (main.cpp:170)."""
        N.check(N.lib().td_synth_seed(self._h, int(seed) & 0xFFFFFFFF))

    def synth_modulation(self, modulation: int) -> None:
        """MODULATION of the generator's frames: 1 BPSK, 2 QPSK, 3 8PSK, 4 16QAM, 6 64QAM."""
        N.check(N.lib().td_synth_modulation(self._h, int(modulation)))

    def synth_seek(self, frame: int) -> None:
        N.check(N.lib().td_synth_seek(self._h, int(frame)))

    def synth(self, B: int, ebn0_db: float, info=None, llr=None, stream=None):
        """The next B frames of the stream: (info uint8 [B, K], llr float64 [B, 3K+12]) tensors
        on this codec's device, bit-identical to main.cpp's frames of the same srand seed."""
        import torch

        dev = torch.device("cuda", self.device)
        if info is None:
            info = torch.empty((B, self.K), dtype=torch.uint8, device=dev)
        if llr is None:
            llr = torch.empty((B, stream_length(self.K)), dtype=torch.float64, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        N.check(N.lib().td_synth_frames(self._h, float(ebn0_db), int(B), C.c_void_p(info.data_ptr()),
                                        C.c_void_p(llr.data_ptr()), C.c_void_p(stream.cuda_stream)))
        return info, llr

    def count_errors(self, bits, info, stream=None):
        """bits uint8 [B, iters, K], info uint8 [B, K] -> int32 [B, iters] bit-error counts."""
        import torch

        B, iters = int(bits.shape[0]), int(bits.shape[1])
        err = torch.empty((B, iters), dtype=torch.int32, device=bits.device)
        if stream is None:
            stream = torch.cuda.current_stream(bits.device)
        N.check(N.lib().td_count_errors(self._h, C.c_void_p(bits.data_ptr()), iters, C.c_void_p(info.data_ptr()), B,
                                        C.c_void_p(err.data_ptr()), C.c_void_p(stream.cuda_stream)))
        return err

    # -- Log_MAP_decoder -----------------------------------------------------------------
    def Log_MAP_decoder(self, recs: np.ndarray, La: np.ndarray, terminated: int = TERMINATED) -> np.ndarray:
        """recs [B, 2L] (ys, yp pairs), La [B, L] -> LLR [B, L] (or 1-D for one codeword)."""
        recs = np.ascontiguousarray(recs, dtype=self.dtype)
        La = np.ascontiguousarray(La, dtype=self.dtype)
        one = La.ndim == 1
        La2 = La.reshape(1, -1) if one else La
        L = La2.shape[1]
        recs2 = recs.reshape(-1, 2 * L)
        B = La2.shape[0]
        out = np.zeros((B, L), dtype=self.dtype)
        N.check(N.lib().td_siso_host(self._h, recs2.ctypes.data_as(C.c_void_p), La2.ctypes.data_as(C.c_void_p),
                                     int(terminated), out.ctypes.data_as(C.c_void_p), L, B))
        return out[0] if one else out


def quantise(llr, steps_per_unit: float):
    """Float LLRs (a torch tensor) -> the int8 a fixed codec takes: round to nearest, clamp +-127."""
    import torch

    return torch.clamp(torch.round(llr * steps_per_unit), -127, 127).to(torch.int8)


def convert_llr(llr, precision: str, steps_per_unit: float = 8.0, out=None, stream=None):
    """td_llr_convert on the GPU: a float64 cuda tensor -> a tensor of the same shape in `precision`'s dtype
    ("f64" a copy, "f32" the rounded narrowing, "fixed" the int8 clamp(rint(llr * steps_per_unit), +-127):
    quantise's values on every finite input, in one kernel)."""
    import torch

    if precision not in _PRECS:
        raise ValueError(f"precision must be one of {sorted(_PRECS)}, got {precision!r}")
    want = {"f64": torch.float64, "f32": torch.float32, "fixed": torch.int8}[precision]
    if llr.dtype != torch.float64 or not llr.is_cuda or not llr.is_contiguous():
        raise ValueError(f"llr must be a contiguous float64 CUDA tensor, got {llr.dtype} {tuple(llr.shape)} on {llr.device}")
    if out is None:
        out = torch.empty(llr.shape, dtype=want, device=llr.device)
    else:
        TurboCodec._check_out("out", out, want, llr.shape, llr.device)
    if stream is None:
        stream = torch.cuda.current_stream(llr.device)
    if llr.numel():   # (an empty tensor has no address to pass)
        with torch.cuda.device(llr.device):
            N.check(N.lib().td_llr_convert(C.c_void_p(llr.data_ptr()), llr.numel(), _PRECS[precision], float(steps_per_unit),
                                           C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)))
    return out


def modulate(bits, modulation: int, stream=None):
    """module (modanddem.cpp:175) on the GPU: uint8 bits [nsym * M] (cuda) -> (si, sq) float64."""
    import torch

    bits = bits.contiguous()
    nsym = bits.numel() // modulation
    si = torch.empty(nsym, dtype=torch.float64, device=bits.device)
    sq = torch.empty_like(si)
    if stream is None:
        stream = torch.cuda.current_stream(bits.device)
    N.check(N.lib().td_modulate(C.c_void_p(bits.data_ptr()), nsym, int(modulation), C.c_void_p(si.data_ptr()),
                                C.c_void_p(sq.data_ptr()), C.c_void_p(stream.cuda_stream)))
    return si, sq


def demodulate(yi, yq, modulation: int, Kf: float, stream=None):
    """demodule (modanddem.cpp:674) on the GPU: float64 symbols [nsym] (cuda) -> LLRs [nsym * M]."""
    import torch

    yi, yq = yi.contiguous(), yq.contiguous()
    out = torch.empty(yi.numel() * modulation, dtype=torch.float64, device=yi.device)
    if stream is None:
        stream = torch.cuda.current_stream(yi.device)
    N.check(N.lib().td_demodulate(C.c_void_p(yi.data_ptr()), C.c_void_p(yq.data_ptr()), yi.numel(), int(modulation),
                                  float(Kf), C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)))
    return out


def rate_match_index(K: int, Ncb: int, rv: int, E: int) -> np.ndarray:
    """int32 [E]: the stream position (index into the 3K+12 stream) of each value a transmission of
    redundancy version rv carries, for a soft buffer of Ncb entries (0: the whole circular buffer).
    Host only (td_rm_index_host): rate_match(x) is x[:, idx], rate_dematch its transpose."""
    idx = np.empty(max(int(E), 0), dtype=np.int32)
    N.check(N.lib().td_rm_index_host(int(K), int(Ncb), int(rv), int(E), idx.ctypes.data_as(C.c_void_p)))
    return idx


def TurboCodingInit(K: int, f1: int, f2: int, **kw) -> TurboCodec:
    """Reference-named constructor (log_map.cpp:349): parameters explicit instead of globals."""
    return TurboCodec(K, f1, f2, **kw)


def device_count() -> int:
    return N.lib().td_device_count()
