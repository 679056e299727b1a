"""Transport blocks over the C ABI (td_tb_*; 3GPP TS 36.212 5.1.2, 5.1.4.1.2, 5.1.5): code block segmentation
with filler bits and both CRCs, rate matching of a transport block's code blocks into one concatenated row, its
soft transpose, and the reassembly; and scrambling (td_gold_sequence, td_scramble, td_descramble_llr; 36.211 7.2)
with the receive front end that demaps, descrambles, converts and de-rate-matches in one launch
(TransportBlock.demod_dematch).

The code blocks of N transport blocks live block-major in two tensors, [C_minus, N, K_minus] and
[C_plus, N, K_plus]; viewed as [C N, K] each is one batch for one TurboCodec (encode, decode, ...).  A class
without blocks (C_minus = 0) is None wherever a pair of tensors goes in or comes out.  Every call runs on the
MI355X; only tb_plan / rm_sizes are host arithmetic.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

from . import _native as N

TbPlan = namedtuple("TbPlan", "A B L C K_plus K_minus C_plus C_minus F")

_PRECISION = {"torch.float64": N.TD_F64, "torch.float32": N.TD_F32, "torch.int8": N.TD_FIXED}


def _plan(s: N.TdTbPlan) -> TbPlan:
    return TbPlan(*(int(getattr(s, f)) for f in TbPlan._fields))


def tb_plan(A: int) -> TbPlan:
    """The segmentation of a transport block of A bits (td_tb_plan_host): B = A + 24, C blocks, the first
    C_minus of size K_minus and the others of size K_plus, L = 24 CRC bits a block when C > 1, F filler bits."""
    s = N.TdTbPlan()
    N.check(N.lib().td_tb_plan_host(int(A), C.byref(s)))
    return _plan(s)


def rm_sizes(plan: TbPlan, G: int, NlQm: int):
    """(E_lo, E_hi, n_lo) of td_tb_rm_sizes_host: blocks r < n_lo send E_lo of a row's G values, the others E_hi."""
    s = N.TdTbPlan(*plan)
    v = [C.c_int() for _ in range(3)]
    N.check(N.lib().td_tb_rm_sizes_host(C.byref(s), int(G), int(NlQm), *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def rate_match_index_filler(K: int, Ncb: int, F: int, rv: int, E: int):
    """td_rm_index_host_filler: rate_match_index for a block whose first F bits are filler."""
    import numpy as np

    idx = np.empty(int(E), dtype=np.int32)
    N.check(N.lib().td_rm_index_host_filler(int(K), int(Ncb), int(F), int(rv), int(E), C.c_void_p(idx.ctypes.data)))
    return idx


def _cuda_in(name, t, dtypes, shape=None) -> None:
    if t.dtype not in dtypes or not t.is_cuda or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name} must be a contiguous CUDA tensor of {' / '.join(map(str, dtypes))}"
                         + (f" and shape {tuple(shape)}" if shape is not None else "")
                         + f", got {t.dtype} {tuple(t.shape)} on {t.device}")


def _words(length: int) -> int:
    return (int(length) + 31) // 32


def _seq_stream(stream, device):
    import torch

    return C.c_void_p((stream if stream is not None else torch.cuda.current_stream(device)).cuda_stream)


def gold_sequence(cinit, length: int, out=None, stream=None):
    """The scrambling sequence of 36.211 7.2 (td_gold_sequence).  cinit: int32 [N] on the GPU, the 31 low bits of
    each c_init (a uint32 viewed as int32; bit 31 is ignored) -> int32 [N, W], W = (length + 31) // 32: bit g of
    row n is (seq[n, g >> 5] >> (g & 31)) & 1 = c(g); the last word's bits >= length are 0."""
    import torch

    _cuda_in("cinit", cinit, (torch.int32,), (cinit.shape[0],) if cinit.ndim == 1 else (-1,))
    length = int(length)
    if length < 0 or length >= 1 << 31:
        raise ValueError(f"length must be in [0, 2^31), got {length}")
    n, W = cinit.shape[0], _words(length)
    if out is None:
        out = torch.empty((n, W), dtype=torch.int32, device=cinit.device)
    else:
        _cuda_in("out", out, (torch.int32,), (n, W))
    if n and length:
        with torch.cuda.device(cinit.device):
            N.check(N.lib().td_gold_sequence(C.c_void_p(cinit.data_ptr()), n, length, C.c_void_p(out.data_ptr()),
                                             _seq_stream(stream, cinit.device)))
    return out


def _apply_seq(name, x, seq, out, dtypes):
    _cuda_in(name, x, dtypes, (x.shape[0], x.shape[1]) if x.ndim == 2 else (-1, -1))
    n, length = x.shape
    import torch

    _cuda_in("seq", seq, (torch.int32,), (n, _words(length)))
    if seq.device != x.device:
        raise ValueError(f"seq is on {seq.device}, {name} on {x.device}")
    if out is None:
        out = torch.empty_like(x)
    else:
        _cuda_in("out", out, (x.dtype,), (n, length))
        if out.device != x.device:
            raise ValueError(f"out is on {out.device}, {name} on {x.device}")
    return n, length, out


def scramble(bits, seq, out=None, stream=None):
    """bits: uint8 [N, len] (any non-zero byte is a 1), seq: gold_sequence's int32 [N, (len + 31) // 32] ->
    uint8 [N, len], (bit != 0) ^ c_n(g), every byte 0 or 1 (td_scramble).  out may be `bits`."""
    import torch

    n, length, out = _apply_seq("bits", bits, seq, out, (torch.uint8,))
    if n and length:
        with torch.cuda.device(bits.device):
            N.check(N.lib().td_scramble(C.c_void_p(bits.data_ptr()), C.c_void_p(seq.data_ptr()), n, length,
                                        C.c_void_p(out.data_ptr()), _seq_stream(stream, bits.device)))
    return out


def descramble(llr, seq, out=None, stream=None):
    """llr: soft values [N, len], float64, float32 or int8 -> the same with the sign flipped where c_n(g) = 1
    (0.0 -> -0.0; int8: -128 read as -127, then negated), copied elsewhere (td_descramble_llr).  out may be `llr`."""
    import torch

    n, length, out = _apply_seq("llr", llr, seq, out, (torch.float64, torch.float32, torch.int8))
    if n and length:
        with torch.cuda.device(llr.device):
            N.check(N.lib().td_descramble_llr(C.c_void_p(llr.data_ptr()), _PRECISION[str(llr.dtype)], C.c_void_p(seq.data_ptr()),
                                              n, length, C.c_void_p(out.data_ptr()), _seq_stream(stream, llr.device)))
    return out


class TransportBlock:
    def __init__(self, A: int, Ncb_cap: int = 0, filler_llr: float = -64.0, device: int = 0):
        p = N.TdTbParams(int(A), int(Ncb_cap), int(device), float(filler_llr))
        h = C.c_void_p()
        N.check(N.lib().td_tb_create(C.byref(h), C.byref(p)))
        self._h = h
        self.device = int(device)
        s = N.TdTbPlan()
        N.check(N.lib().td_tb_get_plan(h, C.byref(s)))
        self.plan = _plan(s)
        self.A = self.plan.A

    def close(self) -> None:
        if getattr(self, "_h", None):
            N.lib().td_tb_destroy(self._h)
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

    # -- shapes and checks -----------------------------------------------------------------
    def block_shapes(self, N_tb: int, cols=lambda K: K):
        """The shapes of the (K_minus, K_plus) pair of tensors for N_tb transport blocks, `cols(K)` columns a
        row (K itself: bits; lambda K: 3 * K + 12: coded streams and soft buffers); None for an empty class."""
        p = self.plan
        return ((p.C_minus, N_tb, cols(p.K_minus)) if p.C_minus else None, (p.C_plus, N_tb, cols(p.K_plus)))

    def _in(self, name, t, dtypes, shape) -> None:
        if t.dtype not in dtypes or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be a contiguous CUDA tensor of {' / '.join(map(str, dtypes))} and shape "
                             f"{tuple(shape)}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        if t.device.index != self.device:
            raise ValueError(f"{name} is on {t.device}, the transport block on cuda:{self.device}")

    def _pair_in(self, name, pair, dtypes, N_tb, cols):
        """A (minus, plus) pair the kernels read or write: checked against the plan; the device pointers."""
        minus, plus = pair
        sm, sp = self.block_shapes(N_tb, cols)
        if plus is None or (sm is not None and minus is None):
            raise ValueError(f"{name}: a tensor is missing for a non-empty class of blocks")
        self._in(f"{name}[1]", plus, dtypes, sp)
        if sm is not None:
            self._in(f"{name}[0]", minus, (plus.dtype,), sm)
        return (C.c_void_p(minus.data_ptr()) if sm is not None else None), C.c_void_p(plus.data_ptr())

    def _pair_out(self, out, dtype, N_tb, cols, device):
        import torch

        if out is not None:
            return tuple(out)
        sm, sp = self.block_shapes(N_tb, cols)
        return (torch.empty(sm, dtype=dtype, device=device) if sm else None, torch.empty(sp, dtype=dtype, device=device))

    @staticmethod
    def _stream(stream, device):
        import torch

        return C.c_void_p((stream if stream is not None else torch.cuda.current_stream(device)).cuda_stream)

    # -- the four device calls -----------------------------------------------------------
    def segment(self, tb, out=None, stream=None):
        """tb: uint8 [N, A] (any non-zero byte is a 1) -> (cb_minus [C_minus, N, K_minus] or None,
        cb_plus [C_plus, N, K_plus]) uint8, every byte 0 or 1: filler, payload, gCRC24A, and gCRC24B when
        C > 1 (td_tb_segment).  out: such a pair to write into."""
        import torch

        self._in("tb", tb, (torch.uint8,), (tb.shape[0] if tb.ndim == 2 else -1, self.A))
        n = tb.shape[0]
        out = self._pair_out(out, torch.uint8, n, lambda K: K, tb.device)
        pm, pp = self._pair_in("out", out, (torch.uint8,), n, lambda K: K)
        if n:
            N.check(N.lib().td_tb_segment(self._h, C.c_void_p(tb.data_ptr()), n, pm, pp, self._stream(stream, tb.device)))
        return out

    def rate_match(self, coded, rv: int, G: int, NlQm: int, out=None, stream=None):
        """coded: the (minus, plus) pair of coded streams uint8 [C, N, 3K+12] (TurboCodec.encode of the two
        arrays) -> f uint8 [N, G], row n = e_0 | e_1 | ... | e_{C-1} (td_tb_rate_match)."""
        import torch

        n = coded[1].shape[1] if coded[1] is not None and coded[1].ndim == 3 else -1
        pm, pp = self._pair_in("coded", coded, (torch.uint8,), n, lambda K: 3 * K + 12)
        rm_sizes(self.plan, G, NlQm)   # raises on a bad G / NlQm
        if out is None:
            out = torch.empty((n, int(G)), dtype=torch.uint8, device=coded[1].device)
        else:
            self._in("out", out, (torch.uint8,), (n, int(G)))
        if n:
            N.check(N.lib().td_tb_rate_match(self._h, pm, pp, n, int(rv), int(G), int(NlQm), C.c_void_p(out.data_ptr()),
                                             self._stream(stream, out.device)))
        return out

    def rate_dematch(self, f, rv: int, NlQm: int, out=None, accumulate: bool = False, stream=None):
        """f: the received soft values [N, G], float64, float32 or int8 (convert_llr of demodulate's output) ->
        the (minus, plus) pair of soft buffers [C, N, 3K+12] of f's dtype, ready for the two decoders
        (td_tb_rate_dematch).  With accumulate the sums are added into `out` (required then): HARQ combining."""
        import torch

        dts = (torch.float64, torch.float32, torch.int8)
        self._in("f", f, dts, (f.shape[0], f.shape[1]) if f.ndim == 2 else (-1, -1))
        n, G = f.shape
        rm_sizes(self.plan, G, NlQm)
        if out is None and accumulate:
            raise ValueError("accumulate adds into `out`: pass the soft buffers")
        out = self._pair_out(out, f.dtype, n, lambda K: 3 * K + 12, f.device)
        pm, pp = self._pair_in("out", out, (f.dtype,), n, lambda K: 3 * K + 12)
        if n:
            N.check(N.lib().td_tb_rate_dematch(self._h, C.c_void_p(f.data_ptr()), _PRECISION[str(f.dtype)], n, int(rv), G,
                                               int(NlQm), pm, pp, int(bool(accumulate)), self._stream(stream, f.device)))
        return out

    def demod_dematch(self, yi, yq, rv: int, NlQm: int, modulation: int, Kf: float, precision: str,
                      steps_per_unit: float = 8.0, seq=None, out=None, accumulate: bool = False, stream=None):
        """yi, yq: the received symbols float64 [N, G / modulation] -> the (minus, plus) pair of soft buffers
        [C, N, 3K+12] in `precision` ("f64", "f32" or "fixed": int8 at steps_per_unit) in one launch
        (td_tb_demod_dematch): byte for byte rate_dematch(convert_llr(descramble(demodulate(yi, yq, modulation,
        Kf).view(N, G), seq), precision, steps_per_unit), rv, NlQm, ...).  seq: gold_sequence's int32
        [N, (G + 31) // 32], or None for no descrambling.  With accumulate the sums are added into `out`."""
        import torch

        dts = {"f64": torch.float64, "f32": torch.float32, "fixed": torch.int8}
        if precision not in dts:
            raise ValueError(f"precision must be one of {sorted(dts)}, got {precision!r}")
        if modulation not in (1, 2, 3, 4, 6):
            raise ValueError(f"modulation must be 1, 2, 3, 4 or 6 bits per symbol, got {modulation}")
        self._in("yi", yi, (torch.float64,), (yi.shape[0], yi.shape[1]) if yi.ndim == 2 else (-1, -1))
        self._in("yq", yq, (torch.float64,), yi.shape)
        n, G = yi.shape[0], yi.shape[1] * int(modulation)
        if int(NlQm) % int(modulation):
            raise ValueError(f"NlQm = {NlQm} is not a multiple of the modulation {modulation}")
        rm_sizes(self.plan, G, NlQm)   # raises on a bad G / NlQm
        if seq is not None:
            self._in("seq", seq, (torch.int32,), (n, _words(G)))
        if out is None and accumulate:
            raise ValueError("accumulate adds into `out`: pass the soft buffers")
        out = self._pair_out(out, dts[precision], n, lambda K: 3 * K + 12, yi.device)
        pm, pp = self._pair_in("out", out, (dts[precision],), n, lambda K: 3 * K + 12)
        if n:
            N.check(N.lib().td_tb_demod_dematch(self._h, C.c_void_p(yi.data_ptr()), C.c_void_p(yq.data_ptr()),
                                                _PRECISION[str(dts[precision])], n, int(rv), G, int(NlQm), int(modulation),
                                                float(Kf), float(steps_per_unit),
                                                C.c_void_p(seq.data_ptr()) if seq is not None else None, pm, pp,
                                                int(bool(accumulate)), self._stream(stream, yi.device)))
        return out

    def concat(self, bits, out=None, cb_rem=True, tb_rem=True, stream=None):
        """bits: the (minus, plus) pair of hard decisions uint8 [C, N, K] -> (tb uint8 [N, A], cb_rem int32
        [N, C], tb_rem int32 [N]): the transport blocks without filler and CRCs, every block's gCRC24B
        remainder (0: the block passes; all 0 when C = 1) and the gCRC24A remainder (td_tb_concat).  cb_rem /
        tb_rem: True to have one made, a tensor to write into, or False / None to skip it (None returned)."""
        import torch

        n = bits[1].shape[1] if bits[1] is not None and bits[1].ndim == 3 else -1
        pm, pp = self._pair_in("bits", bits, (torch.uint8,), n, lambda K: K)
        dev = bits[1].device
        if out is None:
            out = torch.empty((n, self.A), dtype=torch.uint8, device=dev)
        else:
            self._in("out", out, (torch.uint8,), (n, self.A))
        rems = []
        for name, r, shape in (("cb_rem", cb_rem, (n, self.plan.C)), ("tb_rem", tb_rem, (n,))):
            if r is True:
                r = torch.empty(shape, dtype=torch.int32, device=dev)
            elif r is False or r is None:
                r = None
            else:
                self._in(name, r, (torch.int32,), shape)
            rems.append(r)
        if n:
            N.check(N.lib().td_tb_concat(self._h, pm, pp, n, C.c_void_p(out.data_ptr()),
                                         *[C.c_void_p(r.data_ptr()) if r is not None else None for r in rems],
                                         self._stream(stream, dev)))
        return out, rems[0], rems[1]
