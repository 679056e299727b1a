"""Transport blocks on the MI355X (td_tb_* through transport.TransportBlock): every entry point byte for byte
against tb_ref's numpy restatement -- odd input bytes, garbage in the outputs, misaligned tensors, every
redundancy version, uneven E, repetition, a limited soft buffer, all three soft precisions with HARQ
accumulation -- the round trip and what the remainders say, the blocks without filler against the
single-block calls, the closed loop through two decoders, and graph capture.

Shapes: A = 1 (F = 15), 16 (F = 0), 17 (K = 48), 6121 (one block of each size, F = 15), 12217 (two K_minus
blocks, F = 39), 12257 (two K_plus blocks, F = 63), each with N = 1, 3, 65 (65 rows: more than one row a wave
and partial workgroups), and A = 40961, N = 2: seven blocks, F = 63, a gCRC24A table of 160 KiB (beyond LDS).
Misalignment: byte tensors sit 5 bytes into their allocation; float tensors need element alignment and sit
5 elements in.
"""
import ctypes as C

import numpy as np
import pytest

import ratematch_ref as RM
import tb_ref as T
from conftest import gpu_available
from turbo_decoder_cuda_amd import _native as N

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

GUARD = 0xA5
PAD = 64
CASES = [(A, n) for A in (1, 16, 17, 6121, 12217, 12257) for n in (1, 3, 65)] + [(40961, 2)]
# f1, f2 of the sizes the closed loop and the single-block comparison decode: the LTE pairs, which follow
# tests/encode_cases.py's rule (f1 coprime to K, every prime factor of K in f2)
QPP = {3072: (47, 96), 3136: (13, 112), 4096: (31, 64), 4160: (33, 130)}
NP_DT = {"f64": np.float64, "f32": np.float32, "fixed": np.int8}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _tb(A, **kw):
    from turbo_decoder_cuda_amd import TransportBlock
    return TransportBlock(A, **kw)


def _guarded(a, fill=False):
    """A device tensor of a's shape and dtype 5 elements into a buffer of guard bytes, holding a (or, with
    fill, guard bytes: garbage where an output goes).  Returns (view, check): check() synchronises, asserts
    the guard bands and returns the tensor's numpy value."""
    import torch
    a = np.ascontiguousarray(a)
    es, nb = a.dtype.itemsize, a.nbytes
    off = 5 * es
    buf = torch.full((off + nb + PAD,), GUARD, dtype=torch.uint8, device=_dev())
    view = buf[off:off + nb].view(getattr(torch, a.dtype.name)).view(a.shape)
    assert view.data_ptr() % 16 == (buf.data_ptr() + off) % 16
    if not fill:
        view.copy_(torch.from_numpy(a).to(_dev()))

    def check():
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        assert (b[:off] == GUARD).all() and (b[off + nb:] == GUARD).all(), "guard bands"
        return b[off:off + nb].view(a.dtype).reshape(a.shape).copy()
    return view, check


def _guarded_pair(pr, fill=False):
    g = [None if a is None else _guarded(a, fill) for a in pr]
    views = tuple(None if x is None else x[0] for x in g)
    return views, lambda: tuple(None if x is None else x[1]() for x in g)


def _same(got, want):
    """two pairs (or arrays), byte for byte"""
    if isinstance(want, tuple):
        return all(_same(g, w) for g, w in zip(got, want)) and len(got) == len(want)
    if want is None:
        return got is None
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _odd_bits(rng, shape):
    """random bits whose ones are the bytes 0x01, 0x02, 0x80 and 0xFF"""
    return (rng.integers(0, 2, shape, dtype=np.uint8) * rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), shape)).astype(np.uint8)


def _shapes(p, n, cols=lambda K: K):
    return ((p.C_minus, n, cols(p.K_minus)) if p.C_minus else None, (p.C_plus, n, cols(p.K_plus)))


def _rand_pair(rng, p, n, make, cols=lambda K: K):
    return tuple(None if s is None else make(rng, s) for s in _shapes(p, n, cols))


def _cap(p):
    """an Ncb_cap below Kw of both sizes and above Kpi of K_plus: the buffers end inside the parity part"""
    Kpi, Kw = RM.layout(p.K_plus)[2:4]
    cap = Kpi + (Kw - Kpi) // 3
    assert cap < Kw and (not p.C_minus or cap < RM.layout(p.K_minus)[3])
    return cap


def _g_punctured(p, Q):
    """G about 2 sum K_r, a multiple of Q = NlQm, and G' no multiple of C (uneven E) when C > 1"""
    Gp = max(2 * sum(T.block_sizes(p)) // Q, p.C)
    if p.C > 1 and Gp % p.C == 0:
        Gp += 1
    return Gp * Q


def _g_repeated(p, Q):
    """every E_r beyond twice its buffer's non-NULL count: each position sent at least twice, some three times"""
    Gp = p.C * (-(-(2 * (3 * p.K_plus + 12) + 29) // Q))
    if p.C > 1:
        Gp += p.C - 1
    return Gp * Q


# rv, limited buffer?, G, accumulate?
CONFIGS = [(0, False, _g_punctured, False), (1, True, _g_repeated, True), (2, False, _g_repeated, True),
           (3, True, _g_punctured, False)]
FILLER = {False: -63.5, True: -1000.25}   # by limited buffer?: int8 -64 (ties to even) and -127 (clamped)


# ------------------------------------------------------------------ 1: each entry point against tb_ref
@pytest.mark.parametrize("A,n", CASES)
def test_segment_equals_the_restatement(A, n):
    p = T.plan(A)
    x = _odd_bits(np.random.default_rng(A + n), (n, A))
    want = T.segment(p, x)
    with _tb(A) as t:
        assert tuple(t.plan) == tuple(p)
        vin, cin = _guarded(x)
        vout, cout = _guarded_pair(tuple(None if w is None else np.empty_like(w) for w in want), fill=True)
        t.segment(vin, out=vout)
        got = cout()
        assert _same(cin(), x), "d_tb is only read"
        assert _same(got, want)
        assert _same(tuple(None if o is None else o.cpu().numpy() for o in t.segment(vin)), want)   # made outputs


@pytest.mark.parametrize("A,n", CASES)
def test_concat_equals_the_restatement(A, n):
    p = T.plan(A)
    bits = _rand_pair(np.random.default_rng(2 * A + n), p, n, _odd_bits)   # no code words: every remainder non-zero
    tb, cb_rem, tb_rem = T.concat(p, bits)
    with _tb(A) as t:
        vin, cin = _guarded_pair(bits)
        (vtb, ctb), (vcb, ccb), (vtr, ctr) = (_guarded(np.empty(s, d), fill=True) for s, d in
                                              (((n, A), np.uint8), ((n, p.C), np.int32), ((n,), np.int32)))
        t.concat(vin, out=vtb, cb_rem=vcb, tb_rem=vtr)
        assert _same(ctb(), tb) and _same(ccb().view(np.uint32), cb_rem) and _same(ctr().view(np.uint32), tb_rem)
        assert _same(cin(), bits), "the hard decisions are only read"
        assert (cb_rem != 0).all() == (p.C > 1) and (tb_rem != 0).all()
        # either remainder may be left out
        for kw in (dict(cb_rem=None), dict(tb_rem=None), dict(cb_rem=None, tb_rem=None)):
            o, c, r = t.concat(vin, **kw)
            assert _same(o.cpu().numpy(), tb)
            assert (c is None) == ("cb_rem" in kw) and (r is None) == ("tb_rem" in kw)
            assert c is None or _same(c.cpu().numpy().view(np.uint32), cb_rem)
            assert r is None or _same(r.cpu().numpy().view(np.uint32), tb_rem)


@pytest.mark.parametrize("A,n", CASES)
def test_rate_match_equals_the_restatement(A, n):
    """NlQm = 2.  The coded bytes are arbitrary: the call is a gather."""
    p, Q = T.plan(A), 2
    rng = np.random.default_rng(3 * A + n)
    coded = _rand_pair(rng, p, n, lambda r, s: r.integers(0, 256, s, dtype=np.uint8), lambda K: 3 * K + 12)
    vin, cin = _guarded_pair(coded)
    for limited in (False, True):
        cap = _cap(p) if limited else 0
        with _tb(A, Ncb_cap=cap) as t:
            for rv, lim, g, _ in CONFIGS:
                if lim != limited:
                    continue
                G = g(p, Q)
                E = T.block_e(p, G, Q)
                assert p.C == 1 or len(set(E)) == 2
                if g is _g_repeated:
                    assert min(E) > 2 * (3 * p.K_plus + 12)
                want = T.rate_match(p, coded, cap, rv, G, Q)
                vout, cout = _guarded(np.empty((n, G), np.uint8), fill=True)
                t.rate_match(vin, rv, G, Q, out=vout)
                assert _same(cout(), want), (cap, rv, G)
    assert _same(cin(), coded)


def _soft(rng, shape, dtype, extremes=False):
    if dtype == np.int8:
        a = rng.integers(-127, 128, shape).astype(np.int8)
        if extremes:   # a prior buffer: -128 (read as -127 when added to) and +-127
            a[rng.random(shape) < 0.2] = -128
            a[rng.random(shape) < 0.1] = 127
            a[rng.random(shape) < 0.1] = -127
        return a
    return (4 * rng.standard_normal(shape)).astype(dtype)


@pytest.mark.parametrize("precision", ["f64", "f32", "fixed"])
@pytest.mark.parametrize("A,n", CASES)
def test_rate_dematch_equals_the_restatement(A, n, precision):
    p, Q, dt = T.plan(A), 2, NP_DT[precision]
    rng = np.random.default_rng(5 * A + n)
    for limited in (False, True):
        cap = _cap(p) if limited else 0
        with _tb(A, Ncb_cap=cap, filler_llr=FILLER[limited]) as t:
            for rv, lim, g, acc in CONFIGS:
                if lim != limited:
                    continue
                G = g(p, Q)
                f = _soft(rng, (n, G), dt)
                prior = _rand_pair(rng, p, n, lambda r, s: _soft(r, s, dt, extremes=True), lambda K: 3 * K + 12)
                want = T.rate_dematch(p, f, cap, rv, Q, FILLER[limited], prior if acc else None)
                vin, cin = _guarded(f)
                vout, cout = _guarded_pair(prior, fill=not acc)
                t.rate_dematch(vin, rv, Q, out=vout, accumulate=acc)
                got = cout()
                assert _same(got, want), (cap, rv, G, acc)
                assert _same(cin(), f)
                if p.F:   # the filler's d0 and d1, whatever was there; d2 is a sum like any other
                    k = np.arange(p.F)
                    blk0 = got[0][0] if p.C_minus else got[1][0]
                    assert (blk0[:, 3 * k] == T.filler_value(FILLER[limited], dt)).all()
                    assert (blk0[:, 3 * k + 1] == T.filler_value(FILLER[limited], dt)).all()
    assert T.filler_value(-63.5, np.int8) == -64 and T.filler_value(-1000.25, np.int8) == -127


# ------------------------------------------------------------------ 2: the round trip and the remainders
@pytest.mark.parametrize("A,n", [(1, 3), (16, 3), (17, 65), (6121, 3), (12217, 3), (12257, 65), (40961, 2)])
def test_round_trip_and_what_the_remainders_say(A, n):
    import torch
    p = T.plan(A)
    rng = np.random.default_rng(7 * A)
    x = _odd_bits(rng, (n, A))
    xd = torch.from_numpy(x).to(_dev())
    with _tb(A) as t:
        cb = t.segment(xd)
        tb, cbr, tbr = t.concat(cb)
        torch.cuda.synchronize()
        assert _same(tb.cpu().numpy(), (x != 0).astype(np.uint8))
        assert not cbr.any().item() and not tbr.any().item()
        blocks = lambda pr: T.unpair(p, pr)
        # one payload bit of one block of one transport block flipped: that block's gCRC24B remainder and
        # that transport block's gCRC24A remainder, and nothing else
        for r in range(p.C):
            row, i = int(rng.integers(n)), int(rng.integers(p.F if r == 0 else 0, T.block_sizes(p)[r] - p.L))
            hit = [None if b is None else b.clone() for b in cb]
            blocks(hit)[r][row, i] ^= 1
            _, c2, r2 = t.concat(tuple(hit))
            c2, r2 = c2.cpu().numpy(), r2.cpu().numpy()
            want_cb = np.zeros((n, p.C), bool)
            want_cb[row, r] = p.C > 1
            want_tb = np.zeros(n, bool)
            want_tb[row] = True
            assert np.array_equal(c2 != 0, want_cb) and np.array_equal(r2 != 0, want_tb), r
        # decoded filler bits are not believed
        if p.F:
            hit = [None if b is None else b.clone() for b in cb]
            blocks(hit)[0][:, :p.F] = torch.from_numpy(_odd_bits(rng, (n, p.F)) | 0x40).to(_dev())
            tb2, c2, r2 = t.concat(tuple(hit))
            assert _same(tb2.cpu().numpy(), (x != 0).astype(np.uint8)) and not c2.any().item() and not r2.any().item()


# ------------------------------------------------------------------ 3: blocks without filler = the single-block calls
def _codec(K, precision="f64", iterations=6):
    from turbo_decoder_cuda_amd import TurboCodec
    return TurboCodec(K, *QPP[K], iterations=iterations, precision=precision, algo="maxlog" if precision == "fixed" else "logmap")


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("A", [6121, 12257])
def test_blocks_without_filler_equal_the_single_block_calls(A, limited):
    """A = 6121: block 1 (K_plus); A = 12257: blocks 1 and 2 (K_plus), which send different E."""
    import torch
    p, n, Q = T.plan(A), 3, 2
    cap = _cap(p) if limited else 0
    rng = np.random.default_rng(11 * A)
    K = p.K_plus
    coded = _rand_pair(rng, p, n, lambda r, s: r.integers(0, 2, s, dtype=np.uint8), lambda K: 3 * K + 12)
    cd = tuple(torch.from_numpy(c).to(_dev()) for c in coded)
    codecs = {precision: _codec(K, precision) for precision in ("f64", "f32", "fixed")}
    with _tb(A, Ncb_cap=cap) as t, codecs["f64"], codecs["f32"], codecs["fixed"]:
        for c in codecs.values():
            c.set_rate_matching(min(cap, RM.layout(K)[3]) if cap else 0)
        for rv in range(4):
            G = (_g_punctured, _g_repeated)[rv % 2](p, Q)
            E = T.block_e(p, G, Q)
            at = np.concatenate([[0], np.cumsum(E)])
            f = t.rate_match(cd, rv, G, Q)
            for precision, c in codecs.items():
                soft = torch.from_numpy(_soft(rng, (n, G), NP_DT[precision])).to(_dev())
                prior = tuple(torch.from_numpy(_soft(rng, s, NP_DT[precision], True)).to(_dev())
                              for s in _shapes(p, n, lambda K: 3 * K + 12))
                mine = t.rate_dematch(soft, rv, Q, out=tuple(x.clone() for x in prior), accumulate=True)
                for r in range(p.C_minus, p.C):   # r >= 1: no filler
                    sl = slice(int(at[r]), int(at[r + 1]))
                    if precision == "f64":
                        e = c.rate_match(cd[1][r - p.C_minus], rv, E[r])
                        assert torch.equal(e, f[:, sl]), (rv, r)
                    theirs = c.rate_dematch(soft[:, sl].contiguous(), rv, out=prior[1][r - p.C_minus].clone(), accumulate=True)
                    assert theirs.cpu().numpy().tobytes() == mine[1][r - p.C_minus].cpu().numpy().tobytes(), (rv, r, precision)


# ------------------------------------------------------------------ 4: the closed loop
@pytest.mark.parametrize("rvs", [(0,), (0, 2)])
@pytest.mark.parametrize("A", [6121, 12257])
def test_closed_loop_noiseless(A, rvs):
    """segment -> encode (two codecs) -> rate_match -> BPSK -> demodulate -> rate_dematch (accumulated over
    `rvs`) -> decode with the CRC stop rule -> concat: the sent bits, every remainder zero."""
    import torch
    from turbo_decoder_cuda_amd import demodulate, modulate
    p, n = T.plan(A), 65
    x = np.random.default_rng(13 * A).integers(0, 2, (n, A), dtype=np.uint8)
    G = _g_punctured(p, 1)
    sizes = (p.K_minus, p.K_plus)
    codecs = [_codec(K) for K in sizes]
    try:
        for c in codecs:
            c.set_early_stop("crc", crc_poly=N.CRC24B)
        with _tb(A) as t:
            cb = t.segment(torch.from_numpy(x).to(_dev()))
            coded = tuple(c.encode(b.view(-1, K)).view(b.shape[0], n, 3 * K + 12) for c, b, K in zip(codecs, cb, sizes))
            soft = None
            for rv in rvs:
                f = t.rate_match(coded, rv, G, 1)
                si, sq = modulate(f.view(-1), 1)
                llr = demodulate(si, sq, 1, 1.0).view(n, G)
                soft = t.rate_dematch(llr, rv, 1, out=soft, accumulate=soft is not None)
            bits, iters = [], []
            for c, s, K in zip(codecs, soft, sizes):
                b, it = c.decode(s.view(-1, 3 * K + 12), iters_out=True)
                bits.append(b.view(s.shape[0], n, K))
                iters.append(it)
            tb, cbr, tbr = t.concat(tuple(bits))
            torch.cuda.synchronize()
            assert np.array_equal(tb.cpu().numpy(), x)
            assert not cbr.any().item() and not tbr.any().item()
            assert all(int(it.max()) < c.iterations for it, c in zip(iters, codecs)), "the CRC rule stopped every block"
    finally:
        for c in codecs:
            c.close()


# ------------------------------------------------------------------ 5: capture
def test_each_call_captured_into_a_graph_replays_to_the_same_bytes():
    import torch
    A, n, Q, rv = 12257, 3, 2, 1
    p = T.plan(A)
    G = _g_punctured(p, Q)
    rng = np.random.default_rng(17)
    dev = _dev()
    to = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    inputs = []   # two sets of inputs: captured on the first, replayed on the second and the first again
    for _ in range(2):
        inputs.append(dict(x=to(_odd_bits(rng, (n, A))), bits=tuple(map(to, _rand_pair(rng, p, n, _odd_bits))),
                           coded=tuple(map(to, _rand_pair(rng, p, n, _odd_bits, lambda K: 3 * K + 12))),
                           f=to(_soft(rng, (n, G), np.float32))))
    sb = torch.cuda.Stream(dev)
    with _tb(A) as t:
        def run(i, o, stream=None):
            t.segment(i["x"], out=o["cb"], stream=stream)
            t.rate_match(i["coded"], rv, G, Q, out=o["f"], stream=stream)
            t.rate_dematch(i["f"], rv, Q, out=o["soft"], stream=stream)
            t.concat(i["bits"], out=o["tb"], cb_rem=o["cb_rem"], tb_rem=o["tb_rem"], stream=stream)

        def outputs():
            e = lambda s, d: torch.full(s, 77, dtype=d, device=dev)
            return dict(cb=tuple(e(s, torch.uint8) for s in _shapes(p, n)), f=e((n, G), torch.uint8),
                        soft=tuple(e(s, torch.float32) for s in _shapes(p, n, lambda K: 3 * K + 12)),
                        tb=e((n, A), torch.uint8), cb_rem=e((n, p.C), torch.int32), tb_rem=e((n,), torch.int32))

        def flat(o):
            torch.cuda.synchronize()
            return [v.cpu().numpy().tobytes() for k in sorted(o) for v in (o[k] if isinstance(o[k], tuple) else (o[k],))]

        eager = []
        for i in inputs:
            o = outputs()
            run(i, o)
            eager.append(flat(o))
        assert eager[0] != eager[1]
        gin = {k: (tuple(x.clone() for x in v) if isinstance(v, tuple) else v.clone()) for k, v in inputs[0].items()}
        gout = outputs()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sb):
            run(gin, gout, stream=sb)
        for k in (1, 0):
            for name, v in inputs[k].items():
                for dst, src in zip(gin[name] if isinstance(v, tuple) else (gin[name],), v if isinstance(v, tuple) else (v,)):
                    dst.copy_(src)
            graph.replay()
            assert flat(gout) == eager[k], k


# ------------------------------------------------------------------ 6: argument checks; a failed call changes nothing
def test_bad_arguments_are_einval_and_change_nothing():
    import torch
    L = N.lib()
    A, n = 12257, 3
    p = T.plan(A)
    G = _g_punctured(p, 2)
    dev = _dev()
    junk = lambda s, d=torch.uint8: torch.full(s, 77, dtype=d, device=dev)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    with _tb(A) as t, _tb(100) as one:
        h = t._h
        x = junk((n, A))
        cb, coded = [junk(s) for s in _shapes(p, n)], [junk(s) for s in _shapes(p, n, lambda K: 3 * K + 12)]
        soft = [junk(s, torch.float64) for s in _shapes(p, n, lambda K: 3 * K + 12)]
        f, fs = junk((n, G)), junk((n, G), torch.float64)
        tb, cbr, tbr = junk((n, A)), junk((n, p.C), torch.int32), junk((n,), torch.int32)
        bad = [
            lambda: L.td_tb_segment(h, None, n, ptr(cb[0]), ptr(cb[1]), None),
            lambda: L.td_tb_segment(h, ptr(x), n, None, ptr(cb[1]), None),
            lambda: L.td_tb_segment(h, ptr(x), n, ptr(cb[0]), None, None),
            lambda: L.td_tb_segment(h, ptr(x), -1, ptr(cb[0]), ptr(cb[1]), None),
            lambda: L.td_tb_rate_match(h, None, ptr(coded[1]), n, 0, G, 2, ptr(f), None),
            lambda: L.td_tb_rate_match(h, ptr(coded[0]), ptr(coded[1]), n, 0, G, 2, None, None),
            lambda: L.td_tb_rate_match(h, ptr(coded[0]), ptr(coded[1]), n, 4, G, 2, ptr(f), None),
            lambda: L.td_tb_rate_match(h, ptr(coded[0]), ptr(coded[1]), n, -1, G, 2, ptr(f), None),
            lambda: L.td_tb_rate_match(h, ptr(coded[0]), ptr(coded[1]), n, 0, G + 1, 2, ptr(f), None),
            lambda: L.td_tb_rate_match(h, ptr(coded[0]), ptr(coded[1]), n, 0, 2 * (p.C - 1), 2, ptr(f), None),
            lambda: L.td_tb_rate_match(h, ptr(coded[0]), ptr(coded[1]), n, 0, G, 0, ptr(f), None),
            lambda: L.td_tb_rate_match(h, ptr(coded[0]), ptr(coded[1]), -2, 0, G, 2, ptr(f), None),
            lambda: L.td_tb_rate_dematch(h, ptr(fs), 7, n, 0, G, 2, ptr(soft[0]), ptr(soft[1]), 0, None),
            lambda: L.td_tb_rate_dematch(h, ptr(fs), N.TD_F64, n, 5, G, 2, ptr(soft[0]), ptr(soft[1]), 0, None),
            lambda: L.td_tb_rate_dematch(h, ptr(fs), N.TD_F64, n, 0, G + 1, 2, ptr(soft[0]), ptr(soft[1]), 0, None),
            lambda: L.td_tb_rate_dematch(h, None, N.TD_F64, n, 0, G, 2, ptr(soft[0]), ptr(soft[1]), 0, None),
            lambda: L.td_tb_rate_dematch(h, ptr(fs), N.TD_F64, n, 0, G, 2, None, ptr(soft[1]), 0, None),
            lambda: L.td_tb_concat(h, None, ptr(cb[1]), n, ptr(tb), ptr(cbr), ptr(tbr), None),
            lambda: L.td_tb_concat(h, ptr(cb[0]), ptr(cb[1]), n, None, ptr(cbr), ptr(tbr), None),
            lambda: L.td_tb_concat(h, ptr(cb[0]), ptr(cb[1]), -1, ptr(tb), ptr(cbr), ptr(tbr), None),
        ]
        for k, call in enumerate(bad):
            assert call() == N.TD_EINVAL and b"td_tb_" in L.td_last_error(), k
        torch.cuda.synchronize()
        for v in [x, *cb, *coded, *soft, f, fs, tb, cbr, tbr]:
            assert (v == 77).all().item()
        # N = 0 is a no-op, and an empty class takes a null pointer
        assert L.td_tb_segment(h, ptr(x), 0, ptr(cb[0]), ptr(cb[1]), None) == N.TD_OK
        assert one.plan.C_minus == 0
        y, o = junk((2, 100)), junk((1, 2, one.plan.K_plus))
        assert L.td_tb_segment(one._h, ptr(y), 2, None, ptr(o), None) == N.TD_OK
        torch.cuda.synchronize()
        assert ((o == 0) | (o == 1)).all().item() and (cb[0] == 77).all().item()
        # the wrapper refuses shapes the kernels would overrun
        with pytest.raises(ValueError):
            t.segment(x, out=(None, cb[1]))
        with pytest.raises(ValueError):
            t.segment(junk((n, A + 1)))
        with pytest.raises(ValueError):
            t.rate_dematch(fs, 0, 2, accumulate=True)
        with pytest.raises(N.TurboError):
            t.rate_match(tuple(coded), 0, G + 1, 2)
