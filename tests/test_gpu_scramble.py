"""Scrambling and the transport-block receive front end on the MI355X: td_gold_sequence word for word against
gold_ref's restatement of 36.211 7.2; td_scramble / td_descramble_llr against numpy; td_tb_demod_dematch byte
for byte against both the device composition that defines it (demodulate -> descramble -> convert_llr ->
rate_dematch) and the numpy restatement (pyoracle's demapper, gold_ref, frontend_ref's conversion, tb_ref's
de-rate-matching); the closed loop through scrambling; graph capture; argument checks.

Shapes.  Sequence: N = 1, 3, 65 and 257 (past gold_kernel's 256 row groups at 148 runs a row), the lengths
around one run of 1024 bits and 151424.  Front end: A = 1 (F = 15), 17 (K = 48), 6121 (one block of each size,
F = 15), 12257 (two K_plus blocks, F = 63) with N = 1, 3, 65, and A = 17 with N = 513 (past the 512 of the
grid's y).  Misalignment as in test_gpu_tb.py: tensors sit 5 elements into their allocation.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import frontend_ref as FR
import gold_ref as G
import pyoracle as O
import ratematch_ref as RM
import tb_ref as T
from conftest import gpu_available
from turbo_decoder_cuda_amd import _native as N

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

GUARD = 0xA5
PAD = 64
QPP = {3072: (47, 96), 3136: (13, 112)}   # the LTE pairs of the closed loop's two sizes
NP_DT = FR.NP_DT
STEPS = 8.0


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
        return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    if want is None:
        return got is None
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _np(x):
    return None if x is None else x.cpu().numpy()


def _cinits(n, seed):
    """n c_init values as int32: random, with 0, equal neighbours and one with bit 31 set (ignored)"""
    c = np.random.default_rng(seed).integers(0, 1 << 31, n, dtype=np.int64)
    if n > 1:
        c[1] = 0
    if n > 2:
        c[n // 2 + 1] = c[n // 2]
        c[-1] |= 1 << 31
    return c.astype(np.uint32).view(np.int32)


# ------------------------------------------------------------------ 1: the sequence
@pytest.mark.parametrize("n", [1, 3, 65, 257])
def test_gold_sequence_equals_the_restatement(n):
    import torch
    from turbo_decoder_cuda_amd import gold_sequence
    lengths = [151424] if n == 257 else G.edge_lengths(top=False) + [151424]
    cinit = _cinits(n, 100 + n)
    bits = G.bits(cinit.view(np.uint32), max(lengths))
    vin, cin = _guarded(cinit)
    for length in lengths:
        want = G.pack(bits[:, :length])
        vout, cout = _guarded(np.empty(want.shape, np.int32), fill=True)
        gold_sequence(vin, length, out=vout)
        got = cout().view(np.uint32)
        assert np.array_equal(got, want), (n, length)
    assert _same(cin(), cinit)
    made = gold_sequence(torch.from_numpy(cinit).to(_dev()), 77)   # a made output
    assert np.array_equal(made.cpu().numpy().view(np.uint32), G.pack(bits[:, :77]))
    assert gold_sequence(vin, 0).shape == (n, 0)


# ------------------------------------------------------------------ 2: scramble / descramble as calls of their own
def _odd_bits(rng, shape):
    """random bits whose ones are the bytes 0x01, 0x02, 0x80 and 0xFF"""
    return (rng.integers(0, 2, shape, dtype=np.uint8) * rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), shape)).astype(np.uint8)


def _soft(rng, shape, dtype, extremes=False):
    if dtype == np.int8:
        a = rng.integers(-127, 128, shape).astype(np.int8)
        if extremes:   # a prior buffer: -128 (read as -127 when added to) and +-127
            a[rng.random(shape) < 0.2] = -128
            a[rng.random(shape) < 0.1] = 127
            a[rng.random(shape) < 0.1] = -127
        return a
    return (4 * rng.standard_normal(shape)).astype(dtype)


def _special(rng, shape, dtype):
    a = _soft(rng, shape, dtype, extremes=True)
    flat = a.reshape(-1)
    vals = [-128, 127, -127, 0] if dtype == np.int8 else [0.0, -0.0, np.inf, -np.inf]
    for k, v in enumerate(vals * 3):   # each under both values of the sequence's bit, in all likelihood
        flat[(7 * k + 1) % flat.size] = v
    return a


@pytest.mark.parametrize("length", [1, 77, 1000, 4099])
def test_scramble_and_descramble_equal_numpy(length):
    """length 1000 with an aligned tensor takes the four-bytes-a-thread path; 5 elements in, the byte path"""
    import torch
    from turbo_decoder_cuda_amd import descramble, scramble
    n = 3
    rng = np.random.default_rng(length)
    cinit = _cinits(n, length)
    c = G.bits(cinit.view(np.uint32), length)
    seq = torch.from_numpy(G.pack(c).view(np.int32)).to(_dev())
    x = _odd_bits(rng, (n, length))
    for aligned in (False, True):
        hold = (lambda a, fill=False: (torch.from_numpy(a).to(_dev()) if not fill else
                                       torch.full((a.nbytes,), GUARD, dtype=torch.uint8, device=_dev())
                                       .view(getattr(torch, a.dtype.name)).view(a.shape), None)) if aligned else _guarded
        value = lambda v, chk: chk() if chk else v.cpu().numpy()
        # bits: out of place into garbage, then in place
        vin, cin = hold(x)
        vout, cout = hold(np.empty_like(x), fill=True)
        scramble(vin, seq, out=vout)
        assert _same(value(vout, cout), G.scramble(x, c)) and _same(value(vin, cin), x), aligned
        scramble(vin, seq, out=vin)
        assert _same(value(vin, cin), G.scramble(x, c)), aligned
        assert _same(scramble(vout, seq).cpu().numpy(), (x != 0).astype(np.uint8)), "twice: the bits again"
        for dt in NP_DT.values():
            v = _special(rng, (n, length), dt)
            want = G.descramble(v, c)
            vin, cin = hold(v)
            vout, cout = hold(np.empty_like(v), fill=True)
            descramble(vin, seq, out=vout)
            assert _same(value(vout, cout), want) and _same(value(vin, cin), v), (aligned, dt)
            descramble(vin, seq, out=vin)
            assert _same(value(vin, cin), want), (aligned, dt)
    assert np.array_equal(seq.cpu().numpy().view(np.uint32), G.pack(c)), "the sequence is only read"
    assert _same(G.descramble(np.array([[-128, -128, 5]], np.int8), np.array([[1, 0, 1]], np.uint8)), np.array([[127, -128, -5]], np.int8))
    z = G.descramble(np.array([[0.0, -0.0]]), np.array([[1, 1]], np.uint8))
    assert np.signbit(z[0, 0]) and not np.signbit(z[0, 1])


# ------------------------------------------------------------------ 3: the front end
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


# rv, limited buffer?, G, accumulate?: test_gpu_tb.py's four
CONFIGS = [(0, False, _g_punctured, False), (1, True, _g_repeated, True), (2, False, _g_repeated, True),
           (3, True, _g_punctured, False)]
FILLER = {False: -63.5, True: -1000.25}   # by limited buffer?: int8 -64 (ties to even) and -127 (clamped)


def _shapes(p, n, cols=lambda K: K):
    return ((p.C_minus, n, cols(p.K_minus)) if p.C_minus else None, (p.C_plus, n, cols(p.K_plus)))


def _front_end_case(A, n, M, Q, configs, restate=True):
    """td_tb_demod_dematch in all three precisions, with a sequence and without, for the given configs"""
    import torch
    from turbo_decoder_cuda_amd import convert_llr, demodulate, descramble
    p = T.plan(A)
    rng = np.random.default_rng(1000 * A + 10 * n + M)
    for rv, limited, g, acc in configs:
        cap, filler = (_cap(p) if limited else 0), FILLER[limited]
        Gn = g(p, Q)
        E = T.block_e(p, Gn, Q)
        assert all(e % M == 0 for e in E) and (p.C == 1 or len(set(E)) == 2)
        yi, yq = FR.symbols((n, Gn // M), seed=A + n + M + rv)
        cinit = _cinits(n, A + rv)
        c = G.bits(cinit.view(np.uint32), Gn)
        words = G.pack(c).view(np.int32)
        (vyi, cyi), (vyq, cyq), (vseq, cseq) = _guarded(yi), _guarded(yq), _guarded(words)
        llr = demodulate(vyi.view(-1), vyq.view(-1), M, FR.KF).view(n, Gn)
        e_np = O.demodulate(yi.reshape(-1), yq.reshape(-1), M, FR.KF).reshape(n, Gn) if restate else None
        with _tb(A, Ncb_cap=cap, filler_llr=filler) as t:
            for precision, dt in NP_DT.items():
                prior = tuple(None if s is None else _soft(rng, s, dt, extremes=True) for s in _shapes(p, n, lambda K: 3 * K + 12))
                for seq in (vseq, None):
                    soft = llr if seq is None else descramble(llr, seq)
                    f = convert_llr(soft, precision, STEPS)
                    composed = t.rate_dematch(f, rv, Q, accumulate=acc,
                                              out=tuple(None if a is None else torch.from_numpy(a).to(_dev()) for a in prior))
                    vout, cout = _guarded_pair(prior, fill=not acc)
                    t.demod_dematch(vyi, vyq, rv, Q, M, FR.KF, precision, STEPS, seq=seq, out=vout, accumulate=acc)
                    got = cout()
                    assert _same(got, tuple(map(_np, composed))), (rv, cap, Gn, acc, precision, seq is not None)
                    if restate and seq is not None:
                        want = T.rate_dematch(p, FR.convert(G.descramble(e_np, c), precision, STEPS), cap, rv, Q, filler,
                                              prior if acc else None)
                        assert _same(got, want), (rv, cap, Gn, acc, precision)
                    if p.F:
                        k = np.arange(p.F)
                        blk0 = got[0][0] if p.C_minus else got[1][0]
                        assert (blk0[:, 3 * k] == T.filler_value(filler, dt)).all() and (blk0[:, 3 * k + 1] == T.filler_value(filler, dt)).all()
            made = t.demod_dematch(vyi, vyq, rv, Q, M, FR.KF, "f32", seq=vseq) if not acc else None   # made outputs
            if made is not None:
                first = t.rate_dematch(convert_llr(descramble(llr, vseq), "f32"), rv, Q)
                assert _same(tuple(map(_np, made)), tuple(map(_np, first)))
        assert _same(cyi(), yi) and _same(cyq(), yq) and _same(cseq(), words), "the inputs are only read"


@pytest.mark.parametrize("qmul", [1, 2])
@pytest.mark.parametrize("M", FR.MODS)
@pytest.mark.parametrize("A,n", [(A, n) for A in (1, 17, 6121, 12257) for n in (1, 3, 65)])
def test_demod_dematch_equals_the_composition_and_the_restatement(A, n, M, qmul):
    _front_end_case(A, n, M, qmul * M, CONFIGS)


def test_demod_dematch_past_the_grid_cap():
    _front_end_case(17, 513, 2, 2, CONFIGS[:2])


# ------------------------------------------------------------------ 4: the closed loop through scrambling
def test_closed_loop_with_scrambling():
    """segment -> encode -> rate_match -> scramble -> QPSK -> demod_dematch(seq) -> decode -> concat: the sent bits
    and zero remainders with the sender's sequence; with another c_init's, no transport block passes."""
    import torch
    from turbo_decoder_cuda_amd import TurboCodec, gold_sequence, modulate, scramble
    A, n, M = 6121, 3, 2
    p = T.plan(A)
    x = np.random.default_rng(23).integers(0, 2, (n, A), dtype=np.uint8)
    Gn = _g_punctured(p, M)
    sizes = (p.K_minus, p.K_plus)
    codecs = [TurboCodec(K, *QPP[K], iterations=6) for K in sizes]
    try:
        with _tb(A) as t:
            cb = t.segment(torch.from_numpy(x).to(_dev()))
            coded = tuple(c.encode(b.view(-1, K)).view(b.shape[0], n, 3 * K + 12) for c, b, K in zip(codecs, cb, sizes))
            f = t.rate_match(coded, 0, Gn, M)
            cinit = torch.from_numpy(_cinits(n, 7)).to(_dev())
            seq = gold_sequence(cinit, Gn)
            si, sq = modulate(scramble(f, seq).view(-1), M)
            yi, yq = si.view(n, -1), sq.view(n, -1)
            for rx_seq, good in ((seq, True), (gold_sequence(cinit + 1, Gn), False)):
                soft = t.demod_dematch(yi, yq, 0, M, M, 1.0, "f64", seq=rx_seq)
                bits = tuple(c.decode(s.view(-1, 3 * K + 12)).view(s.shape[0], n, K) for c, s, K in zip(codecs, soft, sizes))
                tb, cbr, tbr = t.concat(bits)
                torch.cuda.synchronize()
                if good:
                    assert np.array_equal(tb.cpu().numpy(), x)
                    assert not cbr.any().item() and not tbr.any().item()
                else:
                    assert (tbr != 0).all().item()
    finally:
        for c in codecs:
            c.close()


# ------------------------------------------------------------------ 5: capture
def test_sequence_and_front_end_captured_into_one_graph_replay_to_the_same_bytes():
    import torch
    from turbo_decoder_cuda_amd import gold_sequence
    A, n, M, Q, rv = 12257, 3, 4, 4, 1
    p = T.plan(A)
    Gn = _g_punctured(p, Q)
    dev = _dev()
    sets = []
    for k in range(2):
        yi, yq = FR.symbols((n, Gn // M), seed=50 + k)
        sets.append((torch.from_numpy(yi).to(dev), torch.from_numpy(yq).to(dev), torch.from_numpy(_cinits(n, 60 + k)).to(dev)))
    outputs = lambda: tuple(torch.full(s, 77, dtype=torch.int8, device=dev) for s in _shapes(p, n, lambda K: 3 * K + 12))
    flat = lambda o: [v.cpu().numpy().tobytes() for v in o]
    sb = torch.cuda.Stream(dev)
    with _tb(A) as t:
        def run(yi, yq, cinit, seq, out, stream=None):
            gold_sequence(cinit, Gn, out=seq, stream=stream)
            t.demod_dematch(yi, yq, rv, Q, M, FR.KF, "fixed", STEPS, seq=seq, out=out, stream=stream)

        eager = []
        for yi, yq, cinit in sets:
            o = outputs()
            run(yi, yq, cinit, torch.empty((n, (Gn + 31) // 32), dtype=torch.int32, device=dev), o)
            torch.cuda.synchronize()
            eager.append(flat(o))
        assert eager[0] != eager[1]
        gin = [v.clone() for v in sets[0]]
        gseq, gout = torch.zeros((n, (Gn + 31) // 32), dtype=torch.int32, device=dev), outputs()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sb):
            run(*gin, gseq, gout, stream=sb)
        for k in (1, 0):
            for dst, src in zip(gin, sets[k]):
                dst.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            assert flat(gout) == eager[k], k


# ------------------------------------------------------------------ 6: argument checks; a failed call changes nothing
def test_bad_arguments_are_einval_and_change_nothing():
    import torch
    from turbo_decoder_cuda_amd import descramble, gold_sequence, scramble
    L = N.lib()
    A, n, M, Q = 12257, 3, 2, 4
    p = T.plan(A)
    Gn = _g_punctured(p, Q)
    dev = _dev()
    junk = lambda s, d=torch.uint8: torch.full(s, 77, dtype=d, device=dev)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    with _tb(A) as t:
        h = t._h
        yi, yq = junk((n, Gn // M), torch.float64), junk((n, Gn // M), torch.float64)
        seq = junk((n, (Gn + 31) // 32), torch.int32)
        soft = [junk(s, torch.float64) for s in _shapes(p, n, lambda K: 3 * K + 12)]
        call = lambda **kw: (lambda a: L.td_tb_demod_dematch(a["h"], a["yi"], a["yq"], a["prec"], a["n"], a["rv"], a["G"], a["Q"],
                                                              a["M"], 1.0, a["steps"], ptr(seq), a["minus"], a["plus"], 0, None))(
            {**dict(h=h, yi=ptr(yi), yq=ptr(yq), prec=N.TD_F64, n=n, rv=0, G=Gn, Q=Q, M=M, steps=8.0, minus=ptr(soft[0]),
                    plus=ptr(soft[1])), **kw})
        assert call() == N.TD_OK
        torch.cuda.synchronize()
        for s in soft:
            s.fill_(77)
        nan, inf = float("nan"), float("inf")
        bad = [dict(h=None), dict(yi=None), dict(yq=None), dict(prec=7), dict(n=-1), dict(rv=4), dict(rv=-1), dict(G=Gn + 1),
               dict(G=Q * (p.C - 1)), dict(Q=0), dict(M=5), dict(M=0), dict(M=8), dict(M=3), dict(M=6, Q=4), dict(minus=None),
               dict(plus=None)] + [dict(prec=N.TD_FIXED, steps=s) for s in (0.0, -8.0, nan, inf, -inf)]
        for kw in bad:
            assert call(**kw) == N.TD_EINVAL and b"td_tb_demod_dematch" in L.td_last_error(), kw
        torch.cuda.synchronize()
        for v in (yi, yq, seq, *soft):
            assert (v == 77).all().item()
        assert call(n=0) == N.TD_OK
        assert call(prec=N.TD_F32, steps=nan) == N.TD_OK, "steps_per_unit matters to TD_FIXED only"
        torch.cuda.synchronize()
        # the wrappers refuse shapes the kernels would overrun
        f64 = lambda s: torch.zeros(s, dtype=torch.float64, device=dev)
        with pytest.raises(ValueError):
            t.demod_dematch(f64((n, Gn // M)), f64((n, Gn // M + 1)), 0, Q, M, 1.0, "f64")
        with pytest.raises(ValueError):
            t.demod_dematch(f64((n, Gn // M)), f64((n, Gn // M)), 0, Q, M, 1.0, "f64", seq=seq[:, :-1].contiguous())
        with pytest.raises(ValueError):
            t.demod_dematch(f64((n, Gn // M)), f64((n, Gn // M)), 0, Q, M, 1.0, "f16")
        with pytest.raises(ValueError):
            t.demod_dematch(f64((n, Gn // M)), f64((n, Gn // M)), 0, 3, M, 1.0, "f64")
        with pytest.raises(ValueError):
            t.demod_dematch(f64((n, Gn // M)), f64((n, Gn // M)), 0, Q, M, 1.0, "f64", accumulate=True)
    bits = junk((n, 100))
    with pytest.raises(ValueError):
        scramble(bits, seq)   # 100 bits take 4 words a row
    with pytest.raises(ValueError):
        descramble(bits, seq[:, :4].contiguous())   # uint8 is no soft value
    with pytest.raises(ValueError):
        gold_sequence(junk((n,), torch.int64), 100)
    with pytest.raises(ValueError):
        gold_sequence(junk((n,), torch.int32), 1 << 31)
