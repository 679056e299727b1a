"""Early termination of the fixed-point decoder (td_set_fixed_stop) on the MI355X, bit for bit against
the rule applied to the rows of the full fixed decode (tests/fixed_ref.py, tests/fixed_stop_cases.py):
the frozen rows, the final bits, the counts, and Le for the iterations a codeword used.  The kernel
decodes one codeword per lane and a wave of 64 leaves once all of its codewords have stopped, so the
batches sit round 64 and hold codewords that stop at different iterations."""
import numpy as np
import pytest

import fixed_stop_cases as S
import window_stop_cases as W
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

ITERS = W.ITERS
SENTINEL = 12345


def _dev():
    import torch
    return torch.device("cuda", 0)


def _gpu(a):
    import torch
    return torch.from_numpy(np.array(a)).to(_dev())   # a copy: the references are read-only


def _codec(K, iters=ITERS, setting=None):
    from turbo_decoder_cuda_amd import TurboCodec
    c = TurboCodec(K, *S.QPP[K], iterations=iters, algo="maxlog", precision="fixed")
    if setting is not None:
        c.set_fixed(*setting)
    return c


def _decode(c, q, all_iters=True):
    """(rows or bits, Le prefilled with the sentinel, counts) of one GPU decode, as numpy."""
    import torch
    x = _gpu(q)
    g_le = torch.full((q.shape[0], c.iterations, 2, c.K + 3), SENTINEL, dtype=torch.int16, device=_dev())
    out, n = c.decode(x, all_iters=all_iters, le=g_le, iters_out=True)
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), q), "d_llr is not modified"
    return out.cpu().numpy(), g_le.cpu().numpy(), n.cpu().numpy()


def _equal(got, rows, le, used, all_iters=True):
    """got = _decode(...) against the reference rows / Le of the same codewords and their counts."""
    g_out, g_le, g_used = got
    iters = rows.shape[1]
    assert np.array_equal(g_used, used), (W.spread(g_used), W.spread(used))
    if all_iters:
        assert np.array_equal(g_out, W.frozen(rows, used))
    else:
        assert np.array_equal(g_out, rows[np.arange(len(used)), used - 1])
    mask = S.le_mask(used, iters)   # later entries are unspecified
    assert np.array_equal(np.where(mask, g_le, 0), np.where(mask, le, 0))


def _check(c, ref, used, B=None):
    """The decode with all_iters, then the final bits alone, of the first B codewords of a case."""
    q, rows, le = (a[:B] for a in ref)
    used = used[:B]
    _equal(_decode(c, q), rows, le, used)
    _equal(_decode(c, q, all_iters=False), rows, le, used, all_iters=False)


def _spread_ok(used, iters, below=True, reaches=True):
    """A case whose codewords all stop together cannot pass for nothing."""
    sp = W.spread(used)
    print(sp)
    assert len(sp) >= 3, sp
    assert not below or min(sp) < iters, sp
    assert not reaches or max(sp) == iters, sp
    return sp


# K, Eb/N0, setting, reaches `iterations`
HDA_CASES = [(40, 1.0, (255, 3), True), (200, 1.0, (255, 3), True), (1024, 0.5, (255, 3), True),
             (1024, 1.0, (255, 3), False), (1024, 1.0, (31, 2), True), (1024, 1.0, (255, 4), True)]
CRC_CASES = [(40, 1.1), (200, 1.15), (1024, 1.15)]
B = 130


@pytest.mark.parametrize("K,ebn0,setting,reaches", HDA_CASES)
def test_hda_equals_rule_on_restatement(K, ebn0, setting, reaches):
    key = ("awgn", ebn0, B)
    used = S.used(key, K, ITERS, setting, "hda")
    sp = _spread_ok(used, ITERS, reaches=reaches)
    if (K, ebn0, setting) == (40, 1.0, (255, 3)):
        assert sp == {2: 59, 3: 35, 4: 6, 5: 1, 6: 1, 7: 2, 8: 26}
    if (K, ebn0, setting) == (1024, 0.5, (255, 3)):
        assert sp == {4: 11, 5: 34, 6: 27, 7: 14, 8: 44}
    if (K, ebn0, setting) == (1024, 1.0, (255, 3)):
        assert sp == {3: 14, 4: 81, 5: 30, 6: 5}
    with _codec(K, ITERS, setting) as c:
        c.set_fixed_early_stop("hda")
        _check(c, S.reference(key, K, ITERS, setting), used)


@pytest.mark.parametrize("K,sigma", CRC_CASES)
def test_crc_equals_rule_on_restatement(K, sigma):
    """Frames carrying gCRC24B.  Judged with gCRC24A none of them passes: no false stop.  min_iters = 3
    moves the earlier stops to 3 or later; min_iters == iterations is the rule-off decode on every output
    byte."""
    import torch
    key, setting = ("crc", sigma, B), (255, 3)
    ref = S.reference(key, K, ITERS, setting)
    q, rows, le = ref
    used = S.used(key, K, ITERS, setting, "crc")
    sp = _spread_ok(used, ITERS)
    if K == 40:
        assert sp == {1: 76, 2: 24, 3: 6, 4: 4, 5: 1, 6: 1, 8: 18}
    if K == 1024:
        assert sp == {2: 3, 3: 18, 4: 45, 5: 31, 6: 11, 7: 4, 8: 18}
    with _codec(K) as c:
        c.set_fixed_early_stop("crc")
        _check(c, ref, used)
        other = S.used(key, K, ITERS, setting, "crc", 1, S.CRC24A)
        assert (other == ITERS).all()
        c.set_fixed_early_stop("crc", crc_poly=S.CRC24A)
        _check(c, ref, other)
        late = S.used(key, K, ITERS, setting, "crc", 3)
        assert late.min() == 3 and np.array_equal(late[used >= 3], used[used >= 3])
        if K > 40:   # (at K = 40 a row that passed by chance after 1 or 2 iterations need not pass after 3)
            assert np.array_equal(late, np.maximum(used, 3))
        c.set_fixed_early_stop("crc", min_iters=3)
        _check(c, ref, late)
        c.set_fixed_early_stop(None)
        off = _decode(c, q)
        c.set_fixed_early_stop("crc", min_iters=ITERS)
        full = _decode(c, q)
        for a, b in zip(full, off):
            assert np.array_equal(a, b)
        assert np.array_equal(full[0], rows) and np.array_equal(full[1], le) and (full[2] == ITERS).all()
        assert torch.equal(c.decode(_gpu(q)), _gpu(rows[:, -1]))


def test_hda_min_iters():
    K, key, setting = 40, ("awgn", 1.0, B), (255, 3)
    ref = S.reference(key, K, ITERS, setting)
    q, rows, le = ref
    with _codec(K) as c:
        late = S.used(key, K, ITERS, setting, "hda", 4)
        assert late.min() == 4 and late.max() == ITERS
        c.set_fixed_early_stop("hda", min_iters=4)
        _check(c, ref, late)
        c.set_fixed_early_stop("hda", min_iters=ITERS)
        full = _decode(c, q)
        assert np.array_equal(full[0], rows) and np.array_equal(full[1], le) and (full[2] == ITERS).all()


@pytest.mark.parametrize("rule", ["hda", "crc"])
@pytest.mark.parametrize("K", [40, 1024])
def test_batch_edges_and_codeword_alone(K, rule):
    """B = 1, 63, 64 and 65 (a lane of the padding never runs), and codewords 0, 63, 64 and 129 alone:
    a codeword's rows, count and Le do not depend on its wave or its batch."""
    key = ("awgn", 1.0, B) if rule == "hda" else ("crc", 1.1 if K == 40 else 1.15, B)
    ref = S.reference(key, K, ITERS, (255, 3))
    used = S.used(key, K, ITERS, (255, 3), rule)
    with _codec(K) as c:
        c.set_fixed_early_stop(rule)
        for n in (65, 1, 64, 63):
            _check(c, ref, used, n)
        whole = _decode(c, ref[0])
        for b in (0, 63, 64, 129):
            alone = _decode(c, ref[0][b:b + 1])
            _equal(alone, ref[1][b:b + 1], ref[2][b:b + 1], used[b:b + 1])
            n = int(used[b])
            assert np.array_equal(alone[0][0], whole[0][b]) and alone[2][0] == whole[2][b]
            assert np.array_equal(alone[1][0, :n], whole[1][b, :n])


def test_whole_wave_exit():
    """Wave 0 holds 64 copies of the earliest-stopping frame and leaves at once; waves 1 and 2 go on."""
    ref = S.whole_wave_case(1024)
    used = W.stops(ref[1], "hda")
    assert len(set(used[:64])) == 1 and used[0] == 3 and used[64:].max() == ITERS
    with _codec(1024) as c:
        c.set_fixed_early_stop("hda")
        _check(c, ref, used)


@pytest.mark.parametrize("rule", ["hda", "crc"])
@pytest.mark.parametrize("family", ["zero", "plus127", "minus128", "alternating", "mixed"])
@pytest.mark.parametrize("K", [40, 1024])
def test_saturated_and_zero_inputs(K, family, rule):
    iters, n = 4, 65
    key = ("pattern", family, n)
    ref = S.reference(key, K, iters, (255, 3))
    used = S.used(key, K, iters, (255, 3), rule)
    print(W.spread(used))
    if family == "zero":
        assert (ref[1] == 1).all(), "the all-zero codeword decodes to an all-ones row"
        assert (used == (2 if rule == "hda" else iters)).all()
    with _codec(K, iters) as c:
        c.set_fixed_early_stop(rule)
        _check(c, ref, used)


@pytest.mark.parametrize("K,n,ebn0", [(6144, 3, 1.5), (10000, 2, 2.0)])
def test_long_blocks(K, n, ebn0):
    iters, key = 4, ("awgn", ebn0, n)
    ref = S.reference(key, K, iters, (255, 3))
    used = S.used(key, K, iters, (255, 3), "hda")
    print(W.spread(used))
    assert used.min() < iters
    with _codec(K, iters) as c:
        c.set_fixed_early_stop("hda")
        _check(c, ref, used)


def test_rule_survives_set_fixed_and_none_turns_it_off():
    K, key = 1024, ("awgn", 1.0, B)
    n = 65
    with _codec(K) as c:
        c.set_fixed_early_stop("hda")
        c.set_fixed(31, 2)
        ref = S.reference(key, K, ITERS, (31, 2))
        _check(c, ref, S.used(key, K, ITERS, (31, 2), "hda"), n)
        c.set_fixed_early_stop(None)
        got = _decode(c, ref[0][:n])
        assert (got[2] == ITERS).all() and np.array_equal(got[0], ref[1][:n]) and np.array_equal(got[1], ref[2][:n])
        rows, hle, cnt = c.TurboDecoding(ref[0][:3], return_le=True, return_iters=True)
        assert (cnt == ITERS).all() and np.array_equal(rows, ref[1][:3])
        c.set_fixed_early_stop("hda")   # the host entry points fill the counts too
        u = S.used(key, K, ITERS, (31, 2), "hda")[:3]
        rows, hle, cnt = c.TurboDecoding(ref[0][:3], return_le=True, return_iters=True)
        assert np.array_equal(cnt, u) and np.array_equal(rows, W.frozen(ref[1][:3], u))
        assert np.array_equal(c.TurboDecoding(ref[0][:3]), W.frozen(ref[1][:3], u))


def test_bad_arguments_are_einval_and_change_nothing():
    import ctypes as C
    from turbo_decoder_cuda_amd import TurboCodec, _native as N
    K, key = 40, ("crc", 1.1, B)
    ref = S.reference(key, K, ITERS, (255, 3))
    used = S.used(key, K, ITERS, (255, 3), "crc")
    with _codec(K) as c:
        c.set_fixed_early_stop("crc")
        bad = [N.TdStopParams(3, 1, S.CRC24B), N.TdStopParams(-1, 1, S.CRC24B), N.TdStopParams(N.TD_STOP_HDA, 0, 0),
               N.TdStopParams(N.TD_STOP_HDA, ITERS + 1, 0), N.TdStopParams(N.TD_STOP_CRC, 1, 0),
               N.TdStopParams(N.TD_STOP_CRC, 1, 0x1000000)]
        for s in bad:
            assert N.lib().td_set_fixed_stop(c._h, C.byref(s)) == N.TD_EINVAL, (s.rule, s.min_iters, s.crc_poly)
            assert b"td_set_fixed_stop" in N.lib().td_last_error()
        with pytest.raises(ValueError):
            c.set_fixed_early_stop("sometimes")
        _check(c, ref, used, 65)   # the previous rule is still in force
    with _codec(16) as short:   # CRC needs K > 24
        with pytest.raises(N.TurboError) as e:
            short.set_fixed_early_stop("crc")
        assert e.value.code == N.TD_EINVAL
        short.set_fixed_early_stop("hda")
    with TurboCodec(40, 3, 10, iterations=2) as f64:
        with pytest.raises(N.TurboError) as e:
            f64.set_fixed_early_stop("hda")
        assert e.value.code == N.TD_EINVAL and "td_set_fixed_stop" in str(e.value)


def test_graph_capture_after_reserve_replays_the_eager_result():
    import torch
    K, n = 1024, 65
    refs = [S.reference(("awgn", e, B), K, ITERS, (255, 3)) for e in (1.0, 0.5)]
    useds = [S.used(("awgn", e, B), K, ITERS, (255, 3), "hda")[:n] for e in (1.0, 0.5)]
    sb = torch.cuda.Stream(_dev())
    with _codec(K) as c:
        c.set_fixed_early_stop("hda")
        c.reserve(n)
        gin = _gpu(refs[0][0][:n]).clone()
        gout = torch.empty((n, ITERS, K), dtype=torch.uint8, device=_dev())
        gle = torch.empty((n, ITERS, 2, K + 3), dtype=torch.int16, device=_dev())
        gcnt = torch.empty((n,), dtype=torch.int32, device=_dev())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sb):
            c.decode(gin, gout, all_iters=True, le=gle, stream=sb, iters_out=gcnt)
        for k in (1, 0):
            q, rows, le = (a[:n] for a in refs[k])
            gin.copy_(_gpu(q))
            gle.fill_(SENTINEL)
            graph.replay()
            torch.cuda.synchronize()
            got = (gout.cpu().numpy().copy(), gle.cpu().numpy().copy(), gcnt.cpu().numpy().copy())
            _equal(got, rows, le, useds[k])
            eager = _decode(c, q)
            assert np.array_equal(got[0], eager[0]) and np.array_equal(got[2], eager[2])
            mask = S.le_mask(useds[k], ITERS)
            assert np.array_equal(np.where(mask, got[1], 0), np.where(mask, eager[1], 0))
