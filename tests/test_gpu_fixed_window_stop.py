"""Early termination of the fixed-point decoder's sub-block schedule (td_set_fixed_window_stop) on the
MI355X, bit for bit against the rule applied to the rows of the full windowed fixed decode
(tests/fixed_window_ref.py, tests/fixed_window_stop_cases.py): the frozen rows, the final bits, the counts,
and Le for the iterations a codeword used.  A wave is 64 codewords times one sub-block and returns at
once when none of its codewords runs, so the batches sit round 64 and hold codewords that stop at
different iterations."""
import ctypes as C

import numpy as np
import pytest

import fixed_size_cases as Z
import fixed_stop_cases as S
import fixed_window_ref as FW
import fixed_window_stop_cases as FS
import window_stop_cases as W
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

ITERS = FS.ITERS
B = FS.B
SENTINEL = 12345


def _dev():
    import torch
    return torch.device("cuda", 0)


def _gpu(a):
    import torch
    return torch.from_numpy(np.array(a)).to(_dev())   # a copy: the references are read-only


def _codec(K, win, iters=ITERS, setting=None, qpp=None):
    from turbo_decoder_cuda_amd import TurboCodec
    c = TurboCodec(K, *(qpp or FS.QPP[K]), iterations=iters, algo="maxlog", precision="fixed")
    if setting is not None:
        c.set_fixed(*setting)
    if win is not None:
        c.set_fixed_window(*win)
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
    mask = FS.le_mask(used, iters)   # later entries are unspecified
    assert np.array_equal(np.where(mask, g_le, 0), np.where(mask, le, 0))


def _check(c, ref, used, n=None):
    """The decode with all_iters, then the final bits alone, of the first n codewords of a case."""
    q, rows, le = (a[:n] for a in ref[:3])
    used = used[:n]
    _equal(_decode(c, q), rows, le, used)
    _equal(_decode(c, q, all_iters=False), rows, le, used, all_iters=False)


@pytest.mark.parametrize("K,key,win,rule", FS.CASES)
def test_rule_equals_rule_on_restatement(K, key, win, rule):
    sp = FS.not_for_nothing(key, K, ITERS, win, rule)
    if (K, win, rule) == (40, (16, 5), "hda"):
        assert sp == {2: 46, 3: 37, 4: 9, 5: 5, 6: 3, 7: 1, 8: 29}
    if (K, win, rule) == (40, (16, 5), "crc"):
        assert sp == {1: 60, 2: 29, 3: 10, 4: 3, 5: 3, 8: 25}
    if (K, key, win) == (1024, ("awgn", 1.0, B), (64, 48)):
        assert sp == {3: 15, 4: 83, 5: 27, 6: 5}
    with _codec(K, win) as c:
        c.set_fixed_window_early_stop(rule)
        _check(c, FS.reference(key, K, ITERS, win), FS.used(key, K, ITERS, win, rule))


@pytest.mark.parametrize("rule", ["hda", "crc"])
@pytest.mark.parametrize("K,win", [(40, (16, 5)), (1024, (64, 48))])
def test_batch_edges_and_codeword_alone(K, win, rule):
    """B = 1, 63, 64 and 65 (a lane of the padding never runs), and codewords 0, 63, 64 and 129 alone:
    a codeword's rows, count and Le do not depend on its wave or its batch."""
    key = ("awgn", 1.0, B) if rule == "hda" else ("crc", 1.1 if K == 40 else 1.15, B)
    ref = FS.reference(key, K, ITERS, win)
    used = FS.used(key, K, ITERS, win, rule)
    with _codec(K, win) as c:
        c.set_fixed_window_early_stop(rule)
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
    """Wave 0 holds 64 copies of the earliest-stopping frame and returns at once from its stop on; waves 1
    and 2 go on."""
    ref = FS.whole_wave_case(1024, (64, 48))
    used = W.stops(ref[1], "hda")
    assert len(set(used[:64])) == 1 and used[0] == 3 and used[64:].max() == ITERS
    with _codec(1024, (64, 48)) as c:
        c.set_fixed_window_early_stop("hda")
        _check(c, ref, used)


def test_min_iters():
    """3 and 4 move the earlier stops; == iterations is the rule-off decode on every output byte."""
    import torch
    K, win = 40, (16, 5)
    with _codec(K, win) as c:
        for rule, key in (("hda", ("awgn", 1.0, B)), ("crc", ("crc", 1.1, B))):
            ref = FS.reference(key, K, ITERS, win)
            q, rows, le = ref
            first = FS.used(key, K, ITERS, win, rule)
            for m in (3, 4):
                late = FS.used(key, K, ITERS, win, rule, m)
                assert late.min() == m and late.max() == ITERS and np.array_equal(late[first >= m], first[first >= m])
                c.set_fixed_window_early_stop(rule, min_iters=m)
                _check(c, ref, late)
            c.set_fixed_window_early_stop(None)
            off = _decode(c, q)
            c.set_fixed_window_early_stop(rule, min_iters=ITERS)
            full = _decode(c, q)
            for a, b in zip(full, off):
                assert np.array_equal(a, b)
            assert np.array_equal(full[0], rows) and np.array_equal(full[1], le) and (full[2] == ITERS).all()
            assert torch.equal(c.decode(_gpu(q)), _gpu(rows[:, -1]))


def test_crc24a_on_crc24b_frames_stops_nothing():
    K, win, key = 1024, (64, 48), ("crc", 1.15, B)
    ref = FS.reference(key, K, ITERS, win)
    other = FS.used(key, K, ITERS, win, "crc", 1, FS.CRC24A)
    assert (other == ITERS).all() and FS.used(key, K, ITERS, win, "crc").min() < ITERS
    with _codec(K, win) as c:
        c.set_fixed_window_early_stop("crc", crc_poly=FS.CRC24A)
        _check(c, ref, other)


@pytest.mark.parametrize("rule", ["hda", "crc"])
@pytest.mark.parametrize("family", ["zero", "plus127", "minus128", "alternating", "mixed"])
@pytest.mark.parametrize("K,win", [(40, (16, 5)), (1024, (64, 48))])
def test_saturated_and_zero_inputs(K, win, family, rule):
    iters, n = 4, 65
    key = ("pattern", family, n)
    ref = FS.reference(key, K, iters, win)
    used = FS.used(key, K, iters, win, rule)
    print(W.spread(used))
    if family == "zero":
        assert (ref[1] == 1).all(), "the all-zero codeword decodes to an all-ones row"
        assert (used == (2 if rule == "hda" else iters)).all()
    with _codec(K, win, iters) as c:
        c.set_fixed_window_early_stop(rule)
        _check(c, ref, used)


@pytest.mark.parametrize("K", FS.RESIDUE_SIZES)
def test_a_size_of_every_residue(K):
    """L = K + 3 at every residue modulo the 16-step window through {16, 5} and {64, 48} with both rules, 65
    codewords (the pattern rows among them), 6 iterations; L = 191 has the longest last sub-block."""
    with _codec(K, None, FS.SIZE_ITERS, Z.setting(K), Z.interleaver(K)) as c:
        for win in ((16, 5), (64, 48)):
            c.set_fixed_window(*win)
            for rule in ("hda", "crc"):
                ref = FS.size_case(K, rule, win)
                print(K, win, rule, W.spread(ref[3]))
                assert len(W.spread(ref[3])) >= 2 and ref[3].min() < FS.SIZE_ITERS
                c.set_fixed_window_early_stop(rule, min_iters=1, crc_poly=FS.CRC24B)
                _check(c, ref, ref[3])


@pytest.mark.parametrize("K,n,ebn0", [(6144, 3, 1.5), (10000, 2, 2.0)])
def test_long_blocks(K, n, ebn0):
    iters, key, win = 4, ("awgn", ebn0, n), (64, 48)
    ref = FS.reference(key, K, iters, win)
    used = FS.used(key, K, iters, win, "hda")
    print(W.spread(used))
    assert used.min() < iters
    with _codec(K, win, iters) as c:
        c.set_fixed_window_early_stop("hda")
        _check(c, ref, used)


def test_rule_lifetime_and_host_entry_points():
    """The rule survives set_fixed and a later set_fixed_window with a window; set_fixed_window(0) clears it;
    the host entry points fill the counts."""
    K, key, n = 1024, ("awgn", 1.0, B), 65
    with _codec(K, (64, 48)) as c:
        c.set_fixed_window_early_stop("hda")
        c.set_fixed(31, 2)
        ref = FS.reference(key, K, ITERS, (64, 48), (31, 2))
        _check(c, ref, FS.used(key, K, ITERS, (64, 48), "hda", setting=(31, 2)), n)
        c.set_fixed_window(32, 7)
        ref = FS.reference(key, K, ITERS, (32, 7), (31, 2))
        u = FS.used(key, K, ITERS, (32, 7), "hda", setting=(31, 2))
        assert u.min() < ITERS
        _check(c, ref, u, n)
        rows, hle, cnt = c.TurboDecoding(ref[0][:3], return_le=True, return_iters=True)
        assert np.array_equal(cnt, u[:3]) and np.array_equal(rows, W.frozen(ref[1][:3], u[:3]))
        mask = FS.le_mask(u[:3], ITERS)
        assert np.array_equal(np.where(mask, hle, 0), np.where(mask, ref[2][:3], 0))
        assert np.array_equal(c.TurboDecoding(ref[0][:3]), W.frozen(ref[1][:3], u[:3]))
        c.set_fixed_window(0)   # clears the rule: back with a window, the decode is the full one
        assert c.early_stop is None
        c.set_fixed_window(32, 7)
        got = _decode(c, ref[0][:n])
        assert (got[2] == ITERS).all() and np.array_equal(got[0], ref[1][:n]) and np.array_equal(got[1], ref[2][:n])
        rows, hle, cnt = c.TurboDecoding(ref[0][:3], return_le=True, return_iters=True)
        assert (cnt == ITERS).all() and np.array_equal(rows, ref[1][:3]) and np.array_equal(hle, ref[2][:3])
        c.set_fixed_window_early_stop("hda")
        c.set_fixed_window_early_stop(None)   # None turns it off as well
        got = _decode(c, ref[0][:n])
        assert (got[2] == ITERS).all() and np.array_equal(got[0], ref[1][:n])


def test_bad_arguments_are_einval_and_change_nothing():
    from turbo_decoder_cuda_amd import TurboCodec, _native as N
    L = N.lib()
    K, key, win = 40, ("crc", 1.1, B), (16, 5)
    ref = FS.reference(key, K, ITERS, win)
    used = FS.used(key, K, ITERS, win, "crc")

    def einval(call, who="td_set_fixed_window_stop"):
        assert call() == N.TD_EINVAL
        assert who in L.td_last_error().decode(), L.td_last_error()

    with _codec(K, win) as c:
        c.set_fixed_window_early_stop("crc")
        bad = [N.TdStopParams(3, 1, FS.CRC24B), N.TdStopParams(-1, 1, FS.CRC24B), N.TdStopParams(N.TD_STOP_HDA, 0, 0),
               N.TdStopParams(N.TD_STOP_HDA, ITERS + 1, 0), N.TdStopParams(N.TD_STOP_CRC, 1, 0),
               N.TdStopParams(N.TD_STOP_CRC, 1, 0x1000000)]
        for s in bad:
            einval(lambda: L.td_set_fixed_window_stop(c._h, C.byref(s)))
        with pytest.raises(ValueError):
            c.set_fixed_window_early_stop("sometimes")
        # the exact schedule's rule cannot join a window, with or without the window's rule
        s = N.TdStopParams(N.TD_STOP_HDA, 1, 0)
        einval(lambda: L.td_set_fixed_stop(c._h, C.byref(s)), "td_set_fixed_stop")
        g, ms = C.c_double(), C.c_double()
        einval(lambda: L.td_clock_read(c._h, C.byref(g), C.byref(ms)), "td_clock_read")
        _check(c, ref, used, 65)   # the previous rule is still in force
        # without a window the call is an error, NULL included, and td_set_fixed_stop's rule keeps the window out
        c.set_fixed_window(0)
        einval(lambda: L.td_set_fixed_window_stop(c._h, C.byref(s)))
        einval(lambda: L.td_set_fixed_window_stop(c._h, None))
        with pytest.raises(N.TurboError) as e:
            c.set_fixed_window_early_stop("hda")
        assert e.value.code == N.TD_EINVAL
        c.set_fixed_early_stop("crc")
        w = N.TdFixedWindowParams(*win)
        einval(lambda: L.td_set_fixed_window(c._h, C.byref(w)), "td_set_fixed_window")
        _check(c, S.reference(key, K, ITERS, (255, 3)), S.used(key, K, ITERS, (255, 3), "crc"), 65)
    with _codec(16, (16, 0)) as short:   # CRC needs K > 24
        with pytest.raises(N.TurboError) as e:
            short.set_fixed_window_early_stop("crc")
        assert e.value.code == N.TD_EINVAL
        short.set_fixed_window_early_stop("hda")
    with TurboCodec(40, 3, 10, iterations=2) as f64:
        with pytest.raises(N.TurboError) as e:
            f64.set_fixed_window_early_stop("hda")
        assert e.value.code == N.TD_EINVAL and "td_set_fixed_window_stop" in str(e.value)


def test_graph_capture_after_reserve_replays_the_eager_result():
    import torch
    K, n, win = 1024, 65, (64, 48)
    refs = [FS.reference(("awgn", e, B), K, ITERS, win) for e in (1.0, 0.5)]
    useds = [FS.used(("awgn", e, B), K, ITERS, win, "hda")[:n] for e in (1.0, 0.5)]
    sb = torch.cuda.Stream(_dev())
    with _codec(K, win) as c:
        c.set_fixed_window_early_stop("hda")
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
            mask = FS.le_mask(useds[k], ITERS)
            assert np.array_equal(np.where(mask, got[1], 0), np.where(mask, eager[1], 0))
