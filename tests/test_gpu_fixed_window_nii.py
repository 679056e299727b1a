"""Next-iteration initialisation of the fixed-point decoder's sub-block schedule (td_set_fixed_window_nii) on the
MI355X against its numpy restatement (tests/fixed_window_nii_ref.py): hard-decision rows of every iteration,
final bits and every extrinsic value, bit for bit, with the plain max and the table, with the rules off
and on.  The integer arithmetic rounds nowhere and max is unchanged by the constant the kernel takes off
every stored vector, so every detail of the schedule shows in the bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import fixed_ref as F
import fixed_stop_cases as S
import fixed_window_nii_cases as NC
import fixed_window_nii_ref as FN
import fixed_window_ref as FW
import pyoracle as O
import window_stop_cases as W
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SENTINEL = 12345
ITERS = NC.ITERS
K1, WIN1 = NC.STOP_K, NC.STOP_WIN   # 1024, {64, 16}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _gpu(a):
    import torch
    return torch.from_numpy(np.array(a)).to(_dev())   # a copy: the references are read-only


def _qpp(K):
    return S.QPP.get(K) or NC.interleaver(K)


def _codec(K, iters, win, nii=True, table=False):
    from turbo_decoder_cuda_amd import TurboCodec
    c = TurboCodec(K, *_qpp(K), iterations=iters, algo="maxlog", precision="fixed")
    c.set_fixed(*NC.setting(table))
    if table:
        c.set_fixed_maxstar()
    if win is not None:
        c.set_fixed_window(*win, nii=nii)
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


def _check(c, q, rows, le):
    """Rule off: rows of every iteration, every Le, every count `iterations`; then the final bits alone."""
    g_rows, g_le, g_n = _decode(c, q)
    assert np.array_equal(g_rows, rows) and np.array_equal(g_le, le) and (g_n == c.iterations).all()
    g_bits, g_le, _ = _decode(c, q, all_iters=False)
    assert np.array_equal(g_bits, rows[:, -1]) and np.array_equal(g_le, le)


def _equal_stop(got, rows, le, used, all_iters=True):
    g_out, g_le, g_used = got
    assert np.array_equal(g_used, used), (W.spread(g_used), W.spread(used))
    if all_iters:
        assert np.array_equal(g_out, W.frozen(rows, used))
    else:
        assert np.array_equal(g_out, rows[np.arange(len(used)), used - 1])
    mask = S.le_mask(used, rows.shape[1])   # later entries are unspecified
    assert np.array_equal(np.where(mask, g_le, 0), np.where(mask, le, 0))


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("K,W_,g", NC.GEOMETRIES)
def test_geometry_equals_restatement(K, W_, g, table):
    """The lane-code test's geometries at B = 5 (a frame, the three saturated patterns, a frame), 1, 2, 3 and
    8 iterations: own-end and window-start alpha stores, one and two beta stores, beta taken where states are
    unreachable, overlaps of several sub-blocks and past the trellis."""
    rows, le = NC.reference(K, W_, g, table)
    q = NC.batch(K)[:5]
    for iters in (1, 2, 3, 8):
        with _codec(K, iters, (W_, g), table=table) as c:
            _check(c, q, rows[:5, :iters], le[:5, :iters])


@functools.lru_cache(maxsize=None)
def _long(K, B, win):
    q = F.quantise(O.synth_batch(K, *_qpp(K), 0.5, 5, B)[1], 8)
    return (q, *FN.decode(q, K, *_qpp(K), 2, *win))


@pytest.mark.parametrize("K,B,win", [(6144, 3, (64, 16)), (10000, 2, (64, 32))])
def test_long_blocks(K, B, win):
    q, rows, le = _long(K, B, win)
    off = FW.decode(q[:1], K, *_qpp(K), 2, *win)
    assert (off[0] != rows[:1]).any() or (off[1] != le[:1]).any(), "NII shows on these frames"
    with _codec(K, 2, win) as c:
        _check(c, q, rows, le)


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("table", [False, True])
def test_batches_and_a_codeword_alone(table):
    """B = 1, 65 and 130 (padding, several waves), and codeword 7 alone equals its row in the batch: 130
    frames at 1.0 dB under {64, 16}, 8 iterations, one restatement."""
    q, rows, le = NC.stop_reference(("awgn", 1.0), table)
    with _codec(K1, ITERS, WIN1, table=table) as c:
        for n in (130, 1, 65):
            _check(c, q[:n], rows[:n], le[:n])
        whole, alone = _decode(c, q), _decode(c, q[7:8])
        assert np.array_equal(alone[0][0], whole[0][7]) and np.array_equal(alone[1][0], whole[1][7])
        assert np.array_equal(alone[0][0], rows[7])


def test_nii_is_not_nii_off_on_these_frames():
    """What the tests compare against is not the NII-off decode: a kernel that ignored the flag fails them."""
    q, rows, le = NC.stop_reference(("awgn", 1.0))
    off_rows, off_le = FW.decode(q[:8], K1, *_qpp(K1), ITERS, *WIN1)
    assert np.array_equal(off_rows[:, 0], rows[:8, 0]) and np.array_equal(off_le[:, 0], le[:8, 0])
    assert (off_rows != rows[:8]).any() and (off_le != le[:8]).any()


# ------------------------------------------------------------------ early termination
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("key,rule", [(("awgn", 1.0), "hda"), (("crc", 1.15), "crc")])
def test_rules_judge_the_nii_decodes_rows(key, rule, table):
    """130 codewords that stop at four or more different iterations, at least two in each wave: counts, frozen
    rows, final bits and the Le of the iterations used are the rule applied to the NII restatement's rows;
    min_iters == iterations is the rule-off NII decode byte for byte."""
    q, rows, le = NC.stop_reference(key, table)
    used = NC.stop_used(key, rule, table)
    sp = W.spread(used)
    assert len(sp) >= 3 and min(sp) < ITERS and all(len(W.spread(used[w:w + 64])) >= 2 for w in (0, 64)), sp
    if not table:   # and not the counts of the NII-off decode
        import fixed_window_stop_cases as FS
        assert (FS.used((key[0], key[1], NC.STOP_B), K1, ITERS, WIN1, rule) != used).any()
    with _codec(K1, ITERS, WIN1, table=table) as c:
        c.set_fixed_window_early_stop(rule)
        _equal_stop(_decode(c, q), rows, le, used)
        _equal_stop(_decode(c, q, all_iters=False), rows, le, used, all_iters=False)
        _equal_stop(_decode(c, q[:65]), rows[:65], le[:65], used[:65])
        late = NC.stop_used(key, rule, table, 4)
        c.set_fixed_window_early_stop(rule, min_iters=4)
        _equal_stop(_decode(c, q), rows, le, late)
        c.set_fixed_window_early_stop(None)
        off = _decode(c, q)
        c.set_fixed_window_early_stop(rule, min_iters=ITERS)
        full = _decode(c, q)
        for a, b in zip(full, off):
            assert np.array_equal(a, b)
        assert np.array_equal(full[0], rows) and np.array_equal(full[1], le) and (full[2] == ITERS).all()


# ------------------------------------------------------------------ history
def test_a_decode_does_not_depend_on_the_one_before():
    """Two different batches one after the other on one handle, twice over: each equals its own restatement."""
    a, b = NC.stop_reference(("awgn", 1.0)), NC.stop_reference(("crc", 1.15))
    with _codec(K1, ITERS, WIN1) as c:
        for q, rows, le in (a, b, a):
            _check(c, q[:65], rows[:65], le[:65])
        c.set_fixed_window_early_stop("hda")   # a stopped codeword leaves its state behind: the next decode ignores it
        u = NC.stop_used(("awgn", 1.0), "hda")
        _equal_stop(_decode(c, a[0]), a[1], a[2], u)
        c.set_fixed_window_early_stop(None)
        _check(c, b[0][:65], b[1][:65], b[2][:65])


def test_graph_capture_after_reserve_replays_the_eager_result():
    """reserve() after the setters sizes the NII state too: the captured decode allocates nothing.  Replayed
    twice on one input and once on another, the bytes repeat and equal the eager decode's: the state is
    never read in iteration 1, so what the replay before left in it does not matter."""
    import torch
    n = 65
    refs = [NC.stop_reference(("awgn", 1.0)), NC.stop_reference(("crc", 1.15))]
    sb = torch.cuda.Stream(_dev())
    with _codec(K1, ITERS, WIN1) as c:
        c.reserve(n)
        bytes_reserved = c.workspace_bytes()
        gin = _gpu(refs[0][0][:n]).clone()
        gout = torch.empty((n, ITERS, K1), dtype=torch.uint8, device=_dev())
        gle = torch.empty((n, ITERS, 2, K1 + 3), dtype=torch.int16, device=_dev())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sb):
            c.decode(gin, gout, all_iters=True, le=gle, stream=sb)
        prev = None
        for k in (0, 0, 1):
            q, rows, le = (a[:n] for a in refs[k])
            gin.copy_(_gpu(q))
            gle.fill_(SENTINEL)
            graph.replay()
            torch.cuda.synchronize()
            got = (gout.cpu().numpy().copy(), gle.cpu().numpy().copy())
            assert np.array_equal(got[0], rows) and np.array_equal(got[1], le)
            if prev is not None and k == 0:
                assert all(np.array_equal(x, y) for x, y in zip(got, prev)), "a replay repeats the bytes"
            prev = got
            eager = _decode(c, q)
            assert np.array_equal(got[0], eager[0]) and np.array_equal(got[1], eager[1])
        assert c.workspace_bytes() == bytes_reserved


# ------------------------------------------------------------------ switches
def _parent_workspace_bytes(B, K, iters):
    """fx_carve's layout (csrc/td_fixed.h) restated: what a handle without NII reserves."""
    up = lambda v: (v + 255) // 256 * 256
    L, Bp = K + 3, (B + 63) // 64 * 64
    nW = (L + 15) // 16
    return (up((L + 3) * Bp) + 2 * up(L * Bp) + 2 * up(K * Bp * 2) + up(nW * 8 * Bp * 4) + up(iters * K * Bp)
            + up(Bp * 4) + up(nW * Bp * 4) + up(nW * Bp * 2))


def test_nii_off_again_and_the_workspace():
    """NII on then off gives the NII-off decode's bytes.  A handle that never had NII on reserves the layout it
    always did, for every schedule; with NII on the workspace is larger by the state of the window's
    sub-blocks, and a decode without reserve grows it on demand."""
    B = 70
    q, rows, le = (a[:B] for a in NC.stop_reference(("awgn", 1.0)))
    off_rows, off_le = FW.decode(q[:5], K1, *_qpp(K1), ITERS, *WIN1)
    parent = _parent_workspace_bytes(B, K1, ITERS)
    with _codec(K1, ITERS, None) as c:
        c.reserve(B)
        assert c.workspace_bytes() == parent
    with _codec(K1, ITERS, WIN1, nii=False) as c:
        c.reserve(B)
        assert c.workspace_bytes() == parent
        _check(c, q[:5], off_rows, off_le)
        assert c.workspace_bytes() == parent
        c.set_fixed_window(*WIN1, nii=True)
        _check(c, q, rows, le)   # no reserve: grown on demand
        nS = (K1 + 3) // WIN1[0]
        assert c.workspace_bytes() == parent + 128 * nS * 128   # 128 B per sub-block and codeword of the padded batch
        c.set_fixed_window(*WIN1, nii=False)
        _check(c, q[:5], off_rows, off_le)
        c.set_fixed_window(*WIN1, nii=True)
        c.set_fixed_window(0)   # clears NII with the window
        c.set_fixed_window(*WIN1)
        _check(c, q[:5], off_rows, off_le)
    with _codec(K1, ITERS, WIN1) as c:
        c.reserve(B)
        assert c.workspace_bytes() == parent + 128 * nS * 128
        c.set_fixed_window(32, 16, nii=True)   # more sub-blocks: reserve again
        c.reserve(B)
        assert c.workspace_bytes() == parent + 128 * ((K1 + 3) // 32) * 128


def test_nii_survives_the_other_setters():
    from turbo_decoder_cuda_amd import _native as N
    q = NC.batch(K1)[:5]
    with _codec(K1, ITERS, WIN1) as c:
        c.set_fixed(255, 4)
        c.set_fixed_maxstar()
        c.set_fixed_window_early_stop("hda")
        c.set_fixed_window_early_stop(None)
        rows, le = NC.reference(K1, *WIN1, True)
        _check(c, q, rows[:5], le[:5])
        c.set_fixed_maxstar(None)
        c.set_fixed(255, 3)
        c.set_fixed_window(64, 64, nii=True)
        rows, le = NC.reference(K1, 64, 64, False)
        _check(c, q, rows[:5], le[:5])
        w = N.TdFixedWindowParams(32, 0)   # the C setter alone: NII stays on
        N.check(N.lib().td_set_fixed_window(c._h, C.byref(w)))
        rows, le = NC.reference(K1, 32, 0, False)
        _check(c, q, rows[:5], le[:5])


def test_bad_arguments_are_einval_and_change_nothing():
    from turbo_decoder_cuda_amd import TurboCodec, _native as N
    L = N.lib()
    q = NC.batch(K1)[:5]
    rows, le = (a[:5] for a in NC.reference(K1, *WIN1, False))
    off_rows, off_le = FW.decode(q, K1, *_qpp(K1), ITERS, 64, 5)

    def einval(call, who="td_set_fixed_window_nii"):
        assert call() == N.TD_EINVAL
        assert who in L.td_last_error().decode(), L.td_last_error()

    with TurboCodec(40, 3, 10, iterations=2) as f64:   # another precision
        einval(lambda: L.td_set_fixed_window_nii(f64._h, 1))
        einval(lambda: L.td_set_fixed_window_nii(f64._h, 0))
        with pytest.raises(N.TurboError) as e:
            f64.set_fixed_window(64, 16, nii=True)
        assert e.value.code == N.TD_EINVAL
    with _codec(K1, ITERS, None) as c:   # no window set
        einval(lambda: L.td_set_fixed_window_nii(c._h, 1))
        einval(lambda: L.td_set_fixed_window_nii(c._h, 0))
        ex_rows, ex_le, _ = F.decode(q, K1, *_qpp(K1), ITERS)
        _check(c, q, ex_rows, ex_le)   # still the exact schedule
        c.set_fixed_window(64, 5)   # an overlap of 5: fine without NII, and NII cannot join it
        einval(lambda: L.td_set_fixed_window_nii(c._h, 1))
        _check(c, q, off_rows, off_le)
        with pytest.raises(N.TurboError) as e:
            c.set_fixed_window(64, 21, nii=True)
        assert e.value.code == N.TD_EINVAL
        _check(c, q, off_rows, off_le)   # {64, 5}, NII off: the previous three
        c.set_fixed_window(*WIN1, nii=True)
        w = N.TdFixedWindowParams(64, 5)   # td_set_fixed_window to an overlap of 5 while NII is on
        einval(lambda: L.td_set_fixed_window(c._h, C.byref(w)), "td_set_fixed_window")
        _check(c, q, rows, le)   # {64, 16} with NII, as before
        with pytest.raises(N.TurboError) as e:
            c.set_fixed_window(64, 5, nii=True)
        assert e.value.code == N.TD_EINVAL
        with pytest.raises(N.TurboError):
            c.set_fixed_window(24, 16, nii=True)   # a bad window
        _check(c, q, rows, le)
        c.set_fixed_window(64, 5)   # nii=False turns it off first: the overlap is free again
        _check(c, q, off_rows, off_le)
