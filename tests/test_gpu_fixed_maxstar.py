"""The fixed-point decoder's integer log-MAP (td_set_fixed_maxstar) on the MI355X against its numpy restatement
(tests/fixed_maxstar_ref.py), bit for bit: the hard-decision rows of every iteration, the final bits alone
and every extrinsic value -- on the exact schedule, on the sub-block schedule, with both stop rules on both,
through a hipGraph and behind the int8 rate-matching chain.  A codeword's result does not depend on its
batch, so a reference is computed once for the largest batch of a case and sliced."""
import ctypes as C
import functools

import numpy as np
import pytest

import fixed_maxstar_ref as M
import fixed_ref as F
import fixed_stop_cases as S
import pyoracle as O
import ratematch_ref as RM
import window_stop_cases as W
from conftest import GOLD, gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SENTINEL = 12345
QPP = dict(S.QPP)
_z = np.load(f"{GOLD}/frames_K432_e0.8_s46.npz")
QPP[int(_z["K"])] = (int(_z["f1"]), int(_z["f2"]))
STEPS16 = M.table(16)

# table, (le_max, ext_scale_q), steps per unit LLR of the frames, Eb/N0
CONFIGS = {
    "default-255-4": (M.DEFAULT, (255, 4), 8, 0.5),
    "default-255-3": (M.DEFAULT, (255, 3), 8, 0.5),
    "steps16-127-3": (STEPS16, (127, 3), 16, 1.0),
    "constant-31-2": (M.CONSTANT, (31, 2), 16, 1.0),   # strong inputs: the clamp acts even on one codeword of K = 8
}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _gpu(a):
    import torch
    return torch.from_numpy(np.array(a)).to(_dev())   # a copy: the references are read-only


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _codec(K, iters, setting=None, tab=None, win=None):
    from turbo_decoder_cuda_amd import TurboCodec
    c = TurboCodec(K, *QPP[K], iterations=iters, algo="maxlog", precision="fixed")
    if setting is not None:
        c.set_fixed(*setting)
    if tab is not None:
        c.set_fixed_maxstar(table=tab)
    if win is not None:
        c.set_fixed_window(*win)
    return c


@functools.lru_cache(maxsize=None)
def _awgn(K, B, steps, ebn0, seed=5):
    return _frozen(F.quantise(O.synth_batch(K, *QPP[K], ebn0, seed, B)[1], steps))[0]


def _decode(c, q, all_iters=True, counts=False):
    """(rows or bits, Le prefilled with the sentinel[, counts]) of one GPU decode, as numpy."""
    import torch
    x = _gpu(q)
    g_le = torch.full((q.shape[0], c.iterations, 2, c.K + 3), SENTINEL, dtype=torch.int16, device=_dev())
    out = c.decode(x, all_iters=all_iters, le=g_le, iters_out=True if counts else None)
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), q), "d_llr is not modified"
    if counts:
        return out[0].cpu().numpy(), g_le.cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy(), g_le.cpu().numpy()


def _equal(c, q, rows, le):
    """The three comparisons of a decode without a rule: the rows of all iterations, the final bits alone,
    every Le."""
    g_rows, g_le = _decode(c, q)
    assert g_rows.shape == rows.shape and np.array_equal(g_rows, rows)
    assert np.array_equal(g_le, le)
    g_bits, g_le = _decode(c, q, all_iters=False)
    assert np.array_equal(g_bits, rows[:, -1]) and np.array_equal(g_le, le)


def _equal_stop(c, q, rows, le, used):
    """The same with a rule: the frozen rows, the stop row alone, the counts, and the Le of the iterations a
    codeword used."""
    iters = rows.shape[1]
    mask = S.le_mask(used, iters)
    g_rows, g_le, g_used = _decode(c, q, counts=True)
    assert np.array_equal(g_used, used), (W.spread(g_used), W.spread(used))
    assert np.array_equal(g_rows, W.frozen(rows, used))
    assert np.array_equal(np.where(mask, g_le, 0), np.where(mask, le, 0))
    g_bits, g_le, g_used = _decode(c, q, all_iters=False, counts=True)
    assert np.array_equal(g_used, used) and np.array_equal(g_bits, rows[np.arange(len(used)), used - 1])
    assert np.array_equal(np.where(mask, g_le, 0), np.where(mask, le, 0))


# ------------------------------------------------------------------ the exact schedule
SHAPES = [(8, 1, 1), (8, 4, 65), (40, 8, 63), (40, 4, 130), (432, 4, 65), (1024, 8, 63), (1024, 4, 130), (6144, 8, 2),
          (6144, 4, 65), (10000, 4, 3)]


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("K,iters,B", SHAPES)
def test_exact_schedule_equals_restatement(K, iters, B, config):
    tab, setting, steps, ebn0 = CONFIGS[config]
    q = _awgn(K, B, steps, ebn0)
    rows, le, share = M.decode(q, K, *QPP[K], iters, tab, *setting)
    if config == "constant-31-2":
        assert share > 0, "the clamp is exercised"
    if config == "default-255-4" and K >= 40 and iters > 1:
        assert (rows != F.decode(q, K, *QPP[K], iters, *setting)[0]).any(), "not the Max-Log-MAP rows"
    with _codec(K, iters, setting, tab) as c:
        _equal(c, q, rows, le)


def _saturated(K):
    """+127, -128, alternating +-127, and fixed_stop_cases' mixed batch of four (the three and random bytes)."""
    return np.concatenate([S.FRAMES["pattern"](K, name, 1) for name in ("plus127", "minus128", "alternating")]
                          + [S.FRAMES["pattern"](K, "mixed", 4)])


@pytest.mark.parametrize("K", [6144, 10000])
def test_widest_table_on_saturated_inputs(K):
    """{63 x 7, 0} with shift 8 and {255, 4} at the longest blocks: the metrics' bound, 572 * 10003 < 2^23.  The
    four batches are decoded one by one; their reference is one decode of the seven codewords."""
    iters = 2
    q = _saturated(K)
    rows, le, _ = M.decode(q, K, *QPP[K], iters, M.WIDEST, 255, 4)
    with _codec(K, iters, (255, 4), M.WIDEST) as c:
        for sl in (slice(0, 1), slice(1, 2), slice(2, 3), slice(3, 7)):
            _equal(c, q[sl], rows[sl], le[sl])


def test_all_zero_table_is_the_table_off():
    K, iters, B = 1024, 4, 65
    q = _awgn(K, B, 8, 0.5)
    rows, le, _ = F.decode(q, K, *QPP[K], iters)
    on = M.decode(q, K, *QPP[K], iters, M.DEFAULT, 255, 3)
    assert (on[0] != rows).any()
    with _codec(K, iters) as c:
        off = _decode(c, q)
        c.set_fixed_maxstar(table=M.ZERO)
        zero = _decode(c, q)
        assert np.array_equal(zero[0], off[0]) and np.array_equal(zero[1], off[1])
        assert np.array_equal(off[0], rows) and np.array_equal(off[1], le)
        c.set_fixed_maxstar()   # the default table at 8 steps
        _equal(c, q, on[0], on[1])
        c.set_fixed_maxstar(None)
        _equal(c, q, rows, le)


# ------------------------------------------------------------------ the sub-block schedule
WINDOWS = [(16, 0), (16, 16), (32, 7), (64, 48)]


@functools.lru_cache(maxsize=None)
def _window_ref(K, B, iters, win, ebn0=0.5):
    q = _awgn(K, B, 8, ebn0)
    return _frozen(q, *M.decode(q, K, *QPP[K], iters, M.DEFAULT, 255, 4, win=win)[:2])


@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("K", [40, 1024])
def test_sub_block_schedule_equals_restatement(K, win):
    iters = 3
    q, rows, le = _window_ref(K, 65, iters, win)
    exact = M.decode(q[:8], K, *QPP[K], iters, M.DEFAULT, 255, 4)[0]
    if K == 1024:
        assert (rows[:8] != exact).any(), "not the exact decode"
    with _codec(K, iters, (255, 4), M.DEFAULT, win) as c:
        for n in (65, 1, 64):
            _equal(c, q[:n], rows[:n], le[:n])


def test_sub_block_schedule_long_block():
    K, iters, win = 6144, 2, (64, 48)
    q, rows, le = _window_ref(K, 65, iters, win)
    with _codec(K, iters, (255, 4), M.DEFAULT, win) as c:
        _equal(c, q, rows, le)


def test_overlap_of_the_whole_block_is_the_exact_decode():
    K, iters, B, win = 40, 4, 65, (16, 48)   # overlap 48 >= L = 43
    q = _awgn(K, B, 8, 0.5)
    rows, le, _ = M.decode(q, K, *QPP[K], iters, M.DEFAULT, 255, 4)
    w_rows, w_le, _ = M.decode(q, K, *QPP[K], iters, M.DEFAULT, 255, 4, win=win)
    assert np.array_equal(w_rows, rows) and np.array_equal(w_le, le)
    with _codec(K, iters, (255, 4), M.DEFAULT, win) as c:
        _equal(c, q, rows, le)


# ------------------------------------------------------------------ both stop rules on both schedules
STOP_K, STOP_ITERS, STOP_B = 1024, 8, 130
# "hda" on generator frames at 1.0 and 0.0 dB; "crc" on frames carrying gCRC24B at the same two Eb/N0 of the
# rate 1/3 code: sigma = sqrt(3 / (2 Eb/N0)) = 1.0915 and 1.2247
STOP_FRAMES = {"hda": (("awgn", 1.0, STOP_B), ("awgn", 0.0, STOP_B)), "crc": (("crc", 1.0915, STOP_B), ("crc", 1.2247, STOP_B))}


@functools.lru_cache(maxsize=None)
def _stop_ref(key, win):
    q = np.ascontiguousarray(S.FRAMES[key[0]](STOP_K, *key[1:]))
    return _frozen(q, *M.decode(q, STOP_K, *QPP[STOP_K], STOP_ITERS, M.DEFAULT, 255, 4, win=win)[:2])


@pytest.mark.parametrize("rule", ["hda", "crc"])
@pytest.mark.parametrize("win", [None, (64, 16)])
def test_stop_rules_equal_rule_on_restatement(win, rule):
    refs = [_stop_ref(key, win) for key in STOP_FRAMES[rule]]
    first = [W.stops(r[1], rule, 1, S.CRC24B) for r in refs]
    print([W.spread(u) for u in first])
    both = np.concatenate(first)
    assert (both < STOP_ITERS).any() and (both == STOP_ITERS).any(), "codewords that stop and codewords that do not"
    if rule == "crc":   # a codeword that runs to the end without passing, not one that passes at the end
        last = np.concatenate([r[1][:, -1] for r in refs])
        assert any(W.crc24(row, S.CRC24B) != 0 for row in last[both == STOP_ITERS])
    with _codec(STOP_K, STOP_ITERS, (255, 4), M.DEFAULT, win) as c:
        stop = c.set_fixed_window_early_stop if win else c.set_fixed_early_stop
        for (q, rows, le), u1 in zip(refs, first):
            for min_iters in (1, STOP_ITERS):
                used = u1 if min_iters == 1 else np.full(STOP_B, STOP_ITERS, dtype=np.int32)
                stop(rule, min_iters=min_iters, crc_poly=S.CRC24B)
                _equal_stop(c, q, rows, le, used)


# ------------------------------------------------------------------ the setter
def test_table_survives_the_other_setters_in_any_order():
    K, iters, B = 40, 4, 130
    q = _awgn(K, B, 8, 0.5)
    ref = {(win, s): M.decode(q, K, *QPP[K], iters, M.DEFAULT, *s, win=win)[:2]
           for win in (None, (16, 5)) for s in ((255, 3), (255, 4))}
    maxlog = F.decode(q, K, *QPP[K], iters)
    assert (ref[None, (255, 3)][0] != maxlog[0]).any()
    with _codec(K, iters) as c:   # the table first, the others after it
        c.set_fixed_maxstar(8.0)
        _equal(c, q, *ref[None, (255, 3)])
        c.set_fixed(255, 4)
        _equal(c, q, *ref[None, (255, 4)])
        rows, le = ref[None, (255, 4)]
        c.set_fixed_early_stop("hda")
        _equal_stop(c, q, rows, le, W.stops(rows, "hda"))
        c.set_fixed_early_stop(None)
        c.set_fixed_window(16, 5)
        _equal(c, q, *ref[(16, 5), (255, 4)])
        rows, le = ref[(16, 5), (255, 4)]
        c.set_fixed_window_early_stop("crc")
        _equal_stop(c, q, rows, le, W.stops(rows, "crc", 1, S.CRC24B))
        c.set_fixed_window(0)
        _equal(c, q, *ref[None, (255, 4)])
        # a codeword's result does not depend on its batch companions
        whole = _decode(c, q)
        for b in (0, 63, 64, 129):
            alone = _decode(c, q[b:b + 1])
            assert np.array_equal(alone[0][0], whole[0][b]) and np.array_equal(alone[1][0], whole[1][b])
        c.set_fixed_maxstar(None)
        c.set_fixed()
        _equal(c, q, maxlog[0], maxlog[1])
    with _codec(K, iters, (255, 4)) as c:   # the others first, the table after them
        c.set_fixed_window(16, 5)
        c.set_fixed_window_early_stop("hda", min_iters=2)
        c.set_fixed_maxstar(table=M.DEFAULT)
        rows, le = ref[(16, 5), (255, 4)]
        _equal_stop(c, q, rows, le, W.stops(rows, "hda", 2))
    with _codec(K, iters, (255, 4)) as c:
        c.set_fixed_early_stop("crc")
        c.set_fixed_maxstar(table=M.DEFAULT)
        rows, le = ref[None, (255, 4)]
        _equal_stop(c, q, rows, le, W.stops(rows, "crc", 1, S.CRC24B))


def test_bad_arguments_are_einval_and_change_nothing():
    from turbo_decoder_cuda_amd import TurboCodec, _native as N
    L = N.lib()
    K, iters, B = 40, 4, 65
    q = _awgn(K, B, 8, 0.5)
    rows, le, _ = M.decode(q, K, *QPP[K], iters, M.CONSTANT, 255, 3)

    def einval(m):
        assert L.td_set_fixed_maxstar(c._h, C.byref(m)) == N.TD_EINVAL
        assert "td_set_fixed_maxstar" in L.td_last_error().decode()

    with _codec(K, iters, None, M.CONSTANT) as c:
        for shift, corr in ((-1, M.DEFAULT[1]), (9, M.DEFAULT[1]), (3, (64, 6, 4, 3, 2, 1, 1, 0)), (3, (9, 6, 4, 3, 2, 1, 255, 0)),
                            (3, (9, 6, 4, 3, 2, 1, 1, 1)), (0, (0,) * 7 + (63,))):
            einval(N.TdFixedMaxstarParams(shift, (C.c_uint8 * 8)(*corr)))
            with pytest.raises(N.TurboError) as e:
                c.set_fixed_maxstar(table=(shift, corr))
            assert e.value.code == N.TD_EINVAL
        with pytest.raises(N.TurboError):
            c.set_fixed_maxstar(0.0)
        with pytest.raises(ValueError):
            c.set_fixed_maxstar(table=(3, (1, 0)))
        _equal(c, q, rows, le)   # the previous table is still in force
        c.set_fixed_maxstar(table=(8, (63,) * 7 + (0,)))   # the limits themselves are allowed
        c.set_fixed_maxstar(table=(0, (0,) * 8))
    for prec in ("f64", "f32"):
        with TurboCodec(40, 3, 10, iterations=2, precision=prec) as other:
            m = N.TdFixedMaxstarParams(3, (C.c_uint8 * 8)(*M.DEFAULT[1]))
            assert L.td_set_fixed_maxstar(other._h, C.byref(m)) == N.TD_EINVAL
            assert L.td_set_fixed_maxstar(other._h, None) == N.TD_EINVAL
            with pytest.raises(N.TurboError) as e:
                other.set_fixed_maxstar()
            assert e.value.code == N.TD_EINVAL and "td_set_fixed_maxstar" in str(e.value)
    # td_create keeps TD_FIXED to TD_ALGO_MAXLOG
    with pytest.raises(N.TurboError):
        TurboCodec(40, 3, 10, iterations=2, algo="logmap", precision="fixed")


# ------------------------------------------------------------------ graphs and the rate-matching chain
@pytest.mark.parametrize("win", [None, (64, 48)])
def test_graph_capture_after_reserve_replays_the_eager_result(win):
    """One capture and replay after reserve: the exact schedule, and the sub-block schedule with HDA."""
    import torch
    K, iters, n = 1024, 4, 65
    q = _awgn(K, n, 8, 1.0)
    rows, le, _ = M.decode(q, K, *QPP[K], iters, M.DEFAULT, 255, 4, win=win)
    used = W.stops(rows, "hda") if win else np.full(n, iters, dtype=np.int32)
    sb = torch.cuda.Stream(_dev())
    with _codec(K, iters, (255, 4), M.DEFAULT, win) as c:
        if win:
            c.set_fixed_window_early_stop("hda")
        c.reserve(n)
        gin = _gpu(q).clone()
        gout = torch.empty((n, iters, K), dtype=torch.uint8, device=_dev())
        gle = torch.full((n, iters, 2, K + 3), SENTINEL, dtype=torch.int16, device=_dev())
        gcnt = torch.empty((n,), dtype=torch.int32, device=_dev())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sb):
            c.decode(gin, gout, all_iters=True, le=gle, stream=sb, iters_out=gcnt)
        gle.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        got = (gout.cpu().numpy().copy(), gle.cpu().numpy().copy(), gcnt.cpu().numpy().copy())
        eager = _decode(c, q, counts=True)
        for a, b in zip(got, eager):
            assert np.array_equal(a, b)
        mask = S.le_mask(used, iters)
        assert np.array_equal(got[2], used) and np.array_equal(got[0], W.frozen(rows, used))
        assert np.array_equal(np.where(mask, got[1], 0), np.where(mask, le, 0))


def test_rate_dematch_into_a_decode_with_the_table():
    from turbo_decoder_cuda_amd import decoder
    K, iters, B = 1024, 4, 9
    f1, f2 = QPP[K]
    flow = O.synth_batch(K, f1, f2, 1.5, 21, B)[1]
    E = 2 * K
    with _codec(K, iters, (255, 4), M.DEFAULT) as c:
        c.set_rate_matching(0)
        e1 = c.rate_match(decoder.quantise(_gpu(flow), 8), 0, E)
        buf = c.rate_dematch(e1, 0)
        want = F.dematch(F.quantise(flow, 8)[:, RM.index(K, 0, 0, E)], K, 0, 0)
        assert np.array_equal(buf.cpu().numpy(), want)
        rows, le, _ = M.decode(want, K, f1, f2, iters, M.DEFAULT, 255, 4)
        _equal(c, want, rows, le)
        assert np.array_equal(c.decode(buf, all_iters=True).cpu().numpy(), rows)
