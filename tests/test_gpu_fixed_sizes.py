"""The fixed-point decoder (TD_FIXED) on the MI355X at every residue of the trellis length and at the
edges of the tiles round the lane code (tests/fixed_size_cases.py): L = K + 3 at all 16 residues of the
16-step recomputation window with one, two and eight windows, 3K + 12 and L at multiples of the 64-byte
transpose tile, the longest last sub-block.  The exact schedule, the sub-block schedule and early
termination, each bit for bit against its numpy restatement; the interleavers are not the identity."""
import numpy as np
import pytest

import fixed_size_cases as Z
import window_stop_cases as W
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

B, ITERS = 65, 3   # a full wave plus one lane of a padded second wave
SENTINEL = 12345


def _dev():
    import torch
    return torch.device("cuda", 0)


def _gpu(a):
    import torch
    return torch.from_numpy(np.array(a)).to(_dev())   # a copy: the references are read-only


def _codec(K, iters):
    from turbo_decoder_cuda_amd import TurboCodec
    c = TurboCodec(K, *Z.interleaver(K), iterations=iters, algo="maxlog", precision="fixed")
    c.set_fixed(*Z.setting(K))
    return c


def _decode(c, q, all_iters=True, counts=False):
    """(rows or bits, Le prefilled with the sentinel[, counts]) of one GPU decode, as numpy."""
    import torch
    x = _gpu(q)
    g_le = torch.full((q.shape[0], c.iterations, 2, c.K + 3), SENTINEL, dtype=torch.int16, device=_dev())
    out = c.decode(x, all_iters=all_iters, le=g_le, iters_out=True if counts else None)
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), q), "d_llr is not modified"
    out, n = out if counts else (out, None)
    want = (q.shape[0], c.iterations, c.K) if all_iters else (q.shape[0], c.K)
    assert out.dtype == torch.uint8 and tuple(out.shape) == want
    return (out.cpu().numpy(), g_le.cpu().numpy()) + ((n.cpu().numpy(),) if counts else ())


def _equal(c, q, rows, le):
    g_rows, g_le = _decode(c, q)
    assert np.array_equal(g_rows, rows)
    assert np.array_equal(g_le, le)
    g_bits, g_le = _decode(c, q, all_iters=False)
    assert np.array_equal(g_bits, rows[:, -1]), "all_iters=False gives the last row"
    assert np.array_equal(g_le, le)


@pytest.mark.parametrize("K", Z.SIZES)
def test_exact_schedule_equals_restatement(K):
    """Rows of every iteration, every Le and the final bits alone of 65 codewords, 3 iterations."""
    with _codec(K, ITERS) as c:
        _equal(c, Z.batch(K, B), *Z.exact(K, B, ITERS))


@pytest.mark.parametrize("K", Z.SIZES)
def test_sub_block_schedule_equals_restatement(K):
    """{16, 0}, {16, 5}, {32, 7} and {64, 48} on the same batch.  Where the contract lets the window
    show (more than one sub-block and an overlap short of the trellis; {16, 0} and {16, 5} at every
    K >= 29) the restatement is not the exact decode on this batch, so a kernel that ignored the window
    could not pass; elsewhere the two are equal by contract."""
    rows, le = Z.exact(K, B, ITERS)
    with _codec(K, ITERS) as c:
        for win in Z.WINDOWS:
            w_rows, w_le = Z.windowed(K, win, B, ITERS)
            same = np.array_equal(w_rows, rows) and np.array_equal(w_le, le)
            assert same == Z.window_is_exact_by_contract(K, win), win
            c.set_fixed_window(*win)
            _equal(c, Z.batch(K, B), w_rows, w_le)
    if K >= 29:
        assert not Z.window_is_exact_by_contract(K, (16, 0)) and not Z.window_is_exact_by_contract(K, (16, 5))


def _stop_equal(c, ref):
    q, rows, le, used = ref
    iters = rows.shape[1]
    g_rows, g_le, g_used = _decode(c, q, counts=True)
    assert np.array_equal(g_used, used), (W.spread(g_used), W.spread(used))
    assert np.array_equal(g_rows, W.frozen(rows, used))
    mask = np.broadcast_to((np.arange(iters)[None, :] < used[:, None])[:, :, None, None], le.shape)
    assert np.array_equal(g_le[mask], le[mask]), "Le of the iterations a codeword used"
    assert (g_le[~mask] == SENTINEL).all(), "a stopped codeword writes no Le"
    g_bits, _, g_used = _decode(c, q, all_iters=False, counts=True)
    assert np.array_equal(g_used, used)
    assert np.array_equal(g_bits, rows[np.arange(len(used)), used - 1]), "without all_iters: the stop row"


@pytest.mark.parametrize("K", Z.SIZES)
def test_early_termination_equals_rule_on_restatement(K):
    """HDA, and CRC with gCRC24B where K > 24: 130 codewords, 6 iterations, min_iters 1.  In every wave
    of 64 the reference's counts take at least two values, one below 6: lanes of one wave stop apart."""
    with _codec(K, Z.STOP_ITERS) as c:
        for rule in ("hda", "crc") if K > 24 else ("hda",):
            ref = Z.stop_case(K, rule)
            print(K, rule, [W.spread(ref[3][w0:w0 + 64]) for w0 in range(0, Z.STOP_B, 64)])
            Z.spread_in_every_wave(ref[3], Z.STOP_ITERS)
            c.set_fixed_early_stop(rule, min_iters=1, crc_poly=Z.CRC24B)
            _stop_equal(c, ref)
