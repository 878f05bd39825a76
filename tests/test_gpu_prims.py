"""The device primitives of csrc/dev_prims.hip on their own (blu_dev_*: blutils_amd/devprims.py) against plain numpy:
the exclusive prefix sums (u32 / u64, out of place and in place) across the block sizes of its three launches and the
carry loop of scan_block_offsets (n > 4096 x 1024), the stable radix sort at every pass count and across the 4 M-cell
scan of its (digit, block) table, and the line index across tile boundaries and past 4 GiB."""
import ctypes as C

import numpy as np
import pytest
import torch

from blutils_amd import _native as N
from blutils_amd import devprims as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CARRY = 4096 * 1024            # elements per round of scan_block_offsets' loop over the block sums
SCAN_SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, CARRY - 1, CARRY, CARRY + 1, 2 * CARRY + 1, 30_000_017]
SIGNED = {np.uint32: np.int32, np.uint64: np.int64}


def _to_dev(a):
    return torch.from_numpy(a.view(SIGNED[a.dtype.type])).to(DEV)


def _from_dev(t, dt):
    return t.cpu().numpy().view(dt)


def _scan_values(dt, kind, n, rng):
    if kind == "zeros":
        return np.zeros(n, dt)
    if kind == "equal":                                  # u32: wraps past 2^32 at n > 2^32 / 0x9E3779B9
        return np.full(n, 0x9E3779B9 if dt == np.uint32 else (1 << 40) + 12345, dt)
    if kind == "random":                                 # u32: small; u64: near 2^40, the totals cross 2^32 and 2^53
        return rng.integers(0, 1 << 10, n, dtype=np.uint32) if dt == np.uint32 else \
            (np.uint64(1 << 40) + rng.integers(0, 1 << 32, n, dtype=np.uint64))
    assert kind == "wide"                                # the whole range: the sums wrap
    return rng.integers(0, np.iinfo(dt).max, n, dtype=dt, endpoint=True)


def _excl(x):
    out = np.zeros_like(x)
    np.cumsum(x[:-1], dtype=x.dtype, out=out[1:])
    return out


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("kind", ["zeros", "equal", "random", "wide"])
@pytest.mark.parametrize("dt", [np.uint32, np.uint64], ids=["u32", "u64"])
def test_exclusive_scan(dt, kind, in_place):
    rng = np.random.default_rng(17)
    crossed = False
    for n in SCAN_SIZES:
        x = _scan_values(dt, kind, n, rng)
        exp = _excl(x)
        d = _to_dev(x)
        got = P.exclusive_scan(d, d if in_place else None)
        if in_place:
            assert got.data_ptr() == d.data_ptr()
        else:
            assert np.array_equal(_from_dev(d, dt), x)       # the input is left alone
        g = _from_dev(got, dt)
        if not np.array_equal(g, exp):
            bad = int(np.flatnonzero(g != exp)[0])
            pytest.fail(f"n={n}: first difference at {bad}: {int(g[bad])} != {int(exp[bad])}")
        if dt == np.uint64 and kind == "random" and int(exp[-1]) > 1 << 53:
            crossed = True
    if dt == np.uint64 and kind == "random":
        assert crossed


def test_exclusive_scan_rejects_bad_arguments():
    x = torch.zeros(8, dtype=torch.int16, device=DEV)
    with pytest.raises(ValueError):
        P.exclusive_scan(x)
    L = N.lib()
    y = torch.zeros(8, dtype=torch.int32, device=DEV)
    assert L.blu_dev_exclusive_scan(0, y.data_ptr(), y.data_ptr(), 8, 2) == N.BLU_ERR_INVALID_ARG
    assert L.blu_dev_exclusive_scan(0, None, y.data_ptr(), 8, 4) == N.BLU_ERR_INVALID_ARG
    assert L.blu_dev_exclusive_scan(0, None, None, 0, 4) == N.BLU_OK


# ---- radix sort ------------------------------------------------------------------------------------------------------

SORT_SIZES = [1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 70_000]
SORT_BITS = [0, 1, 7, 8, 9, 16, 17, 24, 25, 32]


def _key_sets(n, bits, rng):
    mask = (1 << bits) - 1
    passes = (bits + 7) // 8
    top = 8 * max(passes - 1, 0)
    const = 0xA5C3_5A3C & mask
    sets = {
        "equal": np.full(n, const, np.uint32),
        "two": np.where(rng.integers(0, 2, n) == 1, mask, mask // 3).astype(np.uint32),
        "descending": ((np.arange(n, dtype=np.uint64)[::-1] * np.uint64(mask)) // np.uint64(max(n - 1, 1))).astype(np.uint32),
        "uniform": rng.integers(0, mask, n, dtype=np.uint64, endpoint=True).astype(np.uint32),
        # only the top digit differs: every pass but the last sees one digit value
        "top_digit": (np.uint64(const & ((1 << top) - 1)) |
                      (rng.integers(0, (mask >> top) + 1, n, dtype=np.uint64) << np.uint64(top))).astype(np.uint32),
    }
    for p in range(passes):                              # one digit varies; each other pass has one digit value
        lo, hi = 8 * p, min(8 * p + 8, bits)
        field = rng.integers(0, 1 << (hi - lo), n, dtype=np.uint64) << np.uint64(lo)
        keep = np.uint64(const & ~(((1 << hi) - 1) ^ ((1 << lo) - 1)) & mask)
        sets[f"digit{p}"] = (keep | field).astype(np.uint32)
    return sets


@pytest.mark.parametrize("bits", SORT_BITS)
def test_radix_sort_pairs(bits):
    rng = np.random.default_rng(bits)
    for n in SORT_SIZES:
        for name, keys in _key_sets(n, bits, rng).items():
            assert int(keys.max()) < 1 << bits, name
            vals = np.arange(n, dtype=np.uint32)
            k, v = _to_dev(keys), _to_dev(vals)
            P.radix_sort_pairs(k, v, bits)
            order = np.argsort(keys, kind="stable")
            gk, gv = _from_dev(k, np.uint32), _from_dev(v, np.uint32)
            assert np.array_equal(gv, order), (n, name)
            assert np.array_equal(gk, keys[order]), (n, name)


def test_radix_sort_pairs_past_a_4m_cell_table():
    """n > 16 384 blocks of 4 096: the (digit, block) table of each pass has more than 4 M cells, so its prefix sum runs
    the carry loop; checked by what a stable sort is rather than by sorting on the host."""
    n = 16_385 * 4096 + 1234
    assert 256 * ((n + 4095) // 4096) > CARRY
    rng = np.random.default_rng(70)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys[::7] = keys[3]                                  # long runs of one key across every block: stability shows
    k = _to_dev(keys)
    v = torch.arange(n, dtype=torch.int32, device=DEV)
    P.radix_sort_pairs(k, v, 32)
    gk, gv = _from_dev(k, np.uint32), _from_dev(v, np.uint32)
    assert np.all(gk[1:] >= gk[:-1])
    same = gk[1:] == gk[:-1]
    assert np.all(gv[1:][same] > gv[:-1][same])
    seen = np.zeros(n, bool)
    seen[gv] = True
    assert seen.all()
    assert np.array_equal(gk, keys[gv])


def test_radix_sort_rejects_bad_bits():
    k = torch.zeros(4, dtype=torch.int32, device=DEV)
    for bits in (-1, 33):
        with pytest.raises(N.BluError) as e:
            P.radix_sort_pairs(k, k.clone(), bits)
        assert e.value.code == N.BLU_ERR_INVALID_ARG


# ---- line index -------------------------------------------------------------------------------------------------------

LINE_SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 8193]


def _padded(body, pad_byte=10):
    buf = np.full(len(body) + P.LINE_PAD, pad_byte, np.uint8)    # newlines in the padding: never counted
    buf[: len(body)] = body
    return torch.from_numpy(buf).to(DEV)


def _check_lines(body):
    line, n = P.line_index(_padded(body), len(body))
    exp = np.concatenate([[0], np.flatnonzero(body == 10) + 1]).astype(np.int64)
    assert n == len(exp) - 1
    assert np.array_equal(line.cpu().numpy(), exp)


@pytest.mark.parametrize("size", LINE_SIZES)
def test_line_index(size):
    rng = np.random.default_rng(size)
    for final_nl in (False, True):
        body = rng.choice(np.frombuffer(b"ACGT\t.0123456789\n", np.uint8), size).astype(np.uint8)
        body[body == 10] = ord("x")
        body[rng.random(size) < 0.05] = 10
        for at in (4095, 4096):                          # the last byte of a tile, the first of the next
            if at < size - 1:
                body[at] = 10
        if size:
            body[-1] = 10 if final_nl else ord("A")
        _check_lines(body)
    _check_lines(np.full(size, 10, np.uint8))            # every byte a newline
    _check_lines(np.zeros(size, np.uint8))               # none


def test_line_index_cap_and_alignment():
    body = np.zeros(5000, np.uint8)
    body[[3, 4095, 4096, 4999]] = 10
    text = _padded(body)
    L = N.lib()
    line = torch.full((8,), -7, dtype=torch.int64, device=DEV)
    n = C.c_uint64(0)
    assert L.blu_dev_line_index(0, text.data_ptr(), 5000, line.data_ptr(), 4, C.byref(n)) == N.BLU_ERR_INVALID_ARG
    assert n.value == 4
    torch.cuda.synchronize()
    assert (line == -7).all()                            # counted first: nothing written when the lines do not fit
    assert L.blu_dev_line_index(0, text.data_ptr(), 5000, line.data_ptr(), 5, C.byref(n)) == N.BLU_OK
    assert line[:5].tolist() == [0, 4, 4096, 4097, 5000] and (line[5:] == -7).all()
    assert L.blu_dev_line_index(0, text.data_ptr() + 1, 4999, line.data_ptr(), 8, C.byref(n)) == N.BLU_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        P.line_index(text, 5000 + 1)                     # less than LINE_PAD bytes past the size


def test_line_index_past_4_gib():
    size = (1 << 32) + (1 << 20) + 5
    text = torch.zeros(size + P.LINE_PAD, dtype=torch.uint8, device=DEV)
    at = [0, 4095, 4096, (1 << 32) - 4097, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 32) + 4095, size - 1]
    text[torch.tensor(at, device=DEV)] = 10
    text[size:] = 10
    line, n = P.line_index(text, size)
    assert n == len(at)
    assert line.cpu().tolist() == [0] + [a + 1 for a in at]
