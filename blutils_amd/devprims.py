"""The device primitives of the GPU ingest on torch tensors (include/blu_consensus.h: blu_dev_*, csrc/dev_prims.hip):
device-wide exclusive prefix sums, the stable LSD radix sort of (key, value) pairs, and the newline index of a text.
Introspection for the tests: the product paths call the primitives inside the library."""
from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _native as N

LINE_PAD = 64   # bytes a text must be readable past its size (16-byte loads over whole tiles)


def _device(t) -> int:
    if not getattr(t, "is_cuda", False):
        raise ValueError("device tensors only")
    if not t.is_contiguous():
        raise ValueError("contiguous tensors only")
    return t.device.index if t.device.index is not None else 0


def exclusive_scan(x, out=None):
    """out[i] = x[0] + ... + x[i - 1], modulo 2^32 or 2^64 by x's element size (4 or 8 bytes: the values are taken as
    unsigned).  out may be x itself (in place); a new tensor like x when None."""
    dev = _device(x)
    if x.element_size() not in (4, 8):
        raise ValueError("4- or 8-byte elements")
    if out is None:
        import torch
        out = torch.empty_like(x)
    if out.numel() != x.numel() or out.element_size() != x.element_size() or _device(out) != dev:
        raise ValueError("out must match x")
    rc = N.lib().blu_dev_exclusive_scan(dev, x.data_ptr(), out.data_ptr(), x.numel(), x.element_size())
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_dev_exclusive_scan")
    return out


def radix_sort_pairs(keys, vals, bits: int = 32):
    """Sorts the 4-byte (keys, vals) in place, stably, by the low 8 * ceil(bits / 8) bits of the keys (keys < 2^bits)."""
    dev = _device(keys)
    if keys.element_size() != 4 or vals.element_size() != 4 or keys.numel() != vals.numel() or _device(vals) != dev:
        raise ValueError("keys and vals: 4-byte elements, as many of each")
    rc = N.lib().blu_dev_radix_sort_pairs(dev, keys.data_ptr(), vals.data_ptr(), keys.numel(), int(bits))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_dev_radix_sort_pairs")
    return keys, vals


def line_index(text, size: Optional[int] = None, cap: Optional[int] = None):
    """(line, n_newlines) of the uint8 tensor text[:size]: line[0] = 0, line[k + 1] = offset after newline k (int64,
    n_newlines + 1 entries).  text must hold LINE_PAD bytes past size.  With cap, the line buffer has cap entries and a
    text with more newlines fails (BLU_ERR_INVALID_ARG) without writing it; without, the newlines are counted first."""
    import torch
    dev = _device(text)
    if text.element_size() != 1:
        raise ValueError("a byte tensor")
    size = text.numel() - LINE_PAD if size is None else int(size)
    if size < 0 or size + LINE_PAD > text.numel():
        raise ValueError(f"text must hold {LINE_PAD} bytes past size")
    L = N.lib()
    n = C.c_uint64(0)
    if cap is None:
        rc = L.blu_dev_line_index(dev, text.data_ptr(), size, None, 0, C.byref(n))
        if rc not in (N.BLU_OK, N.BLU_ERR_INVALID_ARG):
            raise N.BluError(rc, "blu_dev_line_index")
        cap = n.value + 1
    line = torch.empty(max(int(cap), 1), dtype=torch.int64, device=text.device)
    rc = L.blu_dev_line_index(dev, text.data_ptr(), size, line.data_ptr(), int(cap), C.byref(n))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_dev_line_index")
    return line[: n.value + 1], n.value
