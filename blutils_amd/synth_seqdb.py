"""Seeded synthetic `blastdbcmd -entry all` listings with sequences, as `build-db kraken2` (`-outfmt "%a  %T  %s"`) and
`build-db qiime2` (`-outfmt "%a  %T  %o  %s"`) read them: for tests and scripts/seqdb_bench.py.  Lines are written straight
to a file, so listings of several GB never sit in memory whole."""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np

IUPAC = b"ACGTNacgtnRYKMSWBDHVrykmswbdhv"


def _seq(rng: np.random.Generator, n: int, alphabet: bytes = IUPAC) -> bytes:
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return a[rng.integers(0, len(a), n, dtype=np.uint8)].tobytes()


def line(rng: np.random.Generator, qiime: bool, seq_len: int, k: int, odd: bool = True) -> bytes:
    """One listing line.  With odd=True about one line in ten carries what the rules care about: a taxid written `007` or
    `+5`, a CRLF ending, a fourth piece after the sequence, spaces around pieces."""
    acc = b"ACC%07d.%d" % (k, rng.integers(1, 4))
    taxid = b"%d" % rng.integers(1, 3_000_000)
    oid = b"%d" % k
    end = b"\n"
    extra = b""
    if odd and rng.random() < 0.1:
        r = rng.integers(0, 5)
        if r == 0:
            taxid = b"00" + taxid
        elif r == 1:
            taxid = b"+" + taxid
        elif r == 2:
            end = b"\r\n"
        elif r == 3:
            extra = b"  extra piece"
        else:
            acc = b" " + acc + b" "
    pieces = [acc, taxid] + ([oid] if qiime else []) + [_seq(rng, seq_len)]
    return b"  ".join(pieces) + extra + end


def write_listing(path: str, qiime: bool, n_lines: int, seed: int, min_len: int = 0, max_len: int = 3000,
                  long_lines: Sequence[int] = (), long_at: Optional[Iterable[int]] = None, odd: bool = True) -> int:
    """n_lines short lines with sequence lengths in [min_len, max_len], plus len(long_lines) lines of those lengths placed at
    the line numbers long_at (0-based; spread evenly by default).  Returns the bytes written."""
    rng = np.random.default_rng(seed)
    total = n_lines + len(long_lines)
    if long_at is None:
        long_at = [int((i + 1) * total / (len(long_lines) + 1)) for i in range(len(long_lines))]
    where = dict(zip(long_at, long_lines))
    written = 0
    with open(path, "wb") as f:
        buf = []
        size = 0
        for k in range(total):
            if k in where:
                b = line(rng, qiime, where[k], k, odd=False)
            else:
                b = line(rng, qiime, int(rng.integers(min_len, max_len + 1)), k, odd)
            buf.append(b)
            size += len(b)
            if size >= (64 << 20):
                f.write(b"".join(buf))
                written += size
                buf, size = [], 0
        f.write(b"".join(buf))
        written += size
    return written
