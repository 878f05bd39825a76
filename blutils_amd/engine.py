"""Host-side handle objects over the C ABI (include/blu_consensus.h).

Mirrors the reference seam `build_consensus_identities`
(core/src/use_cases/build_consensus_identities/mod.rs:40-47): a taxonomy + a
cutoff configuration (Taxon, Option<CustomTaxon>) on one side, grouped hit rows
on the other, a strategy, one result per query.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _native as N

RESULT_DTYPE = np.dtype([
    ("status", "u1"), ("flags", "u1"), ("bean_index", "u1"), ("max_allowed_level", "u1"),
    ("reached_rank", "<u2"), ("max_allowed_rank", "<u2"), ("identifier_node", "<u4"), ("ref_row", "<u4"),
    ("level_mask", "<u8"), ("ident_used", "<f8"),
])
assert RESULT_DTYPE.itemsize == 32


# include/blu_consensus.h: blu_support
SUPPORT_DTYPE = np.dtype([
    ("n_hits", "<u4"), ("n_matched", "<u4"), ("n_top", "<u4"), ("n_top_support", "<u4"), ("n_support", "<u4"),
    ("top_score", "<i4"), ("bits", "<i8"), ("support_bits", "<i8"),
])
assert SUPPORT_DTYPE.itemsize == 40


def _cutoff_config(taxon: str, custom: Optional[dict]) -> N.CutoffConfig:
    cfg = N.CutoffConfig()
    cfg.taxon = N.TAXON[taxon]
    cfg.has_custom = 1 if custom is not None else 0
    if custom is not None:
        for i, k in enumerate(N.CUSTOM_FIELDS):
            if custom.get(k) is not None:
                cfg.custom[i] = int(custom[k])
                cfg.custom_has[i] = 1
    return cfg


class Taxonomy:
    """Device-resident taxonomy + per-shape cutoff tables (blu_taxonomy_create)."""

    def __init__(self, lin_off, lin_node, lin_rank, rank_names: Sequence[str], taxon: str = "bacteria",
                 custom: Optional[dict] = None, device: int = 0, taxid=None, bad=None):
        L = N.lib()
        self.lin_off = np.ascontiguousarray(lin_off, dtype=np.uint64)
        self.lin_node = np.ascontiguousarray(lin_node, dtype=np.uint32)
        self.lin_rank = np.ascontiguousarray(lin_rank, dtype=np.uint16)
        self.rank_names = list(rank_names)
        self.taxon, self.custom, self.device = taxon, custom, device
        names = [s.encode() for s in self.rank_names]
        arr = (C.c_char_p * max(1, len(names)))(*names)
        desc = N.TaxonomyDesc()
        desc.n_tax = len(self.lin_off) - 1
        desc.lin_off = self.lin_off.ctypes.data
        desc.lin_node = self.lin_node.ctypes.data
        desc.lin_rank = self.lin_rank.ctypes.data
        desc.n_ranks = len(names)
        desc.rank_names = C.cast(arr, C.c_void_p)
        self._taxid = None
        if taxid is not None:
            self._taxid = np.ascontiguousarray(taxid, dtype=np.int64)
            desc.taxid = self._taxid.ctypes.data
        if bad is not None:
            self._bad = np.ascontiguousarray(bad, dtype=np.uint8)
            desc.bad = self._bad.ctypes.data
        cfg = _cutoff_config(taxon, custom)
        h = C.c_void_p()
        rc = L.blu_taxonomy_create(C.byref(desc), C.byref(cfg), device, C.byref(h))
        if rc != N.BLU_OK:
            raise N.BluError(rc, "blu_taxonomy_create")
        self._h = h

    # -- introspection -------------------------------------------------------
    @property
    def handle(self):
        return self._h

    @property
    def n_tax(self) -> int:
        return N.lib().blu_taxonomy_n_tax(self._h)

    @property
    def n_shapes(self) -> int:
        return N.lib().blu_taxonomy_n_shapes(self._h)

    @property
    def max_depth(self) -> int:
        return N.lib().blu_taxonomy_max_depth(self._h)

    @property
    def device_bytes(self) -> int:
        return N.lib().blu_taxonomy_device_bytes(self._h)

    def rank_name(self, code: int, serde: bool = False) -> str:
        p = N.lib().blu_taxonomy_rank_name(self._h, int(code), 1 if serde else 0)
        if p is None:
            raise IndexError(code)
        return p.decode()

    def row_cutoffs(self, row: int):
        cut = np.zeros(64, dtype=np.float64)
        isdef = np.zeros(64, dtype=np.uint8)
        codes = np.zeros(64, dtype=np.uint16)
        n = N.lib().blu_taxonomy_row_cutoffs(self._h, int(row), 64, cut.ctypes.data, isdef.ctypes.data, codes.ctypes.data)
        if n < 0:
            raise IndexError(row)
        return cut[:n], isdef[:n].astype(bool), codes[:n]

    def row_map(self):
        """(desc row -> engine row id, sorted position -> desc row).  Engine row ids (what blu_hits.tax_row holds)
        are opaque: sorted position in lexicographic lineage order | lineage length << 25."""
        if getattr(self, "_row_map", None) is None:
            fwd = np.zeros(max(1, self.n_tax), dtype=np.uint32)
            inv = np.zeros(max(1, self.n_tax), dtype=np.uint32)
            rc = N.lib().blu_taxonomy_row_map(self._h, fwd.ctypes.data, inv.ctypes.data)
            if rc != N.BLU_OK:
                raise N.BluError(rc, "blu_taxonomy_row_map")
            self._row_map = (fwd[: self.n_tax], inv[: self.n_tax])
        return self._row_map

    def engine_rows(self, desc_rows):
        """desc row indices (numpy, or a torch tensor on any device; -1 / 0xFFFFFFFF = unmatched) -> engine row ids."""
        fwd, _ = self.row_map()
        if isinstance(desc_rows, np.ndarray):
            r = desc_rows.view(np.uint32) if desc_rows.dtype == np.int32 else desc_rows.astype(np.uint32)
            ok = r < self.n_tax
            out = np.full(r.shape, N.BLU_UNMATCHED_TAXID, dtype=np.uint32)
            out[ok] = fwd[r[ok]]
            return out
        import torch
        key = str(desc_rows.device)
        cache = self.__dict__.setdefault("_row_map_t", {})
        if key not in cache:
            cache[key] = torch.from_numpy(fwd.view(np.int32).copy()).to(desc_rows.device)   # uint32 bit patterns
        m = cache[key]
        ok = (desc_rows >= 0) & (desc_rows < self.n_tax)
        return torch.where(ok, m[desc_rows.clamp(min=0, max=max(0, self.n_tax - 1)).long()], torch.full_like(desc_rows, -1))

    def lookup(self, taxids) -> np.ndarray:
        t = np.ascontiguousarray(taxids, dtype=np.int64)
        out = np.zeros(len(t), dtype=np.uint32)
        rc = N.lib().blu_taxonomy_lookup(self._h, t.ctypes.data, len(t), out.ctypes.data)
        if rc != N.BLU_OK:
            raise N.BluError(rc, "blu_taxonomy_lookup")
        return out

    def close(self):
        if getattr(self, "_h", None):
            N.lib().blu_taxonomy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.int32 else np.ascontiguousarray(a, dtype=np.uint32)


def pack_records(tax: "Taxonomy", tax_row, pident_milli, align_len, acc_rank, pident=None, wide: bool = False) -> np.ndarray:
    """blu_hits_pack / blu_hits_pack64 on host arrays: the [n, 4] (or, wide, [n, 6]) uint32 side records of the packed
    layouts (include/blu_consensus.h) — {tax_row, pident_milli | shape hint << 17, align_len, acc_rank} (+ the f64
    perc_identity for the wide form).  tax_row: ENGINE row ids."""
    tx, aln, ac = _u32(tax_row), np.ascontiguousarray(align_len, dtype=np.int32), _u32(acc_rank)
    pm = _u32(pident_milli) if pident_milli is not None else None
    pid = np.ascontiguousarray(pident, dtype=np.float64) if pident is not None else None
    n = len(tx)
    out = np.zeros((n, 6 if wide else 4), dtype=np.uint32)
    cols = N.Hits(None, tx.ctypes.data, pid.ctypes.data if pid is not None else None, aln.ctypes.data, ac.ctypes.data, None, n, 0, 0, 0,
                  pm.ctypes.data if pm is not None else None, None, None)
    fn = N.lib().blu_hits_pack64 if wide else N.lib().blu_hits_pack
    rc = fn(tax.handle, C.byref(cols), out.ctypes.data, None)
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_pack")
    return out


def pack_hits_device(tax: "Taxonomy", hits: dict, wide: bool = False):
    """blu_hits_pack / blu_hits_pack64 on torch CUDA columns (keys tax_row, align_len, acc_rank and pident_milli or pident):
    the int32 tensor of 4 (wide: 6) words per hit that goes into `packed` / `packed64`."""
    import torch
    n = hits["tax_row"].numel()
    out = torch.empty((6 if wide else 4) * n, dtype=torch.int32, device=hits["tax_row"].device)
    pm, pid = hits.get("pident_milli"), hits.get("pident")
    if pm is not None:
        pid = None
    for k in ("tax_row", "align_len", "acc_rank"):
        assert hits[k].is_cuda and hits[k].is_contiguous() and hits[k].dtype == torch.int32, k
    cols = N.Hits(None, hits["tax_row"].data_ptr(), pid.data_ptr() if pid is not None else None, hits["align_len"].data_ptr(),
                  hits["acc_rank"].data_ptr(), None, n, 0, 1, 0, pm.data_ptr() if pm is not None else None, None, None)
    fn = N.lib().blu_hits_pack64 if wide else N.lib().blu_hits_pack
    rc = fn(tax.handle, C.byref(cols), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_pack")
    return out


def run_consensus_host(tax: Taxonomy, seg_off, bitscore, tax_row, pident, align_len, acc_rank,
                       strategy: str = "relaxed", pident_milli=None, packed=False) -> np.ndarray:
    """Host buffers in, host records out; the library stages them over PCIe.  tax_row: ENGINE row ids.
    pident_milli (uint32, perc_identity * 1000) replaces the f64 `pident` column when given (pass pident=None);
    packed=True hands the four non-bit-score columns over as 16-byte records built by blu_hits_pack (pident_milli, or an
    f64 column of exact milli-percent values); packed="wide": the 24-byte records of blu_hits_pack64 (any f64)."""
    if packed:
        seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
        bs = np.ascontiguousarray(bitscore, dtype=np.int32)
        wide = packed == "wide"
        rec = pack_records(tax, tax_row, pident_milli, align_len, acc_rank, pident=pident if pident_milli is None else None, wide=wide)
        nq, nh = len(seg) - 1, int(seg[-1])
        assert rec.shape == (nh, 6 if wide else 4) and rec.ctypes.data % 16 == 0
        hits = N.Hits(bs.ctypes.data, None, None, None, None, seg.ctypes.data, nh, nq, 0, 0, None, None if wide else rec.ctypes.data,
                      rec.ctypes.data if wide else None)
        params = N.RunParams(N.STRATEGY[strategy], 0, None)
        out = np.zeros(nq, dtype=RESULT_DTYPE)
        rc = N.lib().blu_consensus_run(tax.handle, C.byref(hits), C.byref(params), out.ctypes.data)
        if rc != N.BLU_OK:
            raise N.BluError(rc, "blu_consensus_run")
        return out
    seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
    bs = np.ascontiguousarray(bitscore, dtype=np.int32)
    tx = np.ascontiguousarray(tax_row)
    tx = tx.view(np.uint32) if tx.dtype == np.int32 else np.ascontiguousarray(tx, dtype=np.uint32)
    pid = np.ascontiguousarray(pident, dtype=np.float64) if pident_milli is None else None
    pm = None
    if pident_milli is not None:
        pm = np.ascontiguousarray(pident_milli)
        pm = pm.view(np.uint32) if pm.dtype == np.int32 else np.ascontiguousarray(pm, dtype=np.uint32)
    aln = np.ascontiguousarray(align_len, dtype=np.int32)
    ac = np.ascontiguousarray(acc_rank)
    ac = ac.view(np.uint32) if ac.dtype == np.int32 else np.ascontiguousarray(ac, dtype=np.uint32)
    nq = len(seg) - 1
    nh = int(seg[-1])
    assert len(bs) == nh and len(tx) == nh and len(pid if pm is None else pm) == nh and len(aln) == nh and len(ac) == nh
    hits = N.Hits(bs.ctypes.data, tx.ctypes.data, pid.ctypes.data if pm is None else None, aln.ctypes.data, ac.ctypes.data,
                  seg.ctypes.data, nh, nq, 0, 0, pm.ctypes.data if pm is not None else None, None, None)
    params = N.RunParams(N.STRATEGY[strategy], 0, None)
    out = np.zeros(nq, dtype=RESULT_DTYPE)
    rc = N.lib().blu_consensus_run(tax.handle, C.byref(hits), C.byref(params), out.ctypes.data)
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_consensus_run")
    return out


def shard_ranges(seg_off, n_shards: int) -> np.ndarray:
    """blu_shard_ranges: query bounds of n_shards contiguous ranges balanced by hit count."""
    seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
    bounds = np.zeros(n_shards + 1, dtype=np.uint64)
    rc = N.lib().blu_shard_ranges(seg.ctypes.data_as(C.c_void_p), C.c_uint64(len(seg) - 1), C.c_uint32(n_shards),
                                  bounds.ctypes.data_as(C.c_void_p))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_shard_ranges")
    return bounds


def run_consensus_multi(taxes: Sequence[Taxonomy], seg_off, bitscore, tax_row, pident, align_len, acc_rank,
                        strategy: str = "relaxed", pident_milli=None, packed=False) -> np.ndarray:
    """blu_consensus_run_multi: one host table over several handles of the same taxonomy (one per GPU); `tax_row` holds
    engine row ids (identical for every handle of one taxonomy).  pident_milli and packed as in run_consensus_host (the
    side records are built with the first handle: shape hints are the same for every handle of one taxonomy)."""
    seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
    bs = np.ascontiguousarray(bitscore, dtype=np.int32)
    nq, nh = len(seg) - 1, int(seg[-1])
    if packed:
        wide = packed == "wide"
        rec = pack_records(taxes[0], tax_row, pident_milli, align_len, acc_rank, pident=pident if pident_milli is None else None, wide=wide)
        assert rec.shape == (nh, 6 if wide else 4) and rec.ctypes.data % 16 == 0
        hits = N.Hits(bs.ctypes.data, None, None, None, None, seg.ctypes.data, nh, nq, 0, 0, None, None if wide else rec.ctypes.data,
                      rec.ctypes.data if wide else None)
    else:
        tx = np.ascontiguousarray(tax_row)
        tx = tx.view(np.uint32) if tx.dtype == np.int32 else np.ascontiguousarray(tx, dtype=np.uint32)
        pid = np.ascontiguousarray(pident, dtype=np.float64) if pident_milli is None else None
        pm = np.ascontiguousarray(pident_milli, dtype=np.uint32) if pident_milli is not None else None
        aln = np.ascontiguousarray(align_len, dtype=np.int32)
        ac = np.ascontiguousarray(acc_rank)
        ac = ac.view(np.uint32) if ac.dtype == np.int32 else np.ascontiguousarray(ac, dtype=np.uint32)
        hits = N.Hits(bs.ctypes.data, tx.ctypes.data, pid.ctypes.data if pm is None else None, aln.ctypes.data, ac.ctypes.data,
                      seg.ctypes.data, nh, nq, 0, 0, pm.ctypes.data if pm is not None else None, None, None)
    params = N.RunParams(N.STRATEGY[strategy], 0, None)
    out = np.zeros(nq, dtype=RESULT_DTYPE)
    handles = (C.c_void_p * len(taxes))(*[t.handle for t in taxes])
    L = N.lib()
    L.blu_consensus_run_multi.restype = C.c_int
    L.blu_consensus_run_multi.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = L.blu_consensus_run_multi(handles, len(taxes), C.byref(hits), C.byref(params), out.ctypes.data)
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_consensus_run_multi")
    return out


def run_consensus_device(tax: Taxonomy, hits: dict, out, strategy: str = "relaxed", stream: Optional[int] = None):
    """torch CUDA tensors in (`hits` keys: seg_off bitscore tax_row align_len acc_rank and either pident (float64) or
    pident_milli (int32 bit pattern of uint32)), records into the uint8 CUDA tensor `out` of 32 * n_queries bytes.
    Asynchronous on `stream` (default: torch's current stream)."""
    import torch

    nq = hits["seg_off"].numel() - 1
    nh = hits["bitscore"].numel()
    milli = hits.get("pident_milli") is not None
    packed = hits.get("packed") is not None
    wide = hits.get("packed64") is not None
    if packed or wide:     # side records next to the bit-score column (blu_hits_pack / blu_hits_pack64)
        want = (("seg_off", torch.int64), ("bitscore", torch.int32), ("packed64" if wide else "packed", torch.int32))
    else:
        want = (("seg_off", torch.int64), ("bitscore", torch.int32), ("tax_row", torch.int32),
                ("pident_milli", torch.int32) if milli else ("pident", torch.float64), ("align_len", torch.int32),
                ("acc_rank", torch.int32))
    for k, dt in want:
        t = hits[k]
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt, (k, t.dtype, t.device)
    assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= 32 * nq
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    if wide:
        assert hits["packed64"].numel() == 6 * nh and hits["packed64"].data_ptr() % 8 == 0
        h = N.Hits(hits["bitscore"].data_ptr(), None, None, None, None, hits["seg_off"].data_ptr(), nh, nq, 1, 0, None, None,
                   hits["packed64"].data_ptr())
    elif packed:
        assert hits["packed"].numel() == 4 * nh and hits["packed"].data_ptr() % 16 == 0
        h = N.Hits(hits["bitscore"].data_ptr(), None, None, None, None, hits["seg_off"].data_ptr(), nh, nq, 1, 0, None,
                   hits["packed"].data_ptr(), None)
    else:
        h = N.Hits(hits["bitscore"].data_ptr(), hits["tax_row"].data_ptr(), None if milli else hits["pident"].data_ptr(),
                   hits["align_len"].data_ptr(), hits["acc_rank"].data_ptr(), hits["seg_off"].data_ptr(), nh, nq, 1, 0,
                   hits["pident_milli"].data_ptr() if milli else None, None, None)
    params = N.RunParams(N.STRATEGY[strategy], 0, stream)
    rc = N.lib().blu_consensus_run(tax.handle, C.byref(h), C.byref(params), out.data_ptr())
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_consensus_run")


def support_host(tax: Taxonomy, seg_off, bitscore, tax_row, records, packed=None, packed64=None) -> np.ndarray:
    """blu_consensus_support on host arrays: the support counts (SUPPORT_DTYPE) of `records`, a run's RESULT_DTYPE array.
    tax_row: ENGINE row ids; or pass the [n, 4] side records as packed= / the [n, 6] ones as packed64= (tax_row=None): their
    word 0 is read."""
    seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
    bs = np.ascontiguousarray(bitscore, dtype=np.int32)
    recs = np.ascontiguousarray(records, dtype=RESULT_DTYPE)
    nq, nh = len(seg) - 1, len(bs)
    assert len(recs) == nq
    tx = _u32(tax_row) if tax_row is not None else None
    pk = np.ascontiguousarray(packed, dtype=np.uint32) if packed is not None else None
    pk64 = np.ascontiguousarray(packed64, dtype=np.uint32) if packed64 is not None else None
    assert (tx is not None) + (pk is not None) + (pk64 is not None) == 1
    assert tx is None or len(tx) == nh
    assert pk is None or pk.size == 4 * nh
    assert pk64 is None or pk64.size == 6 * nh
    hits = N.Hits(bs.ctypes.data, tx.ctypes.data if tx is not None else None, None, None, None, seg.ctypes.data, nh, nq, 0, 0, None,
                  pk.ctypes.data if pk is not None else None, pk64.ctypes.data if pk64 is not None else None)
    out = np.zeros(nq, dtype=SUPPORT_DTYPE)
    L = N.lib()
    L.blu_consensus_support.restype = C.c_int
    L.blu_consensus_support.argtypes = [C.c_void_p, C.POINTER(N.Hits), C.c_void_p, C.c_void_p, C.c_void_p]
    rc = L.blu_consensus_support(tax.handle, C.byref(hits), recs.ctypes.data, None, out.ctypes.data)
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_consensus_support")
    return out


def support_device(tax: Taxonomy, hits: dict, records, stream: Optional[int] = None) -> np.ndarray:
    """blu_consensus_support on torch CUDA tensors: `hits` as for run_consensus_device (seg_off, bitscore and tax_row, packed
    or packed64 are read), `records` the uint8 CUDA tensor a run wrote.  Returns the counts on the host (SUPPORT_DTYPE)."""
    import torch

    nq = hits["seg_off"].numel() - 1
    nh = hits["bitscore"].numel()
    side = "packed64" if hits.get("packed64") is not None else "packed" if hits.get("packed") is not None else "tax_row"
    for k, dt in (("seg_off", torch.int64), ("bitscore", torch.int32), (side, torch.int32)):
        t = hits[k]
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt, (k, t.dtype, t.device)
    assert hits[side].numel() == {"tax_row": 1, "packed": 4, "packed64": 6}[side] * nh
    assert records.is_cuda and records.is_contiguous() and records.numel() * records.element_size() >= 32 * nq
    out = torch.zeros(max(nq, 1) * 5, dtype=torch.int64, device=records.device)   # 40 bytes a query, 8-byte aligned
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    h = N.Hits(hits["bitscore"].data_ptr(), hits["tax_row"].data_ptr() if side == "tax_row" else None, None, None, None,
               hits["seg_off"].data_ptr(), nh, nq, 1, 0, None, hits["packed"].data_ptr() if side == "packed" else None,
               hits["packed64"].data_ptr() if side == "packed64" else None)
    L = N.lib()
    L.blu_consensus_support.restype = C.c_int
    L.blu_consensus_support.argtypes = [C.c_void_p, C.POINTER(N.Hits), C.c_void_p, C.c_void_p, C.c_void_p]
    rc = L.blu_consensus_support(tax.handle, C.byref(h), records.data_ptr(), stream, out.data_ptr())
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_consensus_support")
    return out.cpu().numpy().view(np.uint8)[: 40 * nq].view(SUPPORT_DTYPE).copy()


def _band_c(top_percent_milli, top_bits) -> Optional[N.ScoreBandC]:
    """the two criteria (None = not given) -> blu_score_band, or None when neither is given; values are passed as they are:
    the library refuses the ones out of range"""
    if top_percent_milli is None and top_bits is None:
        return None
    b = N.ScoreBandC(0, 0, 0)
    if top_percent_milli is not None:
        b.top_percent_milli, b.mask = int(top_percent_milli), b.mask | N.BAND_TOP_PERCENT
    if top_bits is not None:
        b.top_bits, b.mask = int(top_bits), b.mask | N.BAND_TOP_BITS
    return b


def score_band_host(seg_off, bitscore, top_percent_milli: Optional[int] = None, top_bits: Optional[int] = None, device: int = 0):
    """blu_hits_score_band on host arrays: -> (the raised int32 column, the counts).  The column and the
    offsets are uploaded and the device kernel runs; top_percent_milli is the percentage times 1000."""
    seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
    bs = np.ascontiguousarray(bitscore, dtype=np.int32)
    out = np.empty_like(bs)
    band, st = _band_c(top_percent_milli, top_bits), N.ScoreBandStats()
    rc = N.lib().blu_hits_score_band(device, bs.ctypes.data if len(bs) else None, seg.ctypes.data, len(bs), len(seg) - 1, 0,
                                     C.byref(band) if band is not None else None, None, out.ctypes.data if len(bs) else None,
                                     C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_score_band")
    return out, N.band_counts(st)


def score_band_device(seg_off, bitscore, top_percent_milli: Optional[int] = None, top_bits: Optional[int] = None, out=None,
                      stream: Optional[int] = None) -> dict:
    """blu_hits_score_band on torch CUDA tensors (seg_off int64, bitscore int32): the raised column goes to `out` (None: in
    place); -> the counts.  Returns when the column is complete."""
    import torch

    if out is None:
        out = bitscore
    for t, dt in ((seg_off, torch.int64), (bitscore, torch.int32), (out, torch.int32)):
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt, (t.dtype, t.device)
    assert out.numel() == bitscore.numel()
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    band, st = _band_c(top_percent_milli, top_bits), N.ScoreBandStats()
    dev = bitscore.device.index or 0
    rc = N.lib().blu_hits_score_band(dev, bitscore.data_ptr(), seg_off.data_ptr(), bitscore.numel(), seg_off.numel() - 1, 1,
                                     C.byref(band) if band is not None else None, stream, out.data_ptr(), C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_score_band")
    return N.band_counts(st)


def subject_keep_host(seg_off, bitscore, acc_rank, device: int = 0):
    """blu_hits_subject_keep on host arrays: -> (the uint32 keep words, the counts).  The two columns and the
    offsets are uploaded and the device kernels run."""
    seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
    bs = np.ascontiguousarray(bitscore, dtype=np.int32)
    acc = np.ascontiguousarray(acc_rank, dtype=np.uint32)
    assert len(acc) == len(bs)
    keep, st = np.empty(len(bs), dtype=np.uint32), N.SubjectBestStats()
    rc = N.lib().blu_hits_subject_keep(device, bs.ctypes.data if len(bs) else None, acc.ctypes.data if len(bs) else None, seg.ctypes.data,
                                       len(bs), len(seg) - 1, 0, None, keep.ctypes.data if len(bs) else None, C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_subject_keep")
    return keep, N.subject_counts(st)


def subject_keep_device(seg_off, bitscore, acc_rank, keep, stream: Optional[int] = None) -> dict:
    """blu_hits_subject_keep on torch CUDA tensors (seg_off int64, bitscore int32, acc_rank int32 holding the uint32 bits, keep
    int32): the verdicts go to `keep`; -> the counts.  Returns when `keep` is complete."""
    import torch

    for t, dt in ((seg_off, torch.int64), (bitscore, torch.int32), (acc_rank, torch.int32), (keep, torch.int32)):
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt, (t.dtype, t.device)
    assert keep.numel() == bitscore.numel() == acc_rank.numel()
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    st = N.SubjectBestStats()
    dev = bitscore.device.index or 0
    rc = N.lib().blu_hits_subject_keep(dev, bitscore.data_ptr(), acc_rank.data_ptr(), seg_off.data_ptr(), bitscore.numel(),
                                       seg_off.numel() - 1, 1, stream, keep.data_ptr(), C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_subject_keep")
    return N.subject_counts(st)


def subject_best_host(seg_off, bitscore, align_len, tax_desc_row, acc_rank, pident, device: int = 0,
                      unmatched_marker: int = N.BLU_UNMATCHED_TAXID, mask: Optional[int] = N.SUBJECT_BEST_PER_QUERY):
    """blu_hits_subject_best on host arrays: -> (a dict of the compacted seg_off and five columns, n_unmatched,
    the counts).  The arguments are not changed; mask None passes a NULL selection."""
    seg = np.array(seg_off, dtype=np.uint64)
    cols = [np.array(bitscore, dtype=np.int32), np.array(align_len, dtype=np.int32), np.array(tax_desc_row, dtype=np.uint32),
            np.array(acc_rank, dtype=np.uint32), np.array(pident, dtype=np.float64)]
    n = len(cols[0])
    assert all(len(c) == n for c in cols)
    sel = N.SubjectBestC(mask, 0) if mask is not None else None
    st, n_out, n_un = N.SubjectBestStats(), C.c_uint64(0), C.c_uint64(0)
    rc = N.lib().blu_hits_subject_best(device, *[c.ctypes.data if n else None for c in cols], seg.ctypes.data, n, len(seg) - 1, 0,
                                       C.byref(sel) if sel is not None else None, None, unmatched_marker, C.byref(n_out),
                                       C.byref(n_un), C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_subject_best")
    k = int(n_out.value)
    names = ("bitscore", "align_len", "tax_desc_row", "acc_rank", "pident")
    out = {name: c[:k].copy() for name, c in zip(names, cols)}
    out["seg_off"] = seg
    return out, int(n_un.value), N.subject_counts(st)


def subject_best_device(seg_off, bitscore, align_len, tax_desc_row, acc_rank, pident, unmatched_marker: int = N.BLU_UNMATCHED_TAXID,
                        stream: Optional[int] = None):
    """blu_hits_subject_best on torch CUDA tensors, in place (seg_off int64, the 32-bit columns int32, pident float64):
    -> (the rows left, n_unmatched, the counts); the kept rows are the front of each tensor."""
    import torch

    for t, dt in ((seg_off, torch.int64), (bitscore, torch.int32), (align_len, torch.int32), (tax_desc_row, torch.int32),
                  (acc_rank, torch.int32), (pident, torch.float64)):
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt, (t.dtype, t.device)
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    sel, st, n_out, n_un = N.SubjectBestC(N.SUBJECT_BEST_PER_QUERY, 0), N.SubjectBestStats(), C.c_uint64(0), C.c_uint64(0)
    dev = bitscore.device.index or 0
    rc = N.lib().blu_hits_subject_best(dev, bitscore.data_ptr(), align_len.data_ptr(), tax_desc_row.data_ptr(), acc_rank.data_ptr(),
                                       pident.data_ptr(), seg_off.data_ptr(), bitscore.numel(), seg_off.numel() - 1, 1, C.byref(sel),
                                       stream, unmatched_marker, C.byref(n_out), C.byref(n_un), C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_subject_best")
    return int(n_out.value), int(n_un.value), N.subject_counts(st)


def _cover_map(tax: Taxonomy, row_map):
    """row_map as the host route takes it: None, or [n_tax] uint32 (True: the handle's own forward map)"""
    if row_map is None:
        return None
    if row_map is True:
        row_map = tax.row_map()[0]
    m = np.ascontiguousarray(row_map, dtype=np.uint32)
    assert len(m) == tax.n_tax, (len(m), tax.n_tax)
    return m


def cover_keep_host(tax: Taxonomy, seg_off, bitscore, tax_row, min_cover_milli: int, row_map=None):
    """blu_hits_cover_keep on host arrays: -> (the uint32 keep words, d* per query as uint8 with 0xFF for a
    query left alone, the counts).  tax_row holds engine row ids, or desc rows when row_map ([n_tax] uint32, or True for the
    handle's own) is given.  The columns, the map and the offsets are uploaded and the device kernels run; min_cover_milli is
    the percentage times 1000 and is passed as it is (the library refuses what is out of range)."""
    seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
    bs = np.ascontiguousarray(bitscore, dtype=np.int32)
    rows = np.ascontiguousarray(tax_row, dtype=np.uint32)
    assert len(rows) == len(bs)
    n, nq = len(bs), len(seg) - 1
    m = _cover_map(tax, row_map)
    keep, depth, st = np.empty(n, dtype=np.uint32), np.empty(nq, dtype=np.uint8), N.MinCoverStats()
    rc = N.lib().blu_hits_cover_keep(tax.handle, bs.ctypes.data if n else None, rows.ctypes.data if n else None,
                                     m.ctypes.data if m is not None else None, seg.ctypes.data, n, nq, 0, int(min_cover_milli), None,
                                     keep.ctypes.data if n else None, depth.ctypes.data if nq else None, C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_cover_keep")
    return keep, depth, N.cover_counts(st)


def cover_keep_device(tax: Taxonomy, seg_off, bitscore, tax_row, min_cover_milli: int, keep, depth=None, row_map=None,
                      stream: Optional[int] = None) -> dict:
    """blu_hits_cover_keep on torch CUDA tensors (seg_off int64, bitscore / tax_row / keep int32 holding the 32-bit words, depth
    uint8 [n_queries] or None, row_map int32 [n_tax] or None): the verdicts go to `keep`, d* to `depth`; -> the counts."""
    import torch

    for t, dt in ((seg_off, torch.int64), (bitscore, torch.int32), (tax_row, torch.int32), (keep, torch.int32)) + \
            (((depth, torch.uint8),) if depth is not None else ()) + (((row_map, torch.int32),) if row_map is not None else ()):
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt, (t.dtype, t.device)
    assert keep.numel() == bitscore.numel() == tax_row.numel()
    assert depth is None or depth.numel() == seg_off.numel() - 1
    assert row_map is None or row_map.numel() == tax.n_tax
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    st = N.MinCoverStats()
    rc = N.lib().blu_hits_cover_keep(tax.handle, bitscore.data_ptr(), tax_row.data_ptr(), row_map.data_ptr() if row_map is not None else None,
                                     seg_off.data_ptr(), bitscore.numel(), seg_off.numel() - 1, 1, int(min_cover_milli), stream,
                                     keep.data_ptr(), depth.data_ptr() if depth is not None else None, C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_cover_keep")
    return N.cover_counts(st)


def cover_apply_host(tax: Taxonomy, seg_off, bitscore, align_len, tax_row, acc_rank, pident, min_cover_milli: int, row_map=None,
                     unmatched_marker: int = N.BLU_UNMATCHED_TAXID):
    """blu_hits_cover_apply on host arrays: -> (a dict of the compacted seg_off and five columns, n_unmatched, the
    counts).  The arguments are not changed; tax_row and row_map as for cover_keep_host."""
    seg = np.array(seg_off, dtype=np.uint64)
    cols = [np.array(bitscore, dtype=np.int32), np.array(align_len, dtype=np.int32), np.array(tax_row, dtype=np.uint32),
            np.array(acc_rank, dtype=np.uint32), np.array(pident, dtype=np.float64)]
    n = len(cols[0])
    assert all(len(c) == n for c in cols)
    m = _cover_map(tax, row_map)
    st, n_out, n_un = N.MinCoverStats(), C.c_uint64(0), C.c_uint64(0)
    rc = N.lib().blu_hits_cover_apply(tax.handle, *[c.ctypes.data if n else None for c in cols], m.ctypes.data if m is not None else None,
                                      seg.ctypes.data, n, len(seg) - 1, 0, int(min_cover_milli), None, unmatched_marker, C.byref(n_out),
                                      C.byref(n_un), C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_cover_apply")
    k = int(n_out.value)
    names = ("bitscore", "align_len", "tax_row", "acc_rank", "pident")
    out = {name: c[:k].copy() for name, c in zip(names, cols)}
    out["seg_off"] = seg
    return out, int(n_un.value), N.cover_counts(st)


def cover_apply_device(tax: Taxonomy, seg_off, bitscore, align_len, tax_row, acc_rank, pident, min_cover_milli: int, row_map=None,
                       unmatched_marker: int = N.BLU_UNMATCHED_TAXID, stream: Optional[int] = None):
    """blu_hits_cover_apply on torch CUDA tensors, in place (seg_off int64, the 32-bit columns int32, pident float64, row_map int32
    [n_tax] or None): -> (the rows left, n_unmatched, the counts); the kept rows are the front of each tensor."""
    import torch

    for t, dt in ((seg_off, torch.int64), (bitscore, torch.int32), (align_len, torch.int32), (tax_row, torch.int32),
                  (acc_rank, torch.int32), (pident, torch.float64)) + (((row_map, torch.int32),) if row_map is not None else ()):
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt, (t.dtype, t.device)
    assert row_map is None or row_map.numel() == tax.n_tax
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    st, n_out, n_un = N.MinCoverStats(), C.c_uint64(0), C.c_uint64(0)
    rc = N.lib().blu_hits_cover_apply(tax.handle, bitscore.data_ptr(), align_len.data_ptr(), tax_row.data_ptr(), acc_rank.data_ptr(),
                                      pident.data_ptr(), row_map.data_ptr() if row_map is not None else None, seg_off.data_ptr(),
                                      bitscore.numel(), seg_off.numel() - 1, 1, int(min_cover_milli), stream, unmatched_marker,
                                      C.byref(n_out), C.byref(n_un), C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_hits_cover_apply")
    return int(n_out.value), int(n_un.value), N.cover_counts(st)


def records_from_tensor(out) -> np.ndarray:
    """uint8 CUDA/CPU tensor -> numpy structured array of blu_result."""
    return out.detach().cpu().numpy().view(np.uint8).reshape(-1)[: (out.numel() * out.element_size()) // 32 * 32].view(RESULT_DTYPE)


def last_launch():
    name = C.create_string_buffer(128)
    grid, block = C.c_uint32(), C.c_uint32()
    N.lib().blu_consensus_last_launch(name, 128, C.byref(grid), C.byref(block))
    return name.value.decode(), grid.value, block.value
