"""The byte-level edge cases of `build-db sintax` and `build-db dada2` (tests/seqdb_label_edges.py) against the restatement
alone (tests/seqdb_label_reference.py), without a GPU: the generator is deterministic, every class puts its cases where it says
(recomputed from the listing's bytes and from the restatement's output: the residue modulo 16 and modulo 4096 of the probe byte,
of the record boundary before a skipped run, of the totals), the set of residues a class reaches is the set it promises, and
every case has its stated outcome, a refused one with the records and the counts of the lines before it."""
import collections

import pytest

from tests import seqdb_label_edges as G
from tests import seqdb_label_reference as LR

SLICE, TILE = G.SLICE, G.TILE


def _ref(case, fmt):
    return LR.export(fmt, G.document(case.doc), case.listing)


def _lines(b: bytes):
    """(start, end without the newline) of every line"""
    out, pos = [], 0
    while pos < len(b):
        nl = b.find(b"\n", pos)
        out.append((pos, len(b) if nl < 0 else nl))
        pos = len(b) if nl < 0 else nl + 1
    return out


def _line_at(b: bytes, p: int):
    """(1-based number, start, end) of the line that holds offset p"""
    return next((no + 1, s, e) for no, (s, e) in enumerate(_lines(b)) if s <= p <= e)


def _kind_of(line: bytes) -> str:
    """What the edge document makes of a line, its bytes >= 0x80 taken out: written, unknown or unlabelled."""
    clean = bytes(c for c in line if c < 0x80) + b"\n"
    clean = clean if clean.split(b"  ")[0] else b"a" + clean
    r = LR.export(G.DADA2, G.document("edges"), clean)
    assert r["outcome"] == ("ok",), line
    return G.WRITTEN if r["records"] else G.SKIP_U if r["n_unknown_taxid"] else G.SKIP_N


def _in_sequence(b: bytes, p: int, n: int) -> bool:
    """Whether bytes [p, p + n) lie in the trimmed third piece of their line."""
    _, s, e = _line_at(b, p)
    parts = b[s:e].split(b"  ")
    if len(parts) < 3:
        return False
    a = s + len(parts[0]) + 2 + len(parts[1]) + 2
    return a <= p and p + n <= a + len(parts[2].rstrip())


def _check_refused(case):
    """The stated outcome; the .fna and the counts are those of the lines before the bad one."""
    line = case.outcome[1]
    before = b"".join(case.listing[s:e] + b"\n" for s, e in _lines(case.listing)[:line - 1])
    for fmt in case.fmts:
        r, good = _ref(case, fmt), LR.export(fmt, G.document(case.doc), before)
        assert r["outcome"] == case.outcome, (case.name, fmt)
        assert good["outcome"] == ("ok",), case.name
        for key in ("fna", "records", "n_unknown_taxid", "n_unlabelled"):
            assert r[key] == good[key], (case.name, fmt, key)
        assert r["input_bytes"] == len(before), case.name


def test_generator_is_deterministic():
    a = [(c.name, c.listing) for c in G.edge_cases()]
    for fn in (G.edge_cases, G.b1_refused, G.b2_accepted, G.b3_several_lines_in_a_slice, G.b4_end_of_file, G.b5_first_of_two, G.b6_precedence,
               G.c1_tiny_records, G.c2_skipped_runs, G.c3_ends_of_a_chunk, G.c4_totals, G.c5_long_pieces, G.c6_no_label, G.d_counts):
        fn.cache_clear()
    assert [(c.name, c.listing) for c in G.edge_cases()] == a
    assert len({(c.cls, c.name) for c in G.edge_cases()}) == len(a)


def test_every_case_has_its_outcome_and_keeps_what_came_before():
    for case in G.edge_cases():
        assert case.fmts and set(case.fmts) <= set(G.FORMATS)
        if case.outcome == ("ok",):
            for fmt in case.fmts:
                r = _ref(case, fmt)
                assert r["outcome"] == ("ok",) and r["input_bytes"] == len(case.listing), (case.name, fmt)
                assert r["records"] + r["n_unknown_taxid"] + r["n_unlabelled"] == len(_lines(case.listing)), case.name
        else:
            _check_refused(case)
        assert case.at_default or len(case.listing) < 8192 or case.cls in ("C6", "D"), case.name     # one chunk at 8192, or the default too


def test_documents():
    edges = {t: lab for t, lab in LR.rows(G.SINTAX, G.document("edges"))}
    assert {t: len(lab) for t, lab in edges.items()} == {**{t: n + 2 for t, n in G.IDENT.items()}, G.UNLABELLED: 0} and G.UNKNOWN not in edges
    for fmt in G.FORMATS:
        for t in list(G.IDENT) + [G.UNLABELLED, G.UNKNOWN]:
            assert G.label_len(fmt, t) == len(dict(LR.rows(fmt, G.document("edges"))).get(t, b""))
        doc = G.document("edges")
        short = LR.export(fmt, doc, b"A  1  \n")["fna"]
        assert len(short) == G.SHORTEST[fmt] and short == (b">A;tax=d:x;\n\n" if fmt == G.SINTAX else b">x;\n\n")
        assert len(LR.export(fmt, doc, b"acc  7  ACGTA\n")["fna"]) == G.record_len(fmt, 3, 7, 5)
        assert all(not lab for _, lab in LR.rows(fmt, G.document("no_label"))) and len(G.document("no_label")["taxonomies"]) == 50
        last = LR.rows(fmt, G.document("no_label_but_the_last"))
        assert all(not lab for _, lab in last[:-1]) and last[-1][1] and len(last) == 51
    corpus = dict(LR.rows(G.DADA2, G.document("corpus")))
    assert corpus[3] == b"" and 5 not in corpus and 15 in corpus and corpus[7] == b"t7;p0;" and max(corpus) == 3999


# ---- A -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", G.FORMATS)
def test_corpus_is_every_kraken2_case_and_mixes_written_and_skipped_lines(fmt):
    """The stated outcome of every kraken2 case of tests/seqdb_edges.py is the labelled restatement's, in both formats; over the
    corpus lines are written, skipped for an unknown taxid and skipped for an empty label (18179, 3735 and 1053 of them)."""
    cases = G.corpus()
    assert len(cases) == 279 and collections.Counter(c.marks["origin"][0] for c in cases) == {
        "accepted": sum(G.E.K in fmts for _, fmts in G.E.ACCEPTED.values()), "small": sum(c.fmt == G.E.K for c in G.E.small(G.E.K)), "cuts": len(G.E.cuts(G.E.K)),
        "stops": sum(c.fmt == G.E.K for c in G.E.stops()), "precedence": sum(c.fmt == G.E.K for c in G.E.precedence()),
        "refused": sum(c.fmt == G.E.K for c in G.E.refused())}
    totals = collections.Counter()
    for case in cases:
        r = _ref(case, fmt)
        assert r["outcome"] == case.outcome, (case.name, fmt)
        for key in ("records", "n_unknown_taxid", "n_unlabelled"):
            totals[key] += r[key]
    print(fmt, dict(totals))
    assert totals["records"] > 0 and totals["n_unknown_taxid"] > 0 and totals["n_unlabelled"] > 0
    assert (totals["records"], totals["n_unknown_taxid"], totals["n_unlabelled"]) == (18179, 3735, 1053)
    extra = [c for c in cases if c.marks.get("run") and any(w == "after_seq" for _, _, w in c.marks["run"])]
    assert extra                                                  # the extra-piece cases: a further separator ends the sequence


# ---- B -------------------------------------------------------------------------------------------------------------------
def _probes(case):
    for p, n, kind, place in case.marks["probe"]:
        assert case.listing[p:p + n] == (G.PROBE if n == 2 else G.PROBE4), case.name
        yield p, n, kind, place


def test_b1_probe_in_a_sequence_at_every_slice_position():
    seen2, seen4, tile = collections.defaultdict(set), set(), set()
    for case in G.b1_refused():
        assert len(case.listing) < 8192
        (p, n, kind, place), = _probes(case)
        no, s, e = _line_at(case.listing, p)
        assert case.outcome == ("error", no, G.NONASCII) and _in_sequence(case.listing, p, n) and _kind_of(case.listing[s:e]) == kind
        sq = case.listing[s:e].split(b"  ")[2]
        assert {"first": sq.startswith, "last": sq.endswith}.get(place, lambda x: x in sq[1:-1])(case.listing[p:p + n])
        assert sum(c >= 0x80 for c in case.listing) == n          # nothing else could be found
        if p % TILE >= TILE - 3:
            tile.add((n, p % TILE, place if n == 2 else "middle"))
        elif n == 2:
            seen2[p % SLICE].add((kind, place))
        else:
            seen4.add(p % SLICE)
    assert set(seen2) == set(range(SLICE))
    for k, got in seen2.items():                                  # per residue: every place, every kind of line
        assert {place for _, place in got} == set(G.PLACES) and {kind for kind, _ in got} == set(G.KINDS), k
    assert seen4 == {13, 14, 15}
    assert tile == {(2, TILE - 1, place) for place in G.PLACES} | {(4, TILE - d, "middle") for d in (1, 2, 3)}


def test_b2_high_bytes_outside_the_sequence_at_every_slice_position():
    case = G.b2_accepted()
    seen = collections.defaultdict(set)
    for p, n, kind, where in _probes(case):
        no, s, e = _line_at(case.listing, p)
        assert not _in_sequence(case.listing, p, n) and _kind_of(case.listing[s:e]) == kind
        parts = case.listing[s:e].split(b"  ")
        assert parts[2].strip() == b"ACGT"
        if where == "accession":
            assert parts[0].endswith(G.PROBE) and len(parts) == 3
        else:
            assert len(parts) == 4 and G.PROBE in parts[3] and (parts[2] == b"ACGT\t") == (where == "fourth_after_tab")
            assert where != "fourth" or case.listing[p - 6:p] == b"ACGT  "
        seen[where].add(TILE - 1 if p % TILE == TILE - 1 else p % SLICE)
    assert set(seen) == {"accession", "fourth", "fourth_after_tab"}
    assert all(got == set(range(SLICE)) | {TILE - 1} for got in seen.values())
    for fmt in G.FORMATS:                                         # only a written accession carries the probe into the output
        r = _ref(case, fmt)
        written = sum(kind == G.WRITTEN and where == "accession" for _, _, kind, where in case.marks["probe"])
        assert r["outcome"] == ("ok",) and r["fna"].count(G.PROBE) == (written if fmt == G.SINTAX else 0) and written > 0


def test_b3_several_line_starts_in_the_slice_of_the_bad_bytes():
    """What the kernel's step `while (p >= line[i + 1]) ++i` and its test of the piece need: both bad bytes in one slice whose
    first byte belongs to an earlier line (one and two line starts between them), and an accepted byte >= 0x80 before them in
    that slice."""
    phases = collections.defaultdict(set)
    earlier_line, two_starts, accepted_first, first_line_bad = set(), set(), set(), set()
    for case in G.b3_several_lines_in_a_slice():
        b = case.listing
        family = case.name.split("-")[0]
        (p, n, kind, _), = _probes(case)
        no, s, e = _line_at(b, p)
        assert case.outcome == ("error", no, G.NONASCII) and _in_sequence(b, p, 2) and len(b) < 8192
        assert all(ln in (7, 8, 9) for _, ln in case.marks["short_line"]) and (s, e - s + 1) in case.marks["short_line"]
        phases[family].add(s % SLICE)
        base = p // SLICE * SLICE
        if (p + 1) // SLICE * SLICE == base:                      # no other thread sees a byte of the probe
            starts = [ls for ls, _ in _lines(b) if base < ls <= p]
            if starts:
                earlier_line.add(family)
            if len(starts) >= 2:
                two_starts.add(family)
            if any(c >= 0x80 for c in b[base:p]):
                assert all(not _in_sequence(b, q, 1) for q in range(base, p) if b[q] >= 0x80)
                accepted_first.add(family)
            if not starts and any(c >= 0x80 for c in b[p + 2:base + SLICE]):
                first_line_bad.add(family)                        # the slice's first line is the bad one, an accepted probe behind it
    assert {f: len(v) for f, v in phases.items()} == {"later": 16, "first_only": 16, "short": 16, "three": 16}
    assert {"later", "first_only", "short", "three"} <= earlier_line and "three" in two_starts
    assert {"later", "short"} <= accepted_first and "later" in first_line_bad


def test_b4_the_probe_ends_the_file():
    seen = set()
    for case in G.b4_end_of_file():
        b = case.listing
        (p, n, kind, _), = _probes(case)
        (mod, s), = case.marks["size"]
        newline = b.endswith(b"\n")
        assert len(b) % mod == s and p + 2 + newline == len(b) and _in_sequence(b, p, 2) and len(b) < 8192
        assert case.outcome == ("error", len(_lines(b)), G.NONASCII)
        seen.add((mod, s, newline))
    assert seen == {(mod, s, nl) for mod, s in G.EOF_SIZES for nl in (False, True)}
    assert {(SLICE, 1), (SLICE, 2), (SLICE, 15), (SLICE, 0), (TILE, 1), (TILE, 0)} == set(G.EOF_SIZES)


def test_b5_b6_two_bad_lines():
    for case in G.b5_first_of_two():
        a, z = case.marks["bad"]
        assert _line_at(case.listing, a)[0] == 3 == case.outcome[1] and z - a > TILE and a // TILE != z // TILE and len(case.listing) < 8192
    assert [c.outcome for c in G.b6_precedence()] == [("error", 2, G.NONASCII), ("error", 2, G.PIECES), ("error", 2, G.PIECES)]
    assert G.b6_precedence()[2].listing.split(b"\n")[1] == G.PROBE
    assert {c.name: c.outcome for c in G.b5_first_of_two()} == {
        "nonascii_then_nonascii": ("error", 3, G.NONASCII), "nonascii_then_pieces": ("error", 3, G.NONASCII),
        "pieces_then_nonascii": ("error", 3, G.PIECES), "nonascii_then_stop": ("error", 3, G.NONASCII), "stop_then_nonascii": ("stop", 3)}


# ---- C -------------------------------------------------------------------------------------------------------------------
def _short_record(fmt):
    return b">A;tax=d:x;\n\n" if fmt == G.SINTAX else b">x;\n\n"


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_c1_tiny_records(fmt):
    firsts = set()
    for case in G.c1_tiny_records(fmt):
        fna = _ref(case, fmt)["fna"]
        starts = case.marks["tiny"]
        n = G.SHORTEST[fmt]
        assert len(starts) >= 48 and starts == list(range(starts[0], starts[0] + n * len(starts), n)) and len(case.listing) < 8192
        assert fna[starts[0]:starts[-1] + n] == _short_record(fmt) * len(starts)
        assert {s % SLICE for s in starts} == set(range(SLICE))
        inside = range(-(-starts[0] // SLICE), (starts[-1] + n) // SLICE)      # the slices that lie in the run
        per_slice = collections.Counter({k: 0 for k in inside})
        per_slice.update(s // SLICE for s in starts if s // SLICE in inside)
        assert len(inside) >= 48 * n // SLICE - 1 and set(per_slice.values()) == ({3, 4} if fmt == G.DADA2 else {1, 2})
        firsts.add(starts[0] % TILE)
    assert firsts == {TILE - 1, 0}


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_c2_skipped_runs_at_every_boundary(fmt):
    seen = set()
    for case in G.c2_skipped_runs(fmt):
        fna = _ref(case, fmt)["fna"]
        lines = _lines(case.listing)
        assert case.at_default == (len(case.listing) >= 8192)
        for at, r, mod, n_before in case.marks["skipped_run"]:
            d = (at + 2) % mod - 2
            assert fna[at - 1:at + G.SHORTEST[fmt] + 1] == b"\n" + _short_record(fmt) + b">"      # the record ends, the shortest follows
            run = [case.listing[s:e] for s, e in lines[n_before:n_before + r]]
            assert run == [b"a  %d  A" % (G.UNKNOWN, G.UNLABELLED)[i % 2] for i in range(r)]
            assert case.listing[slice(*lines[n_before + r])] == b"A  1  " and _kind_of(case.listing[slice(*lines[n_before - 1])]) == G.WRITTEN
            assert len(fna[:at].split(b">")) - 1 == sum(_kind_of(case.listing[s:e]) == G.WRITTEN for s, e in lines[:n_before]) if r < 20 else True
            seen.add((r, d, mod))
    assert seen == {(r, d, SLICE) for r in G.RUNS for d in G.DS} | {(r, d, TILE) for r in G.RUNS if r <= 257 for d in G.DS}
    assert set(G.RUNS) == {1, 2, 3, 15, 16, 17, 255, 256, 257, 4100} and set(G.DS) == {-2, -1, 0, 1} and 4100 > 16 * 256


def test_c3_ends_of_a_chunk():
    names = set()
    for case in G.c3_ends_of_a_chunk():
        kinds, = case.marks["kinds"]
        assert [_kind_of(case.listing[s:e]) for s, e in _lines(case.listing)] == list(kinds) and len(case.listing) < 8192
        for fmt in G.FORMATS:
            r = _ref(case, fmt)
            assert (r["records"], r["n_unknown_taxid"], r["n_unlabelled"]) == tuple(kinds.count(k) for k in G.KINDS)
        written = [i for i, k in enumerate(kinds) if k == G.WRITTEN]
        name = case.name.replace("_open", "")
        assert case.name.endswith("_open") == (not case.listing.endswith(b"\n"))
        if name.startswith("first_"):
            assert written[0] == int(name.split("_")[1])
        elif name.startswith("last_"):
            assert len(kinds) - 1 - written[-1] == int(name.split("_")[1])
        else:
            assert written == [{"only_the_first_written": 0, "only_the_last_written": len(kinds) - 1, "only_line_257_written": 256}[name]]
        names.add(case.name)
    assert names == ({f"{w}_{n}_skipped{o}" for n in (1, 256, 257) for w, o in (("first", ""), ("last", ""), ("last", "_open"))}
                     | {"only_the_first_written", "only_the_last_written", "only_the_last_written_open", "only_line_257_written"})


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_c4_totals(fmt):
    seen = set()
    for case in G.c4_totals(fmt):
        r = _ref(case, fmt)
        total, = case.marks["total"]
        assert len(r["fna"]) == total and case.at_default == (len(case.listing) >= 8192)
        assert [_kind_of(case.listing[s:e]) for s, e in _lines(case.listing)[-3:]] == [G.SKIP_U, G.SKIP_N, G.SKIP_U]
        assert _kind_of(case.listing[slice(*_lines(case.listing)[0])]) == G.SKIP_U
        seen.add(total)
    assert seen == {t for t in (5, 13, 15, 16, 17, 4095, 4096, 4097, 8192, 8193) if t >= G.SHORTEST[fmt]}


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_c5_long_pieces(fmt):
    seen = collections.defaultdict(set)
    for case in G.c5_long_pieces(fmt):
        fna = _ref(case, fmt)["fna"]
        (at, n, what), = case.marks["long"]
        piece = b"Q" * 5000 if what == "accession_5000" else (b"d:" if fmt == G.SINTAX else b"") + G.ident(n).encode()
        n = len(piece)
        assert fna[at:at + n] == piece and fna[at - 1:at] in (b">", b"=") and fna[at + n:at + n + 1] == b";"
        tiny, = case.marks["tiny"]
        assert fna[tiny - 1:tiny + G.SHORTEST[fmt] + 1] == b"\n" + _short_record(fmt) + b">" and at < tiny < at + n + 40
        assert (at + n - 1) // TILE - at // TILE >= n // TILE and case.at_default == (len(case.listing) >= 8192)
        seen[what].add(at % TILE)
    assert set(seen) == {"label_5000", "label_9000"} | ({"accession_5000"} if fmt == G.SINTAX else set())
    assert all(got == {4090, 4091, 4092, 4093, 4094, 4095, 0, 1} for got in seen.values())


def test_c6_no_row_has_a_label():
    none, one = G.c6_no_label()
    taxids = none.marks["taxids"]
    assert len(taxids) == 400 == none.listing.count(b"\n") and none.listing == one.listing
    for fmt in G.FORMATS:
        r = _ref(none, fmt)
        assert sum(len(lab) for _, lab in LR.rows(fmt, G.document(none.doc))) == 0
        assert r["outcome"] == ("ok",) and r["fna"] == b"" and r["records"] == 0
        assert r["n_unlabelled"] == sum(t <= 50 for t in taxids) > 300 and r["n_unknown_taxid"] == sum(t > 50 for t in taxids) > 0
        r = _ref(one, fmt)
        assert r["records"] == taxids.count(51) > 0 and r["n_unlabelled"] == sum(t <= 50 for t in taxids)
        assert r["fna"].count(b">last;one;\n" if fmt == G.DADA2 else b";tax=d:last,p:one;") == r["records"]


# ---- D -------------------------------------------------------------------------------------------------------------------
def test_d_counts_are_the_heads():
    seen = set()
    for case in G.d_counts():
        what, place = case.name.split("-")
        (at, n), = case.marks["bad"]
        head, = case.marks["head"]
        no, s, e = _line_at(case.listing, at)
        assert (s, e + 1) == (at, at + n) and case.outcome[1] == no
        assert {"line_1": no == 1, "line_257": no == 257, "last_of_a_chunk": at + n == TILE and no == 301,
                "first_of_the_next_chunk": at == TILE and no == 301}[place]
        whole = case.listing[:at] + case.listing[at + n:]          # without the bad line: the tail's skipped lines count too
        for fmt in G.FORMATS:
            r = _ref(case, fmt)
            assert (r["records"], r["n_unknown_taxid"], r["n_unlabelled"]) == head
            assert place == "line_1" or min(head) > 50
            w = LR.export(fmt, G.document("edges"), whole)
            assert w["outcome"] == ("ok",) and w["n_unknown_taxid"] >= head[1] + 50 and w["n_unlabelled"] >= head[2] + 50
            assert w["records"] >= head[0] + 50
        behind = case.listing[at + n:at + n + 2000]                # at 8192 the bad line's chunk holds these lines of the tail at least
        assert at + n + 2000 <= 8192 and behind.count(b"  9  ") > 30 and behind.count(b"  8  ") > 30
        seen.add((what, place))
    assert seen == {(w, p) for w in G.D_REASONS for p in G.D_PLACES} and set(G.D_REASONS) == {G.PIECES, G.NONASCII, G.TAXID, "stop"}
