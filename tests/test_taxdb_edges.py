"""The byte-level edge cases of `build-db blu` (tests/taxdb_edges.py) against the oracle alone, without a GPU: every accepted
case builds, every class fires, a respelling that keeps the meaning leaves the oracle's output byte-equal to the base
case's (the oracle is blind to the spelling), one that changes it changes the entry it names, every refused case raises
naming file and line; and the oracle's UTF-8 check and string escapes against statements written out here."""
import functools
import json

import pytest

from oracle import taxdb_oracle as orc
from tests import taxdb_edges as te


def _build(tmp_path, files, name="case", **opts):
    c = te.write(str(tmp_path / name), files)
    return orc.build(c["dir"], c["accessions"], source_database="blast/16S", **opts)


@functools.lru_cache(maxsize=4)
def _base_result(seed, big, tmp):
    c = te.write(tmp, te.base_files(seed, big))
    return orc.build(c["dir"], c["accessions"], source_database="blast/16S")


def _entries(doc):
    return {e["taxid"]: e for e in json.loads(doc)["taxonomies"]}


@pytest.mark.parametrize("cls,seed", te.ACCEPTED_IDS, ids=[f"{c}-{s}" for c, s in te.ACCEPTED_IDS])
def test_accepted(tmp_path, tmp_path_factory, cls, seed):
    case = te.accepted(cls, seed)
    assert te.FIRED[cls] > 0
    assert any(case["files"][n] != case["base"][n] for n in te.FILES)
    doc, tsv, st = _build(tmp_path, case["files"])
    b_doc, b_tsv, b_st = _base_result(seed % 2, case["big"], str(tmp_path_factory.getbasetemp() / f"edges_base{seed % 2}{case['big']}"))
    assert b_st["mapped"] > 100 and b_st["mapped_merged"] > 0 and b_st["deleted"] > 0 and b_st["unknown"] > 0
    if case["preserving"]:
        assert (doc, tsv, st) == (b_doc, b_tsv, b_st)
        return
    assert (doc, tsv) != (b_doc, b_tsv)
    if case["changed"] == "tsv":
        assert tsv != b_tsv
    elif case["changed"] == "doc":
        assert doc != b_doc
    else:
        got, base = _entries(doc), _entries(b_doc)
        same = [t for t in case["changed"] if got.get(t) == base.get(t)]
        assert not same, f"the respelling left the entries of {same} as they were"
    for k, v in case["stat"].items():
        assert st[k] == v and b_st[k] != v
    if "n_ranks" in case:
        assert len({e["rank"] for e in _entries(doc).values()} | {lv.split("__")[0] for e in _entries(doc).values()
                                                                     for lv in e["numericLineage"].split(";") if lv}) <= case["n_ranks"]


def test_every_class_and_every_ill_formed_sequence_fires():
    for cls, seed in te.ACCEPTED_IDS:
        te.accepted(cls, seed)
    for cls in te.ACCEPTED:
        assert te.FIRED[cls] > 0, cls
    for kind in te.INVALID_UTF8:
        assert te.FIRED["utf8_dump:" + kind] > 0 and te.FIRED["utf8_listing:" + kind] > 0, kind


@pytest.mark.parametrize("name", [n for n, _ in te.COUNTS])
def test_counts(tmp_path, name):
    kw = dict(te.COUNTS)[name]
    _, tsv, st = _build(tmp_path, te.sized_files(**kw))
    assert st["nodes"] == kw["n"] + bool(kw.get("top")) and st["accession_lines"] == kw["n_acc"] + 9 * bool(kw.get("top"))
    if kw.get("one_taxid"):
        assert st["distinct_taxids"] == 1 and st["mapped"] == 1
    if kw.get("top"):
        t = kw["top"]
        assert f"{t + 1}\tunknown\n{t + 2}\tunknown\n".encode() in tsv and f"{(1 << 31) + t}\tunknown\n".encode() in tsv
        assert st["mapped"] > 10 and st["deleted"] > 10 and st["mapped_merged"] > 10


@pytest.mark.parametrize("name", sorted(te.REFUSED))
def test_refused(tmp_path, name):
    files, bad_file, line = te.REFUSED[name]
    if name.startswith("ancestor_"):     # the ancestor message names the taxid whose lineage is walked, not the line
        with pytest.raises(orc.TaxdbError, match=rf"taxidlineage\.dmp: .* in the lineage of {te.ANCESTOR_TAXID}$"):
            _build(tmp_path, files)
        assert files["taxidlineage.dmp"].split(b"\n")[line - 1].startswith(b"%d\t" % te.ANCESTOR_TAXID)
        return
    with pytest.raises(orc.TaxdbError, match=rf"/{bad_file.replace('.', chr(92) + '.')}:{line}: "):
        _build(tmp_path, files)


@pytest.mark.parametrize("name", sorted(te.UNREAD_ANCESTORS))
def test_bad_ancestor_of_a_taxid_nobody_names_is_not_read(tmp_path, name):
    doc, _, st = _build(tmp_path, te.UNREAD_ANCESTORS[name])
    assert sorted(_entries(doc)) == [40, 50, 99] and st["deleted"] == 1


@pytest.mark.parametrize("name", sorted(te.PRECEDENCE))
def test_precedence(tmp_path, name):
    files, bad_file, line = te.PRECEDENCE[name]
    with pytest.raises(orc.TaxdbError, match=rf"/{bad_file.replace('.', chr(92) + '.')}:{line}: "):
        _build(tmp_path, files)


@pytest.mark.parametrize("n", [2049, 5000])
def test_oracle_has_no_rank_limit(tmp_path, n):
    doc, _, st = _build(tmp_path, te.many_ranks(n))
    assert st["mapped"] == 2 and _entries(doc)[n]["rank"] == f"r{n}"


def test_refused_tables_hold_one_case_per_kind():
    assert len(te.REFUSED) == 4 + 5 + 5 * len(te.BAD_IDS) + len(te.BAD_IDS) + 9 + len(te.BAD_ANCESTORS)
    assert len(te.PRECEDENCE) == 6 + 5 + 1


# ---- the oracle's UTF-8 check and escapes against statements of their own --------------------------------------------------
def _well_formed(b: bytes) -> bool:
    """The Unicode standard's table of well-formed UTF-8 byte sequences (table 3-7), one row per branch."""
    i, n = 0, len(b)
    tail = lambda k, lo=0x80, hi=0xBF: i + k < n and lo <= b[i + k] <= hi
    while i < n:
        c = b[i]
        if c <= 0x7F:
            i += 1
        elif 0xC2 <= c <= 0xDF and tail(1):
            i += 2
        elif c == 0xE0 and tail(1, 0xA0) and tail(2):
            i += 3
        elif (0xE1 <= c <= 0xEC or 0xEE <= c <= 0xEF) and tail(1) and tail(2):
            i += 3
        elif c == 0xED and tail(1, 0x80, 0x9F) and tail(2):
            i += 3
        elif c == 0xF0 and tail(1, 0x90) and tail(2) and tail(3):
            i += 4
        elif 0xF1 <= c <= 0xF3 and tail(1) and tail(2) and tail(3):
            i += 4
        elif c == 0xF4 and tail(1, 0x80, 0x8F) and tail(2) and tail(3):
            i += 4
        else:
            return False
    return True


def test_oracle_utf8_check_against_the_well_formed_table():
    for a in range(256):
        assert orc._valid_utf8(bytes([a])) == _well_formed(bytes([a])) == (a < 0x80)
        for b in range(256):
            for rest in (b"", b"\x80", b"\x80\x80", b"\xbf\xbf", b"A"):
                s = bytes([a, b]) + rest
                assert orc._valid_utf8(s) == _well_formed(s), s
    for u in te.VALID_UTF8:
        assert orc._valid_utf8(b"x" + u + b"y") and _well_formed(u)
        assert not orc._valid_utf8(u[:-1]) and not orc._valid_utf8(u[:-1] + b"y")
    for kind, bad in te.INVALID_UTF8.items():
        line = te._bad_line(kind, b"BAD.1  5  1")
        assert not orc._valid_utf8(line) and not _well_formed(line), kind
    assert not _well_formed(b"\xed\xa0\x80") and _well_formed(b"\xed\x9f\xbf\xee\x80\x80") and not _well_formed(b"\xf4\x90\x80\x80")


def test_oracle_escapes_against_the_serde_json_table():
    short = {0x08: "\\b", 0x0C: "\\f", 0x0A: "\\n", 0x0D: "\\r", 0x09: "\\t", 0x22: '\\"', 0x5C: "\\\\"}
    for c in range(0x80):
        want = short.get(c) or ("\\u00%02x" % c if c < 0x20 else chr(c))
        assert orc._jstr(bytes([c])) == '"' + want + '"', c
        assert orc._jstr(b"a" + bytes([c]) * 3 + b"z") == '"a' + want * 3 + 'z"'
    assert orc._jstr(b"\x1f\x7f") == '"\\u001f\x7f"'
    for u in te.VALID_UTF8:
        assert orc._jstr(b"a" + u).encode("utf-8", "surrogatepass") == b'"a' + u + b'"'      # kept as they are, never \uXXXX
