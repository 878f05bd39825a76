"""The best hit per subject where no GPU is needed: the restatement (tests/subject_best_reference.py) against
hand cases, the ctypes mirrors, the command line's flag, the C ABI's refusals, and the NULL selection on the CPU path."""
import ctypes as C

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import blast, cli, pipeline
from tests import hit_filter_reference as hf
from tests import subject_best_reference as ref


def test_the_restatement_on_hand_cases():
    seg = [0, 4, 4, 9]
    bs = [100, 100, 90, 120, 5, 7, 7, 3, 7]
    acc = [1, 1, 2, 1, 9, 9, 9, 8, 1]
    v, n_kept, n_thinned = ref.keep(seg, bs, acc)
    assert v == [0, 0, 1, 1, 0, 1, 0, 1, 1] and (n_kept, n_thinned) == (5, 2)
    # first wins on ties, wherever the tie stands
    assert ref.keep([0, 3], [7, 7, 7], [4, 4, 4])[0] == [1, 0, 0]
    assert ref.keep([0, 3], [6, 7, 7], [4, 4, 4])[0] == [0, 1, 0]
    # the query is part of the pair: one accession under two queries is two pairs
    assert ref.keep([0, 2, 4], [5, 4, 5, 4], [3, 3, 3, 3]) == ([1, 0, 1, 0], 2, 2)
    assert ref.keep([0, 1, 2, 3, 4], [5, 4, 5, 4], [3, 3, 3, 3]) == ([1, 1, 1, 1], 4, 0)
    # idempotent: the compacted table loses nothing more
    off, (bs2, acc2) = ref.compact(seg, v, bs, acc)
    assert off == [0, 2, 2, 5] and bs2 == [90, 120, 7, 3, 7] and acc2 == [2, 1, 9, 8, 1]
    assert ref.keep(off, bs2, acc2) == ([1] * 5, 5, 0)
    # negative scores and the ends of the range
    lo, hi = -(1 << 31), (1 << 31) - 1
    assert ref.keep([0, 4], [lo, -1, hi, 0], [1, 1, 1, 1])[0] == [0, 0, 1, 0]
    assert ref.keep([0, 2], [-1, 0], [1, 1])[0] == [0, 1] and ref.keep([0, 2], [0, -1], [1, 1])[0] == [1, 0]
    # offsets as the library reads them: clamped, a decreasing pair empty, unnamed rows dropped
    assert ref.keep([0, 2, 50, 1], [3, 3, 3], [1, 1, 1]) == ([1, 0, 1], 2, 1)
    assert ref.keep([0], [3, 3], [1, 1]) == ([0, 0], 0, 0)


def test_rewrite_table_deletes_all_but_the_best_line_of_a_pair(tmp_path):
    line = lambda q, acc, bs, taxid=100, eol="\n": f"{q}\t{acc}\t{taxid}\t99.0\t400\t0\t0\t1\t400\t1\t400\t1e-50\t{bs}{eol}"
    src, dst = tmp_path / "a.tsv", tmp_path / "b.tsv"
    body = [line("a", "X.1", "99.6"), line("b", "X.1", "8"), line("a", "X.1", "99.5", 101, "\r\n"), "\n", line("a", "Y.1", "98"),
            line("b", "X.1", "9.99e0"), line("a", "X.1", "100")]
    src.write_text("".join(body), newline="")
    assert ref.rewrite_table(str(src), str(dst)) == (6, 3, 2, 2)
    got = dst.read_bytes().decode().splitlines(keepends=True)
    assert got == ["\n", body[4], body[5], body[6]]                      # b: 9 > 8; a / X.1: 100 wins; the empty line stays
    # 99.6 and 99.5 both truncate to 99: whichever comes first is kept, with its own taxid
    assert ref.rewrite_table(str(src), str(dst), kept=[True, True, True, True, True, False]) == (5, 3, 2, 2)
    got = dst.read_bytes().decode().splitlines(keepends=True)
    assert got == [body[0], "\n", body[4], body[5]]
    # idempotent
    again = tmp_path / "c.tsv"
    assert ref.rewrite_table(str(dst), str(again)) == (3, 3, 0, 2) and again.read_bytes() == dst.read_bytes()


def test_struct_mirrors_and_exports():
    assert C.sizeof(N.SubjectBestC) == 8 and C.sizeof(N.SubjectBestStats) == 32
    assert [getattr(N.SubjectBestC, f).offset for f in ("mask", "reserved")] == [0, 4]
    assert [getattr(N.SubjectBestStats, f).offset for f in ("n_hits", "n_kept", "n_queries", "n_thinned")] == [0, 8, 16, 24]
    assert N.SUBJECT_BEST_PER_QUERY == 1
    assert {"blu_hits_subject_keep", "blu_hits_subject_best"} <= set(N.EXPORTS)
    assert {"blu_build_consensus", "blu_ingest_columns_selected"} <= set(N.PIPELINE_EXPORTS)
    L = N.lib()
    for name in ("blu_hits_subject_keep", "blu_hits_subject_best", "blu_build_consensus", "blu_ingest_columns_selected"):
        assert hasattr(L, name)


def test_cli_flag_parses_and_reaches_the_pipeline(tmp_path, monkeypatch):
    ap = cli.build_parser()
    common = ["-t", "t.json", "--taxon", "bacteria", "--strategy", "relaxed"]
    for head in (["blastn", "build-consensus", "b.tsv"],
                 ["blastn", "run-with-consensus", "q.fa", "-d", "db", "--blast-out-file", "b.tsv"]):
        assert ap.parse_args(head + common + ["--best-hit-per-subject"]).best_hit_per_subject is True
        assert ap.parse_args(head + common).best_hit_per_subject is False
    for sub in ("build-tabular", "build-report"):
        with pytest.raises(SystemExit):
            ap.parse_args(["blastn", sub, "doc.json", "--best-hit-per-subject"])
    # build-consensus hands the keyword to the pipeline (and not without the flag)
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        return "{}", {"subject_best": {"n_hits": 5, "n_kept": 3, "n_queries": 2, "n_thinned": 1}} if kw.get("best_hit_per_subject") else {}

    monkeypatch.setattr(pipeline, "build_consensus_identities", fake)
    base = ["blastn", "build-consensus", "b.tsv", "-t", "t.json", "--taxon", "bacteria", "--strategy", "relaxed"]
    assert cli.main(base + ["--best-hit-per-subject"]) == 0 and seen[-1].get("best_hit_per_subject") is True
    assert cli.main(base) == 0 and "best_hit_per_subject" not in seen[-1]
    # run-with-consensus hands it to blast.run_blast_and_build_consensus
    seen_b = []
    monkeypatch.setattr(blast, "run_blast_and_build_consensus", lambda *a, **kw: seen_b.append(kw) or "{}")
    run = ["blastn", "run-with-consensus", "q.fa", "-d", "db", "--blast-out-file", str(tmp_path / "b.tsv"), "-t", "t.json",
           "--taxon", "bacteria", "--strategy", "relaxed"]
    assert cli.main(run + ["--best-hit-per-subject"]) == 0 and seen_b[-1].get("best_hit_per_subject") is True
    assert cli.main(run) == 0 and "best_hit_per_subject" not in seen_b[-1]


def test_the_count_line_stands_between_the_filter_lines_and_the_band_line(capsys):
    cli._say_kept({"n_lines": 9, "n_kept": 7, "subject_best": {"n_hits": 7, "n_kept": 5, "n_queries": 3, "n_thinned": 2},
                   "score_band": {"n_hits": 5, "n_raised": 1, "n_queries": 3, "n_widened": 1}})
    err = capsys.readouterr().err
    line = "subject best hit: kept 5 of 7 lines, thinned 2 of 3 queries"
    assert err.index("hit filter: kept 7 of 9 lines") < err.index(line) < err.index("score band: raised 1 of 5 lines")


def test_c_abi_refusals_need_no_device():
    L = N.lib()
    bs, acc = np.array([5, 4, 3], np.int32), np.array([1, 1, 2], np.uint32)
    aln, tax, pid = np.zeros(3, np.int32), np.zeros(3, np.uint32), np.zeros(3, np.float64)
    seg, keep = np.array([0, 3], np.uint64), np.zeros(3, np.uint32)
    st, n_out = N.SubjectBestStats(), C.c_uint64(0)
    p = lambda a: a.ctypes.data

    def best(sel, n_hits=3, n_queries=1, device=-1, **null):
        cols = [None if name in null else p(a) for name, a in (("bs", bs), ("aln", aln), ("tax", tax), ("acc", acc), ("pid", pid))]
        return L.blu_hits_subject_best(device, *cols, None if "seg" in null else p(seg), n_hits, n_queries, 0,
                                       C.byref(sel) if sel is not None else None, None, 0xFFFFFFFF, C.byref(n_out), None, C.byref(st))

    on = N.SubjectBestC(N.SUBJECT_BEST_PER_QUERY, 0)
    # unknown mask bits
    for mask in (2, 3, 0x80000000):
        assert best(N.SubjectBestC(mask, 0)) == N.BLU_ERR_INVALID_ARG and "mask" in N.last_error()
    # a NULL array with a non-zero count
    for name in ("bs", "aln", "tax", "acc", "pid", "seg"):
        assert best(on, **{name: True}) == N.BLU_ERR_INVALID_ARG and "null" in N.last_error()
    for kw in (dict(b=None), dict(a=None), dict(s=None), dict(k=None)):
        rc = L.blu_hits_subject_keep(-1, kw.get("b", p(bs)), kw.get("a", p(acc)), kw.get("s", p(seg)), 3, 1, 0, None, kw.get("k", p(keep)),
                                     C.byref(st))
        assert rc == N.BLU_ERR_INVALID_ARG and "null" in N.last_error()
    # n_hits >= 2^32 (the arrays are not read), n_queries >= 2^32
    for n_hits, n_queries, word in ((1 << 32, 1, "n_hits"), ((1 << 40) + 5, 1, "n_hits"), (3, 1 << 32, "n_queries")):
        assert best(on, n_hits, n_queries) == N.BLU_ERR_INVALID_ARG and word in N.last_error()
        rc = L.blu_hits_subject_keep(-1, p(bs), p(acc), p(seg), n_hits, n_queries, 0, None, p(keep), C.byref(st))
        assert rc == N.BLU_ERR_INVALID_ARG and word in N.last_error()
    # a NULL selection and an empty mask, host pointers: the table as it is, no device asked for
    tax[1] = 0xFFFFFFFF
    n_un = C.c_uint64(9)
    for sel in (None, N.SubjectBestC(0, 0)):
        rc = L.blu_hits_subject_best(-1, p(bs), p(aln), p(tax), p(acc), p(pid), p(seg), 3, 1, 0, C.byref(sel) if sel is not None else None,
                                     None, 0xFFFFFFFF, C.byref(n_out), C.byref(n_un), C.byref(st))
        assert rc == N.BLU_OK and (n_out.value, n_un.value) == (3, 1) and bs.tolist() == [5, 4, 3] and seg.tolist() == [0, 3]
        assert (st.n_hits, st.n_kept, st.n_queries, st.n_thinned) == (3, 3, 1, 0)
    # the pipeline's entry points refuse unknown bits before they read a file
    cols = pipeline.IngestColumns()
    sel = pipeline.HitSelection(subject_best=C.pointer(N.SubjectBestC(4, 0)))
    rc = pipeline._bind().blu_ingest_columns_selected(b"/nonexistent.tsv", b"/nonexistent.json", 0, -1, C.byref(sel), C.byref(cols), None)
    assert rc == N.BLU_ERR_INVALID_ARG and "mask" in N.last_error()


def _duplicated_rows(rng):
    rows = hf.make_rows(40, 6, rng, sample_names=True)
    return rows + [r for r in rows[::3]]                                 # a third of the lines twice: scattered pairs


def test_a_null_selection_is_the_older_entry_point_on_the_cpu_path(tmp_path, monkeypatch):
    """blu_ingest_columns_selected with a NULL subject_best member, with the member present and its mask empty, and with a
    selection struct that is all NULL (and no struct at all): the same bytes (device -1, the CPU parser).  The documents of
    such requests are compared where there is a device: tests/test_gpu_subject_best.py, tests/test_gpu_consensus_request.py."""
    monkeypatch.setenv("BLU_INGEST", "cpu")
    rng = np.random.default_rng(91)
    src = tmp_path / "b.tsv"
    src.write_bytes(("\n".join(_duplicated_rows(rng)) + "\n").encode())
    tj = hf.write_db(tmp_path / "t.json")
    L = pipeline._bind()

    def columns(c):
        out = {k: np.ctypeslib.as_array(getattr(c, k), shape=(int(c.n_hits),)).copy() for k in ("bitscore", "align_len", "tax_desc_row", "acc_rank", "pident")}
        out["seg_off"] = np.ctypeslib.as_array(c.seg_off, shape=(int(c.n_queries) + 1,)).copy()
        out["names"] = C.string_at(c.query_names, int(c.query_names_bytes)) + C.string_at(c.accessions, int(c.accessions_bytes))
        return out

    old = pipeline.IngestColumns()
    assert L.blu_ingest_columns_selected(str(src).encode(), tj.encode(), 0, -1, None, C.byref(old), None) == N.BLU_OK
    want = columns(old)
    L.blu_ingest_columns_free(C.byref(old))
    empty_band = C.pointer(N.ScoreBandC(0, 0, 0))
    for sel in (pipeline.HitSelection(), pipeline.HitSelection(score_band=empty_band),                 # all NULL; the member NULL
                pipeline.HitSelection(subject_best=C.pointer(N.SubjectBestC(0, 0))),                    # present, mask 0
                pipeline.HitSelection(score_band=empty_band, subject_best=C.pointer(N.SubjectBestC(0, 0)))):
        new, st = pipeline.IngestColumns(), pipeline.HitSelectionStats()
        rc = L.blu_ingest_columns_selected(str(src).encode(), tj.encode(), 0, -1, C.byref(sel), C.byref(new), C.byref(st))
        assert rc == N.BLU_OK
        got = columns(new)
        L.blu_ingest_columns_free(C.byref(new))
        assert all(np.array_equal(got[k], want[k]) if k != "names" else got[k] == want[k] for k in want)
        st = st.subject_best
        assert (st.n_hits, st.n_kept, st.n_thinned) == (len(want["bitscore"]), len(want["bitscore"]), 0)
    # the keyword left False is the call of before, and the stats carry no counts
    a = pipeline.ingest_columns(str(src), tj, device=-1)
    b = pipeline.ingest_columns(str(src), tj, device=-1, best_hit_per_subject=False)
    hf.assert_columns_equal(a, b)
    assert "subject_best" not in b
    # a selection with a non-empty mask needs a device, whichever parser ran
    with pytest.raises(N.BluError):
        pipeline.ingest_columns(str(src), tj, device=-1, best_hit_per_subject=True)
