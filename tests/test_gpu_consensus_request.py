"""One blu_build_consensus request with every option set at once (include/blu_pipeline.h: blu_consensus_request): the report,
the per-sample table, the support table, a hit filter, a taxon exclude list, the best hit per subject and a bit-score band.
The rule is the sum of the options' own: the run gives, byte for byte, what the plain request gives on the
table that the Python restatements of the options, applied in the order of §18, make of the input.  The per-feature suites
cover each option alone and in pairs; this is the request in which no pointer is NULL."""
import numpy as np
import pytest

from blutils_amd import blast, pipeline
from tests import hit_filter_reference as hf
from tests import score_band_reference as band_ref
from tests import subject_best_reference as subject_ref
from tests import taxon_filter_reference as tf

pytestmark = pytest.mark.gpu

POOL = list(range(tf.FIRST_TAXID, tf.FIRST_TAXID + tf.N_TAXIDS + tf.N_UNKNOWN))
LONG, GONE = "s0.900", "s1.901"
HIT_FILTER = {"min_perc_identity": 92.0, "min_align_length": 150}
TOP_BITS = 2


def _rows(rng):
    """32 queries named `<sample>.<n>`.  A subject aligns in one to four places (HSPs), the scores of a query lie within 30 bits
    of its top, a third of them with a decimal.  LONG names every taxid four times — well over 64 lines after the filters — and
    GONE keeps no line: one fails the identity threshold, the other is a chloroplast."""
    rows = []

    def query(name, taxids, hsps):
        top, mine = int(rng.integers(300, 3000)), []
        for t in taxids:
            for _ in range(int(rng.choice(hsps))):
                b = top - int(rng.choice([0, 0, 1, 2, 5, 30]))
                mine.append(tf.line(name, int(t), pid=f"{88 + int(rng.integers(0, 12001)) / 1000:.3f}", aln=str(int(rng.integers(100, 600))),
                                    bs=f"{b}.5" if rng.random() < 0.33 else str(b), acc=f"NR_{t:06d}.1"))
        rows.extend(mine[i] for i in rng.permutation(len(mine)))

    for q in range(30):
        query(f"s{q % 3}.{q}", rng.choice(POOL, int(rng.integers(1, 7)), replace=False), [1, 1, 2, 3])
    query(LONG, POOL, [4])
    chloroplast = next(t for t in POOL[:tf.N_TAXIDS] if (t - tf.FIRST_TAXID) % 3 == 2 and (t - tf.FIRST_TAXID) % 4 == 3)
    rows += [tf.line(GONE, POOL[0], pid="80.0", acc="NR_1.1"), tf.line(GONE, chloroplast, acc="NR_2.1")]
    return rows


def _run(tmp_path, tag, table, tj, headers, cfg, **selection):
    """the request once to a file and once into text -> ({doc, report, table, support: bytes} of each, the stats of the first)"""
    out = []
    for to_file in (True, False):
        paths = {k: str(tmp_path / f"{tag}{int(to_file)}.{k}") for k in ("doc", "report", "table", "support")}
        text, stats = pipeline.build_consensus_identities_with_tables(
            table, tj, "bacteria", "relaxed", headers=headers, out_format="json", lenient=True, parse=False, config=cfg,
            out_path=paths["doc"] if to_file else None, report_path=paths["report"], sample_table_path=paths["table"],
            support_table_path=paths["support"], **selection)
        files = {k: open(paths[k], "rb").read() for k in ("report", "table", "support")}
        files["doc"] = open(paths["doc"], "rb").read() if to_file else text.encode()
        out.append((files, stats))
    timings = lambda s: {k: v for k, v in s.items() if not k.startswith("t_")}
    assert out[0][0] == out[1][0] and timings(out[0][1]) == timings(out[1][1])
    return out[0]


@pytest.mark.parametrize("mode", ["gpu", "host_columns"])
def test_every_option_at_once_is_the_plain_request_on_the_restated_table(tmp_path, monkeypatch, mode):
    monkeypatch.setenv("BLU_INGEST", "gpu")
    if mode == "host_columns":
        monkeypatch.setenv("BLU_PIPELINE_HOST_COLUMNS", "1")
    else:
        monkeypatch.delenv("BLU_PIPELINE_HOST_COLUMNS", raising=False)
    rows = _rows(np.random.default_rng(119))
    src, tj = str(tmp_path / "b.tsv"), tf.write_db(tmp_path / "t.json")
    open(src, "wb").write(("\n".join(rows) + "\n").encode())
    # §18's order: the taxon verdict and the thresholds (the parser), the best hit per subject, the band
    c1, c2, c3 = (str(tmp_path / f"c{k}.tsv") for k in (1, 2, 3))
    taxa = tf.filter_text(src, c1, tj, exclude=tf.EXCLUDE, keep=lambda fields: hf.keep(fields, HIT_FILTER))
    n_in, n_best, n_thinned, n_q = subject_ref.rewrite_table(c1, c2)
    b_hits, n_raised, n_widened, b_q = band_ref.rewrite_table(c2, c3, D=TOP_BITS)
    left = [l.split(b"\t")[0].decode() for l in open(c1, "rb").read().splitlines()]
    assert left.count(LONG) > 64 and GONE not in left and n_q == b_q == len(set(left)) < 32   # the long-segment path; queries filtered away
    assert 0 < taxa["n_excluded"] and taxa["n_kept"] == n_in < len(rows) and n_best < n_in and n_thinned > 1 and n_raised > 0
    headers = sorted({r.split("\t")[0] for r in rows}) + ["s2.777777"]                # GONE and a FASTA id without a hit: null taxa
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")                      # (one run id for every document)
    got, stats = _run(tmp_path, "all", src, tj, headers, cfg, hit_filter=HIT_FILTER, taxon_filter={"exclude": tf.EXCLUDE},
                      best_hit_per_subject=True, score_band={"top_bits": TOP_BITS})
    assert pipeline.last_ingest_path() == "gpu"
    want, plain = _run(tmp_path, "plain", c3, tj, headers, cfg)
    assert got == want and len(want["doc"]) > 5000 and want["support"].count(b"\n") == len(headers) + 1
    # the counts: each option's, over the table the ones before it left
    assert (stats["n_lines"], stats["n_kept"]) == (len(rows), n_in)
    assert stats["taxon_filter"] == {"n_lines": len(rows), "n_excluded": taxa["n_excluded"], "n_not_only": 0, "exclude": tf.EXCLUDE,
                                     "excluded_by": taxa["excluded_by"]}
    assert stats["subject_best"] == {"n_hits": n_in, "n_kept": n_best, "n_queries": n_q, "n_thinned": n_thinned}
    assert stats["score_band"] == {"n_hits": b_hits, "n_raised": n_raised, "n_queries": b_q, "n_widened": n_widened}
    assert b_hits == n_best and set(plain) == {f for f, _ in pipeline.PipelineStats._fields_}
    assert all(stats[k] == plain[k] for k in ("n_hits", "n_queries", "n_taxids", "n_unmatched_rows"))
