"""What the labelled exports (`build-db sintax`, `build-db dada2`; csrc/seqdb_gpu.hip) cost beside `build-db kraken2` on the two
synthetic listings of scripts/seqdb_bench.py: many short lines (about 1.5 kB) and a few huge ones.  One
process: per listing kraken2 first as the yardstick, then sintax and dada2 against a taxonomies file of about 2 M rows (read
from its cache-db cache).  Records read, GPU, write and wall per format, `t_labels_ms`, and the ratio of the sintax GPU stage
to the kraken2 GPU stage on the same listing.  Everything lives under a temporary directory that is removed at the end.

    python scripts/seqdb_label_bench.py [--gb 3] [--rows 2000000] [--out profiles/seqdb_label_bench.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from blutils_amd import pipeline, seqdb, synth_seqdb  # noqa: E402


def write_taxonomies(path: str, n_rows: int) -> None:
    """Taxids spread over [1, 3 000 000) as the listings' are (synth_seqdb), so that about n_rows / 3 M of the lines join; seven
    ranked elements and two unranked ones per lineage, one row in 50 without a kind."""
    step = 3_000_000 / n_rows
    with open(path, "w") as f:
        f.write('{"blutilsVersion": "8.3.1", "ignoreTaxids": null, "replaceRank": null, "dropNonLinnaeanTaxonomies": false, '
                '"sourceDatabase": "bench", "taxonomies": [\n')
        for i in range(n_rows):
            t = 1 + int(i * step)
            if i % 50 == 49:
                text = f"no-rank__cellular-organisms;clade__group-{t % 977}"
            else:
                text = (f"no-rank__cellular-organisms;d__bacteria;p__phylum-{t % 41};c__class-{t % 211};o__order-{t % 997};"
                        f"f__family-{t % 4999};clade__group-{t % 977};g__genus-{t % 49999};s__genus-{t % 49999}-species-{t}")
            f.write('%s{"taxid": %d, "rank": "s", "numericLineage": "d__2;s__%d", "textLineage": "%s", "accessions": []}'
                    % (",\n" if i else "", t, t, text))
        f.write("\n]}\n")


def stages(st: dict) -> dict:
    return {"read": st["t_read_ms"], "gpu": st["t_gpu_ms"], "write": st["t_write_ms"], "wall": st["t_wall_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=3.0, help="size of each listing")
    ap.add_argument("--rows", type=int, default=2_000_000, help="rows of the taxonomies file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqdb_label_bench.json"))
    ap.add_argument("--tmp", default="/tmp")
    a = ap.parse_args()
    target = int(a.gb * 1e9)
    tmp = tempfile.mkdtemp(prefix="seqdb-label-bench-", dir=a.tmp)
    res = {"listing_gb": a.gb, "taxonomy_rows": a.rows, "cases": {}}
    try:
        tax, cache = os.path.join(tmp, "tax.blutils.json"), os.path.join(tmp, "tax.cache")
        t0 = time.perf_counter()
        write_taxonomies(tax, a.rows)
        res["taxonomies_json_bytes"] = os.path.getsize(tax)
        res["taxonomies_generate_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        pipeline.build_db_cache(tax, cache)
        res["cache_db_s"] = time.perf_counter() - t0
        print(json.dumps({k: v for k, v in res.items() if k != "cases"}), flush=True)
        cases = {"short_lines": dict(n_lines=target // 1520, min_len=1000, max_len=2000),
                 "huge_lines": dict(n_lines=1000, long_lines=[int(target / 12)] * 12)}
        for name, kw in cases.items():
            lst = os.path.join(tmp, name + ".txt")
            t0 = time.perf_counter()
            size = synth_seqdb.write_listing(lst, False, seed=7, odd=False, **kw)
            gen_s = time.perf_counter() - t0
            out = os.path.join(tmp, name + "_out")
            os.makedirs(out)
            k = seqdb.export(seqdb.KRAKEN2, os.path.join(out, "library.fna"), os.path.join(out, "prelim_map.txt"), listing_path=lst)
            case = {"input_bytes": size, "lines": k["n_lines"], "chunks": k["n_chunks"], "generate_s": gen_s,
                    "kraken2": {"fna_bytes": k["fna_bytes"], "stage_ms": stages(k), "gb_per_s": size / k["t_wall_ms"] / 1e6}}
            os.remove(os.path.join(out, "library.fna"))
            for fmt, code in (("sintax", seqdb.SINTAX), ("dada2", seqdb.DADA2)):
                fna = os.path.join(out, fmt + ".fna")
                st = seqdb.export_labelled(code, cache, fna, listing_path=lst)
                case[fmt] = {"fna_bytes": st["fna_bytes"], "stage_ms": stages(st), "t_labels_ms": st["t_labels_ms"],
                             "gb_per_s": size / st["t_wall_ms"] / 1e6, "n_unknown_taxid": st["n_unknown_taxid"],
                             "n_unlabelled": st["n_unlabelled"], "label_bytes": st["label_bytes"], "n_rows": st["n_rows"]}
                os.remove(fna)
            # the labelled exports write no record for a line that does not join: GPU time per byte moved (in and out) too
            moved = {"kraken2": size + k["fna_bytes"] + k["map_bytes"], "sintax": size + case["sintax"]["fna_bytes"],
                     "dada2": size + case["dada2"]["fna_bytes"]}
            for fmt, b in moved.items():
                case[fmt]["gpu_ms_per_gb_moved"] = case[fmt]["stage_ms"]["gpu"] / (b / 1e9)
            case["gpu_stage_sintax_over_kraken2"] = case["sintax"]["stage_ms"]["gpu"] / case["kraken2"]["stage_ms"]["gpu"]
            case["gpu_stage_dada2_over_kraken2"] = case["dada2"]["stage_ms"]["gpu"] / case["kraken2"]["stage_ms"]["gpu"]
            res["cases"][name] = case
            print(name, json.dumps(case), flush=True)
            os.remove(lst)
            shutil.rmtree(out, ignore_errors=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
